#!/usr/bin/env python
"""Event-timed B = 1 decode of the FFHQ VAE decoder class at the released size (latent [1, 12, 16, 16] -> planes [1, 96, 256, 256];
synthetic weights), and of its two roll-out convolutions alone: the fused ln3d_conv3x3_rollout_bf16 against the
ln3d_im2col3x3_rollout + ln3d_gemm_bf16 + ln3d_resize_add_lrelu composition on the same operands, in the same process (C = 128 with the
low-resolution base: conv3D_0; C = 32 with the full-resolution base: conv3D_1).  Prints one JSON line per case: median / min over the
timed runs, and the GPU clock read before / after.  GPU box only.

    python tools/ffhq_decoder_bench.py [--runs 20] [--warmup 3]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/ffhq_decoder_bench.py --runs 5        (per-kernel table, a run of its own)
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from encoder_bench import sclk, timed  # noqa: E402


def conv_case(ops, C, lowres, runs, warmup, R=256, Co=32):
    dev = 'cuda'
    g = torch.Generator().manual_seed(C)
    x = torch.randn(3, R, R, C, generator=g).to(dev)
    xb = x.to(torch.bfloat16) if lowres else x                 # conv3D_0 reads the bf16 up-sampled planes, conv3D_1 the fp32 x0
    K = 27 * C
    w = (torch.randn(3, Co, K, generator=g) / K ** 0.5).to(dev).to(torch.bfloat16)
    bias = torch.randn(3, Co, generator=g).to(dev)
    bh = R // 4 if lowres else R
    base = torch.randn(3, bh, bh, Co, generator=g).to(dev)
    rowm, colm = torch.empty(3, R, C, device=dev), torch.empty(3, R, C, device=dev)
    ops.rollout_means(xb, rowm, colm, 3, R, R, C)
    out = torch.empty(3, R, R, Co, device=dev)
    fused = timed(lambda: ops.conv3x3_rollout(xb, rowm, colm, w, bias, base, out, R, R, C, Co, 0.01), runs, warmup)
    Kpad = (K + 63) // 64 * 64
    col = torch.empty(R * R, Kpad, device=dev, dtype=torch.bfloat16)
    wpad = torch.zeros(3, Co, Kpad, device=dev, dtype=torch.bfloat16)
    wpad[:, :, :K] = w
    t = torch.empty(3, R * R, Co, device=dev)
    comp_out = torch.empty(3, R, R, Co, device=dev)
    xf = xb.float().contiguous()
    bi = [bias[i].contiguous() for i in range(3)]

    def composition():
        for i in range(3):
            ops.im2col3x3_rollout(xf, rowm, colm, col, i, R, R, C, Kpad)
            ops.gemm(col, wpad[i], bi[i], ops.EPI_F32, t[i])
        ops.resize_add_lrelu(base, t, comp_out, 3, bh, bh, R, R, Co, 0.01)
    comp = timed(composition, runs, warmup)
    gflop = 2.0 * 3 * R * R * Co * K / 1e9
    print(json.dumps({'case': f'rollout conv C={C} {R}x{R} -> {Co} ({"low-res" if lowres else "full-res"} base)', 'runs': runs,
                      'fused_median_ms': round(fused[0], 4), 'fused_min_ms': round(fused[1], 4),
                      'im2col_gemm_median_ms': round(comp[0], 4), 'im2col_gemm_min_ms': round(comp[1], 4),
                      'speedup_median': round(comp[0] / fused[0], 2), 'gflop': round(gflop, 1), 'fused_tflops': round(gflop / fused[0], 1),
                      'max_abs_diff': float((out - comp_out).abs().max())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    from ln3diff_amd import ops
    from ln3diff_amd.nsr.triplane import Triplane
    from ln3diff_amd.synth import fill_module_random_
    from ln3diff_amd.vit import vit_triplane_ffhq as ff
    dev = 'cuda'
    clk0 = sclk()
    tp = Triplane(img_resolution=128, rendering_kwargs=ff.ffhq_rendering_kwargs('ffhq'), decoder_output_dim=32)
    dec = fill_module_random_(getattr(ff, ff.CLASS_NAME)(ff.dinov2_vitb14(), tp, False).to(dev), 1, dev)
    lat = torch.randn(1, 12, 16, 16, device=dev)

    def decode():
        return dec.vit_decode_postprocess(dec.vit_decode_backbone(lat, 128), {}, want_nchw=False)
    vit = dec.vit_decode_backbone(lat, 128)
    d_med, d_min = timed(decode, args.runs, args.warmup)
    b_med, _ = timed(lambda: dec.vit_decode_backbone(lat, 128), args.runs, args.warmup)
    p_med, _ = timed(lambda: dec.vit_decode_postprocess(vit, {}, want_nchw=False), args.runs, args.warmup)
    print(json.dumps({'case': 'ffhq decode B=1 (latent -> planes 96 x 256 x 256)', 'median_ms': round(d_med, 3), 'min_ms': round(d_min, 3),
                      'runs': args.runs, 'backbone_median_ms': round(b_med, 3), 'postprocess_median_ms': round(p_med, 3)}), flush=True)
    conv_case(ops, 128, True, args.runs, args.warmup)
    conv_case(ops, 32, False, args.runs, args.warmup)
    print(json.dumps({'sclk_before': clk0, 'sclk_after': sclk()}), flush=True)


if __name__ == '__main__':
    main()
