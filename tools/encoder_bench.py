#!/usr/bin/env python
"""Event-timed `encoder_vae` of the released multi-view VAE encoder (B = 1 object at 256 x 256, F = 6 and F = 40 views; synthetic
weights), and of its joint attention launch alone.  Prints one JSON line per case: median / min over the timed runs, the achieved
rate against the reference's FLOP count (torch FLOP counter on the reference module: 376 GFLOP at F = 6; scaled for other F from
the per-view convolution part plus the F^2 attention part), and the GPU clock read before / after.  GPU box only.

    python tools/encoder_bench.py [--frames 6 40] [--runs 20] [--warmup 3]
"""
import argparse
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ATTN_GFLOP_F6 = 78.0                        # joint attention of the 6-view object as torch counts it (QK^T and PV: 4 * 6144^2 * 512)
TOTAL_GFLOP_F6 = 376.0


def ref_gflop(F):
    """376 GFLOP at F = 6, of which ~78 GFLOP joint attention (grows with F^2); the rest is per view."""
    return (TOTAL_GFLOP_F6 - ATTN_GFLOP_F6) * F / 6 + ATTN_GFLOP_F6 * (F / 6) ** 2


def sclk():
    try:
        out = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True, timeout=20).stdout
        return [l.strip() for l in out.splitlines() if 'sclk' in l][:1]
    except Exception as e:                   # informational only
        return [f'unavailable: {e}']


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, nargs='+', default=[6, 40])
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    from ln3diff_amd import ops
    from ln3diff_amd.dit.dit_decoder import DiT2
    from ln3diff_amd.nsr.script_util import AE
    from ln3diff_amd.nsr.triplane import Triplane
    from ln3diff_amd.synth import fill_module_random_
    from ln3diff_amd.vit.mv_encoder import RELEASED_DINO_VERSION, create_encoder
    from ln3diff_amd.vit.vit_triplane import RodinSR_256_fusionv6_ConvQuant_liteSR_dinoInit3DAttn_SD_B_3L_C_withrollout_withSD_D_ditDecoder as Dec
    dev = 'cuda'
    vit = DiT2(input_size=16, patch_size=2, in_channels=128, hidden_size=128, depth=2, num_heads=2, num_classes=0, learn_sigma=False,
               mixed_prediction=False, context_dim=None, roll_out=True, plane_n=3)
    dec = Dec(vit_decoder=vit, triplane_decoder=Triplane(img_resolution=128), cls_token=False, vae_p=2, ldm_z_channels=4, ldm_embed_dim=4)
    dec = fill_module_random_(dec.to(dev), 1, dev)
    clk0 = sclk()
    for F in args.frames:
        enc = fill_module_random_(create_encoder(num_frames=F).to(dev), 0, dev)
        ae = AE(enc, dec, 128, dino_version=RELEASED_DINO_VERSION)
        x = torch.randn(F, 10, 256, 256, device=dev)
        eps = torch.randn(1, 4, 3, 1024)
        med, best = timed(lambda: ae(img=x, behaviour='encoder_vae', eps=eps), args.runs, args.warmup)
        # the joint attention launch alone at this F (B = 1 object, 8 heads of 64, F * 1024 tokens)
        N = F * 1024
        q = torch.randn(1, 8, N, 64, device=dev).to(torch.bfloat16)
        k = torch.randn(1, 8, N, 64, device=dev).to(torch.bfloat16)
        vt = torch.randn(1, 8, 64, N, device=dev).to(torch.bfloat16)
        o = torch.empty(1, N, 512, device=dev, dtype=torch.bfloat16)
        a_med, _ = timed(lambda: ops.attention(q, k, vt, o, 1, 8, N, N, N, N, 64), args.runs, args.warmup)
        attn_flop = 4.0 * N * N * 64 * 8
        gf = ref_gflop(F)
        print(json.dumps({'case': f'encoder_vae B=1 F={F} 256x256', 'median_ms': round(med, 3), 'min_ms': round(best, 3), 'runs': args.runs,
                          'ref_gflop': round(gf, 1), 'tflops': round(gf / med, 1),
                          'joint_attention_ms': round(a_med, 3), 'joint_attention_tflops': round(attn_flop / a_med / 1e9, 1)}), flush=True)
        del enc, ae, q, k, vt, o
        torch.cuda.empty_cache()
    print(json.dumps({'sclk_before': clk0, 'sclk_after': sclk()}), flush=True)


if __name__ == '__main__':
    main()
