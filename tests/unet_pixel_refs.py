"""Per-pixel criterion for the U-Net denoiser, block by block (CPU only: torch and the oracle, no HIP) - the analogue of
dit_token_refs.py, whose criterion it reuses unchanged (token_rho / worst_token / yardstick).

A GROUP is the C numbers at one (sample, y, x) of a block's output (the time embedding: one row).  End to end the criterion cannot
hold for a conv net: every GroupNorm -> conv re-rounds the whole activation and two correct bf16 implementations decorrelate to the
full bf16 noise level within a few layers (tests/test_unet_pixels_cpu.py records the measurement).  So every block is judged on its
own, on the SAME input x_in for both oracles and the HIP block:

    y64 = oracle.unet.run_block in float64
    y16 = the same under operand_rounding(bf16, kernel_arith=True)
    d = ||y16 - y64||,  e = ||y_hip - y16||,  rho = e / max(d, 0.1 median d)        per group, every group counted

and the wiring between the blocks is checked exactly (tests/test_unet_pixels_gpu.py).

Tier A: three whole networks walked block by block (batch 3, timesteps 999 / 500 / 37: every sample its own embedding row); the block
inputs are the taps of the end-to-end y16 forward cast to fp32.  Tier B: single blocks at the shapes where kernels go wrong, driven
at any N, H, W with synth_input.  Every case states the launch it expects - the attention kernel (or 'small'), the shortcut form and
whether a GEMM leaves the 128x128 tile - and tests/test_unet_pixels_cpu.py holds the statements to ln3diff_amd.convstack and
csrc/kernel_plan.h.  B * heads stays below the CU count, so the K-resident attention kernel (not restated by the oracle) never runs."""
import functools
import os
import subprocess
import sys

import torch
import torch.nn as nn

from conftest import ROOT, load_synth
from dit_token_refs import YARD_MAX, YARD_MEDIAN, to64, token_rho, worst_token      # noqa: F401  (the criterion, not forked)
from ln3diff_amd.synth import synth_input
from oracle import dit as odit
from oracle import unet as ounet

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
from unet_configs import CONFIGS      # noqa: E402

CUS = 256                       # MI355X; the GPU test repeats the K-resident assertion with the device's own count
GEMM_RING_ROWS = 1536           # csrc/kernel_plan.h: a GEMM leaves the 128x128 register-staged tile at M >= 1536 and N >= 128
TIMESTEPS = (999., 500., 37.)
TED = 256                       # emb width of the single ResBlocks
CONTEXT_DIM = 768


# ------------------------------------------------------------------------------------------------ groups
def pixels(y):
    """[B, C, H, W] -> [B, H*W, C]; the time embedding [B, D] -> [B, 1, D]"""
    y = torch.as_tensor(y).detach()
    if y.dim() == 2:
        return y[:, None]
    B, C, H, W = y.shape
    return y.permute(0, 2, 3, 1).reshape(B, H * W, C)


def pixel_rho(y_hip, y16, y64):
    """-> (rho, d), one entry per (sample, y, x); every pixel is in it"""
    rho, d = token_rho(pixels(y_hip), pixels(y16), pixels(y64), None)
    assert rho.numel() == y16.numel() // y16.shape[1] and y_hip.shape == y16.shape == y64.shape, (rho.shape, y_hip.shape, y16.shape)
    return rho, d


def pixel_yardstick(y16, y64):
    """per-group d / ||y64||: (median, max)"""
    g16, g64 = pixels(y16).double(), pixels(y64).double()
    r = (g16 - g64).norm(dim=-1) / g64.norm(dim=-1)
    return float(r.median()), float(r.max())


def worst_pixel(rho):
    (b, _, l), w = worst_token(rho)
    return (b, l), w


# ------------------------------------------------------------------------------------------------ tier A: networks
_DEF = dict(num_heads=-1, num_head_channels=-1, num_heads_upsample=-1, legacy=True, transformer_depth=1, context_dim=None)
NETS = {
    'st': dict(_DEF, **CONFIGS['tiny_st']),
    'attn-roll': dict(_DEF, **CONFIGS['tiny_attn']),
    'attn-96': dict(_DEF, image_size=16, in_channels=4, model_channels=64, out_channels=4, num_res_blocks=1, attention_resolutions=[1, 2],
                    channel_mult=(1, 1.5), num_heads=2, num_heads_upsample=1, use_spatial_transformer=False, use_scale_shift_norm=True,
                    roll_out=False),
    # not walked: its attention layers are single cases below
    'nhc32': dict(_DEF, image_size=16, in_channels=4, model_channels=128, out_channels=4, num_res_blocks=1, attention_resolutions=[1, 2],
                  channel_mult=(1, 2), num_head_channels=32, legacy=False, use_spatial_transformer=False, use_scale_shift_norm=True,
                  roll_out=False),
}
WALKED = ('st', 'attn-roll', 'attn-96')
# What each walked network is expected to launch: {(head size, tokens): self-attention launch}, the cross-attention key count (always
# ln3d_attention_small), {shortcut input width: 'gemm' | 'centre'} (the centre tap of a 3x3 where the width is no multiple of 64), the
# largest row count of a GEMM and whether any GEMM leaves the 128x128 tile.
NET_LAUNCH = {
    'st': dict(self_attn={(32, 256): 'stream', (64, 64): 'small'}, cross_keys=77, skips={128: 'gemm', 256: 'gemm', 384: 'gemm', 512: 'gemm'},
               rows=768, ring_gemm=False),
    'attn-roll': dict(self_attn={(32, 768): 'stream', (64, 192): 'small'}, cross_keys=None, skips={128: 'gemm', 256: 'gemm', 384: 'gemm', 512: 'gemm'},
                      rows=2304, ring_gemm=True),
    'attn-96': dict(self_attn={(32, 256): 'stream', (48, 64): 'small', (96, 64): 'small', (64, 256): 'stream'}, cross_keys=None,
                    skips={64: 'gemm', 192: 'gemm', 160: 'centre', 128: 'gemm'}, rows=768, ring_gemm=False),
}


def build_net(net):
    """the product module of a network (a parameter container until it runs: built on the CPU too, for its state dict)"""
    from ln3diff_amd.guided_diffusion.unet import UNetModel
    c = NETS[net]
    return UNetModel(image_size=c['image_size'], in_channels=c['in_channels'], model_channels=c['model_channels'], out_channels=c['out_channels'],
                     num_res_blocks=c['num_res_blocks'], attention_resolutions=tuple(c['attention_resolutions']), channel_mult=c['channel_mult'],
                     num_heads=c['num_heads'], num_head_channels=c['num_head_channels'], num_heads_upsample=c['num_heads_upsample'],
                     use_scale_shift_norm=c['use_scale_shift_norm'], use_spatial_transformer=c['use_spatial_transformer'],
                     transformer_depth=c['transformer_depth'], context_dim=c['context_dim'] if c['use_spatial_transformer'] else -1,
                     legacy=c['legacy'], roll_out=c['roll_out'])


@functools.lru_cache(maxsize=None)
def net_sd(net):
    """the synthetic fp32 state dict of a network (seed 0); shared, never modified"""
    return load_synth(build_net(net), 0)[0]


def net_inputs(net):
    """(x [3, C, S, S], timesteps [3], context [3, 77, 768] or None)"""
    c = NETS[net]
    B, S = len(TIMESTEPS), c['image_size']
    x = synth_input('x', (B, c['in_channels'] * (3 if c['roll_out'] else 1), S, S), 31)
    ctx = synth_input('c', (B, 77, c['context_dim']), 31) if c['use_spatial_transformer'] else None
    return x, torch.tensor(TIMESTEPS), ctx


def block_names(net):
    return ['time_embed'] + [n for n, _ in ounet.blocks(NETS[net])]


def rounded_forward(net, sd=None, taps=None):
    """the end-to-end y16 of a network, computed afresh (the injected-defect tests call it with oracle functions or weights replaced)"""
    x, t, ctx = net_inputs(net)
    with torch.no_grad(), odit.operand_rounding(torch.bfloat16, kernel_arith=True):
        return ounet.unet_forward(to64(net_sd(net) if sd is None else sd), NETS[net], x.double(), t.double(), to64(ctx), taps)


@functools.lru_cache(maxsize=None)
def net_oracles(net):
    """(y64, y16, taps of the y16 forward): one computation per process"""
    x, t, ctx = net_inputs(net)
    with torch.no_grad():
        y64 = ounet.unet_forward(to64(net_sd(net)), NETS[net], x.double(), t.double(), to64(ctx))
    taps = {}
    y16 = rounded_forward(net, taps=taps)
    assert y64.dtype == y16.dtype == torch.float64
    return y64, y16, taps


def run_net_block(net, name, x_in, emb, sd=None, rounded=True):
    """one block of a walked network on (x_in, emb) in float64: the time embedding (x_in: the timesteps) or a block of oracle.unet.blocks"""
    cfg, sd = NETS[net], to64(net_sd(net) if sd is None else sd)
    ctx = to64(net_inputs(net)[2])

    def run():
        if name == 'time_embed':
            return ounet.time_embed(sd, cfg, x_in.double())
        return ounet.run_block(sd, cfg, name, x_in.double(), emb.double(), ctx)
    with torch.no_grad():
        if not rounded:
            return run()
        with odit.operand_rounding(torch.bfloat16, kernel_arith=True):
            return run()


@functools.lru_cache(maxsize=None)
def block_pair(net, name):
    """(x_in fp32, emb fp32, y64, y16) of one block: its input is the tap of the end-to-end y16 forward cast to fp32 (the time
    embedding's: the timesteps), and both oracles - and the HIP block - get exactly that."""
    taps = net_oracles(net)[2]
    x_in, emb = taps[name][0].float(), taps['time_embed'][1].float()
    y64, y16 = run_net_block(net, name, x_in, emb, rounded=False), run_net_block(net, name, x_in, emb)
    assert y64.dtype == y16.dtype == torch.float64
    return x_in, emb, y64, y16


def emb_silu_bf16(emb):
    """SiLU(emb) as the ResBlocks' emb Linear takes it, in the oracle's own arithmetic: the same bits on both sides"""
    return torch.nn.functional.silu(emb.double()).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ tier B: single blocks
def _single(cid, kind, p, N, H, W, Lc=None, ss=True, attn=(), skip='none', scale=1.0, raises=False, net=None, path=None, why=''):
    """attn: [(head size, keys, launch, self-attention)] of the block; net / path: the layer lives in a network (its state dict, its module)"""
    cin = p.get('cin', p['ch'] if 'ch' in p else None)
    heads = p.get('heads', 1)
    assert N * heads < CUS, "the K-resident attention kernel must not be what runs"
    widths = [p.get('cout', cin)] + ([3 * cin] if kind == 'attention' else []) + ([8 * cin, 3 * cin] if kind == 'transformer' else [])
    rows = N * H * W * (4 if kind == 'up' else 1)
    return dict(id=cid, kind=kind, p=p, N=N, H=H, W=W, Lc=Lc, ss=ss, attn=list(attn), skip=skip, scale=scale, raises=raises, net=net, path=path,
                cin=cin, rows=rows, nmax=max(widths), ring_gemm=rows >= GEMM_RING_ROWS and max(widths) >= 128, why=why)


def _ab(cid, C, heads, H, W, route, N=2, why='', **kw):
    return _single(cid, 'attention', dict(ch=C, heads=heads), N, H, W, attn=[(C // heads, H * W, route, True)], why=why, **kw)


def _st(cid, C, heads, H, W, route, Lc, depth=1, N=2, why=''):
    dh = C // heads
    return _single(cid, 'transformer', dict(ch=C, heads=heads, dim_head=dh, depth=depth, context_dim=CONTEXT_DIM), N, H, W, Lc=Lc,
                   attn=[(dh, H * W, route, True), (dh, Lc, 'small', False)], why=why)


def _nhc32_cases():
    """the attention layers of the num_head_channels=32, legacy=False network (heads = ch // 32 everywhere, output blocks included)"""
    cs = []
    for name, layers in ounet.blocks(NETS['nhc32']):
        for li, (kind, p) in enumerate(layers):
            if kind == 'attention':
                S = 16 if p['ch'] == 128 else 8
                blk, _, idx = name.partition('.')
                cs.append(_single(f'nhc32-{name}', kind, p, 2, S, S, attn=[(32, S * S, 'stream' if S == 16 else 'small', True)],
                                  net='nhc32', path=(blk, int(idx) if idx else None, li), why='num_head_channels=32, legacy=False'))
                assert p['heads'] == p['ch'] // 32
    return cs


def _cases():
    cs = [
        _ab('ab-128h4-16x16', 128, 4, 16, 16, 'stream', why='256 tokens, dh 32 -> 64'),
        _ab('ab-128h4-32x32', 128, 4, 32, 32, 'stream', N=1, why='1024 tokens: four key blocks of 256'),
        _ab('ab-128h4-16x18', 128, 4, 16, 18, 'ring64', why='288 tokens: half a 64-key block of tail'),
        _ab('ab-128h4-17x17', 128, 4, 17, 17, 'small', why='289 tokens: lanes past the last key'),
        _ab('ab-128h4-15x17', 128, 4, 15, 17, 'small', why='255 tokens: one below the MFMA threshold'),
        _ab('ab-160h2-16x16', 160, 2, 16, 16, 'ring80', why='dh 80'),
        _ab('ab-192h2-16x16', 192, 2, 16, 16, 'ring128', why='dh 96 -> 128'),
        _ab('ab-96h8-16x16', 96, 8, 16, 16, 'small', why='dh 12: refused by the MFMA route'),
        _ab('ab-320h2-8x8', 320, 2, 8, 8, 'small', why='dh 160 at 64 tokens'),
        _ab('ab-320h2-33x32', 320, 2, 33, 32, 'small', N=1, raises=True, why='dh 160 at 1056 tokens: the ValueError of self_attend'),
        _st('st-128h4-d2-lc1', 128, 4, 16, 16, 'stream', 1, depth=2, why='one context key'),
        _st('st-128h4-d2-lc64', 128, 4, 16, 16, 'stream', 64, depth=2, why='one lane round of keys exactly'),
        _st('st-128h4-d2-lc65', 128, 4, 16, 16, 'stream', 65, depth=2, why='one key behind 64'),
        _st('st-128h4-d2-lc77', 128, 4, 16, 16, 'stream', 77, depth=2, why='the CLIP context'),
        _st('st-256h4-8x8', 256, 4, 8, 8, 'small', 77, why='dh 64 at 64 tokens'),
        _st('st-256h4-16x16', 256, 4, 16, 16, 'stream', 77, why='dh 64 at 256 tokens: nothing to pad'),
        _single('down-7x9', 'down', dict(ch=64), 2, 7, 9, why='odd H x W through the strided conv'),
        _single('down-8x8', 'down', dict(ch=64), 2, 8, 8),
        _single('down-1x1', 'down', dict(ch=64), 2, 1, 1, why='every tap but the centre is padding'),
        _single('up-5x7', 'up', dict(ch=64), 2, 5, 7, why='odd H x W through the nearest-2x conv'),
        _single('up-1x1', 'up', dict(ch=64), 2, 1, 1),
        _single('res-n1-160to96', 'res', dict(cin=160, cout=96), 1, 5, 6, skip='centre', why='N = 1; centre-tap shortcut; scale-shift'),
        _single('res-1x1-128', 'res', dict(cin=128, cout=128), 3, 1, 1, ss=False, why='H * W = 1: 4 numbers per group; h + emb'),
    ] + _nhc32_cases()
    return {c['id']: c for c in cs}


CASES = _cases()
CASE_IDS = list(CASES)


def build_single(c):
    """the product module of a single case (from its network, with the network's synthetic weights, where it lives in one)"""
    from ln3diff_amd.guided_diffusion import unet as pu
    if c['net'] is not None:
        m = build_net(c['net'])
        m.load_state_dict(net_sd(c['net']), strict=True)
        blk, idx, li = c['path']
        return (getattr(m, blk) if idx is None else getattr(m, blk)[idx])[li]
    p = c['p']
    if c['kind'] == 'attention':
        m = pu.AttentionBlock(p['ch'], num_heads=p['heads'])
    elif c['kind'] == 'transformer':
        m = pu.SpatialTransformer(p['ch'], p['heads'], p['dim_head'], depth=p['depth'], context_dim=p['context_dim'])
    elif c['kind'] == 'down':
        m = pu.Downsample(p['ch'], True)
    elif c['kind'] == 'up':
        m = pu.Upsample(p['ch'], True)
    else:
        m = pu.ResBlock(p['cin'], TED, 0, out_channels=p['cout'], use_scale_shift_norm=c['ss'])
    m.load_state_dict({k[len('blk.0.'):]: v for k, v in single_sd(c['id']).items()}, strict=True)
    return m


@functools.lru_cache(maxsize=None)
def single_sd(cid):
    """-> the state dict the oracle reads the case's layer from (run_layers: prefix 'blk', layer 0; in a network: the network's)"""
    c = CASES[cid]
    if c['net'] is not None:
        return net_sd(c['net'])
    from ln3diff_amd.guided_diffusion import unet as pu
    p = c['p']
    shell = {'attention': lambda: pu.AttentionBlock(p['ch'], num_heads=p['heads']),
             'transformer': lambda: pu.SpatialTransformer(p['ch'], p['heads'], p['dim_head'], depth=p['depth'], context_dim=p['context_dim']),
             'down': lambda: pu.Downsample(p['ch'], True), 'up': lambda: pu.Upsample(p['ch'], True),
             'res': lambda: pu.ResBlock(p['cin'], TED, 0, out_channels=p['cout'], use_scale_shift_norm=c['ss'])}[c['kind']]()
    return load_synth(nn.ModuleDict({'blk': nn.ModuleList([shell])}), 0)[0]


def single_inputs(cid):
    """(x [N, C, H, W], emb [N, TED] or None, context [N, Lc, 768] or None) of a single case, fp32"""
    c = CASES[cid]
    seed = 40 + CASE_IDS.index(cid)
    x = synth_input('h', (c['N'], c['cin'], c['H'], c['W']), seed) * c['scale']
    emb = synth_input('emb', (c['N'], TED), seed) if c['kind'] == 'res' else None
    ctx = synth_input('c', (c['N'], c['Lc'], CONTEXT_DIM), seed) if c['Lc'] else None
    return x, emb, ctx


def run_single(cid, sd=None, rounded=True, x=None, ctx=None):
    """sd / x / ctx: replacements for the case's own (the injected-defect tests)"""
    c = CASES[cid]
    x0, emb, ctx0 = single_inputs(cid)
    x, ctx = x0 if x is None else x, ctx0 if ctx is None else ctx
    sd = to64(single_sd(cid) if sd is None else sd)
    if c['net'] is not None:
        blk, idx, li = c['path']
        prefix, first = (blk if idx is None else f'{blk}.{idx}'), li
    else:
        prefix, first = 'blk', 0

    def run():
        return ounet.run_layers(sd, prefix, [(c['kind'], c['p'])], x.double(), to64(emb), to64(ctx), c['ss'], first=first)
    with torch.no_grad():
        if not rounded:
            return run()
        with odit.operand_rounding(torch.bfloat16, kernel_arith=True):
            return run()


@functools.lru_cache(maxsize=None)
def single_pair(cid):
    """(y64, y16) of a single case: one computation per process"""
    y64, y16 = run_single(cid, rounded=False), run_single(cid)
    assert y64.dtype == y16.dtype == torch.float64
    return y64, y16


# ------------------------------------------------------------------------------------------------ the plan of csrc/kernel_plan.h
ATTN_KERNELS = ['short', 'kres', 'stream', 'ring64_occ4', 'ring64_occ2', 'ring80', 'ring80_t72', 'ring128', 'ring128_t72']   # enum Ln3dAttnKernel
ROUTE_OF_KERNEL = {'stream': 'stream', 'ring64_occ4': 'ring64', 'ring64_occ2': 'ring64', 'ring80': 'ring80', 'ring128': 'ring128'}
TILE_S128 = 0                                                                                                             # enum Ln3dTileRow
_PROBE = r'''
#include <stdio.h>
#include "kernel_plan.h"
int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  int Dp, dh_true, L, BH, M, N, K, cus;
  while (f && fscanf(f, "%d %d %d %d %d %d %d %d", &Dp, &dh_true, &L, &BH, &M, &N, &K, &cus) == 8) {
    const int lpad = (L + 63) / 64 * 64;
    printf("%d %d\n", ln3d_plan_attention(Dp, dh_true, L, lpad, L, lpad, BH, false, cus),
           ln3d_plan_gemm(M, N, K, LN3D_EPI_GATE_RES, false, true, cus, -1));
  }
  return 0;
}
'''


def plan(lines, tmp_path):
    """lines: [(Dp, dh_true, L, B * heads, M, N, K, cus)] -> [(attention kernel name or the negative error, GEMM left the 128x128 tile)]:
    what ops.attention (self_attention_hip's launch: keys padded to 64) and ln3d_gemm_bf16 are planned to run, from the header itself"""
    with open(tmp_path / 'unet_probe.cpp', 'w') as f:
        f.write(_PROBE)
    with open(tmp_path / 'unet_lines.txt', 'w') as f:
        f.write(''.join('%d %d %d %d %d %d %d %d\n' % tuple(ln) for ln in lines))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-I', os.path.join(ROOT, 'ln3diff_amd', 'csrc'), 'unet_probe.cpp', '-o',
                           'unet_probe'], cwd=tmp_path)
    out = subprocess.check_output([str(tmp_path / 'unet_probe'), 'unet_lines.txt'], cwd=tmp_path, text=True).splitlines()
    assert len(out) == len(lines)
    rows = [[int(v) for v in ln.split()] for ln in out]
    return [(ATTN_KERNELS[a] if a >= 0 else a, g != TILE_S128) for a, g in rows]


def launch_line(who, dh, L, route, BH, rows, nmax, cus=CUS):
    """one stated self-attention launch (and the widest GEMM beside it) as a plan() line, with the statement: (who, route, line)"""
    from ln3diff_amd.dit.dit_models_xformers import attn_head_pad, attn_out_dim
    Dp = attn_head_pad(dh)
    return who, route, (Dp, dh if attn_out_dim(dh) != Dp else 0, L, BH, rows, nmax, 128, cus)


def mfma_launches(cus=CUS):
    """every self-attention the cases state to be an MFMA launch, as plan() lines, with the statement: [(who, route, line)]"""
    out = []

    def add(who, dh, L, route, BH, rows, nmax):
        out.append(launch_line(who, dh, L, route, BH, rows, nmax, cus))
    for net in WALKED:
        B = len(TIMESTEPS)
        heads = {(p['ch'] // p['heads'], p['heads']) for _, layers in ounet.blocks(NETS[net]) for k, p in layers if k in ('attention', 'transformer')}
        for (dh, L), route in NET_LAUNCH[net]['self_attn'].items():
            add(net, dh, L, route, B * max(h for d, h in heads if d == dh), NET_LAUNCH[net]['rows'], 128)
    for c in CASES.values():
        for dh, L, route, is_self in c['attn']:
            if is_self and not c['raises']:
                add(c['id'], dh, L, route, c['N'] * c['p']['heads'], c['rows'], c['nmax'])
    return out
