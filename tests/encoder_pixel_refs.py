"""Per-pixel criterion for the multi-view VAE encoder, stage by stage (CPU only: torch and the oracle, no HIP) - the analogue of
unet_pixel_refs.py, whose criterion (that of dit_token_refs.py) it reuses unchanged.

A GROUP is the C numbers at one (frame, y, x) of a stage's output.  Every stage of oracle.encoder.stages is judged on its own, on the
SAME input x_in for both oracles and the HIP stage (GroupNorm -> conv decorrelates two correct bf16 implementations end to end:
tests/test_unet_pixels_cpu.py):

    y64 = oracle.encoder.run_stage in float64
    y16 = the same under operand_rounding(bf16, kernel_arith=True)
    d = ||y16 - y64||,  e = ||y_hip - y16||,  rho = e / max(d, 0.1 median d)        per group, every group counted

and the wiring between the stages is checked exactly (tests/test_encoder_pixels_gpu.py).

Tier A (NETS): three whole encoders walked stage by stage; the stage inputs are the taps of the end-to-end y16 forward cast to fp32.
Tier B (the other CASES): one stage of an encoder, driven directly with a synthetic activation.  Every case states the launches it
expects - the attention kernel of attn1 (over the F*H*W tokens of an object) and of attn2 (over the H*W tokens of a frame), whether
each meets the padded output projection, the shortcut forms and whether a GEMM leaves the 128x128 tile - and
tests/test_encoder_pixels_cpu.py holds the statements to ln3diff_amd.convstack and csrc/kernel_plan.h.  Sequences * heads of every MFMA
launch stays below the CU count, so the K-resident attention kernel (not restated by the oracle) never runs."""
import functools

import torch

from conftest import load_synth
from dit_token_refs import YARD_MAX, YARD_MEDIAN, to64, token_rho, worst_token              # noqa: F401  (the criterion, not forked)
from ln3diff_amd.synth import synth_input
from oracle import dit as odit
from oracle import encoder as oenc
from unet_pixel_refs import (CUS, GEMM_RING_ROWS, ROUTE_OF_KERNEL, launch_line, mfma_launches, pixel_rho, pixel_yardstick,    # noqa: F401
                             pixels, plan, worst_pixel)

ROUTES = ('small', 'stream', 'ring64', 'ring80', 'ring128')


# ------------------------------------------------------------------------------------------------ configurations
def _cfg(ch=32, in_channels=10, n_heads=8, d_head=64, depth=1, num_frames=6, num_res_blocks=1):
    return dict(ch=ch, ch_mult=(1, 2, 4, 4), num_res_blocks=num_res_blocks, in_channels=in_channels, z_channels=12, double_z=True,
                n_heads=n_heads, d_head=d_head, depth=depth, num_frames=num_frames)


CFGS = {
    'released': _cfg(ch=64),                                   # create_encoder()
    'ch32-f5': _cfg(num_frames=5),
    'dh48': _cfg(d_head=48, num_res_blocks=2, in_channels=3),
    'ch32': _cfg(),
    'f9': _cfg(num_frames=9), 'f1': _cfg(num_frames=1), 'f2': _cfg(num_frames=2), 'f8': _cfg(num_frames=8),
    'dh16': _cfg(d_head=16), 'dh80': _cfg(d_head=80), 'dh128': _cfg(n_heads=2, d_head=128, num_frames=5), 'dh12': _cfg(n_heads=32, d_head=12),
    'depth2': _cfg(depth=2),
    'cin3': _cfg(in_channels=3, num_frames=5), 'cin16': _cfg(in_channels=16, num_frames=5),
}


def build_enc(cfg_name):
    """the product module of a configuration (a parameter container until it runs: built on the CPU too, for its state dict); the
    MVEncoderGSDynamicInp subclass where its guard (num_frames > 4) allows, the base Encoder otherwise"""
    from ln3diff_amd.vit import mv_encoder as pe
    c = CFGS[cfg_name]
    if cfg_name == 'released':
        return pe.create_encoder()
    kw = dict(double_z=True, resolution=64, in_channels=c['in_channels'], ch=c['ch'], ch_mult=list(c['ch_mult']),
              num_res_blocks=c['num_res_blocks'], num_frames=c['num_frames'], dropout=0.0, attn_resolutions=[], out_ch=3,
              z_channels=c['z_channels'], attn_kwargs={'n_heads': c['n_heads'], 'd_head': c['d_head'], 'depth': c['depth']})
    if c['num_frames'] > 4:
        return pe.MVEncoderGSDynamicInp(**kw)
    return pe.Encoder(attn_type='mv-vanilla', **kw)


@functools.lru_cache(maxsize=None)
def cfg_sd(cfg_name):
    """the synthetic fp32 state dict of a configuration (seed 0); shared, never modified"""
    return load_synth(build_enc(cfg_name), 0)[0]


def stage_width(cfg, name):
    """channels of a stage's INPUT"""
    ch, cm = cfg['ch'], cfg['ch_mult']
    if name == 'conv_in':
        return cfg['in_channels']
    if name.startswith('down'):
        lvl = int(name[4:].split('_')[0])
        return ch * cm[lvl] if name.endswith('_ds') else ch * ((1,) + tuple(cm))[lvl]
    return ch * cm[-1]


# ------------------------------------------------------------------------------------------------ the cases
def _case(cid, cfg, stage, objects, H, W, a1=None, a2=None, skips=None, ring_gemm=False, scale=1.0, raises=False, why=''):
    """stage None: a whole network (tier A), H x W its input; otherwise the one stage and the H x W of ITS input.
    a1 / a2: (tokens, launch) of attn1 / attn2; the padded flag of ConvStack.self_attend - the MFMA route ran and its output meets the
    o1p / o2p projection - is launch != 'small'.  skips: {input width of a nin_shortcut: 'gemm' | 'centre'}."""
    c = CFGS[cfg]
    N = objects * c['num_frames']
    for a in (a1, a2):
        assert a is None or a[1] in ROUTES
    return dict(id=cid, cfg=cfg, stage=stage, objects=objects, N=N, H=H, W=W, attn1=a1, attn2=a2, skips=skips or {}, ring_gemm=ring_gemm,
                scale=scale, raises=raises, why=why)


def _mid(cid, cfg, objects, H, W, r1, r2, **kw):
    F = CFGS[cfg]['num_frames']
    return _case(cid, cfg, 'mid_attn_1', objects, H, W, a1=(F * H * W, r1), a2=(H * W, r2), **kw)


def _cases():
    cs = [
        # ---- tier A: whole networks (H x W of the network input; the middle is H/8 x W/8)
        _case('rel64', 'released', None, 2, 64, 64, a1=(384, 'ring64'), a2=(64, 'small'), skips={64: 'gemm', 128: 'gemm'}, ring_gemm=True,
              why='the released widths 64 / 128 / 256; in_channels 10 -> 16'),
        _case('ch32-128', 'ch32-f5', None, 1, 128, 128, a1=(1280, 'stream'), a2=(256, 'stream'), skips={32: 'centre', 64: 'gemm'}, ring_gemm=True,
              why='attn2 on the MFMA route; a 32-wide nin_shortcut as a centre tap'),
        _case('dh48-rect', 'dh48', None, 2, 64, 48, a1=(288, 'ring64'), a2=(48, 'small'), skips={32: 'centre', 64: 'gemm'}, ring_gemm=True,
              why='non-square at every level; heads padded 48 -> 64 and o1p; attn2 with the plain o2; in_channels 3 -> 8'),
        # ---- tier B: single stages at block_in = 128
        _mid('f9-6x6', 'f9', 2, 6, 6, 'small', 'small', why='324 joint tokens: at least 256 but no multiple of 32'),
        _mid('f1-16x16', 'f1', 2, 16, 16, 'stream', 'stream', why='base Encoder(num_frames=1): joint equals per-frame'),
        _mid('f2-8x16', 'f2', 2, 8, 16, 'stream', 'small', why='256 joint vs 128 per frame'),
        _mid('f8-8x8', 'f8', 2, 8, 8, 'stream', 'small', why='512 joint tokens'),
        _mid('obj3-f5', 'ch32-f5', 3, 8, 8, 'ring64', 'small', why='N = 15 and the object grouping of rows; 320 tokens'),
        _mid('dh16', 'dh16', 2, 8, 8, 'ring64', 'small', why='inner 128; heads padded 16 -> 64'),
        _mid('dh80', 'dh80', 2, 8, 8, 'ring80', 'small', why='inner 640'),
        _mid('dh128', 'dh128', 2, 8, 8, 'ring128', 'small', why='2 heads of 128 at 320 tokens'),
        _mid('dh12', 'dh12', 2, 8, 8, 'small', 'small', why='head size no multiple of 8: small at 384 keys, plain projection'),
        _mid('dh12-raises', 'dh12', 1, 16, 16, 'small', 'small', raises=True, ring_gemm=True,
             why='1536 tokens with no MFMA route: the ValueError of self_attend (after proj_in, a 1536-row GEMM)'),
        _mid('depth2', 'depth2', 2, 8, 8, 'ring64', 'small', why='the second block reads the first block\'s stream'),
        _case('ds-8x24-c32', 'ch32', 'down0_ds', 1, 8, 24, why='Downsample on a non-square map, K = 288 -> kpad 320'),
        _case('ds-16x16-c256', 'released', 'down2_ds', 1, 16, 16, why='Downsample at the widest level'),
        _case('cin3', 'cin3', 'conv_in', 1, 16, 24, why='channel padding 3 -> 8'),
        _case('cin10', 'ch32-f5', 'conv_in', 1, 16, 24, why='channel padding 10 -> 16, N = 5'),
        _case('cin16', 'cin16', 'conv_in', 1, 16, 24, why='no channel padding'),
        _case('out-24', 'released', 'conv_out', 2, 8, 8, why='norm_out + swish + a 24-column GEMM at 256 wide, N = 12'),
    ]
    return {c['id']: c for c in cs}


CASES = _cases()
CASE_IDS = list(CASES)
WALKED = tuple(i for i in CASE_IDS if CASES[i]['stage'] is None)
SINGLES = tuple(i for i in CASE_IDS if CASES[i]['stage'] is not None)


def case_cfg(cid):
    return CFGS[CASES[cid]['cfg']]


def stage_names(cid):
    c = CASES[cid]
    return oenc.stages(case_cfg(cid)) if c['stage'] is None else [c['stage']]


def ids():
    """every (case, stage) the GPU test judges, as 'case/stage' (a single stage: the case id)"""
    return [f'{i}/{s}' for i in WALKED for s in stage_names(i)] + [i for i in SINGLES if not CASES[i]['raises']]


def case_input(cid):
    """tier A: the network input [N, in_channels, H, W]; tier B: the stage's input activation, fp32"""
    c = CASES[cid]
    cfg = case_cfg(cid)
    C = cfg['in_channels'] if c['stage'] is None else stage_width(cfg, c['stage'])
    return synth_input('mv' if c['stage'] in (None, 'conv_in') else 'h', (c['N'], C, c['H'], c['W']), 60 + CASE_IDS.index(cid)) * c['scale']


def run(cid, name, x, sd=None, rounded=True, whole=False):
    """one stage (whole: the forward, with `name` the taps dict or None) of a case's encoder on x, in float64.  sd: a replacement for
    the case's own state dict (the injected-defect tests)."""
    cfg, sd = case_cfg(cid), to64(cfg_sd(CASES[cid]['cfg']) if sd is None else sd)

    def go():
        return oenc.forward(sd, cfg, x.double(), name) if whole else oenc.run_stage(sd, cfg, name, x.double())
    with torch.no_grad(), odit.operand_rounding(torch.bfloat16 if rounded else None, kernel_arith=rounded):
        return go()


@functools.lru_cache(maxsize=None)
def net_taps(cid):
    """the taps {stage: (input, output)} of the end-to-end y16 forward of a walked network: one computation per process"""
    assert CASES[cid]['stage'] is None
    taps = {}
    run(cid, taps, case_input(cid), whole=True)
    return taps


@functools.lru_cache(maxsize=None)
def stage_pair(cid, name):
    """(x_in fp32, y64, y16) of one stage of a case.  A walked network's stage input is the tap of the end-to-end y16 forward cast to
    fp32; both oracles - and the HIP stage - get exactly that."""
    c = CASES[cid]
    x_in = net_taps(cid)[name][0].float() if c['stage'] is None else case_input(cid)
    y64, y16 = run(cid, name, x_in, rounded=False), run(cid, name, x_in)
    assert y64.dtype == y16.dtype == torch.float64
    return x_in, y64, y16


# ------------------------------------------------------------------------------------------------ the launches, as plan() lines
def stage_shapes(cid):
    """[(stage, H, W at its input)] of a case"""
    c = CASES[cid]
    if c['stage'] is not None:
        return [(c['stage'], c['H'], c['W'])]
    out, H, W = [], c['H'], c['W']
    for name in stage_names(cid):
        out.append((name, H, W))
        if name.endswith('_ds'):
            H, W = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    return out


def gemms(cid):
    """[(rows, N)] of every GEMM a case launches (3x3 convs, shortcuts, the transformer's linears)"""
    c, cfg = CASES[cid], case_cfg(cid)
    inner = cfg['n_heads'] * cfg['d_head']
    out = []
    for name, H, W in stage_shapes(cid):
        rows, cin = c['N'] * H * W, stage_width(cfg, name)
        if name == 'conv_in':
            out.append((rows, cfg['ch']))
        elif name.endswith('_ds'):
            out.append((c['N'] * (H // 2) * (W // 2), cin))
        elif name.startswith('down'):
            out.append((rows, cfg['ch'] * cfg['ch_mult'][int(name[4:])]))
        elif name == 'mid_attn_1':
            out += [(rows, n) for n in (inner, 3 * inner, 8 * inner, cin)]
        elif name == 'conv_out':
            out.append((rows, 2 * cfg['z_channels']))
        else:
            out.append((rows, cin))
    return out


def enc_launches(cus=CUS):
    """every attention the cases state, as plan() lines with the statement [(who, route, line)] (launch_line of unet_pixel_refs:
    sequences * heads of the launch, and beside it the GEMM of the case with the most rows among those at least 128 wide)"""
    out = []
    for c in CASES.values():
        if c['attn1'] is None or c['raises']:
            continue
        cfg = case_cfg(c['id'])
        wide = [g for g in gemms(c['id']) if g[1] >= 128]
        rows, nmax = max(wide) if wide else max(gemms(c['id']))
        for tag, (L, route), seqs in (('attn1', c['attn1'], c['objects']), ('attn2', c['attn2'], c['N'])):
            out.append(launch_line(f"{c['id']}/{tag}", cfg['d_head'], L, route, seqs * cfg['n_heads'], rows, nmax, cus))
    return out
