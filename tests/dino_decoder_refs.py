"""Per-token / per-pixel criterion for the two DINOv2-based tri-plane VAE decoder classes, stage by stage (CPU only: torch and the
oracle, no HIP) - the analogue of unet_pixel_refs.py / encoder_pixel_refs.py, whose criterion (dit_token_refs.token_rho) it reuses
unchanged.

A GROUP is the D numbers of one token, or the C numbers at one (object, plane, y, x).  Every stage of oracle.dino_decoder is judged on
its own, on the SAME input for both oracles and the HIP stage:

    y64 = the stage in float64;  y16 = the same under operand_rounding(bf16, kernel_arith=True)
    d = ||y16 - y64||,  e = ||y_hip - y16||,  rho = e / max(d, 0.1 median d)        per group, every group counted

A stage without a bf16 operand has d = 0 exactly (F32_STAGES): it is judged against float64 by the first-order fp32 bounds of
tests/kernel_refs.py instead.  The wiring between the stages is checked exactly (tests/test_dino_decoder_pixels_gpu.py).

Tier A: the two decoders at D = 128, 2 heads, 12 blocks, walked stage by stage at B = 1 (768 token rows: the 128x128 GEMM tile) and
B = 3 (2304 rows: the GEMMs leave that tile); conv_sr resizes 64 -> 128 (input_resolution is read at run time) so that the float64
convolutions stay cheap - the 64 -> 256 tail stays under the golden gates of the existing tests.  The stage inputs are the taps of the
end-to-end y16 forward, cast to fp32.  Tier B: single stages at the smallest shapes that can still go wrong (SINGLES).
Every case states what it launches; tests/test_dino_decoder_pixels_cpu.py holds the statements to csrc/kernel_plan.h and to the
product's dispatch code.  B * 3 * heads stays below the CU count, so the K-resident attention kernel (not restated) never runs."""
import functools

import torch

from dit_token_refs import YARD_MAX, YARD_MEDIAN, to64, token_rho, worst_token      # noqa: F401  (the criterion, not forked)
from unet_pixel_refs import CUS, GEMM_RING_ROWS, plan                                  # noqa: F401
from ln3diff_amd.synth import synth_input, synth_vit_state_dict
from oracle import dino_decoder as odd
from oracle import dit as odit

D, HEADS, DEPTH = 128, 2, 12
R_TIER_A = 128
CM, CO = 128, 32
LATENT = {'shapenet': (12, 32, 32), 'ffhq': (12, 16, 16)}
SHAPENET_CFG = 'shapenet_tuneray_aug_resolution_64_64_nearestSR'


# ------------------------------------------------------------------------------------------------ modules and weights
def build_dec(cls, D_=D, heads=HEADS, conv_sr=None):
    """the product module of a class (a parameter container until it runs), conv_sr optionally replaced by one of (Cm, Co) per plane"""
    from ln3diff_amd.nsr.triplane import Triplane
    if cls == 'shapenet':
        from ln3diff_amd.vit import vit_triplane_shapenet as m
        tp = Triplane(img_resolution=128, rendering_kwargs=m.shapenet_rendering_kwargs(SHAPENET_CFG, 0.6, 1.8), decoder_output_dim=32)
        dec = m.RodinSR_256_fusionv5_ConvQuant_liteSR_dinoInit3DAttn(m.DinoVisionTransformer(D_, DEPTH, heads), tp, False)
        if conv_sr is not None:
            dec.superresolution['conv_sr'] = m.RodinConv3D4X_lite_mlp_as_residual_lite(3 * conv_sr[0], 3 * conv_sr[1])
    else:
        from ln3diff_amd.vit import vit_triplane_ffhq as m
        tp = Triplane(img_resolution=128, rendering_kwargs=m.ffhq_rendering_kwargs('ffhq'), decoder_output_dim=32)
        dec = getattr(m, m.CLASS_NAME)(m.DinoVisionTransformer(D_, DEPTH, heads), tp, False)
        if conv_sr is not None:
            dec.superresolution['conv_sr'] = m.RodinConv3D4X_lite_mlp_as_residual(3 * conv_sr[0], 3 * conv_sr[1])
    return dec


@functools.lru_cache(maxsize=None)
def dec_sd(cls, D_=D, heads=HEADS, conv_sr=None, seed=0):
    """the synthetic fp32 state dict (the goldens' recipe: synth_vit_state_dict, sigma bias + 4); shared, never modified"""
    dec = build_dec(cls, D_, heads, conv_sr)
    sd = synth_vit_state_dict({k: tuple(v.shape) for k, v in dec.state_dict().items()}, seed)
    b = 'triplane_decoder.decoder.net.2.bias'
    sd[b] = sd[b].clone()
    sd[b][0] += 4.0
    return sd


def loaded_dec(cls, conv_sr=None, R=None):
    dec = build_dec(cls, conv_sr=conv_sr)
    dec.load_state_dict(dec_sd(cls, conv_sr=conv_sr), strict=True)
    if R is not None:
        dec.superresolution['conv_sr'].input_resolution = R           # read at run time; set before the first pack
    return dec


# ------------------------------------------------------------------------------------------------ groups and the criterion
def groups(y, kind):
    """kind 'tok': [B, L, D] stays; 'px': NCHW [B, 3C, R, R] -> [B, 3 * R * R, C] (one group per (object, plane, y, x))"""
    y = torch.as_tensor(y).detach()
    if kind == 'tok':
        assert y.dim() == 3
        return y
    cl = odd.to_cl(y)
    return cl.reshape(cl.shape[0], -1, cl.shape[-1])


def group_rho(y_hip, y16, y64, kind):
    """-> (rho, d) [B, 1, groups]; every group is in it"""
    assert y_hip.shape == y16.shape == y64.shape, (y_hip.shape, y16.shape, y64.shape)
    rho, d = token_rho(groups(y_hip, kind), groups(y16, kind), groups(y64, kind), None)
    assert rho.numel() == y16.numel() // groups(y16, kind).shape[-1]
    return rho, d


def group_yardstick(y16, y64, kind):
    g16, g64 = groups(y16, kind).double(), groups(y64, kind).double()
    r = (g16 - g64).norm(dim=-1) / g64.norm(dim=-1)
    return float(r.median()), float(r.max())


def where(rho, kind, R=None):
    """the worst group as (object, token) or (object, plane, y, x) and its rho"""
    (b, _, l), w = worst_token(rho)
    if kind == 'tok' or R is None:
        return (b, l), w
    return (b, l // (R * R), (l // R) % R, l % R), w


def judge(key, y_hip, y16, y64, kind, cap, failures, R=None):
    """the check of a rho stage (the GPU tests and the CPU stand-in tests run this same function) -> worst rho"""
    rho, d = group_rho(torch.as_tensor(y_hip).double().cpu(), y16, y64, kind)
    at, worst = where(rho, kind, R)
    print(f'{key}: worst group {at} rho = {worst:.4g}; median rho {float(rho.median()):.3g}; d median {float(d.median()):.3e}; '
          f'groups {rho.numel()} (cap {cap:g})')
    assert torch.isfinite(rho).all(), key
    if not worst <= cap:
        failures.append((key, at, worst, cap))
    return worst, at


# fp32 stages: (ulps, how the bound's scale is built) - the counts of the kernels' own element tests (tests/test_glue_kernels_gpu.py,
# tests/test_stage_kernels_gpu.py), each derived from the operation:
#   embed (shapenet)  16 fma and the bias of a sequential fp32 sum: K / 2 + 1 = 9 ulps of sum |w x| + |b|
#   embed (ffhq)      [xh | xh | xl] . [wh | wl | wh] with u = 2^-8 the unit roundoff of bf16: the dropped xl . wl term is u^2 |x w|, and
#                     the bf16 roundings of xl and of wl (each u of a low part that is u of its operand) u^2 |x w| each: 3 * 2^-16 = 384
#                     fp32 ulps, and the fp32 accumulation of 12 products and the bias, <= 8: 392 ulps of sum |w x| + |b|
#   pos               one fp32 addition: 1 ulp of |x| + |pos|
#   norm              LayerNorm: 8 ulps of (|x| + |mean|) rstd |w| + |b| (kernel_refs.layernorm), and the term that scale leaves out:
#                     the mean is an fp32 sum of D numbers, whatever its order within (depth) * 2^-24 * sum |x| - two numbers per lane
#                     and a 64-lane wave reduction, depth 7, then the division: 4 ulps of mean|x| rstd |w|.  The token stream has
#                     channels 1000 times smaller than the token's mean |x| (|x| 0.025, |mean| 0.004, mean |x| 8.5), where that
#                     term is all there is; with random normal rows (the kernel's own element test) it never shows.
#   unpatchify        a copy: 0 ulps (and short_cut's bf16 view is bf16_rne of the copied values, compared exactly)
#   x0 / planes (shapenet)   resize + leaky ReLU + add: 6 ulps of the weighted tap magnitudes + |act|   (kernel_refs.resize_add_lrelu)
F32_ULPS = {'embed-shapenet': 9, 'embed-ffhq': 392, 'pos': 1, 'norm': 8, 'unpatchify': 0, 'x0': 6, 'planes': 6}


def f32_check(cls, sd, name, ins, y_hip, what):
    """hold a stage without a bf16 operand to its fp32 bound against float64 (ins: the stage's fp32 inputs) -> worst error / scale"""
    import kernel_refs as kr
    sd = to64(sd)
    i64 = [t.double() for t in ins]
    if name == 'embed':
        if cls == 'shapenet':
            w, b = sd[odd.SR + 'ldm_upsample.proj.weight'], sd[odd.SR + 'ldm_upsample.proj.bias']
            ref, mag = kr.patch_embed_triplane(i64[0], w, b, w.shape[-1], w.shape[0] // 3)
        else:
            w, b = sd[odd.SR + 'ldm_upsample.weight'], sd[odd.SR + 'ldm_upsample.bias']
            tok = odd.ffhq_tokens(i64[0])
            ref, mag = torch.nn.functional.linear(tok, w, b), torch.nn.functional.linear(tok.abs(), w.abs(), b.abs())
        return kr.assert_f32_close(y_hip, ref, mag, F32_ULPS[f'embed-{cls}'], what)
    if name == 'pos':
        pe = sd[odd.VD + 'pos_embed']
        return kr.assert_f32_close(y_hip, i64[0] + pe, i64[0].abs() + pe.abs(), F32_ULPS['pos'], what)
    if name == 'norm':
        v = i64[0].reshape(-1, i64[0].shape[-1])
        ref, mag = kr.layernorm(v, sd[odd.VD + 'norm.weight'], sd[odd.VD + 'norm.bias'], 1e-6)
        rstd = (v.var(-1, unbiased=False, keepdim=True) + 1e-6).rsqrt()
        mag = mag + 0.5 * v.abs().mean(-1, keepdim=True) * rstd * sd[odd.VD + 'norm.weight'].abs()      # 4 of the 8 ulps: the mean's own sum
        return kr.assert_f32_close(y_hip, ref, mag, F32_ULPS['norm'], what)
    if name == 'unpatchify':
        ref = odd.unpatchify_triplane(i64[0])
        return kr.assert_f32_close(y_hip, ref, ref.abs(), 0, what)
    if name in ('x0', 'planes') and cls == 'shapenet':
        base, t = (odd.to_cl(v) for v in i64)                                  # [B, 3, h, h, C]
        R = t.shape[2]
        ref, mag = kr.resize_add_lrelu(base.reshape(-1, *base.shape[2:]), t.reshape(-1, *t.shape[2:]), R, R, odd.SLOPE)
        return kr.assert_f32_close(odd.to_cl(torch.as_tensor(y_hip)).reshape(ref.shape), ref, mag, F32_ULPS[name], what)
    raise KeyError((cls, name))


# ------------------------------------------------------------------------------------------------ stages
def stage_names(cls):
    vit = ['embed', 'pos']
    for j in range(DEPTH // 2):
        vit += ([f'skip{j}'] if j >= DEPTH // 4 else []) + [f'group{j}']
    tail = ['conv0', 'x0', 'conv1', 'planes'] if cls == 'shapenet' else ['x0', 'planes']
    return vit + ['norm', 'decoder_pred', 'unpatchify', 'short_cut', 'upsample'] + tail


def stage_kind(name):
    return 'px' if name in ('unpatchify', 'short_cut', 'upsample', 'conv0', 'x0', 'conv1', 'planes') else 'tok'


def f32_stages(cls):
    """the stages without a bf16 operand (oracle d exactly 0): judged by fp32 bounds"""
    return ['embed', 'pos', 'norm', 'unpatchify'] + (['x0', 'planes'] if cls == 'shapenet' else [])


def run_stage(sd, cls, name, ins, R=R_TIER_A, rounded=True):
    """one stage of oracle.dino_decoder on `ins` in their dtype (the state dict is cast to it)"""
    dt = ins[0].dtype
    sd = {k: v.to(dt) if v.is_floating_point() else v for k, v in sd.items()}

    def run():
        if name == 'embed':
            return odd.embed(sd, cls, ins[0])
        if name == 'pos':
            return odd.add_pos(sd, ins[0])
        if name.startswith('skip'):
            return odd.skip_step(sd, cls, int(name[4:]), ins[0], ins[1])
        if name.startswith('group'):
            return odd.group(sd, cls, int(name[5:]), ins[0], HEADS)
        if name == 'norm':
            return odd.final_norm(sd, ins[0])
        if name == 'decoder_pred':
            return odd.decoder_pred(sd, ins[0])
        if name == 'unpatchify':
            return odd.unpatchify_triplane(ins[0])
        if name == 'short_cut':
            return odd.short_cut(sd, ins[0])
        if name == 'upsample':
            return odd.upsample_t(ins[0], R)
        if name == 'conv0':
            return odd.conv0(sd, cls, ins[0])
        if name == 'conv1':
            return odd.conv1(sd, ins[0])
        if name == 'x0':
            return odd.resize_add_lrelu(ins[0], ins[1]) if cls == 'shapenet' else odd.conv_x0(sd, cls, ins[0], ins[1])
        if name == 'planes':
            return odd.resize_add_lrelu(ins[0], ins[1]) if cls == 'shapenet' else odd.conv_planes(sd, ins[0])
        if name == 'cross':                                  # tier B: the nested cross-plane block / the fusion block of group 0
            p = f'{odd.VD}blocks.0.'
            return odd.cross_block(sd, p + 'vit_blks.1.', ins[0], HEADS) if cls == 'shapenet' else odd.fusion(sd, p + 'fusion.', ins[0], HEADS)
        raise KeyError(name)
    with torch.no_grad():
        if not rounded:
            return run()
        with odit.operand_rounding(torch.bfloat16, kernel_arith=True):
            return run()


def stage_inputs(cls, taps, name):
    """the inputs of a stage among the taps of oracle.dino_decoder.decode (the FFHQ class's fused tail takes two oracle steps each)"""
    if cls == 'ffhq' and name == 'x0':
        return (taps['conv0'][0][0], taps['short_cut'][1])
    if cls == 'ffhq' and name == 'planes':
        return (taps['x0'][1],)
    return taps[name][0]


# ------------------------------------------------------------------------------------------------ tier A
TIER_A = {f'{cls}-b{B}': dict(cls=cls, B=B, rows=B * 768, ring_gemm=B * 768 >= GEMM_RING_ROWS,
                              attn=('stream', 64, 256, B * 3 * HEADS), conv='im2col+gemm' if cls == 'shapenet' else 'fused')
          for cls in odd.CLASSES for B in (1, 3)}


def latent(cid):
    c = TIER_A[cid]
    return synth_input(f"{c['cls']}_pixels_latent", (c['B'], *LATENT[c['cls']]), 61 + c['B'])


def rounded_decode(cid, sd=None, taps=None, dtype=torch.float64):
    """the end-to-end y16 of a tier A case, computed afresh (the seeded-defect tests call it with oracle functions replaced)"""
    c = TIER_A[cid]
    sd = dec_sd(c['cls']) if sd is None else sd
    sd = {k: v.to(dtype) for k, v in sd.items()}
    with torch.no_grad(), odit.operand_rounding(torch.bfloat16, kernel_arith=True):
        return odd.decode(sd, c['cls'], latent(cid).to(dtype), HEADS, R_TIER_A, taps)


@functools.lru_cache(maxsize=None)
def case_taps(cid):
    taps = {}
    rounded_decode(cid, taps=taps)
    return taps


@functools.lru_cache(maxsize=None)
def stage_pair(cid, name):
    """(inputs fp32, y64, y16) of one stage of a tier A case: both oracles - and the HIP stage - get exactly these inputs"""
    c = TIER_A[cid]
    ins = tuple(t.float().contiguous() for t in stage_inputs(c['cls'], case_taps(cid), name))     # taps may carry permuted strides
    i64 = tuple(t.double() for t in ins)
    y64 = run_stage(dec_sd(c['cls']), c['cls'], name, i64, rounded=False)
    y16 = run_stage(dec_sd(c['cls']), c['cls'], name, i64)
    assert y64.dtype == y16.dtype == torch.float64
    return ins, y64, y16


# ------------------------------------------------------------------------------------------------ tier B
def _scaled_planes(name, B, seed, scales=(1.0, 4.0, 0.25)):
    """tokens [B, 768, D] whose three planes have clearly different scales (a plane permutation changes every score's size)"""
    x = synth_input(name, (B, 3, 256, D), seed)
    return (x * torch.tensor(scales).view(1, 3, 1, 1)).reshape(B, 768, D)


def _conv_case(cls, r, R, Cm, Co, B):
    narrow = (Cm, Co) != (CM, CO)
    return dict(kind='conv', cls=cls, r=r, R=R, Cm=Cm, Co=Co, B=B, conv_sr=(Cm, Co) if narrow else None,
                conv='im2col+gemm' if cls == 'shapenet' else 'fused', refused=cls == 'ffhq' and Co % 32 != 0,
                rows=R * R, ring_gemm=False)


def _singles():
    cs = {}
    for cls in odd.CLASSES:
        for B in (1, 2):
            cs[f'{cls}-cross-b{B}'] = dict(kind='cross', cls=cls, B=B, rows=B * 768, ring_gemm=B * 768 >= GEMM_RING_ROWS)
        cs[f'{cls}-skip'] = dict(kind='skip', cls=cls, B=1, j=3, rows=768, ring_gemm=False)
        for r, R in ((8, 32), (16, 64)):
            for B in (1, 2):
                cs[f'{cls}-conv-r{r}-b{B}'] = _conv_case(cls, r, R, CM, CO, B)
        cs[f'{cls}-conv-narrow'] = _conv_case(cls, 8, 32, 16, 8, 2)
    cs['ffhq-embed-lowhalf'] = dict(kind='embed', cls='ffhq', B=2, rows=2 * 768, ring_gemm=True)
    return cs


SINGLES = _singles()


def single_inputs(sid):
    c = SINGLES[sid]
    seed = 71 + sorted(SINGLES).index(sid)
    if c['kind'] == 'cross':
        return (_scaled_planes('cross_x', c['B'], seed),)
    if c['kind'] == 'skip':
        return (synth_input('skip_x', (1, 768, D), seed), synth_input('skip_s', (1, 768, D), seed).to(torch.bfloat16).float())
    if c['kind'] == 'conv':
        B, r, R, Cm, Co = c['B'], c['r'], c['R'], c['Cm'], c['Co']
        return (synth_input('conv_up', (B, 3 * Cm, R, R), seed).to(torch.bfloat16).float(), synth_input('conv_res', (B, 3 * Co, r, r), seed))
    if c['kind'] == 'embed':                              # magnitudes spread over 2^-6 .. 2^6: every entry needs its low half
        mag = 2.0 ** (synth_input('embed_e', (c['B'], *LATENT['ffhq']), seed).clamp(-1.5, 1.5) * 4.0)
        return (synth_input('embed_s', (c['B'], *LATENT['ffhq']), seed).sign() * mag * (1 + synth_input('embed_m', (c['B'], *LATENT['ffhq']), seed).abs()),)
    raise KeyError(sid)


def single_stages(sid):
    """the oracle stages a single case is judged at, in the order the product runs them"""
    c = SINGLES[sid]
    if c['kind'] == 'conv':
        return (['conv0', 'x0', 'conv1', 'planes'] if c['cls'] == 'shapenet' else ['x0', 'planes'])
    return [{'cross': 'cross', 'skip': f"skip{c.get('j')}", 'embed': 'embed'}[c['kind']]]


def single_sd(sid):
    c = SINGLES[sid]
    return dec_sd(c['cls'], conv_sr=c.get('conv_sr'))


def single_pair(sid, name, ins):
    """(y64, y16) of one stage of a single case on fp32 inputs"""
    c = SINGLES[sid]
    i64 = tuple(t.double() for t in ins)
    R = c.get('R', R_TIER_A)
    return run_stage(single_sd(sid), c['cls'], name, i64, R, rounded=False), run_stage(single_sd(sid), c['cls'], name, i64, R)


# ------------------------------------------------------------------------------------------------ the ShapeNet encoder side
def reparam_inputs():
    """(encoder tokens [2, 256, 384], fp16-exact as tests/golden/shapenet_reparam_b2.npz stores them; eps [2, 4, 3, 1024])"""
    return synth_input('shapenet_enc_tokens', (2, 256, 384), 91).half().float(), synth_input('shapenet_eps', (2, 4, 3, 1024), 92)


def reparam_tokens(h):
    """the posterior's input h [B, 24, 32, 32] regrouped into the rows ldm_downsample wrote: [B, 256, 96] (one group per encoder token)"""
    B = h.shape[0]
    v = h.reshape(B, 3, 8, 16, 2, 16, 2)                                    # b d c h p w q
    return v.permute(0, 3, 5, 4, 6, 1, 2).reshape(B, 256, 96)


def reparam_pair(eps=None):
    """(y64, y16): dicts of oracle.dino_decoder.vae_reparameterization"""
    tok, _ = reparam_inputs()
    sd = to64(dec_sd('shapenet'))
    with torch.no_grad():
        y64 = odd.vae_reparameterization(sd, tok.double(), eps)
        with odit.operand_rounding(torch.bfloat16, kernel_arith=True):
            y16 = odd.vae_reparameterization(sd, tok.double(), eps)
    return y64, y16


# ------------------------------------------------------------------------------------------------ launches
def launch_lines(cus=CUS):
    """every per-plane attention and the widest / narrowest GEMM rows the cases state, as unet_pixel_refs.plan() lines:
    (Dp, dh_true, L, B * heads, M, N, K, cus) -> [(who, stated attention route, stated 'left the 128x128 tile', line)]"""
    out = []
    for cid, c in TIER_A.items():
        out.append((cid, c['attn'][0], c['ring_gemm'], (64, 0, 256, c['attn'][3], c['rows'], D, D, cus)))
    for sid, c in SINGLES.items():
        if c['kind'] in ('cross', 'skip', 'embed'):
            out.append((sid, None, c['ring_gemm'], (64, 0, 256, 6, c['rows'], D, D, cus)))
    return out
