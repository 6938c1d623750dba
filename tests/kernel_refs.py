"""Float64 restatements of the glue kernels of include/ln3d.h and of the stage headers (ln3d_shapenet.h, ln3d_encoder.h, ln3d_ffhq.h)
and per-element bounds for their outputs.

Every reference is computed in double from the same fp32 / bf16 inputs the kernel received, from the operation's definition (the
reference source lines each kernel's comment cites) or torch.nn.functional in double.  Besides the value, the fp32-sensitive
references return a `scale` per element: the magnitude of the terms the kernel summed (first-order error propagation), so that a
result which cancels to near zero is judged against the rounding of its terms, not against its own tiny size.

Bounds (tests/test_kernel_refs_cpu.py shows that they can fail):
  assert_bf16_close: |y - ref| <= max(1 bf16 ulp of ref, floor_ulps fp32 ulps of scale) for every element, and the fraction of
                     elements with y != bf16_rne(ref) at most max_mismatch (a correct fp32 kernel flips only near rounding ties);
  assert_f32_close:  |y - ref| <= ulps * 2^-23 * scale for every element.

The bf16 GEMM and the fused attention (last section) are held per element too.  fp32 GEMM outputs: c = GEMM_F32_ULPS = 5.74 fp32 ulps of
scale = sum_k |x w| + |b|, 4 x the worst (1.434) that a sequential and a 16-grouped fp32 restatement of the sum reach on the tests' own
inputs, never above K; bf16 outputs: assert_bf16_close with floor_ulps = c, at most 1 % of elements off bf16_rne(ref), the erf-GELU
polynomial's documented 1.5e-4 added; nothing is added for the __expf / tanhf epilogues (their fp32 formulas stay within 2^-10 of a bf16
ulp of the float64 value, tests/test_gemm_attn_refs_cpu.py).  Attention outputs: 2^-8 * sum_j p_j |v_j| + 1 bf16 ulp (attention_bound).
"""
import math

import torch
import torch.nn.functional as F

F32_EPS = 2.0 ** -23            # fp32 ulp of 1
BF16_MAX = (2.0 - 2.0 ** -7) * 2.0 ** 127


# ---------------------------------------------------------------- bf16 rounding in double
def bf16_ulp(ref):
    """Spacing of bf16 at |ref| (subnormal spacing 2^-133 below the smallest normal)."""
    a = ref.double().abs()
    _, e = torch.frexp(a)                                  # a = m * 2^e, m in [0.5, 1)
    e = torch.where(a > 0, e - 1, torch.full_like(e, -126)).clamp(min=-126)
    return torch.ldexp(torch.ones_like(a), e - 7)


def bf16_rne(ref):
    """ref (double) rounded once, to nearest even, to a bf16 value (returned in double).  Rounding through fp32 first would round
    twice."""
    ref = ref.double()
    u = bf16_ulp(ref)
    r = torch.round(ref / u) * u                           # torch.round: half to even; ref / u is exact
    return torch.where(r.abs() > BF16_MAX, torch.copysign(torch.full_like(r, math.inf), r), r)


def _where(mask):
    return int(mask.reshape(-1).nonzero()[0])


def assert_bf16_close(y, ref, scale=None, floor_ulps=4.0, max_mismatch=0.01, what="", flips_over=None):
    """bf16 output y against the float64 reference.  flips_over: boolean mask of the elements over which the mismatch fraction is
    taken (default all) - rows or groups far off zero mean are held to the per-element bound only, since there the fp32 rounding of
    the mean alone (|mean| * 2^-24) moves a good share of the outputs across a rounding boundary.
    Returns (worst error in bf16 ulps of ref, mismatch fraction)."""
    y = y.detach().double().cpu().reshape(-1)
    ref = ref.detach().double().cpu().reshape(-1)
    assert y.numel() == ref.numel(), (what, y.numel(), ref.numel())
    ulp = bf16_ulp(ref)
    tol = ulp
    if scale is not None:
        s = torch.as_tensor(scale, dtype=torch.float64).cpu().reshape(-1).expand_as(ref)
        tol = torch.maximum(ulp, floor_ulps * F32_EPS * s)
    err = (y - ref).abs()
    err = torch.where(y == ref, torch.zeros_like(err), err)                        # equal infinities
    worst_ulp = float((err / ulp).max())
    worst_tol = float((err / tol).max())
    flips = y != bf16_rne(ref)
    mism = float(flips.double().mean() if flips_over is None else flips[flips_over.cpu().reshape(-1)].double().mean())
    print(f"[kref] {what}: bf16 worst {worst_ulp:.3g} ulp ({worst_tol:.3g} of the bound), mismatch {mism:.3g}")
    bad = ~(err <= tol)
    if bad.any():
        i = _where(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} / {y.numel()} elements beyond the bound; first at flat index {i}: "
                             f"y {float(y[i])!r} ref {float(ref[i])!r} bound {float(tol[i]):.3g} ({float(err[i] / ulp[i]):.3g} bf16 ulp); "
                             f"worst {worst_ulp:.3g} ulp, mismatch fraction {mism:.3g}")
    assert mism <= max_mismatch, f"{what}: mismatch fraction {mism:.4g} > {max_mismatch} (worst {worst_ulp:.3g} ulp)"
    return worst_ulp, mism


def assert_f32_close(y, ref, scale, ulps, what=""):
    """fp32 output y: |y - ref| <= ulps * 2^-23 * scale per element.  Returns the worst |y - ref| / scale."""
    y = y.detach().double().cpu().reshape(-1)
    ref = ref.detach().double().cpu().reshape(-1)
    assert y.numel() == ref.numel(), (what, y.numel(), ref.numel())
    s = torch.as_tensor(scale, dtype=torch.float64).cpu().reshape(-1).expand_as(ref)
    err = (y - ref).abs()
    rel = err / s.clamp(min=1e-300)
    worst = float(rel.max())
    print(f"[kref] {what}: f32 worst {worst / F32_EPS:.3g} ulp of the terms (rel {worst:.3g})")
    bad = ~(err <= ulps * F32_EPS * s)
    if bad.any():
        i = _where(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} / {y.numel()} elements beyond {ulps} fp32 ulps of the terms; first at {i}: "
                             f"y {float(y[i])!r} ref {float(ref[i])!r} scale {float(s[i]):.3g}; worst {worst / F32_EPS:.3g} ulps")
    return worst


def _d(t):
    return None if t is None else t.detach().double().cpu()


def silu64(t):
    return t * torch.sigmoid(t)


# ---------------------------------------------------------------- normalisations
def groupnorm(x, w, b, groups, eps, swish, add_row=None, mod_scale=None, mod_shift=None):
    """x f32 [N, HW, C] -> (ref, scale) [N, HW, C]: act(GN(x + add_row[n]) * w + b [* (1 + mod_scale[n]) + mod_shift[n]])
    (ldm model.py:45-51 Normalize + nonlinearity; guided_diffusion/unet.py:267-273 for add_row / mod)."""
    v = _d(x)
    N, HW, C = v.shape
    if add_row is not None:
        v = v + _d(add_row)[:, None, :]
    w64, b64 = _d(w), _d(b)
    vg = v.reshape(N, HW, groups, C // groups)
    mean = vg.mean(dim=(1, 3), keepdim=True)
    rstd = (((vg - mean) ** 2).mean(dim=(1, 3), keepdim=True) + eps).rsqrt()        # biased variance, as torch.nn.GroupNorm
    t = ((vg - mean) * rstd).reshape(N, HW, C) * w64 + b64                         # (F.group_norm refuses one-element groups)
    scale = ((vg.abs() + mean.abs()) * rstd).reshape(N, HW, C) * w64.abs() + b64.abs()
    if mod_scale is not None:
        ms, mh = _d(mod_scale)[:, None, :], _d(mod_shift)[:, None, :]
        t = t * (1 + ms) + mh
        scale = scale * (1 + ms).abs() + mh.abs()
    if swish:
        t = silu64(t)
    return t, scale


def layernorm(x, w, b, eps):
    """x f32 [rows, D] -> (ref, scale): F.layer_norm in double (CLIP final_layer_norm / open_clip ln_post)."""
    v = _d(x)
    D = v.shape[-1]
    w64 = _d(w) if w is not None else torch.ones(D, dtype=torch.float64)
    b64 = _d(b) if b is not None else torch.zeros(D, dtype=torch.float64)
    t = F.layer_norm(v, (D,), w64, b64, eps)
    mean = v.mean(-1, keepdim=True)
    rstd = (v.var(-1, unbiased=False, keepdim=True) + eps).rsqrt()
    return t, (v.abs() + mean.abs()) * rstd * w64.abs() + b64.abs()


def norm_modulate(x, kind, eps, weight=None, shift=None, scale=None, mod_rows=1, shift_table=None, scale_table=None):
    """x f32 [rows, D] -> (ref, scale) [rows, D] in INPUT row order: LayerNorm (kind 0, no affine) or RMSNorm (kind 1), times weight,
    then * (1 + scale[r / mod_rows] + scale_table) + shift[..] + shift_table  (dit_models_xformers.py:48,52,249-258; dit/norm.py:27-40).
    shift / scale: [rows / mod_rows, D] (already gathered from their leading dimension)."""
    v = _d(x)
    D = v.shape[-1]
    if kind == 0:
        t = F.layer_norm(v, (D,), None, None, eps)
        mean = v.mean(-1, keepdim=True)
        rstd = (v.var(-1, unbiased=False, keepdim=True) + eps).rsqrt()
        mag = (v.abs() + mean.abs()) * rstd
    else:
        rstd = ((v * v).mean(-1, keepdim=True) + eps).rsqrt()
        t = v * rstd
        mag = t.abs()
    if weight is not None:
        t, mag = t * _d(weight), mag * _d(weight).abs()
    if scale is not None:
        sc = _d(scale).repeat_interleave(mod_rows, 0)[:v.shape[0]]
        sh = _d(shift).repeat_interleave(mod_rows, 0)[:v.shape[0]]
        if scale_table is not None:
            sc, sh = sc + _d(scale_table), sh + _d(shift_table)
        t = t * (1 + sc) + sh
        mag = mag * (1 + sc).abs() + sh.abs()
    return t, mag


# ---------------------------------------------------------------- sampler and ODE steps (value, magnitude of the terms)
def ddpm_step(x, eps, noise, a, b, c1, c2, sig, clip):
    """GaussianDiffusion.p_sample, EPSILON (gaussian_diffusion.py:252-271,422-427,535-545)."""
    x, eps, noise = _d(x), _d(eps), _d(noise)
    x0 = a * x - b * eps
    m0 = (a * x).abs() + (b * eps).abs()
    if clip:
        x0 = x0.clamp(-1, 1)
    out = c1 * x0 + c2 * x + sig * noise
    return out, abs(c1) * m0 + (c2 * x).abs() + (sig * noise).abs()


def ddim_step(x, eu, ec, noise, s, a, b, sqrt_ab_prev, coef_eps, sigma, clip):
    """GaussianDiffusion.ddim_sample (gaussian_diffusion.py:729-866): with clip_denoised, p_mean_variance clips pred_xstart of EACH
    model output and _predict_eps_from_xstart re-derives eps = (a*x - x0) / b from it; CFG combines the two eps."""
    x, eu, ec, noise = _d(x), _d(eu), _d(ec), _d(noise)

    def branch(e):
        if not clip:
            return e, e.abs()
        x0 = (a * x - b * e).clamp(-1, 1)
        mag_x0 = (a * x).abs() + (b * e).abs()
        return (a * x - x0) / b, ((a * x).abs() + mag_x0) / abs(b)
    e_u, m_u = branch(eu)
    if ec is not None:
        e_c, m_c = branch(ec)
        eps, m_eps = e_u + s * (e_c - e_u), m_u + abs(s) * (m_c + m_u)
    else:
        eps, m_eps = e_u, m_u
    x0 = a * x - b * eps
    m_x0 = (a * x).abs() + abs(b) * m_eps
    out = x0 * sqrt_ab_prev + coef_eps * eps
    mag = m_x0 * abs(sqrt_ab_prev) + abs(coef_eps) * m_eps
    if noise is not None:
        out, mag = out + sigma * noise, mag + (sigma * noise).abs()
    return out, mag


def edm_euler_step(x, eps2, sigma, sigma_next, s):
    """EulerEDMSampler step + VanillaCFG on the eps model (sgm sampling.py:93-104, guiders.py:29-42, denoiser.py:36-41)."""
    x, eps2 = _d(x), _d(eps2)
    n = x.numel()
    eu, ec = eps2[:n].view_as(x), eps2[n:].view_as(x)
    du, dc = x - sigma * eu, x - sigma * ec
    mu, mc = x.abs() + (sigma * eu).abs(), x.abs() + (sigma * ec).abs()
    den = du + s * (dc - du)
    m_den = mu + abs(s) * (mc + mu)
    d = (x - den) / sigma
    m_d = (x.abs() + m_den) / abs(sigma)
    return x + d * (sigma_next - sigma), x.abs() + m_d * abs(sigma_next - sigma)


def flow_euler_step(x2, v2, dt, s):
    """transport/integrators.py:101-120 with forward_with_cfg (dit/dit_i23d.py:155-168): v2 = [cond ; uncond]."""
    x2, v2 = _d(x2), _d(v2)
    n = x2.numel() // 2
    vc, vu = v2[:n], v2[n:]
    v = vu + s * (vc - vu)
    mv = vu.abs() + abs(s) * (vc.abs() + vu.abs())
    return torch.cat([x2[:n] + dt * v, x2[n:] + dt * v]), torch.cat([x2[:n].abs() + abs(dt) * mv, x2[n:].abs() + abs(dt) * mv])


def cfg_combine_dup(v2, s):
    v2 = _d(v2)
    n = v2.numel() // 2
    vc, vu = v2[:n], v2[n:]
    h, m = vu + s * (vc - vu), vu.abs() + abs(s) * (vc.abs() + vu.abs())
    return torch.cat([h, h]), torch.cat([m, m])


def axpby(x, y, a, b):
    x, y = _d(x), _d(y)
    return a * x + b * y, (a * x).abs() + (b * y).abs()


def lincomb(y, ks, cs, n):
    """out = y + sum_j cs[j] * ks[j] (y None = 0)"""
    out = _d(y) if y is not None else torch.zeros(n, dtype=torch.float64)
    mag = out.abs()
    for k, c in zip(ks, cs):
        out, mag = out + c * _d(k), mag + (c * _d(k)).abs()
    return out, mag


def err_ratio_sq(err, y0, y1, atol, rtol):
    """sum((err / (atol + rtol * max(|y0|, |y1|)))^2) (torchdiffeq's _rms_norm of the error ratio, before the mean and sqrt)."""
    err, y0 = _d(err), _d(y0)
    m = y0.abs() if y1 is None else torch.maximum(y0.abs(), _d(y1).abs())
    return float(((err / (atol + rtol * m)) ** 2).sum())


# ---------------------------------------------------------------- embeddings
def timestep_embedding(t, dim):
    """TimestepEmbedder.timestep_embedding (dit_models_xformers.py:101-122) in double: [cos | sin](t * exp(-ln(1e4) k / half)).
    Returns (ref, |argument|)."""
    half = dim // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
    args = _d(t)[:, None] * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], -1), torch.cat([args.abs(), args.abs()], -1)


def patch_embed_triplane(latent, w, bias, p, D):
    """PatchEmbedTriplane (vit/vit_triplane.py:82-106): Conv2d(groups=3, kernel = stride = p), then the literal regroup
    x.reshape(B, C // 3, 3, H, W).flatten(2).transpose(1, 2) -> (raw [B, 3L, D], sum of |terms|)."""
    lat, w64, b64 = _d(latent), _d(w), _d(bias)
    B = lat.shape[0]

    def regroup(y):
        return y.reshape(B, y.shape[1] // 3, 3, y.shape[-2], y.shape[-1]).flatten(2).transpose(1, 2)
    raw = regroup(F.conv2d(lat, w64, b64, stride=p, groups=3))
    mag = regroup(F.conv2d(lat.abs(), w64.abs(), b64.abs(), stride=p, groups=3))
    return raw, mag


# ================================================================ stage kernels (U-Net, VAE decoders, encoder, DiT boundary)
def _f32(v):
    """the fp32 value of a Python scalar argument, as the kernel receives it"""
    return float(torch.tensor(v, dtype=torch.float32))


# ---------------------------------------------------------------- softmax attention
def attention_floor(score_mag, n_dot, Nk):
    """Per-row floor of the attention bound, in fp32 ulps (2^-23) of sum_j p_j |v_j|.
    A score is a sequential fp32 sum whose n_dot roundings (one per fma, or a product and an add rounding per term where the products
    are not exact, and one for the multiplication by the softmax scale) each cost at most 2^-24 of the summed magnitudes:
    |ds_j| <= n_dot * 2^-24 * score_mag, score_mag = |scale| * max_j sum_d |q_d k_jd|.  An absolute score error is a relative error
    of exp(s_j - max); it reaches the output through the numerator and through the normaliser: 2 * max_j |ds_j| relative to
    sum p |v|.  The rest, in units of 2^-24: Nk for the sequential value sum; Nk / 64 + 6 for the normaliser (strided partial sums
    and a 6-level butterfly); 4 ln(Nk) for the exp argument (s - max and its product with log2(e) are each rounded, an absolute
    2^-24 |s_j - max| per rounding on a term of weight p_j, and sum_j p_j |s_j - max| <= ln Nk; numerator and normaliser); 12 for the
    exp itself, the reciprocal or division and the final product (2 ulps each at most).  In ulps (two units each):
      floor = n_dot * score_mag + (Nk + Nk / 64 + 4 ln(max(Nk, 2)) + 18) / 2"""
    return n_dot * score_mag + (Nk + Nk / 64.0 + 4.0 * math.log(max(Nk, 2)) + 18.0) / 2.0


def attention_small(q, k, v, scale):
    """q [B, Nq, H, Dh], k / v [B, Nk, H, Dh] bf16 (views) -> (ref [B, Nq, H, Dh], sum_j p_j |v_j| of the same shape, floor
    [B, Nq, H, 1] in fp32 ulps of that sum: attention_floor with n_dot = Dh + 1, the bf16 x bf16 products being exact in fp32).
    CrossAttention (attention_compat.py:161-202) / QKVAttentionLegacy (unet.py:359-389): softmax(scale * q k^T) v."""
    q, k, v = _d(q), _d(k), _d(v)
    sc = _f32(scale)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * sc
    smag = torch.einsum("bqhd,bkhd->bhqk", q.abs(), k.abs()).amax(-1) * abs(sc)               # [B, H, Nq]
    p = torch.softmax(s, -1)
    out = torch.einsum("bhqk,bkhd->bqhd", p, v)
    mag = torch.einsum("bhqk,bkhd->bqhd", p, v.abs())
    floor = attention_floor(smag, q.shape[-1] + 1, k.shape[1]).permute(0, 2, 1)[..., None]
    return out, mag, floor


def triplane_axis_attention(qkv, B, p, H, scale):
    """qkv f32 [B*3*p*p, >= 3*H*64] -> (ref [rows, H*64], sum p |v|, floor [rows, H*64]).  Conv3DCrossAttentionBlockXformerMHANested:
    the query of plane i at (y, x) attends to tokens (y, j) of plane (i+1) % 3 and tokens (j, x) of plane (i+2) % 3, j < p, in
    one softmax over the 2p keys.  floor: attention_floor with n_dot = 2 * 64 + 1 (fp32 x fp32 products are rounded, so a term costs
    a product and an add rounding where the compiler does not contract them into an fma)."""
    D = H * 64
    t = _d(qkv)
    sc = _f32(scale)
    q, k, v = (t[:, i * D:(i + 1) * D].reshape(B, 3, p, p, H, 64) for i in range(3))
    nxt = [1, 2, 0]
    prv = [2, 0, 1]
    k1, v1, k2, v2 = k[:, nxt], v[:, nxt], k[:, prv], v[:, prv]

    def scores(qq, ka, kb):
        return torch.cat([torch.einsum("biyxhd,biyjhd->biyxhj", qq, ka), torch.einsum("biyxhd,bijxhd->biyxhj", qq, kb)], -1)
    s = scores(q, k1, k2) * sc
    smag = scores(q.abs(), k1.abs(), k2.abs()).amax(-1) * abs(sc)
    pr = torch.softmax(s, -1)

    def av(va, vb):
        return torch.einsum("biyxhj,biyjhd->biyxhd", pr[..., :p], va) + torch.einsum("biyxhj,bijxhd->biyxhd", pr[..., p:], vb)
    out, mag = av(v1, v2), av(v1.abs(), v2.abs())
    floor = attention_floor(smag, 2 * 64 + 1, 2 * p)[..., None].expand_as(out)
    rows = B * 3 * p * p
    return out.reshape(rows, D), mag.reshape(rows, D), floor.reshape(rows, D)


# ---------------------------------------------------------------- GEGLU, mixed prediction
def geglu(x, inner):
    """x f32 [rows, 2 * inner] = [a | gate] -> (a * gelu(gate), scale) with the exact erf GELU (attention_compat.py:45-53).
    gelu(g) = 0.5 g (1 + erf(g / sqrt 2)): its terms are 1 and |erf|, which cancel for g << 0, so
    scale = |a| * 0.5 |g| * (1 + |erf(g / sqrt 2)|)."""
    v = _d(x)
    a, g = v[:, :inner], v[:, inner:]
    e = torch.erf(g / math.sqrt(2.0))
    return a * 0.5 * g * (1 + e), a.abs() * 0.5 * g.abs() * (1 + e.abs())


def mix_prediction(eps, x, logit, sqrt_one_minus_ab):
    """eps, x f32 [N, C, HW], logit f32 [C] -> (ref, scale): (1 - s_c) * sqrt(1 - ab) * x + s_c * eps, s = sigmoid(logit)
    (continuous_diffusion_utils.py:748-754).  1 - s has the terms 1 and s; the fp32 sigmoid carries a relative error of about
    (|logit| / 2 + 3) ulps (the exp argument's rounding is an absolute error of the exponent), which the s-dependent terms are
    weighted with: scale = |c x| + s (|c x| + |eps|) (1 + |logit| / 8), to be used with 8 ulps."""
    e, xx, lg = _d(eps), _d(x), _d(logit)[None, :, None]
    c = _f32(sqrt_one_minus_ab)
    s = torch.sigmoid(lg)
    return (1 - s) * (c * xx) + s * e, (c * xx).abs() + s * ((c * xx).abs() + e.abs()) * (1 + lg.abs() / 8)


# ---------------------------------------------------------------- bilinear resize
def bilinear_taps(n_in, n_out):
    """(i0, i1, l1, src) of every output index along one axis, computed in fp32 as ATen's upsample_bilinear2d does with
    align_corners=False: scale = in / out, src = max(scale * (o + 0.5) - 0.5, 0), i0 = min(int(src), in - 1), i1 = min(i0 + 1, in - 1),
    l1 = src - i0.  The taps are part of the operation's definition: for a non-dyadic ratio a float64 source index differs from this
    by about src * 2^-24, far over a few ulps of the result."""
    scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    o = torch.arange(n_out, dtype=torch.float32)
    src = (scale * (o + 0.5) - 0.5).clamp(min=0)
    i0 = src.to(torch.int64).clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    l1 = src - i0.to(torch.float32)
    return i0, i1, l1.double(), src.double()


def resize_bilinear(x, Ho, Wo):
    """x f32 [N, h, w, C] channel-last -> (ref [N, Ho, Wo, C], scale): the four fp32 taps of bilinear_taps blended in float64.
    scale = the four weighted magnitudes + (src_y + src_x) * amax / 4, amax the largest |x| within two pixels of the first tap: a
    kernel that contracts scale * (o + 0.5) - 0.5 into one fma rounds src once where ATen rounds twice, an absolute 2^-24 src on
    l1 (and, where src sits on an integer, the neighbouring cell); with the 4 ulps of the blend this term admits 1 ulp of src."""
    v = _d(x)
    N, h, w, C = v.shape
    y0, y1, ly, sy = bilinear_taps(h, Ho)
    x0, x1, lx, sx = bilinear_taps(w, Wo)
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]

    def tap(t, yi, xi):
        return t[:, yi][:, :, xi]
    ref = (1 - ly) * ((1 - lx) * tap(v, y0, x0) + lx * tap(v, y0, x1)) + ly * ((1 - lx) * tap(v, y1, x0) + lx * tap(v, y1, x1))
    a = v.abs()
    mag = (1 - ly) * ((1 - lx) * tap(a, y0, x0) + lx * tap(a, y0, x1)) + ly * ((1 - lx) * tap(a, y1, x0) + lx * tap(a, y1, x1))
    amax = F.max_pool2d(a.permute(0, 3, 1, 2), 5, 1, 2).permute(0, 2, 3, 1)
    slack = (sy[None, :, None, None] + sx[None, None, :, None]) * tap(amax, y0, x0) / 4
    return ref, mag + slack


def resize_add_lrelu(base, t, Ho, Wo, slope):
    """(resize(base) + leaky_relu(t, slope), scale): the residual step of RodinConv3D4X_lite_mlp_as_residual"""
    r, mag = resize_bilinear(base, Ho, Wo)
    tt = _d(t)
    act = torch.where(tt >= 0, tt, tt * _f32(slope))
    return r + act, mag + act.abs()


# ---------------------------------------------------------------- sequential means
def mean_over(x, dim):
    """(mean over dim, sum |x| / n): an n-term sequential fp32 sum is within (n - 1) * 2^-24 * sum |x| and the division rounds once
    more, so the bound is (n - 1) / 2 + 1 fp32 ulps of sum |x| / n (mean_ulps)."""
    v = _d(x)
    return v.mean(dim), v.abs().mean(dim)


def mean_ulps(n):
    return (n - 1) / 2.0 + 1.0


# ---------------------------------------------------------------- multi-view posterior
def mv_posterior(h, qw, qb, eps, B, F_, E=4):
    """h f32 [B*F, 6E, HW] (any strides), qw [6E, 2E], qb [6E], eps [B, E, 3, HW] or None -> dict name -> (ref, scale) for mean, logvar,
    z, latent_tok, log_q, entropy, and 'ulps' (vit_triplane.py:912-933, 1152-1199; distributions.py:44-88, soft_clamp).
    With U = F / 2 + 5 fp32 ulps for a moment (pooling: (F - 1) / 2 + 1; eight fma and the bias: 4.5) of magnitude
    m_mag = sum |qw| avg|h| + |qb|, every output is held to ulps = U + 4 of:
      mean     m_mag
      logvar   s_lv = m_mag + |logvar|     (20 tanh(. / 20): slope <= 1, and tanh, the division and the product within 4 ulps)
      z, tok   m_mag + |mean| + |std eps| (1 + s_lv)      (std = exp(logvar / 2): an absolute logvar error is a relative one of std)
      entropy  s_lv + 0.5 (log 2 pi + 1)
      log_q    |ns| (|z| + |mean|) / var + ns^2 (1.5 s_lv + 2) + s_lv + 0.5 log 2 pi + |logvar|
               (ns = (z - mean) / var: z - mean cancels when |mean| >> std |eps|, term magnitude (|z| + |mean|) / var; var carries the
               whole logvar error, the std inside z half of it: 1.5 s_lv per ns, and ns is squared)."""
    hh = _d(h).reshape(B, F_, 6 * E, -1)
    HW = hh.shape[-1]
    avg, amag = hh.mean(1), hh.abs().mean(1)                                          # [B, 6E, HW]
    w, b = _d(qw), _d(qb)
    G = 2 * E
    mom = torch.einsum("goj,bgjp->bgop", w.reshape(3, G, G), avg.reshape(B, 3, G, HW)).reshape(B, 6 * E, HW) + b[None, :, None]
    mmag = torch.einsum("goj,bgjp->bgop", w.abs().reshape(3, G, G), amag.reshape(B, 3, G, HW)).reshape(B, 6 * E, HW) + b.abs()[None, :, None]
    mom, mmag = mom.reshape(B, 2 * E, 3, HW), mmag.reshape(B, 2 * E, 3, HW)
    mean, m_mag = mom[:, :E], mmag[:, :E]
    lv = 20.0 * torch.tanh(mom[:, E:] / 20.0)
    s_lv = mmag[:, E:] + lv.abs()
    std, var = torch.exp(0.5 * lv), torch.exp(lv)
    se = std * _d(eps) if eps is not None else torch.zeros_like(mean)
    z = mean + se
    z_mag = m_mag + mean.abs() + se.abs() * (1 + s_lv)
    ns = se / var
    c = 0.5 * math.log(2 * math.pi)
    log_q = -0.5 * ns * ns - c - lv
    lq_mag = ns.abs() * (z.abs() + mean.abs()) / var + ns * ns * (1.5 * s_lv + 2) + s_lv + c + lv.abs()
    tok = lambda t: t.permute(0, 2, 3, 1).reshape(B, 3 * HW, E)                          # noqa: E731
    return dict(mean=(mean, m_mag), logvar=(lv, s_lv), z=(z, z_mag), latent_tok=(tok(z), tok(z_mag)), log_q=(log_q, lq_mag),
                entropy=(lv + c + 0.5, s_lv + c + 0.5), ulps=F_ / 2.0 + 9.0)


# ---------------------------------------------------------------- DiT boundary
def patch_embed(x, in_scale, w, bias, pos, Bn, p):
    """x f32 [Bx, C*3, S, S] (channel c*3 + n: plane n), in_scale [Bn] or None, w [D, C, p, p], bias [D], pos [3L, D] ->
    (tokens [Bn, 3L, D], sum of |terms|): token n*L + ph*G + pw = bias + pos + conv_{kernel = stride = p}(s_b * x[b % Bx, plane n]).
    A chain of C*p*p fma, the input scale and the two adds: C*p*p / 2 + 2 fp32 ulps of the terms."""
    xx, ww, bb, pp = _d(x), _d(w), _d(bias), _d(pos)
    Bx, C3, S, _ = xx.shape
    C = C3 // 3
    xb = xx[torch.arange(Bn) % Bx]
    if in_scale is not None:
        xb = xb * _d(in_scale)[:, None, None, None]
    xb = xb.reshape(Bn, C, 3, S, S)
    D = ww.shape[0]
    out, mag = [], []
    for n in range(3):
        out.append(F.conv2d(xb[:, :, n], ww, bb, stride=p).flatten(2).transpose(1, 2))               # [Bn, L, D]
        mag.append(F.conv2d(xb[:, :, n].abs(), ww.abs(), bb.abs(), stride=p).flatten(2).transpose(1, 2))
    return torch.cat(out, 1) + pp[None], torch.cat(mag, 1) + pp.abs()[None]


def final_layer(tokens, shift, scale, shift_table, scale_table, w, bias, Bn, C, S, p):
    """tokens f32 [Bn*3L, D], shift / scale [Bn, D], tables [D] or None, w [p*p*C, D], bias [p*p*C] -> (out [Bn, C*3, S, S], scale):
    LayerNorm(eps 1e-6, no affine) * (1 + scale + table) + shift + table, the linear, and the unpatchify
    out[b, c*3 + n, p*ph + i, p*pw + j] = y[b, n*L + ph*G + pw, (i*p + j)*C + c]  (dit_models_xformers.py FinalLayer / unpatchify).
    Bound: D / 128 + 8 fp32 ulps of sum_d |w_od| mag_d + |bias| (mag: norm_modulate's; a lane sums D / 64 fma, then a 6-level
    butterfly: (D / 64 + 6) / 2 ulps; the normalised row itself within 4; the bias)."""
    D = tokens.shape[-1]
    G = S // p
    L = G * G
    t, mag = norm_modulate(tokens, 0, 1e-6, shift=shift, scale=scale, mod_rows=3 * L, shift_table=shift_table, scale_table=scale_table)
    ww, bb = _d(w), _d(bias)
    y, ymag = t @ ww.t() + bb, mag @ ww.abs().t() + bb.abs()

    def unpatch(v):
        return v.reshape(Bn, 3, G, G, p, p, C).permute(0, 6, 1, 2, 4, 3, 5).reshape(Bn, C * 3, S, S)
    return unpatch(y), unpatch(ymag)


def rmsnorm_heads(x, w, eps, true_dim=0):
    """x bf16 [rows, Dh], w f32 [Dh] -> (ref, |ref|): x * rsqrt(sum x^2 / true_dim + eps) * w (dit/norm.py RMSNorm on each head;
    heads stored zero-padded to Dh are normalised by their true width)."""
    v = _d(x)
    td = true_dim or v.shape[-1]
    t = v * ((v * v).sum(-1, keepdim=True) / td + _f32(eps)).rsqrt() * _d(w)
    return t, t.abs()


# ================================================================ bf16 GEMM (include/ln3d.h ln3d_gemm_bf16) and fused attention
# Epilogue numbers of include/ln3d.h (the GPU test asserts that they equal ops.EPI_*).
EPI_F32, EPI_BF16, EPI_GELU_ERF, EPI_GELU_TANH, EPI_SILU, EPI_GATE_RES, EPI_HEADS, EPI_F32_SILU, EPI_QUICK_GELU, EPI_CROSS_ATTN = range(10)

# fp32 GEMM outputs are held to |y - ref| <= gemm_ulps(K) * 2^-23 * scale, scale = sum_k |x w| + |b| (propagated through the epilogue).
# GEMM_F32_ULPS = 4 x the worst |y32 - ref| / (2^-23 scale) that two fp32 restatements of the sum reach on the tests' own random inputs
# (gemm_inputs at every shape of gemm_shapes for the six tile sizes, K in {64, 320, 1024}, and (512, 512, 512)): gemm_f32_sequential adds
# the exact bf16 x bf16 products one by one in k, gemm_f32_grouped16 adds 16-term partial sums (the grouping of the MFMA 32x32x16) one by
# one.  Measured worst: 1.434 (sequential, at (512, 512, 512)) and 0.742 (grouped), so c = 4 x 1.434 = 5.74;
# tests/test_gemm_attn_refs_cpu.py re-measures both at every shape.
# The factor 4 covers an accumulation order and adder rounding mode that cannot be read off the ISA.  Never above the a-priori cap K: K
# additions, each off by at most 2^-23 of a partial sum that is at most scale, hold for any order and for truncating adders.
GEMM_F32_WORST_SEQ = 1.434
GEMM_F32_WORST_G16 = 0.742
GEMM_F32_ULPS = 5.74             # c = 4 x 1.434, rounded up
GELU_ERF_ABS = 1.5e-4            # documented absolute error of the erf polynomial of csrc/common.h (test_gemm_gelu_erf_epilogue_tail)
ATTN_P_REL = 2.0 ** -8           # attention bound: |o - ref| <= 2^-8 * sum_j p_j |v_j| + 1 bf16 ulp of ref (see attention_bound)


def gemm_ulps(K):
    return min(GEMM_F32_ULPS, float(K))


def vt_key_order(n_pad):
    """ops.vt_key_order on the CPU: position p of every 16-key group of a V^T row holds key p with bits 2 and 3 swapped."""
    from ln3diff_amd.ops import vt_key_order as order
    return order(n_pad)


def gemm_inputs(M, N, K, seed=0, device=None):
    """The random-data convention of tests/test_kernels_gpu.py: asymmetric operands (x rows and w columns scaled by index) so that
    transposes show.  -> x bf16 [M, K], w bf16 [N, K], bias f32 [N] (on the CPU unless device is given)."""
    g = torch.Generator().manual_seed(1000003 * seed + 4099 * M + 17 * N + K)
    x = (torch.randn(M, K, generator=g) * (1 + torch.arange(M)[:, None] / M)).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * 0.05 * (1 + torch.arange(K)[None, :] / K)).to(torch.bfloat16)
    b = torch.randn(N, generator=g)
    return tuple(t if device is None else t.to(device) for t in (x, w, b))


def gemm_shapes(F, T):
    """(M, N) at a tile of F features x T tokens: one row, one short of a tile, one past it (a 2 x 2 grid of ragged tiles), and two
    token tiles less a row."""
    return [(1, 4), (T - 1, F - 4), (T + 1, F + 4), (2 * T - 1, F)]


TILE_SHAPE = {"auto": (128, 128), "s": (128, 128), "x7": (256, 256), "x8": (128, 384), "x9": (256, 192), "x12": (384, 192),
              "x13": (256, 256), "x14": (128, 192), "x16": (256, 256)}     # LN3D_GEMM_TILE -> features x tokens of the tile it forces


def act64(t, epilogue):
    """The activation of an epilogue in double, and the upper bound of |f'| the scale is multiplied with."""
    if epilogue == EPI_GELU_ERF:
        return 0.5 * t * (1 + torch.erf(t / math.sqrt(2.0))), 1.13
    if epilogue == EPI_GELU_TANH:
        return 0.5 * t * (1 + torch.tanh(0.7978845608028654 * (t + 0.044715 * t ** 3))), 1.13
    if epilogue in (EPI_SILU, EPI_F32_SILU):
        return silu64(t), 1.1
    if epilogue == EPI_QUICK_GELU:
        return t * torch.sigmoid(1.702 * t), 1.1
    return t, 1.0


def gemm_lin(x, w, bias):
    """(sum_k x w + b, sum_k |x w| + |b|) in double"""
    x, w = _d(x), _d(w)
    ref, scale = x @ w.t(), x.abs() @ w.abs().t()
    if bias is not None:
        ref, scale = ref + _d(bias), scale + _d(bias).abs()
    return ref, scale


def gemm_ref(x, w, bias, epilogue, gate=None, gate_rows=1, res=None, res_bias=None, lin=None):
    """x bf16 [M, K], w bf16 [N, K], bias f32 [N] or None -> (ref, scale) [M, N] in double of the epilogue's (bf16 or activated)
    output; for EPI_F32_SILU that is out1 (out0 is the EPI_F32 result).  EPI_GATE_RES: res + gate[m / gate_rows] * (.) +
    res_bias[m / gate_rows] (gate / res_bias [samples, N] or None).  scale is propagated to first order: times the bound of |f'| for an
    activation, times |gate| plus |res| and |res_bias| for GATE_RES.  lin: a gemm_lin result to reuse."""
    ref, scale = lin if lin is not None else gemm_lin(x, w, bias)
    if epilogue == EPI_GATE_RES:
        M = ref.shape[0]
        if gate is not None:
            g = _d(gate).repeat_interleave(gate_rows, 0)[:M]
            ref, scale = g * ref, g.abs() * scale
        ref, scale = ref + _d(res), scale + _d(res).abs()
        if res_bias is not None:
            rb = _d(res_bias).repeat_interleave(gate_rows, 0)[:M]
            ref, scale = ref + rb, scale + rb.abs()
        return ref, scale
    out, slope = act64(ref, epilogue)
    return out, scale * slope


def gemm_f32_sequential(x, w, bias):
    """fp32 restatement: the exact products added one by one in k, then the bias."""
    xf, wf = x.float(), w.float()
    acc = torch.zeros(x.shape[0], w.shape[0])
    for k in range(x.shape[1]):
        acc += xf[:, k, None] * wf[None, :, k]
    return acc + bias if bias is not None else acc


def gemm_f32_grouped16(x, w, bias):
    """fp32 restatement: 16-term partial sums (added in order), then added one by one, then the bias."""
    xf, wf = x.float(), w.float()
    acc = torch.zeros(x.shape[0], w.shape[0])
    for k0 in range(0, x.shape[1], 16):
        part = torch.zeros_like(acc)
        for k in range(k0, min(k0 + 16, x.shape[1])):
            part += xf[:, k, None] * wf[None, :, k]
        acc += part
    return acc + bias if bias is not None else acc


def assert_bf16_close_abs(y, ref, scale, floor_ulps, extra_abs, what="", max_mismatch=0.01):
    """assert_bf16_close with a documented absolute error of the formula added to every element's bound: |y - ref| <=
    max(1 bf16 ulp, floor) + extra_abs.  The mismatch fraction is taken over the elements whose bf16 spacing is at least 100 extra_abs
    (the formula's error moves at most about 1 % of those across a rounding boundary, which the fraction's own 1 % does not notice
    because it is spent on near-ties)."""
    yd = y.detach().double().cpu().reshape(-1)
    rd = ref.detach().double().cpu().reshape(-1)
    ulp = bf16_ulp(rd)
    s = torch.as_tensor(scale, dtype=torch.float64).cpu().reshape(-1).expand_as(rd)
    tol = torch.maximum(ulp, floor_ulps * F32_EPS * s) + extra_abs
    err = (yd - rd).abs()
    worst = float((err / tol).max())
    wide = ulp >= 100 * extra_abs
    mism = float((yd != bf16_rne(rd))[wide].double().mean()) if bool(wide.any()) else 0.0
    print(f"[kref] {what}: bf16 worst {worst:.3g} of the bound (+{extra_abs:g} absolute), mismatch {mism:.3g} over {int(wide.sum())} wide elements")
    bad = ~(err <= tol)
    if bad.any():
        i = _where(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} / {yd.numel()} elements beyond the bound; first at flat index {i}: y {float(yd[i])!r} "
                             f"ref {float(rd[i])!r} bound {float(tol[i]):.3g}; worst {worst:.3g} of the bound")
    assert mism <= max_mismatch, f"{what}: mismatch fraction {mism:.4g} > {max_mismatch}"
    return worst, mism


def ulp_dominated(ref, scale, floor_ulps):
    """True where 1 bf16 ulp of ref is at least the fp32 term floor_ulps * 2^-23 * scale of the bound: there a correct fp32 kernel
    differs from bf16_rne(ref) only near rounding ties."""
    return bf16_ulp(ref) >= floor_ulps * F32_EPS * torch.as_tensor(scale, dtype=torch.float64)


def heads_split_ref(M, N, tokens, tok_pad, heads, head_dim, head_dim_pad=0, transpose_mask=0):
    """The layout map of LN3D_EPI_HEADS (include/ln3d.h): column n -> output n / (heads * head_dim), head, dim; row m -> sample
    m / tokens, token m % tokens.  -> (shapes, which [N], index [M, N], untouched): shapes[w] the shape of out{w} ([B, heads, tok_pad,
    head_dim_pad], or [B, heads, head_dim_pad, tok_pad] with the tokens of every 16-group in vt_key_order when bit w of transpose_mask
    is set), index[m, n] the flat position of element (m, n) in out{which[n]}, untouched[w] a boolean tensor over out{w}.reshape(-1)
    that is True where the GEMM writes nothing (padding rows and columns)."""
    Dp = head_dim_pad or head_dim
    B = (M + tokens - 1) // tokens
    n_out = N // (heads * head_dim)
    m, n = torch.arange(M)[:, None], torch.arange(N)[None, :]
    b, t = m // tokens, m % tokens
    which, h, d = n // (heads * head_dim), (n // head_dim) % heads, n % head_dim
    order = vt_key_order(tok_pad)
    nat = ((b * heads + h) * tok_pad + t) * Dp + d
    tr = ((b * heads + h) * Dp + d) * tok_pad + order[t]
    transposed = ((transpose_mask >> which) & 1).bool()
    index = torch.where(transposed, tr, nat)
    shapes, untouched = [], []
    for wi in range(n_out):
        shapes.append((B, heads, Dp, tok_pad) if (transpose_mask >> wi) & 1 else (B, heads, tok_pad, Dp))
        u = torch.ones(B * heads * tok_pad * Dp, dtype=torch.bool)
        u[index[:, wi * heads * head_dim:(wi + 1) * heads * head_dim].reshape(-1)] = False
        untouched.append(u)
    return shapes, which.reshape(-1), index, untouched


def heads_norm_ref(lin, scale, weight, eps, head_dim=64):
    """RMSNorm over each head of 64 of the fp32 accumulators (+ bias), in double: y_i = x_i * r * w_i, r = rsqrt(mean(x^2) + eps).
    First order, with s the scale of the linear part: dy_i = w_i (r dx_i + x_i dr), dr = -r^3 sum_j x_j dx_j / 64, and
    |sum_j x_j dx_j| <= ||x||_2 ||s||_2 <= (8 / r) ||s||_2, so the scale is (s_i + |x_i| r ||s||_2 / 8) * r * |w_i|, plus |y_i| for the
    roundings of the normalisation itself (as kernel_refs.groupnorm: own term plus the shared statistic's)."""
    M, W = lin.shape
    v, s = lin.reshape(M, W // head_dim, head_dim), scale.reshape(M, W // head_dim, head_dim)
    rstd = ((v * v).mean(-1, keepdim=True) + _f32(eps)).rsqrt()
    w64 = _d(weight)
    ref = v * rstd * w64
    sc = (s + v.abs() * rstd * s.norm(dim=-1, keepdim=True) / 8.0) * rstd * w64.abs() + ref.abs()
    return ref.reshape(M, W), sc.reshape(M, W)


def attention_ref(q, k, v, scale, Nk=None, causal=False, base2=False):
    """q [B, H, Nq(+), Dh], k / v [B, H, Nk(+), Dh] bf16 in natural key order -> (ref, S) [B, H, Nq, Dh] in double:
    ref = softmax(scale * q k^T) v over the first Nk keys (query i sees keys <= i when causal), S = softmax(.) |v|.
    base2: the scores q k^T are already scaled and in the exp2 domain (requantised_query): softmax(ln 2 * q k^T)."""
    q, k, v = _d(q), _d(k), _d(v)
    Nk = k.shape[2] if Nk is None else Nk
    k, v = k[:, :, :Nk], v[:, :, :Nk]
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * (math.log(2.0) if base2 else _f32(scale))
    if causal:
        keep = torch.arange(Nk)[None, :] <= torch.arange(q.shape[2])[:, None]
        s = s.masked_fill(~keep, -math.inf)
    p = torch.softmax(s, -1)
    return p @ v, p @ v.abs()


def attention_bound(ref, S):
    """|o - ref| <= 2^-8 S + 1 bf16 ulp of ref.  Derived, not measured: every attention kernel rounds the probabilities to bf16 before
    the P V MFMA (relative error <= 2^-9 each: 2^-9 S) and rounds the output once (half an ulp); both are doubled to cover exp2, the
    fp32 scale and the re-basing of the online softmax."""
    return ATTN_P_REL * S + bf16_ulp(ref)


def assert_attention_close(o, ref, S, what="", factor=1.0, extra=None):
    """o bf16 (any shape of ref's size) within factor * attention_bound (+ extra, a per-element term argued from the kernel's arithmetic) of
    ref.  Returns the worst ratio."""
    od = o.detach().double().cpu().reshape(-1)
    rd, tol = ref.reshape(-1), factor * attention_bound(ref, S).reshape(-1)
    if extra is not None:
        tol = tol + extra.reshape(-1)
    assert od.numel() == rd.numel(), (what, od.numel(), rd.numel())
    err = (od - rd).abs()
    worst = float((err / tol).max())
    print(f"[kref] {what}: attention worst {worst:.3g} of the bound")
    bad = ~(err <= tol)
    if bad.any():
        i = _where(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} / {od.numel()} elements beyond the bound; first at flat index {i}: o {float(od[i])!r} "
                             f"ref {float(rd[i])!r} bound {float(tol[i]):.3g}; worst {worst:.3g} of the bound")
    return worst


def attention_q_rounding_term(q, k, v, scale, ref, Nk=None):
    """The term the streaming and the K-resident kernel (attn_stream_kernel, attn_kres_kernel; Dh 64, Nk a multiple of 256) add to
    attention_bound, from their arithmetic: they fold scale * log2(e) into the query fragment and round it to bf16 a SECOND time
    (csrc/attention.hip read_q), a relative 2^-9 on every q_d.  Score j is then off by at most
    d_j = 2^-9 |scale| sum_d |q_d k_jd|, the probabilities become p_j e^(delta_j) / Z with Z = sum_i p_i e^(delta_i) in
    [e^-D, Zmax], Zmax = sum_i p_i e^(d_i) (Jensen: D = sum p_i d_i <= ln Zmax), so |p'_j / p_j - 1| <= e^(d_j) Zmax - 1 and, because
    the changes of p sum to zero, |o' - o| <= sum_j p_j (e^(d_j) Zmax - 1) |v_j - o|.  Same shapes as attention_ref's result."""
    q, k, v = _d(q), _d(k), _d(v)
    Nk = k.shape[2] if Nk is None else Nk
    k, v = k[:, :, :Nk], v[:, :, :Nk]
    sc = _f32(scale)
    p = torch.softmax(torch.einsum("bhqd,bhkd->bhqk", q, k) * sc, -1)
    d = torch.einsum("bhqd,bhkd->bhqk", q.abs(), k.abs()) * abs(sc) * 2.0 ** -9
    zmax = (p * d.exp()).sum(-1, keepdim=True)
    wgt = p * (d.exp() * zmax - 1)                                                   # [B, H, Nq, Nk]
    return torch.einsum("bhqk,bhqkd->bhqd", wgt, (v[:, :, None] - ref[:, :, :, None]).abs())


def attention_inputs(B, H, Nq, Nk, Dh, seed=0, dh_pad=None, pad_value=0.0):
    """Random attention operands by the convention of tests/test_kernels_gpu.py: q, k ~ 1.5 N(0, 1), v ~ N(0, 1) + d / Dh (asymmetric in
    d), and, where Nk > 128, a late key that scores far above the rest for query 3 (the online softmax must re-base).  -> q
    [B, H, Nq_pad, dh_pad], k, v [B, H, Nk_pad, dh_pad] bf16 (rows padded to multiples of 64; key rows >= Nk hold pad_value in the
    first Dh dims, dims >= Dh hold zero)."""
    Dp = dh_pad or Dh
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * Nq + 31 * Nk + Dh + B)
    nqp, nkp = (Nq + 63) // 64 * 64, (Nk + 63) // 64 * 64
    q, k, v = torch.zeros(B, H, nqp, Dp), torch.zeros(B, H, nkp, Dp), torch.zeros(B, H, nkp, Dp)
    k[..., :Dh], v[..., :Dh] = pad_value, pad_value
    q[:, :, :Nq, :Dh] = torch.randn(B, H, Nq, Dh, generator=g) * 1.5
    k[:, :, :Nk, :Dh] = torch.randn(B, H, Nk, Dh, generator=g) * 1.5
    v[:, :, :Nk, :Dh] = torch.randn(B, H, Nk, Dh, generator=g) + torch.arange(Dh) / Dh
    if Nk > 128:
        k[:, :, Nk - 5, :Dh] = q[:, :, min(3, Nq - 1), :Dh] * 4.0
    return q.to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16)


def to_vt(v):
    """v [..., Nk_pad, Dh] in natural order -> the key-permuted V^T layout [..., Dh, Nk_pad] ln3d_attention_bf16 reads."""
    return v.transpose(-1, -2)[..., vt_key_order(v.shape[-2]).to(v.device)].contiguous()


def selector_code(n, Dh, width=None):
    """code(n)[d] = +32 where bit d mod 11 of n is set, else -32 (dims >= Dh of a wider row are zero)."""
    n = torch.as_tensor(n)
    d = torch.arange(Dh)
    c = torch.where(((n[..., None] >> (d % 11)) & 1).bool(), 32.0, -32.0)
    if width and width > Dh:
        c = F.pad(c, (0, width - Dh))
    return c


def selector_perm(Nq, Nk, causal=False):
    """the key each query selects: (7 i + 3) mod Nk, or i - (i mod 3) (>= 0) when causal"""
    i = torch.arange(Nq)
    return (i - i % 3).clamp(min=0) if causal else (7 * i + 3) % Nk


def selector_values(B, H, Nk, Dh):
    """V of the selector test, bf16 [B, H, Nk, Dh]: element (b, h, key, d) is a 64-bit mix (two multiply / xor-shift rounds) of its flat
    index, reduced modulo the prime 16381 onto bf16 values of either sign and magnitude 2^-31 .. 2^33.  bf16 has too few values for
    every element to differ, but no two (b, h, key) ROWS coincide and there is no period in key, head or batch
    (tests/test_gemm_attn_refs_cpu.py asserts the rows pairwise distinct at every GPU shape), so a row read from the wrong batch, head,
    key block or ring lap cannot pass."""
    z = torch.arange(B * H * Nk * Dh, dtype=torch.int64) + 1
    z = z * -7046029254386353131                       # 0x9E3779B97F4A7C15; int64 products wrap
    z = z ^ (z >> 31)
    z = z * -4658895280553007687                       # 0xBF58476D1CE4E5B9
    z = z ^ (z >> 29)
    hsh = z % 16381
    bits = (0x3000 + (hsh >> 1) + ((hsh & 1) << 15)).to(torch.int32).to(torch.int16)
    return bits.view(torch.bfloat16).reshape(B, H, Nk, Dh)


def selector_inputs(B, H, Nq, Nk, Dh, Dp, nkp=None, causal=False):
    """-> q [B, H, Nq_pad, Dp], k, v [B, H, Nk_pad, Dp] bf16 (natural key order) and pi: q_i = code(pi(i)), k_j = code(j), v =
    selector_values; key rows >= Nk hold 1e4 in the first Dh dims, dims >= Dh hold zero."""
    nqp, nkp = (Nq + 63) // 64 * 64, nkp or (Nk + 63) // 64 * 64
    pi = selector_perm(Nq, Nk, causal)
    q = torch.zeros(B, H, nqp, Dp)
    q[:, :, :Nq] = selector_code(pi, Dh, Dp)
    k = torch.full((B, H, nkp, Dp), 1e4)
    k[:, :, :Nk] = selector_code(torch.arange(Nk), Dh, Dp)
    v = torch.full((B, H, nkp, Dp), 1e4, dtype=torch.bfloat16)
    v[:, :, :Nk, :Dh] = selector_values(B, H, Nk, Dh)
    v[:, :, :, Dh:] = 0
    k[:, :, :, Dh:] = 0
    return q.to(torch.bfloat16), k.to(torch.bfloat16), v, pi


def attention_cases():
    """(path, Dh stored, Dh_true or 0, Nq, Nk, Nk_pad or None, causal): one set per kernel ln3d_attention_bf16 can reach (attn_kres, which
    needs a head for every CU, is apart: KRES_SHAPES)."""
    out = []
    for Nk in (1, 63, 64, 65, 128):
        for Nq in (1, 63, 65):
            out.append(("attn64x2", 64, 0, Nq, Nk, None, False))
    for Nk, nkp in ((129, None), (191, None), (257, None), (256, 320)):
        out.append(("attn64x4", 64, 0, 65, Nk, nkp, False))
    for Nq, Nk in ((1, 256), (65, 256), (200, 512), (256, 1280)):
        out.append(("stream", 64, 0, Nq, Nk, None, False))
    for Dh, dt in ((80, 0), (80, 72), (128, 0), (128, 72)):
        for Nq, Nk in ((33, 77), (65, 129)):
            out.append((f"attn{Dh}" + (f"_{dt}" if dt else ""), Dh, dt, Nq, Nk, None, False))
    for n in (1, 31, 32, 33, 64, 77, 128):
        out.append(("short_causal", 64, 0, n, n, None, True))
    return out


ATTENTION_BH = [(1, 1), (2, 3)]
KRES_SHAPES = [(256, 512), (256, 768)]


def requantised_query(q, scale):
    """attn_stream_kernel / attn_kres_kernel fold scale * log2(e) into the query fragment and round it to bf16 a second time
    (csrc/attention.hip read_q: pack2bf(q * scale_log2), scale_log2 the fp32 product of the fp32 scale and 1.4426950408889634f).  -> that
    query, bf16; the scores it forms are in the exp2 domain (attention_ref(..., base2=True))."""
    sl2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    return (q.float() * sl2).to(torch.bfloat16)
