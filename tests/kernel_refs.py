"""Float64 restatements of the glue kernels of include/ln3d.h and per-element bounds for their outputs.

Every reference is computed in double from the same fp32 / bf16 inputs the kernel received, from the operation's definition (the
reference source lines each kernel's comment cites) or torch.nn.functional in double.  Besides the value, the fp32-sensitive
references return a `scale` per element: the magnitude of the terms the kernel summed (first-order error propagation), so that a
result which cancels to near zero is judged against the rounding of its terms, not against its own tiny size.

Bounds (tests/test_kernel_refs_cpu.py shows that they can fail):
  assert_bf16_close: |y - ref| <= max(1 bf16 ulp of ref, floor_ulps fp32 ulps of scale) for every element, and the fraction of
                     elements with y != bf16_rne(ref) at most max_mismatch (a correct fp32 kernel flips only near rounding ties);
  assert_f32_close:  |y - ref| <= ulps * 2^-23 * scale for every element.
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
