"""Float64 restatements of the stages of the tri-plane ray-marcher (csrc/render.hip: ln3d_render_triplane, ln3d_query_points) and
per-element bounds for every output the kernels write.

The renderer is cut at its discontinuities: EACH STAGE'S REFERENCE TAKES THE KERNEL'S OWN fp32 OUTPUTS OF THE STAGE BEFORE IT, so no
comparison crosses a searchsorted, a sort or a box test that was evaluated in another precision:

  limits         rays (explicit, or from `cams`) -> slab test (math_utils.py:46-118)                  vs out['ray_limits']
  coarse_coords  out['ray_limits'] + the call-wide fix-up (renderer.py:151-155) + jitter -> o + z d    vs out['coarse_coords']
  coarse_sigma   decoder at out['coarse_coords'] (renderer.py:55-104, triplane.py:339-372)             vs out['coarse_sigma']
  fine_depths    coarse depths (double) + out['coarse_sigma'] -> march weights, pools, pdf, cdf,
                 inverse cdf (ray_marcher.py:26-68, renderer.py:479-552)                               vs out['fine_depths']
  fine_coords    o + out['fine_depths'] d                                                              vs out['fine_coords']
  fine_sigma     decoder at out['fine_coords']                                                         vs out['fine_sigma']
  merge          out['all_coords'] is bitwise a permutation of cat(coarse_coords, fine_coords) per ray, non-decreasing in depth
  feature_volume decoder colours at out['all_coords']                                                  vs out['feature_volume']
  weights, rgb, depth, wsum, visibility   the final march over the merged samples (ray_marcher.py:26-68)

Every reference returns (value, scale).  `scale` is the first-order error budget of an fp32 evaluation of the same formula in ANY
order: every rounding contributes 1/2 ulp of the magnitude it rounds (the coefficients 0.5 below, one per operation, are the
rounding count), errors of earlier quantities are carried through the derivatives, and sums / products over n terms add 1/2 ulp per
level of the longest chain: NCHAIN = 10, a 6-level wave scan + up to 4 in-lane steps - the kernels' chains.  (The fp32 oracle sums
serially, up to 255 levels; that it stays inside these bounds all the same, at <= 0.37 of them, is an empirical observation about
the oracle in tests/test_render_refs_cpu.py - its errors do not line up - and no part of the derivation of the kernels' bound.)
The bound is |y - ref| <= STAGE_ULPS * 2^-23 * scale with STAGE_ULPS = 2: one factor of 2 for the hardware exp2 / log2 / rcp (1 ulp,
not 1/2) and for the second-order terms.  The decoder's bound is DEC_K * 2^-16 of ITS scale (see decoder()).
tests/test_render_refs_cpu.py shows that the fp32 oracle sits inside every bound and that five seeded faults do not.
"""
import math

import numpy as np
import torch

from kernel_refs import F32_EPS

STAGE_ULPS = 2.0
NCHAIN = 10
RAY_ULPS = 8.0          # camera ray generation: ~12 fp32 operations on the way from (cam, pixel) to a unit direction, 1/2 ulp each, + slack
# decoder: features x and weights w are split into hi = truncated bf16 and lo = RNE bf16 of the remainder.  |x - hi| < 2^-7 |x|
# (truncation keeps 8 bits) and lo has 8 bits of that: |x - hi - lo| <= 2^-9 * 2^-7 |x| = 2^-16 |x|.  One product w x is evaluated as
# wh xh + wh xl + wl xh: the representation errors give 2 * 2^-16 |w x|, the dropped wl xl is < 2^-7 * 2^-7 |w x| = 4 * 2^-16 |w x|:
# 6 * 2^-16 per product in the worst case.  fp32 accumulation of 32 (64) x 3 products, the fp32 pre-scaling of the weights by
# gain * log2 e (ln 2) and the C-operand bias are < 200 * 2^-24 = 0.1 * 2^-16: DEC_K = 7.
DEC_K = 7.0
DEC_ULPS = DEC_K * 128.0                       # DEC_K * 2^-16 in fp32 ulps
FILL_SIGMA = float(np.float32(-3.4028234663852886e38) / np.float32(3.0))       # nan_to_num(-inf) / 3 (renderer.py:354-407)


def _d(t):
    return None if t is None else torch.as_tensor(t).detach().double().cpu()


# ---------------------------------------------------------------- rays and limits
def camera_rays(cams, res):
    """cams f32 [V,25] -> (o, d, sd) [V, res*res, 3]: ray_sampler.py:262-331 with patch == image.  sd = magnitude of the terms behind each
    component of d (the kernel and the reference form R (x, y, 1) + t and subtract t again: the translation cancels with ITS size)."""
    c = _d(cams)
    V = c.shape[0]
    c2w = c[:, :16].reshape(V, 4, 4)
    fx, sk, cx, fy, cy = (c[:, k, None] for k in (16, 17, 18, 20, 21))
    pix = torch.arange(res * res)
    x = ((pix % res).double() + 0.5) / res
    y = ((pix // res).double() + 0.5) / res
    xl = (x - cx + cy * sk / fy - sk * y / fy) / fx
    yl = (y - cy) / fy
    sxl = (x.abs() + cx.abs() + (cy * sk / fy).abs() * 2 + (sk * y / fy).abs() * 2 + xl.abs() * fx.abs()) / fx.abs()
    syl = (y.abs() + cy.abs() + yl.abs() * fy.abs()) / fy.abs()
    R, t = c2w[:, None, :3, :3], c2w[:, None, :3, 3]
    dv = R[..., 0] * xl[..., None] + R[..., 1] * yl[..., None] + R[..., 2]
    sdv = R[..., 0].abs() * (sxl + xl.abs())[..., None] + R[..., 1].abs() * (syl + yl.abs())[..., None] + R[..., 2].abs() + 2 * t.abs() + dv.abs()
    nrm = dv.norm(dim=-1, keepdim=True).clamp(min=1e-12)
    d = dv / nrm
    sd = sdv / nrm + d.abs() * ((d.abs() * sdv).sum(-1, keepdim=True) / nrm + 2)
    return t.expand_as(d).contiguous(), d, sd


def slab_limits(o, d, sd, box_warp):
    """get_ray_limits_box (math_utils.py:46-118).  o, d, sd double [..., 3] -> dict(tmin, tmax, smin, smax, hit, margin): -1 / -2 on a miss.
    A slab limit (bound - o) * (1 / d) rounds three times; max / min over the axes are 1-Lipschitz, so the scale is that of the axes
    that can win (those within their own bounds of the winner).  margin: the float64 hit / miss decision is further from the edge
    than 16 bounds - the rays on which a per-element comparison is meaningful, chosen here from the reference alone."""
    half = float(np.float32(box_warp) * np.float32(0.5))
    with np.errstate(divide='ignore'):
        inv = 1.0 / d
    neg = inv < 0
    lo = torch.where(neg, torch.full_like(d, half), torch.full_like(d, -half))
    tn, tf = (lo - o) * inv, (-lo - o) * inv
    fin = torch.isfinite(inv)

    def sc(t, b):
        s = 0.5 * (b.abs() + o.abs()) * inv.abs() + 1.0 * t.abs() + (RAY_ULPS / STAGE_ULPS) * t.abs() * sd / d.abs()
        return torch.where(fin, s, torch.zeros_like(s))
    sn, sf = sc(tn, lo), sc(tf, -lo)
    bn, bf = STAGE_ULPS * F32_EPS * sn, STAGE_ULPS * F32_EPS * sf
    tmin, tmax = tn.max(-1).values, tf.min(-1).values
    act_n = torch.where(fin, tn + bn, tn) >= (tn - bn).max(-1, keepdim=True).values
    act_f = torch.where(fin, tf - bf, tf) <= (tf + bf).min(-1, keepdim=True).values
    smin = torch.where(act_n, sn, torch.zeros_like(sn)).max(-1).values
    smax = torch.where(act_f, sf, torch.zeros_like(sf)).max(-1).values
    hit = tmin <= tmax
    margin = (tmax - tmin).abs() > 16 * STAGE_ULPS * F32_EPS * (smin + smax)
    return dict(tmin=torch.where(hit, tmin, torch.full_like(tmin, -1.0)), tmax=torch.where(hit, tmax, torch.full_like(tmax, -2.0)),
                smin=smin, smax=smax, hit=hit, margin=margin)


def fixed_limits(limits, V, M, vpc):
    """renderer.py:151-155 on the kernel's own fp32 slab limits [V*M, 2]: a ray that misses takes (min, max) of the valid STARTS (sic) of
    its call group (views_per_call consecutive views); a group without a hit keeps -1 / -2."""
    lim = _d(limits).reshape(V, M, 2)
    t0, t1 = lim[..., 0].clone(), lim[..., 1].clone()
    vpc = V if (vpc <= 0 or vpc > V) else vpc
    for g0 in range(0, V, vpc):
        a, b = t0[g0:g0 + vpc], t1[g0:g0 + vpc]
        ok = b > a
        if ok.any():
            lo, hi = a[ok].min(), a[ok].max()
            t0[g0:g0 + vpc] = torch.where(ok, a, lo)
            t1[g0:g0 + vpc] = torch.where(ok, b, hi)
    return t0, t1, vpc


def coarse_depths(t0, t1, jitter, S, numeric):
    """t0, t1 double [V, M] (or the two numbers of numeric mode), jitter [V, M, S] -> (z, scale) [V, M, S].
    'auto' (math_utils.py:121-137): t0 + i / (S-1) (t1 - t0) + jitter (t1 - t0) / (S-1); numbers (renderer.py:463-474): torch.linspace
    (from the start below the midpoint, from the end above it) + jitter * delta.  Each of the two products rounds three times."""
    j = _d(jitter)
    i = torch.arange(S, dtype=torch.float64)
    if numeric is not None:
        a, b = float(np.float32(numeric[0])), float(np.float32(numeric[1]))
        delta = (b - a) / (S - 1)
        lo = i < S // 2
        base = torch.where(lo, a + delta * i, b - delta * (S - 1 - i))
        sbase = torch.where(lo, abs(a) + 1.5 * abs(delta) * i, abs(b) + 1.5 * abs(delta) * (S - 1 - i)) * 0.5 + 0.5 * base.abs()
        z = base + j * delta
        return z, sbase + 1.5 * j * abs(delta) + 0.5 * z.abs()
    t0, t1 = t0[..., None], t1[..., None]
    step = i / (S - 1)
    term1, term2 = step * (t1 - t0), j * (t1 - t0) / (S - 1)
    z = t0 + term1 + term2
    return z, 1.5 * term1.abs() + 0.5 * (t0 + term1).abs() + 1.5 * term2.abs() + 0.5 * z.abs()


def positions(o, d, sd, z, ez):
    """o + z d (renderer.py:232): o, d, sd [V, M, 3], z and its absolute error ez (in fp32 ulps of 1) [V, M, n] -> (p, scale) [V, M, n, 3].
    The expression has one product and one sum, so two roundings (1/2 ulp of |z d|, 1/2 ulp of |p|) are the worst case of EVERY way to
    evaluate it: mul then add rounds twice, an fma (or addcmul) once, and there is no other order.  An implementation that rounds
    twice can therefore reach, but never pass, half of the bound (STAGE_ULPS = 2) - the fp32 oracle's 0.50 on fine_coords is that
    ceiling, not a lack of slack."""
    o, d, sd, z, ez = o[:, :, None, :], d[:, :, None, :], sd[:, :, None, :], z[..., None], ez[..., None]
    p = o + z * d
    return p, 0.5 * (z * d).abs() + 0.5 * p.abs() + d.abs() * ez / STAGE_ULPS + (RAY_ULPS / STAGE_ULPS) * (z.abs() + 1) * sd


# ---------------------------------------------------------------- tri-plane gather + OSGDecoder
def decoder(planes, pts, dec, box_warp, bbox=None):
    """planes f32 channel-last [3, H, W, 32], pts f32 [P, 3], dec = (w0 [64,32], b0, w1 [4,64], b1) -> dict(sigma [P], rgb [P,3], their scales
    in units of DEC_K * 2^-16 (bound = DEC_ULPS * 2^-23 * scale), inb [P]).
    sample_from_planes (renderer.py:55-104): projections (x,y) (y,z) (z,x) of 2 / box_warp * p, F.grid_sample(bilinear, zeros, align_corners
    False), mean over the planes; OSGDecoder (triplane.py:339-372): FC(gain 1/sqrt 32) - softplus - FC(gain 1/sqrt 64), sigma = y0,
    rgb = sigmoid(y1..3) * 1.002 - 0.001; bbox filter (renderer.py:354-407) on the fp32 coordinates: exact.
    Error budget, in fp32 ulps of 1 until the end: the texel coordinate ix = ((gx + 1) W - 1) / 2 is rounded 5 times, which moves the
    sample by e_ix texels and the feature by |df/dix| e_ix (for W = 128 and texel-to-texel differences of the texels' own size this is
    2^-16 of the feature - as large as the split-bf16 term); tap weights and the 4-tap / 3-plane sums round 3.5 + 1 times; the two
    layers carry DEC_K * 2^-16 of sum |w| |x| each (DEC_K above), softplus has slope sigmoid(h) <= 1 and an ABSOLUTE error of ~2 ulp of
    1 + softplus (hardware exp2 / log2 without a log1p correction: 1 + 2^x rounds at 1)."""
    pl = _d(planes)
    _, H, W, C = pl.shape
    p32 = torch.as_tensor(pts).detach().float().cpu()
    cs = 2.0 / float(np.float32(box_warp))
    g = p32.double() * cs
    feat = torch.zeros(g.shape[0], C, dtype=torch.float64)
    efeat = torch.zeros_like(feat)
    for k, (a, b) in enumerate(((0, 1), (1, 2), (2, 0))):
        gx, gy = g[:, a], g[:, b]
        ix, iy = ((gx + 1) * W - 1) / 2, ((gy + 1) * H - 1) / 2
        eix = 0.5 * W * (gx.abs() + (gx + 1).abs()) + 0.25 * (2 * ix).abs()
        eiy = 0.5 * H * (gy.abs() + (gy + 1).abs()) + 0.25 * (2 * iy).abs()
        x0, y0 = torch.floor(ix), torch.floor(iy)
        wx1, wy1 = (ix - x0)[:, None], (iy - y0)[:, None]
        flat = pl[k].reshape(H * W, C)

        def tap(dx, dy):
            xi, yi = (x0 + dx).long(), (y0 + dy).long()
            ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            return flat[yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)] * ok[:, None]
        v00, v01, v10, v11 = tap(0, 0), tap(1, 0), tap(0, 1), tap(1, 1)
        feat += v00 * (1 - wx1) * (1 - wy1) + v01 * wx1 * (1 - wy1) + v10 * (1 - wx1) * wy1 + v11 * wx1 * wy1
        mag = v00.abs() * (1 - wx1) * (1 - wy1) + v01.abs() * wx1 * (1 - wy1) + v10.abs() * (1 - wx1) * wy1 + v11.abs() * wx1 * wy1
        dfdx = ((v01 - v00) * (1 - wy1) + (v11 - v10) * wy1).abs()
        dfdy = ((v10 - v00) * (1 - wx1) + (v11 - v01) * wx1).abs()
        efeat += dfdx * eix[:, None] + dfdy * eiy[:, None] + 4.5 * mag
    feat, efeat = feat / 3, efeat / 3 + 1.0 * feat.abs() / 3
    w0, b0, w1, b1 = (_d(t) for t in dec)
    W0, W1 = w0 / math.sqrt(w0.shape[1]), w1 / math.sqrt(w1.shape[1])
    h = feat @ W0.t() + b0
    s1 = feat.abs() @ W0.abs().t() + b0.abs()
    eh = efeat @ W0.abs().t() + DEC_ULPS * s1
    sp = torch.where(h > 20, h, torch.log1p(torch.exp(h.clamp(max=20))))
    esp = torch.sigmoid(h) * eh + 4.0 * (1 + sp)
    y = sp @ W1.t() + b1
    ey = esp @ W1.abs().t() + DEC_ULPS * (sp @ W1.abs().t() + b1.abs())
    sg = torch.sigmoid(y[:, 1:])
    rgb, ergb = sg * 1.002 - 0.001, 1.002 * sg * (1 - sg) * ey[:, 1:] + 3.0
    sigma, esigma = y[:, 0].clone(), ey[:, 0].clone()
    inb = torch.ones(g.shape[0], dtype=torch.bool)
    if bbox is not None:
        lo, hi = np.float32(bbox[0]), np.float32(bbox[1])
        inb = ((p32 >= float(lo)) & (p32 <= float(hi))).all(-1)
        sigma[~inb] = FILL_SIGMA
        rgb[~inb] = 0.0
    return dict(sigma=sigma, sigma_scale=esigma / DEC_ULPS, rgb=rgb, rgb_scale=ergb / DEC_ULPS, inb=inb)


# ---------------------------------------------------------------- MipRayMarcher2
def march(z, ez, sig, col, ecol):
    """ray_marcher.py:26-68 over n samples per ray: z, ez (absolute error of z in fp32 ulps of 1), sig (fp32 values, exact) [R, n];
    col, ecol [R, n, 3].  Returns the n - 1 weights, the sums over them and T behind the last interval, each with its error in fp32
    ulps of 1 (divide by STAGE_ULPS for the `scale` of Report.cmp)."""
    z0, z1, s0, s1 = z[:, :-1], z[:, 1:], sig[:, :-1], sig[:, 1:]
    dl = z1 - z0
    edl = ez[:, :-1] + ez[:, 1:] + 0.5 * dl.abs()
    m = (s0 + s1) * 0.5 - 1
    em = 0.25 * (s0 + s1).abs() + 0.5 * m.abs()
    dm = torch.where(m > 20, m, torch.log1p(torch.exp(m.clamp(max=20))))           # F.softplus, threshold 20
    slope = torch.where(m > 20, torch.ones_like(m), torch.sigmoid(m))
    edm = torch.nan_to_num(slope * em, nan=0.0) + 2.5 * dm
    x = dm * dl
    ex = dl.abs() * edm + dm * edl + 0.5 * x.abs()
    e = torch.exp(-x)
    ee = e * (ex + 1.0 * x.abs()) + 1.0 * e
    al = 1 - e
    eal = ee + 0.5 * al.abs()
    f = 1 - al + 1e-10
    ef = eal + 0.5 * (1 - al).abs() + 0.5 * f.abs()
    ones = torch.ones_like(f[:, :1])
    Tin = torch.cumprod(torch.cat([ones, f], 1), 1)                                # Tin[:, i] = prod_{k<i} f_k, i = 0 .. n-1
    rel = torch.cumsum(torch.cat([torch.zeros_like(ones), ef / f.abs()], 1), 1) + 0.5 * NCHAIN
    eT = Tin * rel
    T, w = Tin[:, :-1], al * Tin[:, :-1]
    ew = al.abs() * eT[:, :-1] + T * eal + 0.5 * w.abs() + 1e-30
    cm, zm = (col[:, :-1] + col[:, 1:]) / 2, (z0 + z1) / 2
    ecm = (ecol[:, :-1] + ecol[:, 1:]) / 2 + 0.25 * (col[:, :-1] + col[:, 1:]).abs()
    ezm = (ez[:, :-1] + ez[:, 1:]) / 2 + 0.25 * (z0 + z1).abs()

    def wsum(v, ev):
        t = w[..., None] * v if v.dim() == 3 else w * v
        wa, ewa = (w.abs()[..., None], ew[..., None]) if v.dim() == 3 else (w.abs(), ew)
        return t.sum(1), (v.abs() * ewa + wa * ev + 0.5 * t.abs()).sum(1) + 0.5 * NCHAIN * t.abs().sum(1)
    rgb, ergb = wsum(cm, ecm)
    dep, edep = wsum(zm, ezm)
    ws, ews = w.sum(1), ew.sum(1) + 0.5 * NCHAIN * w.abs().sum(1)
    return dict(w=w, ew=ew, rgb=rgb, ergb=ergb, depth=dep, edepth=edep, wsum=ws, ewsum=ews, vis=Tin[:, -1], evis=eT[:, -1] + 1e-30)


def importance(zc, ezc, w, ew, u):
    """sample_importance / sample_pdf (renderer.py:479-552): zc, ezc [R, S]; w, ew [R, S-1] (march); u f32 [R, NI] -> (z_fine, its error in fp32
    ulps of 1) [R, NI].  The inverse cdf is the piecewise-linear, continuous map through the nodes (cdf_k, bin_k): an error of a node's
    ordinate moves it by at most that error, an error of the abscissae by the local slope (bin width / pdf mass - the 1 / denom
    amplification; the slopes of the two neighbouring bins are included because the kernel's cdf may place u in one of them)."""
    R, S = zc.shape
    ninf = torch.full_like(w[:, :1], -math.inf)
    wp, ewp = torch.cat([ninf, w, ninf], 1), torch.cat([torch.zeros_like(ninf), ew, torch.zeros_like(ninf)], 1)
    mp, emp = torch.maximum(wp[:, :-1], wp[:, 1:]), torch.maximum(ewp[:, :-1], ewp[:, 1:])              # max_pool1d(2, 1, padding 1)
    av = (mp[:, :-1] + mp[:, 1:]) / 2 + 0.01                                                           # avg_pool1d(2, 1) + 0.01
    eav = (emp[:, :-1] + emp[:, 1:]) / 2 + 0.25 * (mp[:, :-1] + mp[:, 1:]).abs() + 0.5 * av.abs()
    wv = av[:, 1:-1] + 1e-5
    ewv = eav[:, 1:-1] + 0.5 * wv
    tot = wv.sum(1, keepdim=True)
    etot = ewv.sum(1, keepdim=True) + 0.5 * NCHAIN * tot
    pdf = wv / tot
    epdf = ewv / tot + pdf * etot / tot + 0.5 * pdf
    zero = torch.zeros_like(pdf[:, :1])
    cdf = torch.cat([zero, torch.cumsum(pdf, 1)], 1)                                                    # S - 2 entries
    ecdf = torch.cat([zero, torch.cumsum(epdf, 1)], 1) + 0.5 * NCHAIN * cdf
    bins = (zc[:, :-1] + zc[:, 1:]) / 2                                                                 # S - 1 entries
    ebin = (ezc[:, :-1] + ezc[:, 1:]) / 2 + 0.25 * (zc[:, :-1] + zc[:, 1:]).abs()
    u = _d(u)
    n_s = S - 3
    inds = torch.searchsorted(cdf.contiguous(), u.contiguous(), right=True)
    below, above = (inds - 1).clamp(0, n_s), inds.clamp(0, n_s)
    cb, ca, bb, ba = cdf.gather(1, below), cdf.gather(1, above), bins.gather(1, below), bins.gather(1, above)
    den = ca - cb
    den = torch.where(den < 1e-5, torch.ones_like(den), den)
    t = (u - cb) / den
    zf = bb + t * (ba - bb)
    seg = (bins[:, 1:n_s + 1] - bins[:, :n_s]).abs() / (cdf[:, 1:] - cdf[:, :-1])                      # slope of bin k, k = 0 .. n_s - 1
    nb = lambda a, idx, lo, hi: torch.stack([a.gather(1, (idx + s).clamp(lo, hi)) for s in (-1, 0, 1, 2)]).max(0).values
    slope = nb(seg, below, 0, n_s - 1)
    # nodes; abscissae (+ the rounding of u - cdf); the quotient, the bin width and the product round; the final sum rounds
    ezf = nb(ebin, below, 0, S - 2) + slope * (nb(ecdf, below, 0, n_s) + 0.5 * (u - cb).abs()) + 2.0 * (t * (ba - bb)).abs() + 0.5 * zf.abs()
    return zf, ezf


# ---------------------------------------------------------------- the stage-by-stage check
class Report:
    """worst fraction of the bound per stage; failures name stage, kernel, ray (view, pixel) and sample index (= lane + 64 j)"""
    def __init__(self, kernel):
        self.kernel, self.worst, self.failed, self.notes, self.stages = kernel, {}, {}, {}, {}

    def cmp(self, stage, y, ref, scale, ulps, per_ray, M):
        y64, ref = _d(y).reshape(-1), _d(ref).reshape(-1)
        s = _d(scale).reshape(-1).expand_as(ref)
        err = (y64 - ref).abs()
        err = torch.where(y64 == ref, torch.zeros_like(err), err)
        frac = err / (ulps * F32_EPS * s).clamp(min=1e-300)
        self.stages[stage] = (y64, ref, ulps * F32_EPS * s, per_ray, M)          # for check_pair
        bad = ~(frac <= 1.0)
        self.worst[stage] = max(self.worst.get(stage, 0.0), float(torch.nan_to_num(frac, nan=math.inf).max()) if frac.numel() else 0.0)
        if bad.any():
            i = int(bad.nonzero()[0])
            ray, lane = i // per_ray, i % per_ray
            msg = (f"stage {stage} of {self.kernel}: {int(bad.sum())} / {y64.numel()} elements beyond the bound; first at ray {ray} (view {ray // M}, "
                   f"ray-in-view {ray % M}) element {lane} (lane {lane % 64}): y {float(y64[i])!r} ref {float(ref[i])!r} bound "
                   f"{float(ulps * F32_EPS * s[i]):.3g}; worst {self.worst[stage]:.3g} of the bound; rays affected "
                   f"{sorted(set((bad.nonzero().reshape(-1) // per_ray).tolist()))[:8]}")
            self.failed.setdefault(stage, msg)
        else:
            print(f"[rref] {self.kernel} {stage}: worst {self.worst[stage]:.3g} of the bound")

    def exact(self, stage, ok, msg):
        self.worst.setdefault(stage, 0.0)
        if not ok:
            self.failed.setdefault(stage, f"stage {stage} of {self.kernel}: {msg}")

    def raise_if_failed(self):
        if self.failed:
            raise AssertionError("\n".join(self.failed.values()))


def check_pair(ra, rb):
    """Two implementations (Reports of check_render on the SAME inputs) against each other, stage for stage and element for element:
        |y_a - y_b| <= bound_a + bound_b + |ref_a - ref_b|.
    ref_a - ref_b is what the difference of the two implementations' EARLIER stage outputs does to this stage, propagated exactly:
    each float64 reference is evaluated at its own implementation's inputs (across the searchsorted, the sort and the box test as
    well: the inverse cdf and the composite are continuous, and the references cross them in double).  Where the earlier stages are
    bit-equal it vanishes and the two outputs are held to the sum of their bounds.  Returns a Report over the stages both have."""
    rep = Report(f"{ra.kernel} vs {rb.kernel}")
    for stage in ra.stages:
        if stage not in rb.stages:
            continue
        (ya, fa, ba, per_ray, M), (yb, fb, bb, _, _) = ra.stages[stage], rb.stages[stage]
        assert ya.numel() == yb.numel(), (stage, ya.numel(), yb.numel())
        same_fill = (ya == fa) & (yb == fb) & (ya == yb)                      # filtered samples: the fill value, exact in both
        tol = ba + bb + torch.nan_to_num((fa - fb).abs(), nan=0.0)
        rep.cmp(stage, torch.where(same_fill, torch.zeros_like(ya), ya - yb), torch.zeros_like(ya), tol / F32_EPS, 1.0, per_ray, M)
    return rep


def _rowkeys(c):
    """[R, n, 3] f32 -> order that sorts every ray's samples by the bits of (x, y, z): equal rows are interchangeable"""
    b = c.contiguous().view(torch.int32).numpy().astype(np.int64)
    R, n, _ = b.shape
    ray = np.repeat(np.arange(R), n)
    order = np.lexsort((b[..., 2].reshape(-1), b[..., 1].reshape(-1), b[..., 0].reshape(-1), ray))
    return order.reshape(R, n) - (np.arange(R) * n)[:, None]


def check_render(inp, out, kernel):
    """inp: planes [NP,3,H,W,32], plane_index [V], cams [V,25] + res, or ray_o / ray_d [V,M,3]; jitter [V,M,S], u_fine [V*M,NI], dec, box_warp,
    bbox (min, max) or None, white_back, views_per_call, S, NI, numeric (start, end) or None.  out: the kernel's (or a stand-in's) fp32
    outputs, CPU tensors.  Returns the Report (call .raise_if_failed())."""
    rep = Report(kernel)
    S, NI, NT = inp['S'], inp['NI'], inp['S'] + inp['NI']
    if inp.get('ray_o') is not None:
        o, d = _d(inp['ray_o']), _d(inp['ray_d'])
        sd = torch.zeros_like(d)
    else:
        o, d, sd = camera_rays(inp['cams'], inp['res'])
    V, M, _ = o.shape
    R = V * M
    numeric, bbox = inp.get('numeric'), inp.get('bbox')
    f32 = lambda k: torch.as_tensor(out[k]).detach().float().cpu()
    # ---- limits
    if numeric is None:
        lim = f32('ray_limits').reshape(R, 2)
        sl = slab_limits(o.reshape(R, 3), d.reshape(R, 3), sd.reshape(R, 3), inp['box_warp'])
        mg = sl['margin']
        rep.notes['limits_without_margin'] = float((~mg).double().mean())
        k_hit = lim[:, 1] > lim[:, 0]
        rep.exact('limits', bool((k_hit == sl['hit'])[mg].all()), "hit / miss differs from the float64 slab test on rays with a margin: rays "
                  f"{(k_hit != sl['hit'])[mg].nonzero().reshape(-1)[:8].tolist()}")
        both = mg & sl['hit'] & k_hit
        miss = mg & ~sl['hit'] & ~k_hit
        rep.exact('limits', bool((lim[miss] == torch.tensor([-1.0, -2.0])).all()), "a miss is not (-1, -2)")
        rep.cmp('limits', lim[both], torch.stack([sl['tmin'], sl['tmax']], -1)[both], torch.stack([sl['smin'], sl['smax']], -1)[both],
                STAGE_ULPS, 2, M)
        t0, t1, vpc = fixed_limits(lim, V, M, inp.get('views_per_call', 0))
    else:
        t0 = t1 = None
        vpc = inp.get('views_per_call', 0)
        vpc = V if (vpc <= 0 or vpc > V) else vpc
    # ---- coarse positions
    zc, szc = coarse_depths(t0, t1, inp['jitter'].reshape(V, M, S), S, numeric)
    zc, szc = zc.expand(V, M, S), szc.expand(V, M, S)
    ezc = STAGE_ULPS * szc
    pc, spc = positions(o, d, sd, zc, ezc)
    rep.cmp('coarse_coords', f32('coarse_coords'), pc, spc, STAGE_ULPS, 3 * S, M)
    # ---- decoder at the kernel's coordinates
    pidx = torch.as_tensor(inp['plane_index']).long().cpu()

    def decode(coords, n):
        c = coords.reshape(V, M * n, 3)
        res = [decoder(inp['planes'][int(pidx[v])], c[v], inp['dec'], inp['box_warp'], bbox) for v in range(V)]
        return {k: torch.cat([r[k] for r in res]) for k in res[0]}

    def cmp_sigma(stage, y, dd, n):
        y = y.reshape(-1)
        rep.exact(stage, bool((y[~dd['inb']] == FILL_SIGMA).all()), "a point outside the sampler bbox does not carry the fill density")
        ref = torch.where(dd['inb'], dd['sigma'], y.double())
        rep.cmp(stage, y, ref, dd['sigma_scale'], DEC_ULPS, n, M)
    dc = decode(f32('coarse_coords'), S)
    sig_c = f32('coarse_sigma').reshape(R, S)
    cmp_sigma('coarse_sigma', sig_c, dc, S)
    # ---- importance sampling
    zc2, ezc2 = zc.reshape(R, S), ezc.reshape(R, S)
    zero3 = torch.zeros(R, S, 3, dtype=torch.float64)
    mc = march(zc2, ezc2, sig_c.double(), zero3, zero3)
    zf_ref, ezf = importance(zc2, ezc2, mc['w'], mc['ew'], inp['u_fine'].reshape(R, NI))
    zf = f32('fine_depths').reshape(R, NI)
    rep.cmp('fine_depths', zf, zf_ref, ezf / STAGE_ULPS, STAGE_ULPS, NI, M)
    # ---- fine positions
    pf, spf = positions(o, d, sd, zf.double().reshape(V, M, NI), torch.zeros(V, M, NI, dtype=torch.float64))
    rep.cmp('fine_coords', f32('fine_coords'), pf, spf, STAGE_ULPS, 3 * NI, M)
    df = decode(f32('fine_coords'), NI)
    sig_f = f32('fine_sigma').reshape(R, NI)
    cmp_sigma('fine_sigma', sig_f, df, NI)
    # ---- merge
    z_cat = torch.cat([zc2, zf.double()], 1)
    ez_cat = torch.cat([ezc2, torch.zeros(R, NI, dtype=torch.float64)], 1)
    sig_cat = torch.cat([sig_c, sig_f], 1).double()
    if out.get('all_coords') is not None:
        cat_c = torch.cat([f32('coarse_coords').reshape(R, S, 3), f32('fine_coords').reshape(R, NI, 3)], 1)
        allc = f32('all_coords').reshape(R, NT, 3)
        oa, ob = _rowkeys(allc), _rowkeys(cat_c)
        perm = np.empty_like(oa)
        np.put_along_axis(perm, oa, ob, axis=1)                      # all_coords[r, i] == cat[r, perm[r, i]]
        perm = torch.from_numpy(perm)
        same = (allc.view(torch.int32) == cat_c.gather(1, perm[..., None].expand(-1, -1, 3)).view(torch.int32)).all(-1)
        rep.exact('merge', bool(same.all()), f"all_coords is not bitwise a permutation of cat(coarse_coords, fine_coords) on rays "
                  f"{(~same).any(1).nonzero().reshape(-1)[:8].tolist()} (first element {(~same).nonzero()[:1].tolist()})")
        zs, ezs = z_cat.gather(1, perm), ez_cat.gather(1, perm)
        dec_ok = zs[:, 1:] - zs[:, :-1] >= -F32_EPS * (ezs[:, 1:] + ezs[:, :-1])
        rep.exact('merge', bool(dec_ok.all()), f"merged samples not in depth order on rays {(~dec_ok).any(1).nonzero().reshape(-1)[:8].tolist()}"
                  f" (first element {(~dec_ok).nonzero()[:1].tolist()})")
        sig_s = sig_cat.gather(1, perm)
        da = decode(allc, NT)
        fv = f32('feature_volume').reshape(R, NT, 3)
        rep.exact('feature_volume', bool((fv.reshape(-1, 3)[~da['inb']] == 0).all()), "a filtered sample's colour is not 0")
        rep.cmp('feature_volume', fv, da['rgb'], da['rgb_scale'], DEC_ULPS, 3 * NT, M)
        col_s, ecol_s = fv.double(), torch.zeros(R, NT, 3, dtype=torch.float64)
    else:
        # no merged outputs: the reference sorts itself (stable).  Two samples at nearly equal depth lie at nearly the same point: the
        # composite is continuous under their swap
        perm = torch.sort(z_cat, dim=1, stable=True).indices
        zs, ezs, sig_s = z_cat.gather(1, perm), ez_cat.gather(1, perm), sig_cat.gather(1, perm)
        col = torch.cat([dc['rgb'].reshape(R, S, 3), df['rgb'].reshape(R, NI, 3)], 1)
        ecol = torch.cat([dc['rgb_scale'].reshape(R, S, 3), df['rgb_scale'].reshape(R, NI, 3)], 1) * DEC_ULPS
        p3 = perm[..., None].expand(-1, -1, 3)
        col_s, ecol_s = col.gather(1, p3), ecol.gather(1, p3)
    # ---- final march
    mf = march(zs, ezs, sig_s, col_s, ecol_s)
    if out.get('weights') is not None:
        rep.cmp('weights', f32('weights'), mf['w'], mf['ew'] / STAGE_ULPS, STAGE_ULPS, NT - 1, M)
    ws, ews = mf['wsum'], mf['ewsum']
    acc, eacc = mf['rgb'], mf['ergb']
    if inp.get('white_back', True):
        bg = (1 - ws)[:, None]
        eacc = eacc + ews[:, None] + 0.5 * bg.abs() + 0.5 * (acc + bg).abs()
        acc = acc + bg
    img, eimg = acc * 2 - 1, 2 * eacc + 0.5 * (acc * 2 - 1).abs()
    rgb_k = f32('rgb').reshape(V, 3, M).permute(0, 2, 1).reshape(R, 3)
    rep.cmp('rgb', rgb_k, img, eimg / STAGE_ULPS, STAGE_ULPS, 3, M)
    rep.cmp('wsum', f32('wsum'), ws, ews / STAGE_ULPS, STAGE_ULPS, 1, M)
    if out.get('visibility') is not None:
        rep.cmp('visibility', f32('visibility'), mf['vis'], mf['evis'] / STAGE_ULPS, STAGE_ULPS, 1, M)
    # depth: nan_to_num(inf), then the clamp to [min, max] of ALL sample depths of the ray's call group (ray_marcher.py:57-61)
    dep = torch.nan_to_num(mf['depth'], nan=math.inf)
    grp = (torch.arange(R) // (M * vpc))
    lo_g = torch.stack([zs[grp == g].min() for g in range(int(grp.max()) + 1)])
    hi_g = torch.stack([zs[grp == g].max() for g in range(int(grp.max()) + 1)])
    dref = torch.minimum(torch.maximum(dep, lo_g[grp]), hi_g[grp])
    edep = mf['edepth'] + ezs.max()
    rep.cmp('depth', f32('depth'), dref, edep / STAGE_ULPS, STAGE_ULPS, 1, M)
    return rep


def check_query(inp, pts, sigma, rgb, kernel='query_points_kernel'):
    """ln3d_query_points: decoder at the given points, no bbox filter, plane set 0."""
    rep = Report(kernel)
    dd = decoder(inp['planes'][0], pts, inp['dec'], inp['box_warp'], None)
    P = pts.shape[0]
    rep.cmp('query_sigma', sigma, dd['sigma'], dd['sigma_scale'], DEC_ULPS, 1, P)
    rep.cmp('query_rgb', rgb, dd['rgb'], dd['rgb_scale'], DEC_ULPS, 3, P)
    return rep


# ---------------------------------------------------------------- scenes (inputs only; shared by the CPU calibration and the GPU cases)
def make_decoder(seed, sigma_bias=0.0, hidden_gain=1.0):
    g = torch.Generator().manual_seed(1000 + seed)
    w0 = torch.randn(64, 32, generator=g) * hidden_gain
    b0 = torch.randn(64, generator=g) * 0.5
    w1 = torch.randn(4, 64, generator=g)
    b1 = torch.randn(4, generator=g) * 0.5
    b1[0] += sigma_bias
    return (w0, b0, w1, b1)


def orbit_rays(V, M, seed, radius=1.8, spread=0.35, inside=False):
    """explicit rays [V, M, 3]: origins on a sphere (or inside the box), unit directions towards points scattered round the origin"""
    g = torch.Generator().manual_seed(2000 + seed)
    o = torch.nn.functional.normalize(torch.randn(V, 1, 3, generator=g), dim=-1) * radius * (1 + 0.3 * torch.rand(V, 1, 1, generator=g))
    o = o.expand(V, M, 3).clone()
    if inside:
        o = (torch.rand(V, M, 3, generator=g) - 0.5) * 0.6
    tgt = (torch.rand(V, M, 3, generator=g) - 0.5) * 2 * spread
    d = torch.nn.functional.normalize(tgt - o + (1e-3 if inside else 0.0), dim=-1)
    return o.contiguous(), d.contiguous()


def make_scene(seed, V, M=None, res=None, S=64, NI=64, H=16, W=24, NP=1, plane_scale=2.0, sigma_bias=0.0, hidden_gain=1.0, box_warp=0.9,
               bbox=(-0.45, 0.45), white_back=True, views_per_call=0, numeric=None, rays=None, cams=None, plane_index=None,
               jitter_edge=False):
    """inputs of one ln3d_render_triplane call (CPU f32 tensors)"""
    g = torch.Generator().manual_seed(seed)
    inp = dict(S=S, NI=NI, box_warp=box_warp, bbox=bbox, white_back=white_back, views_per_call=views_per_call, numeric=numeric, H=H, W=W)
    inp['planes'] = torch.randn(NP, 3, H, W, 32, generator=g) * plane_scale
    inp['dec'] = make_decoder(seed, sigma_bias, hidden_gain)
    if cams is not None:
        inp['cams'], inp['res'], M = cams.float(), res, res * res
        inp['ray_o'] = inp['ray_d'] = None
    else:
        inp['ray_o'], inp['ray_d'] = rays if rays is not None else orbit_rays(V, M, seed)
        inp['cams'], inp['res'] = None, 0
    inp['V'], inp['M'] = V, M
    inp['plane_index'] = (torch.arange(V) * 5 % NP).int() if plane_index is None else torch.as_tensor(plane_index).int()
    inp['jitter'] = torch.rand(V, M, S, generator=g)
    inp['u_fine'] = torch.rand(V * M, NI, generator=g)
    if jitter_edge:                     # the ends of [0, 1): columns of 0 and of 1 - 2^-24, bit-equal uniforms (bit-equal fine depths)
        top = 1.0 - 2.0 ** -24
        inp['jitter'][..., 0::7] = 0.0
        inp['jitter'][..., 3::7] = top
        inp['u_fine'][:, 0] = 0.0
        inp['u_fine'][:, 1] = top
        inp['u_fine'][:, 2] = top
        inp['u_fine'][:, 5] = inp['u_fine'][:, 4]
    return inp


def oracle_outputs(inp):
    """the project's fp32 oracle (oracle/render.py, fp32 torch, a third implementation with its own summation orders) in the layout of
    the kernel's outputs - the stand-in the bounds are calibrated on without a GPU"""
    from oracle import render as orender
    V, M, S, NI = inp['V'], inp['M'], inp['S'], inp['NI']
    if inp['cams'] is not None:
        o, d = orender.make_rays(inp['cams'], inp['res'])
    else:
        o, d = inp['ray_o'], inp['ray_d']
    opts = dict(depth_resolution=S, depth_resolution_importance=NI, box_warp=inp['box_warp'], white_back=inp['white_back'],
                clamp_mode='softplus', disparity_space_sampling=False, filter_out_of_bbox=inp['bbox'] is not None)
    if inp['bbox'] is not None:
        opts.update(sampler_bbox_min=inp['bbox'][0], sampler_bbox_max=inp['bbox'][1])
    opts['ray_start'], opts['ray_end'] = ('auto', 'auto') if inp['numeric'] is None else inp['numeric']
    planes = inp['planes'][inp['plane_index'].long()].permute(0, 1, 4, 2, 3).contiguous()          # [V, 3, C, H, W]
    sd = {'net.0.weight': inp['dec'][0], 'net.0.bias': inp['dec'][1], 'net.2.weight': inp['dec'][2], 'net.2.bias': inp['dec'][3]}
    vpc = inp['views_per_call']
    vpc = V if (vpc <= 0 or vpc > V) else vpc
    parts = []
    for g0 in range(0, V, vpc):
        sl = slice(g0, g0 + vpc)
        nv = len(range(V)[sl])
        parts.append(orender.render(planes[sl], sd, o[sl], d[sl], inp['jitter'][sl].reshape(nv, M, S, 1),
                                    inp['u_fine'].reshape(V, M, NI)[sl].reshape(nv * M, NI), opts))
    cat = lambda k: torch.cat([p[k] for p in parts])
    a, b = orender.ray_limits_box(o, d, inp['box_warp'])
    return dict(ray_limits=torch.cat([a, b], -1).reshape(-1, 2), rgb=cat('rgb').permute(0, 2, 1).contiguous(), depth=cat('depth').reshape(V, M),
                wsum=cat('weights_sum').reshape(V, M), visibility=cat('visibility').reshape(V, M), coarse_coords=cat('coarse_coords'),
                coarse_sigma=cat('coarse_densities').reshape(V, M, S), fine_depths=cat('fine_depths').reshape(V, M, NI),
                fine_coords=cat('fine_coords'), fine_sigma=cat('fine_densities').reshape(V, M, NI), weights=cat('weights').reshape(V, M, -1),
                all_coords=cat('all_coords'), feature_volume=cat('feature_volume'), coarse_depths=cat('coarse_depths').reshape(V, M, S))
