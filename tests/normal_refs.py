"""Float64 restatement of the density gradient and the surface points behind include/ln3d_normals.h (csrc/render.hip:
ln3d_query_points_grad, ln3d_surface_normals), with a per-point error scale, and an fp32 torch restatement of the same formula that the
GPU bound is calibrated on without a GPU (tests/test_normals_cpu.py).

The field: g = 2 / box_warp * p; planes (x,y) (y,z) (z,x); ix = ((gx + 1) W - 1) / 2; bilinear taps with zero padding; f = mean over the
planes; h = W0 f / sqrt 32 + b0; sigma = w1[0] . softplus(h) / sqrt 64 + b1[0] (softplus: beta 1, threshold 20).

The reference is written Jacobian-first (d f / d p [P, 32, 3], then the chain), the kernel runs it adjoint-first (d sigma / d f, then one
dot product per tap): two different evaluation orders of the same derivative.
"""
import math

import numpy as np
import torch

F32_EPS = 2.0 ** -23
PLANE_AXES = ((0, 1), (1, 2), (2, 0))


def _d(t):
    return torch.as_tensor(t).detach().double().cpu()


def _texel_coords(pts, H, W, box_warp, dtype=torch.float64):
    """the six projected texel coordinates [P, 3 planes, 2 (ix, iy)] of fp32 points, evaluated in `dtype`"""
    p = torch.as_tensor(pts).detach().float().cpu().to(dtype)
    cs = torch.tensor(2.0 / float(np.float32(box_warp)), dtype=torch.float64).to(dtype)         # the kernel's (float)(2.0 / box_warp)
    g = p * cs
    out = []
    for a, b in PLANE_AXES:
        out.append(torch.stack([((g[:, a] + 1) * W - 1) / 2, ((g[:, b] + 1) * H - 1) / 2], -1))
    return torch.stack(out, 1)


def texel_margin(pts, H, W, box_warp):
    """[P]: the smallest distance, in texels, of any of the six projected coordinates from an integer - where a coordinate crosses a texel
    centre the bilinear piece changes and the gradient jumps."""
    t = _texel_coords(pts, H, W, box_warp)
    return (t - torch.round(t)).abs().reshape(t.shape[0], -1).min(-1).values


def sigma_and_grad(planes, pts, dec, box_warp):
    """planes [3, H, W, 32] f32 or f16 (values read exactly), pts f32 [P, 3], dec = (w0 [64,32], b0 [64], w1 [>=1,64], b1 [>=1]) ->
    dict(sigma [P], sigma_scale [P], grad [P,3] = d sigma / d p in world units, scale [P,3], all_padding [P]).

    scale: the sum of the absolute values of the terms of the chain, the error budget of an fp32 evaluation in any order in units of
    2^-23 (render_refs.decoder's manner): every tap term |texel| |d weight| |d sigma / d f|, where |d sigma / d f| is taken with absolute
    weights and includes what an error of h (itself sum |W0| |f| + |b0|) does to sigmoid(h); plus the rounding of the texel coordinate of
    the OTHER axis (e_iy texels, 5 roundings on the way from p) times the mixed difference of the four taps."""
    pl = _d(planes)
    _, H, W, C = pl.shape
    P = torch.as_tensor(pts).shape[0]
    cs = 2.0 / float(np.float32(box_warp))
    g = torch.as_tensor(pts).detach().float().cpu().double() * cs
    tc = _texel_coords(pts, H, W, box_warp)
    feat = torch.zeros(P, C, dtype=torch.float64)
    afeat = torch.zeros(P, C, dtype=torch.float64)
    J = torch.zeros(P, C, 3, dtype=torch.float64)            # d feat / d p
    aJ = torch.zeros(P, C, 3, dtype=torch.float64)           # its terms in absolute value (+ the coordinate-rounding term)
    any_tap = torch.zeros(P, dtype=torch.bool)
    for k, (a, b) in enumerate(PLANE_AXES):
        ix, iy = tc[:, k, 0], tc[:, k, 1]
        eix = 0.5 * W * (g[:, a].abs() + (g[:, a] + 1).abs()) + 0.25 * (2 * ix).abs()
        eiy = 0.5 * H * (g[:, b].abs() + (g[:, b] + 1).abs()) + 0.25 * (2 * iy).abs()
        x0, y0 = torch.floor(ix), torch.floor(iy)
        wx, wy = (ix - x0)[:, None], (iy - y0)[:, None]
        flat = pl[k].reshape(H * W, C)

        def tap(dx, dy):
            xi, yi = (x0 + dx).long(), (y0 + dy).long()
            ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            any_tap.__ior__(ok)
            return flat[yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)] * ok[:, None]
        v00, v01, v10, v11 = tap(0, 0), tap(1, 0), tap(0, 1), tap(1, 1)
        feat += v00 * (1 - wx) * (1 - wy) + v01 * wx * (1 - wy) + v10 * (1 - wx) * wy + v11 * wx * wy
        afeat += v00.abs() * (1 - wx) * (1 - wy) + v01.abs() * wx * (1 - wy) + v10.abs() * (1 - wx) * wy + v11.abs() * wx * wy
        dfx = (v01 - v00) * (1 - wy) + (v11 - v10) * wy
        dfy = (v10 - v00) * (1 - wx) + (v11 - v01) * wx
        mixed = (v11 - v10 - v01 + v00).abs()
        adfx = (v01.abs() + v00.abs()) * (1 - wy) + (v11.abs() + v10.abs()) * wy + mixed * eiy[:, None]
        adfy = (v10.abs() + v00.abs()) * (1 - wx) + (v11.abs() + v01.abs()) * wx + mixed * eix[:, None]
        J[:, :, a] += dfx * (cs * W / 2)
        J[:, :, b] += dfy * (cs * H / 2)
        aJ[:, :, a] += adfx * (cs * W / 2)
        aJ[:, :, b] += adfy * (cs * H / 2)
    feat, afeat, J, aJ = feat / 3, afeat / 3, J / 3, aJ / 3
    w0, b0, w1, b1 = (_d(t) for t in dec)
    W0, w1r = w0 / math.sqrt(w0.shape[1]), w1[0] / math.sqrt(w1.shape[1])
    h = feat @ W0.t() + b0
    ah = afeat @ W0.abs().t() + b0.abs()
    lin = h > 20
    sp = torch.where(lin, h, torch.log1p(torch.exp(h.clamp(max=20))))
    sg = torch.sigmoid(h)
    slope = torch.where(lin, torch.ones_like(h), sg)
    dslope = torch.where(lin, torch.zeros_like(h), sg * (1 - sg))
    sigma = sp @ w1r + b1[0]
    q = (slope * w1r) @ W0                                    # d sigma / d feat [P, 32]
    aq = ((slope + dslope * ah) * w1r.abs()) @ W0.abs()
    grad = torch.einsum('pc,pca->pa', q, J)
    scale = torch.einsum('pc,pca->pa', aq, aJ)
    sigma_scale = sp.abs() @ w1r.abs() + b1[0].abs() + (slope * ah) @ w1r.abs()            # the terms of sigma itself, in absolute value
    return dict(sigma=sigma, sigma_scale=sigma_scale, grad=grad, scale=scale, all_padding=~any_tap)


def surface_points(o, d, depth, wsum):
    """o, d [..., 3], depth, wsum [...] (the renderer's fp32 outputs, read exactly) -> (p, scale) [..., 3] in float64: p = o + (depth / wsum) d.
    scale in units of 2^-23: render_refs.positions' two roundings (1/2 ulp of |t d|, 1/2 ulp of |p|) plus the division (1/2 ulp of t,
    carried by |d|)."""
    o, d, depth, wsum = _d(o), _d(d), _d(depth), _d(wsum)
    t = (depth / wsum)[..., None]
    p = o + t * d
    return p, 0.5 * (t * d).abs() + 0.5 * p.abs() + 0.5 * t.abs() * d.abs()


def unit_outward(grad):
    """float64 -g / |g|, 0 where g = 0"""
    n = grad.norm(dim=-1, keepdim=True)
    return torch.where(n > 0, -grad / n.clamp(min=1e-300), torch.zeros_like(grad))


def normal_bound(grad, gscale, ulps):
    """per-component bound of n = -g / |g| given |delta g_b| <= ulps * 2^-23 * gscale_b: |d n_a / d g_b| = |delta_ab - n_a n_b| / |g|, plus 4 ulp
    of 1 for the normalisation itself (a scaling, three squares, two sums, a square root, a division, a product: <= 8 half-ulps)."""
    nrm = grad.norm(dim=-1, keepdim=True).clamp(min=1e-300)
    n = grad / nrm
    jac = (torch.eye(3, dtype=torch.float64) - n[..., :, None] * n[..., None, :]).abs() / nrm[..., None]
    return torch.einsum('...ab,...b->...a', jac, ulps * F32_EPS * gscale) + 4 * F32_EPS


# ---------------------------------------------------------------- the fp32 stand-in (CPU calibration) and its seeded faults
FAULTS = ('sign', 'no_coord_scale', 'no_plane_mean', 'no_linear_branch', 'border_clamped')


def grad_f32(planes, pts, dec, box_warp, fault=None):
    """The same derivative in fp32 torch, adjoint-first with its own summation order (torch's matmul / sum reductions): the stand-in for the
    kernel that the bound is calibrated on.  fault: one of FAULTS -
      sign             the gradient comes out negated
      no_coord_scale   d g / d p = 2 / box_warp left out
      no_plane_mean    the 1/3 of the mean over the planes left out of the derivative
      no_linear_branch hidden units on softplus' linear branch (h > 20, slope 1) contribute nothing
      border_clamped   an out-of-range tap reads the clamped border texel instead of 0"""
    pl = torch.as_tensor(planes).detach().cpu().float()
    _, H, W, C = pl.shape
    p = torch.as_tensor(pts).detach().float().cpu()
    cs = torch.tensor(2.0 / float(np.float32(box_warp))).float()
    g = p * cs
    w0, b0, w1, b1 = (torch.as_tensor(t).detach().float().cpu() for t in dec)
    W0, w1r = w0 * torch.tensor(1.0 / math.sqrt(32.0)).float(), w1[0] * 0.125
    taps, feat = [], torch.zeros(p.shape[0], C)
    for k, (a, b) in enumerate(PLANE_AXES):
        ix, iy = ((g[:, a] + 1) * W - 1) * 0.5, ((g[:, b] + 1) * H - 1) * 0.5
        x0, y0 = torch.floor(ix), torch.floor(iy)
        wx1, wy1, wx0, wy0 = ix - x0, iy - y0, x0 + 1 - ix, y0 + 1 - iy
        flat = pl[k].reshape(H * W, C)
        vs = []
        for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
            xi, yi = (x0 + dx).long(), (y0 + dy).long()
            ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            v = flat[yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)]
            vs.append(v if fault == 'border_clamped' else v * ok[:, None])
        feat = feat + (((vs[0] * (wx0 * wy0)[:, None] + vs[1] * (wx1 * wy0)[:, None]) + vs[2] * (wx0 * wy1)[:, None]) + vs[3] * (wx1 * wy1)[:, None])
        taps.append((vs, wx0, wx1, wy0, wy1))
    feat = feat * torch.tensor(1.0 / 3.0).float()
    h = feat @ W0.t() + b0
    lin = h > 20
    slope = torch.where(lin, torch.zeros_like(h) if fault == 'no_linear_branch' else torch.ones_like(h), torch.sigmoid(h))
    q = (slope * w1r) @ W0
    grad = torch.zeros(p.shape[0], 3)
    third = 1.0 if fault == 'no_plane_mean' else torch.tensor(1.0 / 3.0).float()
    csg = 1.0 if fault == 'no_coord_scale' else cs
    for k, (a, b) in enumerate(PLANE_AXES):
        vs, wx0, wx1, wy0, wy1 = taps[k]
        t = [(v * q).sum(-1) for v in vs]
        grad[:, a] += ((t[1] - t[0]) * wy0 + (t[3] - t[2]) * wy1) * (csg * W * 0.5 * third)
        grad[:, b] += ((t[2] - t[0]) * wx0 + (t[3] - t[1]) * wx1) * (csg * H * 0.5 * third)
    return -grad if fault == 'sign' else grad


def sample_points(n, seed, H, W, box_warp, margin=0.02, spread=0.75):
    """n fp32 points with texel_margin >= margin, drawn uniformly from a cube of side 2 * spread * box_warp: about a third inside the box,
    the rest with some or all taps in the padding (reject-sampling on the reference alone)."""
    g = torch.Generator().manual_seed(seed)
    out, have = [], 0
    while have < n:
        p = ((torch.rand(4 * n + 64, 3, generator=g) - 0.5) * 2 * spread * box_warp).float()
        p = p[texel_margin(p, H, W, box_warp) >= margin]
        out.append(p)
        have += p.shape[0]
    return torch.cat(out)[:n].contiguous()
