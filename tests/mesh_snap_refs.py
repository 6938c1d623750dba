"""Float64 restatement of the level-set snapping of include/ln3d_meshsnap.h (csrc/render.hip: ln3d_snap_points) on top of
normal_refs.sigma_and_grad, first-order bounds for what an fp32 evaluation of the same loop may return, an fp32 torch stand-in of the loop
with seeded faults, and the checks that tests/test_mesh_snap_gpu.py applies to the kernel and tests/test_mesh_snap_cpu.py to the stand-in.

The loop (the header's, per point):
    p = in; (s, g) = field(p); r = s - level; f = 1; evals = 1
    repeat at most iters times:
        g2 = |g|^2;  stalled when in, r or g2 is not finite or g2 == 0;  converged when |r| <= tol
        len = |r| / sqrt(g2); a = f min(1, max_step / len); c = p - (a r / g2) g
        not |c - in| <= max_dist: f /= 2, next iteration (no evaluation)
        (sc, gc) = field(c); rc = sc - level; evals += 1;  |rc| < |r|: p, r, g, f = c, rc, gc, 1  else f /= 2
    state = 0 if |r| <= tol, else 2 if stalled, else 1

The float64 loop evaluates the field where the kernel can: every candidate is rounded to fp32 before it is evaluated and becomes the
iterate as rounded (normal_refs.sigma_and_grad reads fp32 points), so `points` of the reference are fp32 values and that one rounding is
part of the bound.

Bounds, first order.  With dr the bound of r and dg_b that of g_b at the iterate p (whose own position is known to e_p, 0 at the input):
    dr   = SIGMA_BOUND_ULPS 2^-23 sigma_scale + 2^-23 |r| + sum_b |g_b| e_p,b
    dg_b = GRAD_BOUND_ULPS 2^-23 scale_b
    unclamped step  c_a = p_a - f r g_a / |g|^2:   dc_a = f (|g_a| / |g|^2 dr + |r| sum_b |delta_ab - 2 n_a n_b| / |g|^2 dg_b)
    clamped step    c_a = p_a - f max_step sign(r) n_a:   dc_a = f max_step sum_b |delta_ab - n_a n_b| / |g| dg_b
    plus e_p,a, plus OPS_ULPS 2^-23 |c_a - p_a| for the ten-odd roundings between g and the step (three squares, two sums, a root, three
    divisions, a minimum, three products: each half an ulp of the step) and 2 * 2^-23 |c_a| for the subtraction and the reference's own
    rounding of c to fp32.  Within 1e-4 (relative) of the clamp threshold the larger of the two is taken.
A decision is IN DOUBT when the two sides of its comparison are closer than their bounds: | |r| - tol | <= dr; | |c - in| - max_dist | <=
sum_a |d_a| / |d| dc_a + 4 * 2^-23 |d|; | |rc| - |r| | <= drc + dr, where drc takes e_p = dc (the kernel's candidate is anywhere in the
box around the reference's).  A point is also left out when any point the reference evaluates for it lies within TEXEL_MARGIN of a texel
centre (normal_refs.texel_margin): across it the gradient jumps and the two loops may take different pieces.
After an accepted step e_p = dc.  What the change of the gradient over e_p adds to dg is of second order (|Hessian| e_p, with e_p of the
order of 1e-7 of the box) and is left out, as first order says; the 4 x of the two calibrated constants is the headroom it lives in.
"""
import functools
import math

import numpy as np
import torch

import normal_refs as nr
import render_refs as rr
from test_normals_cpu import GRAD_BOUND_ULPS

F32_EPS = nr.F32_EPS
TEXEL_MARGIN = 1e-3
OPS_ULPS = 8.0
# sigma of the all-fp32 path (ln3d_query_points_grad's, not the bf16-split query's that render_refs.DEC_ULPS is sized for), by the
# project's rule: 4 x the worst error of the fp32 torch stand-in (sigma_f32) against float64 in units of 2^-23 * sigma_scale, over
# calibration_cases() - scenes of the family the GPU test draws from (plane_scale 2, sigma_bias 6, hidden_gain 1), f32 and f16 texels,
# points inside, across and beyond the box.  Produced by `python tests/test_mesh_snap_cpu.py`, which printed
# MEASURED_SIGMA_F32_ULPS = 0.9674   SIGMA_BOUND_ULPS = 3.87.  (With hidden_gain 12 - units on softplus' linear branch, which no scene of
# these tests has - the stand-in itself reaches 6.6: sigma_scale is not sized for that regime, and this constant is not either.)
MEASURED_SIGMA_F32_ULPS = 0.9674
SIGMA_BOUND_ULPS = 4.0 * MEASURED_SIGMA_F32_ULPS

FAULTS = ('sign', 'norm_for_square', 'no_step_clamp', 'no_max_dist', 'accept_worse', 'f_not_reset', 'no_tol')


def calibration_cases():
    """(planes [3,H,W,32], pts, dec) of the sigma calibration"""
    for seed, half in ((11, False), (12, False), (13, True), (14, True)):
        inp = rr.make_scene(seed, 1, M=1, H=16, W=24, NP=1, plane_scale=2.0, sigma_bias=6.0)
        planes = inp['planes'][0]
        yield (planes.half() if half else planes), nr.sample_points(4096, seed, 16, 24, 0.9, 0.02), inp['dec']


# ---------------------------------------------------------------- the field
def field64(planes, dec, box_warp):
    def f(pts):
        d = nr.sigma_and_grad(planes, pts, dec, box_warp)
        return d['sigma'], d['grad'], d['sigma_scale'], d['scale']
    return f


def sigma_f32(planes, pts, dec, box_warp):
    """sigma of normal_refs.grad_f32's forward pass: fp32 torch, its own summation orders"""
    pl = torch.as_tensor(planes).detach().cpu().float()
    _, H, W, C = pl.shape
    p = torch.as_tensor(pts).detach().float().cpu()
    g = p * torch.tensor(2.0 / float(np.float32(box_warp))).float()
    w0, b0, w1, b1 = (torch.as_tensor(t).detach().float().cpu() for t in dec)
    W0, w1r = w0 * torch.tensor(1.0 / math.sqrt(32.0)).float(), w1[0] * 0.125
    feat = torch.zeros(p.shape[0], C)
    for k, (a, b) in enumerate(nr.PLANE_AXES):
        ix, iy = ((g[:, a] + 1) * W - 1) * 0.5, ((g[:, b] + 1) * H - 1) * 0.5
        x0, y0 = torch.floor(ix), torch.floor(iy)
        wx1, wy1, wx0, wy0 = ix - x0, iy - y0, x0 + 1 - ix, y0 + 1 - iy
        flat = pl[k].reshape(H * W, C)
        vs = []
        for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
            xi, yi = (x0 + dx).long(), (y0 + dy).long()
            ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            vs.append(flat[yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)] * ok[:, None])
        feat = feat + (((vs[0] * (wx0 * wy0)[:, None] + vs[1] * (wx1 * wy0)[:, None]) + vs[2] * (wx0 * wy1)[:, None]) + vs[3] * (wx1 * wy1)[:, None])
    feat = feat * torch.tensor(1.0 / 3.0).float()
    h = feat @ W0.t() + b0
    return torch.nn.functional.softplus(h, beta=1, threshold=20) @ w1r + b1[0]


def field_f32(planes, dec, box_warp):
    def f(pts):
        return sigma_f32(planes, pts, dec, box_warp), nr.grad_f32(planes, pts, dec, box_warp), None, None
    return f


# ---------------------------------------------------------------- the loop
def _f32(x):
    return torch.as_tensor(float(np.float32(x)))


def run_loop(field, pts, level, iters, tol, max_step, max_dist, dtype=torch.float64, fault=None, margin=None):
    """The loop over all points at once in `dtype` (float64: the reference, with bounds and doubts; float32: the stand-in, every operation
    rounded once as the kernel's).  field(pts fp32 [P,3]) -> (sigma, grad, sigma_scale, scale).  margin(pts) -> [P] texel margin, or None.
    -> dict(points [P,3] fp32, residual, state, evals, initial (|r| of the input), and for float64: cand [P,3] / cand_bound [P,3] / accept0 /
    evaluated0 of the FIRST iteration, doubt [P] (any decision in doubt or an evaluated point too close to a texel centre), doubt1 (the same
    for the first iteration only), n_worse / n_far [P] (rejections of either kind))."""
    ref = dtype == torch.float64
    x0 = torch.as_tensor(pts).detach().float().cpu()
    P = x0.shape[0]
    inp = x0.to(dtype)
    lv, tl, ms, md = (_f32(v).to(dtype) for v in (level, tol, max_step, max_dist))
    z = lambda *s, **k: torch.zeros(*s, dtype=dtype, **k)                                     # noqa: E731
    s, g, ss, gs = field(x0)
    p, g = inp.clone(), g.to(dtype)
    r = s.to(dtype) - lv
    f = torch.ones(P, dtype=dtype)
    evals = torch.ones(P, dtype=torch.int32)
    active = torch.ones(P, dtype=torch.bool)
    stalled = torch.zeros(P, dtype=torch.bool)
    initial = r.abs().clone()
    out = dict(initial=initial)
    if ref:
        e_p = z(P, 3)
        doubt = (margin(x0) < TEXEL_MARGIN) if margin is not None else torch.zeros(P, dtype=torch.bool)
        n_worse, n_far = torch.zeros(P, dtype=torch.int32), torch.zeros(P, dtype=torch.int32)
        ss, gs = ss.clone(), gs.clone()
        why = {k: torch.zeros(P, dtype=torch.bool) for k in ('tol', 'max_dist', 'accept', 'texel')}
        why['texel'] |= doubt
    for it in range(iters):
        g2 = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        stall = active & ~(torch.isfinite(inp).all(-1) & torch.isfinite(r) & torch.isfinite(g2) & (g2 != 0))
        stalled |= stall
        active = active & ~stall
        if ref:
            dr = SIGMA_BOUND_ULPS * F32_EPS * ss + F32_EPS * r.abs() + (g.abs() * e_p).sum(-1)
            dg = GRAD_BOUND_ULPS * F32_EPS * gs
            why['tol'] |= active & ((r.abs() - tl).abs() <= dr)
        conv = active & (r.abs() <= tl) if fault != 'no_tol' else torch.zeros(P, dtype=torch.bool)
        active = active & ~conv
        safe = torch.where(active, g2, torch.ones_like(g2))
        rs = torch.where(active, r, torch.ones_like(r))
        root = torch.sqrt(safe)
        ln = rs.abs() / root
        ratio = torch.where(ln > 0, ms / ln, torch.full_like(ln, float('inf')))
        clamped = ratio < 1
        al = f * (torch.ones_like(ratio) if fault == 'no_step_clamp' else torch.minimum(torch.ones_like(ratio), ratio))
        t = (al * rs) / (root if fault == 'norm_for_square' else safe)
        step = t[:, None] * torch.where(active[:, None], g, torch.zeros_like(g))
        c = p + step if fault == 'sign' else p - step
        if ref:
            c = c.float().to(dtype)                                                         # evaluated, and kept, as the fp32 point it is
        d = c - inp
        dist = torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        far = active & ~(dist <= md)
        if fault == 'no_max_dist':
            far = torch.zeros(P, dtype=torch.bool)
        ev = active & ~far
        if ref:
            n = g / root[:, None]
            eye = torch.eye(3, dtype=dtype)
            ju = (eye - 2 * n[:, :, None] * n[:, None, :]).abs() / safe[:, None, None]
            jc = (eye - n[:, :, None] * n[:, None, :]).abs() / root[:, None, None]
            bu = al[:, None] * (g.abs() / safe[:, None] * dr[:, None] + rs.abs()[:, None] * torch.einsum('pab,pb->pa', ju, dg))
            bc = (f * ms)[:, None] * torch.einsum('pab,pb->pa', jc, dg)
            near = (ratio - 1).abs() < 1e-4
            dc = torch.where(near[:, None], torch.maximum(bu, bc), torch.where(clamped[:, None], bc, bu))
            dc = dc + e_p + OPS_ULPS * F32_EPS * step.abs() + 2 * F32_EPS * c.abs()
            ddist = (d.abs() / dist.clamp(min=1e-300)[:, None] * dc).sum(-1) + 4 * F32_EPS * dist
            why['max_dist'] |= active & ((dist - md).abs() <= ddist)
            n_far += far.int()
        sc, gc, ssc, gsc = field(torch.where(ev[:, None], c, p).float())
        rc = sc.to(dtype) - lv
        gc = gc.to(dtype)
        better = ev & ((rc.abs() < r.abs()) if fault != 'accept_worse' else torch.ones(P, dtype=torch.bool))
        if ref:
            drc = SIGMA_BOUND_ULPS * F32_EPS * ssc + F32_EPS * rc.abs() + (gc.abs() * dc).sum(-1)
            why['accept'] |= ev & ((rc.abs() - r.abs()).abs() <= drc + dr)
            if margin is not None:
                why['texel'] |= ev & (margin(c.float()) < TEXEL_MARGIN)
            doubt = why['tol'] | why['max_dist'] | why['accept'] | why['texel']
            n_worse += (ev & ~better).int()
            if it == 0:
                out.update(cand=c.clone(), cand_bound=dc.clone(), accept0=better.clone(), evaluated0=ev.clone(), doubt1=doubt.clone())
            e_p = torch.where(better[:, None], dc, e_p)
            ss, gs = torch.where(better, ssc, ss), torch.where(better[:, None], gsc, gs)
        evals += ev.int()
        b3 = better[:, None]
        p, g = torch.where(b3, c, p), torch.where(b3, gc, g)
        r = torch.where(better, rc, r)
        half = active & ~better
        f = torch.where(half, f * 0.5, f if fault == 'f_not_reset' else torch.where(better, torch.ones_like(f), f))
    state = torch.where(r.abs() <= tl, 0, torch.where(stalled, 2, 1)).int()
    out.update(points=p.float(), residual=r, state=state, evals=evals, stalled=stalled)
    if ref:
        if iters == 0:
            doubt1 = doubt
            out.update(doubt1=doubt1)
        # the final |r| <= tol decides the state: it is a decision like the others
        dr = SIGMA_BOUND_ULPS * F32_EPS * ss + F32_EPS * r.abs() + (g.abs() * e_p).sum(-1)
        why['tol'] |= torch.isfinite(r) & ((r.abs() - tl).abs() <= dr)
        out.update(doubt=doubt | why['tol'], why=why, n_worse=n_worse, n_far=n_far)
    return out


# ---------------------------------------------------------------- the test's inputs
def crossings(planes, dec, box_warp, level, G=12, lo=-0.45, hi=0.45):
    """the points where the float64 field crosses `level` along the x, y and z edges of a G^3 grid over the box (linear interpolation of the
    two samples, as marching cubes places its vertices) [N,3] float64, and the cell size"""
    ax = torch.linspace(lo, hi, G, dtype=torch.float64)
    pts = torch.stack(torch.meshgrid(ax, ax, ax, indexing='ij'), -1)
    s = nr.sigma_and_grad(planes, pts.reshape(-1, 3).float(), dec, box_warp)['sigma'].reshape(G, G, G) - level
    out = []
    for axis in range(3):
        a, b = s.narrow(axis, 0, G - 1), s.narrow(axis, 1, G - 1)
        pa, pb = pts.narrow(axis, 0, G - 1), pts.narrow(axis, 1, G - 1)
        hit = (a < 0) != (b < 0)
        t = (a / (a - b))[hit][:, None]
        out.append(pa[hit] + t * (pb[hit] - pa[hit]))
    return torch.cat(out), (hi - lo) / (G - 1)


def start_points(planes, dec, box_warp, level, P, seed, H, W, far_share=0.15):
    """P fp32 start points: level-set crossings of a 12^3 grid displaced by up to a quarter cell per axis (cycled when there are fewer than
    needed, each copy with its own displacement), and a share of normal_refs.sample_points - far from the surface, two thirds of them outside
    the box.  -> (points [P,3] fp32, cell)"""
    g = torch.Generator().manual_seed(seed)
    x, cell = crossings(planes, dec, box_warp, level)
    assert x.shape[0] >= 32, "the scene has no surface at this level"
    n_far = int(round(P * far_share)) if P >= 8 else 0
    n = P - n_far
    idx = torch.randperm(x.shape[0], generator=g)[torch.arange(n) % x.shape[0]]
    near = x[idx] + (torch.rand(n, 3, generator=g, dtype=torch.float64) - 0.5) * 0.5 * cell
    far = nr.sample_points(n_far, seed + 1, H, W, box_warp, 0.02).double() if n_far else torch.zeros(0, 3, dtype=torch.float64)
    return torch.cat([near, far]).float().contiguous(), cell


# ---------------------------------------------------------------- the cases of tests/test_mesh_snap_gpu.py (shared, computed once)
H, W, BOX = 16, 24, 0.9
SIZES = (1, 63, 64, 65, 257, 4099)
ITERS = 8
MAX_ONE_STEP_LEFT_OUT, MAX_CONTROL_LEFT_OUT = 0.05, 0.10


SEEDS = {1: 201, 63: 263, 64: 364, 65: 265, 257: 457, 4099: 4299}   # 200 + P, but for 64: there seed 264 leaves 7 of the 64 points (0.109) out of
                                                                   # the control-flow comparison by the reference alone, one point above the cap


def seed_of(P):
    return SEEDS[P]


@functools.lru_cache(maxsize=None)
def case(P):
    """the scene, the level (the median of the float64 field over the 12^3 grid, as fp32), the start points and the float64 loops of one
    size: 'one' (iters = 1) and 'full' (iters = 8) at max_dist = one cell, 'tight' (iters = 8) at a quarter cell; max_step = 0.4 cell
    (not half a cell: a halved step would then be as long as the tight max_dist to the last bit, and every such decision in doubt).
    Nobody writes to what this returns."""
    seed = seed_of(P)
    inp = rr.make_scene(seed, 3, M=1, H=H, W=W, NP=2, plane_scale=2.0, sigma_bias=6.0)
    planes, dec = inp['planes'][1].contiguous(), inp['dec']
    ax = torch.linspace(-0.45, 0.45, 12)
    grid = torch.stack(torch.meshgrid(ax, ax, ax, indexing='ij'), -1).reshape(-1, 3)
    level = float(np.float32(nr.sigma_and_grad(planes, grid, dec, BOX)['sigma'].median()))
    pts, cell = start_points(planes, dec, BOX, level, P, seed, H, W)
    c = dict(planes=planes, dec=dec, level=level, points=pts, cell=cell, tol=1e-3 * max(1.0, abs(level)), max_step=0.4 * cell,
             max_dist=cell, tight=0.25 * cell)
    f64, mg = field64(planes, dec, BOX), (lambda x: nr.texel_margin(x, H, W, BOX))
    c['one'] = run_loop(f64, pts, level, 1, c['tol'], c['max_step'], c['max_dist'], margin=mg)
    c['full'] = run_loop(f64, pts, level, ITERS, c['tol'], c['max_step'], c['max_dist'], margin=mg)
    c['tight_full'] = run_loop(f64, pts, level, ITERS, c['tol'], c['max_step'], c['tight'], margin=mg)
    return c


def run_all(c, snap, sigma_at):
    """every check of the GPU test on one case.  snap(points, iters, max_dist) -> dict(points, residual, state, evals) of the implementation
    under test; sigma_at(points) -> its sigma.  -> (failures, the outputs)"""
    pts = c['points']
    zero = snap(pts, 0, c['max_dist'])
    fails = []
    if not torch.equal(bits(zero['points']), bits(pts)) or not bool((zero['evals'] == 1).all()):
        fails.append("iters = 0 moved a point or counted more than one evaluation")
    want = sigma_at(pts).float() - _f32(c['level'])
    if not bool(((bits(want) == bits(zero['residual'].float())) | (torch.isnan(want) & torch.isnan(zero['residual'].float()))).all()):
        fails.append("iters = 0: residual is not fl(sigma - level)")
    outs = {'zero': zero}
    one = dict(snap(pts, 1, c['max_dist']), input=pts)
    fails += check_one_step(one, c['one'], MAX_ONE_STEP_LEFT_OUT)
    outs['one'] = one
    for name, md in (('full', c['max_dist']), ('tight_full', c['tight'])):
        got = dict(snap(pts, ITERS, md), input=pts, initial=zero['residual'].abs())
        fails += [f"{name}: {m}" for m in check_invariants(got, c['tol'], md, sigma_at, c['level']) + check_control(got, c[name], MAX_CONTROL_LEFT_OUT)
                  + check_convergence(got, c[name])]
        outs[name] = got
    return fails, outs


# ---------------------------------------------------------------- the checks (kernel on the GPU, stand-in on the CPU)
def bits(t):
    return torch.as_tensor(t).detach().cpu().contiguous().view(torch.int32)


def check_one_step(got, ref, max_left_out=0.05):
    """iters = 1 against the float64 loop from the same input: where nothing is in doubt, `points` is the candidate within its bound (an
    accepted step) or the input bit for bit (a rejection, a stall, a converged input), and evals is the reference's.  -> list of failures"""
    fails = []
    P = ref['points'].shape[0]
    ok = ~ref['doubt1']
    left = 1.0 - float(ok.float().mean())
    if left > max_left_out:
        fails.append(f"one step: {left:.4f} of the points left out, above {max_left_out}")
    acc = ok & ref['accept0']
    err = (got['points'].double() - ref['cand']).abs()
    bad = acc[:, None] & ~(err <= ref['cand_bound'])
    if bool(bad.any()):
        worst = float((err / ref['cand_bound'].clamp(min=1e-300))[bad].max())
        fails.append(f"one step: {int(bad.any(-1).sum())} accepted candidates outside the bound, worst {worst:.3g} x")
    rej = ok & ~ref['accept0']
    same = (bits(got['points']) == bits(got['input'])).all(-1)
    if bool((rej & ~same).any()):
        fails.append(f"one step: {int((rej & ~same).sum())} rejected points moved")
    if bool((ok & (got['evals'].int() != ref['evals'])).any()):
        fails.append(f"one step: evals differs on {int((ok & (got['evals'].int() != ref['evals'])).sum())} points")
    return fails


def check_invariants(got, tol, max_dist, sigma_at, level):
    """every point, no exclusions.  got: input, points, residual, state, evals, initial (the |residual| of an iters = 0 run of the same
    implementation); sigma_at(points) -> that implementation's sigma there (fp32)."""
    fails = []
    res, ini = got['residual'].float(), got['initial'].float()
    fin = torch.isfinite(ini)
    if bool((fin & ~(res.abs() <= ini)).any()):
        fails.append(f"|residual| grew on {int((fin & ~(res.abs() <= ini)).sum())} points")
    moved = (got['points'].double() - got['input'].double()).norm(dim=-1)
    lim = float(np.float32(max_dist)) * (1 + 4 * F32_EPS)
    finp = torch.isfinite(got['input']).all(-1)
    if bool((finp & ~(moved <= lim)).any()):
        fails.append(f"{int((finp & ~(moved <= lim)).sum())} points ended farther than max_dist, worst {float(moved[finp].max()):.6g} > {lim:.6g}")
    conv = res.abs() <= float(np.float32(tol))
    if not torch.equal(conv, got['state'] == 0):
        fails.append(f"state 0 <=> |residual| <= tol fails on {int((conv != (got['state'] == 0)).sum())} points")
    if not bool((bits(got['points']) == bits(got['input']))[~finp].all()):
        fails.append("a non-finite input lost its bits")
    still = (got['evals'] == 1)
    if not bool((bits(got['points']) == bits(got['input']))[still].all()):
        fails.append("a point with one evaluation moved")
    want = sigma_at(got['points']).float() - _f32(level)
    same = (bits(want) == bits(res)) | (torch.isnan(want) & torch.isnan(res))
    if not bool(same.all()):
        fails.append(f"residual is not sigma(points) - level on {int((~same).sum())} points")
    if bool(((got['evals'] < 1) | (got['state'] < 0) | (got['state'] > 2)).any()):
        fails.append("evals or state out of range")
    return fails


def check_control(got, ref, max_left_out=0.10):
    fails = []
    ok = ~ref['doubt']
    left = 1.0 - float(ok.float().mean())
    if left > max_left_out:
        fails.append(f"control flow: {left:.4f} of the points left out, above {max_left_out}")
    for k in ('state', 'evals'):
        bad = ok & (got[k].int() != ref[k])
        if bool(bad.any()):
            fails.append(f"control flow: {k} differs on {int(bad.sum())} of {int(ok.sum())} points")
    return fails


def check_convergence(got, ref):
    a, b = float((got['state'] == 0).float().mean()), float((ref['state'] == 0).float().mean())
    return [] if a >= b - 0.01 else [f"convergence: {a:.4f} of the points, the float64 loop reaches {b:.4f}"]
