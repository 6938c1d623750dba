"""Float64 restatement of the volume-composited normal of include/ln3d_normals.h (mode 1 of ln3d_surface_normals), its per-ray error
bound, the synthetic weights the tests feed it, and an fp32 torch restatement with its own summation order and five seeded faults that
the bound is calibrated on without a GPU (tests/test_normals_composite_cpu.py).

    omega_0 = fl(0.5 w_0), omega_j = fl(0.5 fl(w_{j-1} + w_j)), omega_{T-1} = fl(0.5 w_{T-2});  sample j counts iff omega_j > floor
    N = sum_j omega_j n_j,  n_j = -grad sigma / |grad sigma| at coords[ray, j] (0 where the gradient is 0)

omega is computed in fp32 torch - one rounding per addition, the halving exact - so the skip rule is decided on the bits the kernel sees.
"""
import math

import torch

import normal_refs as nr

U = 2.0 ** -24                    # one fp32 rounding, relative
FAULTS = ('unaveraged', 'last_dropped', 'gradients', 'sign', 'first64_only')


def omegas(weights):
    """weights [R, T - 1] -> omega [R, T], fp32, the kernel's bits (fp32 torch rounds every addition once; * 0.5 is exact)"""
    w = torch.as_tensor(weights).detach().cpu().float()
    R, T = w.shape[0], w.shape[1] + 1
    om = torch.empty(R, T)
    om[:, 0] = 0.5 * w[:, 0]
    om[:, T - 1] = 0.5 * w[:, T - 2]
    if T > 2:
        om[:, 1:T - 1] = 0.5 * (w[:, :-1] + w[:, 1:])
    return om


def summation_ulps(T):
    """roundings between the fl'd terms omega_j n_j and N, in the stated order: the product, ceil(T / 64) additions in the owning lane
    and six butterfly steps; each is relative 2^-24 of a partial sum, and every partial sum is at most sum_j omega_j |n_j| <= sum_j
    omega_j.  gamma_k = k u / (1 - k u) is the rigorous form of "k roundings"."""
    k = math.ceil(T / 64) + 6 + 1
    return k * U / (1 - k * U)


def composite64(planes, ray_plane, coords, weights, dec, box_warp, ulps, floor=0.0, chunk=16384):
    """planes [NP, 3, H, W, 32], ray_plane [R] (which tri-plane a ray reads), coords [R, T, 3] f32, weights [R, T - 1] f32 ->
    dict(omega [R, T] f32, active [R, T], accum [R, 3] f64 = N, bound [R, 3] = the error bound of an fp32 N per component,
    unit [R, 3] = N / |N| (0 where N = 0), mass [R] = sum of the active omega).
    bound = sum_j omega_j normal_bound(grad_j, scale_j, ulps) + summation_ulps(T) * sum_j omega_j."""
    coords = torch.as_tensor(coords).detach().cpu().float()
    R, T = coords.shape[0], coords.shape[1]
    om = omegas(weights)
    active = om > torch.tensor(floor, dtype=torch.float32)            # False for a NaN
    omd = torch.where(active, om, torch.zeros_like(om)).double()
    accum = torch.zeros(R, 3, dtype=torch.float64)
    bound = torch.zeros(R, 3, dtype=torch.float64)
    ray_of = torch.arange(R)[:, None].expand(R, T)
    for p in sorted(set(int(x) for x in ray_plane)):
        sel = active & (torch.as_tensor(ray_plane).long() == p)[:, None]
        pts, rays, o = coords[sel], ray_of[sel], omd[sel]
        for a in range(0, pts.shape[0], chunk):
            ref = nr.sigma_and_grad(planes[p], pts[a:a + chunk], dec, box_warp)
            n = nr.unit_outward(ref['grad'])
            nb = nr.normal_bound(ref['grad'], ref['scale'], ulps)
            nb = torch.where((ref['grad'].norm(dim=-1, keepdim=True) > 0).expand_as(nb), nb, torch.zeros_like(nb))     # exactly 0 both sides
            accum.index_add_(0, rays[a:a + chunk], o[a:a + chunk, None] * n)
            bound.index_add_(0, rays[a:a + chunk], o[a:a + chunk, None] * nb)
    mass = omd.sum(-1)
    bound = bound + summation_ulps(T) * mass[:, None]
    return dict(omega=om, active=active, accum=accum, bound=bound, unit=unit64(accum), mass=mass)


def unit64(N):
    """float64 N / |N| per row, 0 where N is 0 or not finite"""
    N = torch.as_tensor(N).double()
    ok = torch.isfinite(N).all(-1, keepdim=True) & (N.abs().amax(-1, keepdim=True) > 0)
    Nz = torch.where(ok, N, torch.ones_like(N))
    return torch.where(ok, Nz / Nz.norm(dim=-1, keepdim=True), torch.zeros_like(N))


def composite_f32(planes, ray_plane, coords, weights, dec, box_warp, floor=0.0, fault=None):
    """The same sum in fp32 torch with torch's own summation order over the samples: the stand-in for the kernel.  fault -
      unaveraged    the interval weights w_j used as they are instead of omega_j (sample T - 1 gets none)
      last_dropped  sample T - 1 left out
      gradients     -grad sigma composited instead of the unit normal
      sign          the result negated
      first64_only  samples j >= 64 ignored (one pass of the wave instead of ceil(T / 64))"""
    coords = torch.as_tensor(coords).detach().cpu().float()
    R, T = coords.shape[0], coords.shape[1]
    om = omegas(weights)
    if fault == 'unaveraged':
        om = torch.cat([torch.as_tensor(weights).detach().cpu().float(), torch.zeros(R, 1)], 1)
    active = om > torch.tensor(floor, dtype=torch.float32)
    if fault == 'last_dropped':
        active[:, T - 1] = False
    if fault == 'first64_only':
        active[:, 64:] = False
    terms = torch.zeros(R, T, 3)
    for p in sorted(set(int(x) for x in ray_plane)):
        sel = active & (torch.as_tensor(ray_plane).long() == p)[:, None]
        g = nr.grad_f32(planes[p], coords[sel], dec, box_warp)
        m = g.abs().amax(-1, keepdim=True)
        ok = m > 0
        u = g / torch.where(ok, m, torch.ones_like(m))
        n = torch.where(ok, -u / u.norm(dim=-1, keepdim=True).clamp(min=0.5), torch.zeros_like(g))
        terms[sel] = om[sel][:, None] * (-g if fault == 'gradients' else n)
    out = terms.sum(1)
    return -out if fault == 'sign' else out


def make_weights(R, T, seed):
    """[R, T - 1] fp32 interval weights shaped like a render's: most rays carry a window of at most 40 non-zero intervals (so leading
    and trailing exact zeros), with runs of exact zeros inside it; every seventh ray is dense, every fifth window ends at the last
    interval and every third starts at the first one; each ray sums to a random mass <= 1.  Then, where R allows: ray 0 is all zero,
    ray 1 carries one NaN, ray 2 a single non-zero interval."""
    g = torch.Generator().manual_seed(seed)
    K = T - 1
    w = torch.rand(R, K, generator=g) + 0.01
    idx = torch.arange(K)[None]
    length = torch.randint(1, min(K, 40) + 1, (R, 1), generator=g)
    start = (torch.rand(R, 1, generator=g) * (K - length + 1)).long()
    r = torch.arange(R)[:, None]
    start = torch.where(r % 3 == 0, torch.zeros_like(start), start)
    start = torch.where(r % 5 == 4, K - length, start)
    dense = r % 7 == 6
    inside = ((idx >= start) & (idx < start + length)) | dense
    hole_at = (torch.rand(R, 1, generator=g) * K).long()
    hole = (idx >= hole_at) & (idx < hole_at + torch.randint(1, 6, (R, 1), generator=g)) & (idx > start) & (idx < start + length - 1)
    w = torch.where(inside & ~hole & (torch.rand(R, K, generator=g) > 0.15), w, torch.zeros_like(w))
    w[torch.arange(R), start[:, 0]] += 0.05                      # no accidental all-zero ray
    w[torch.arange(R) % 5 == 4, K - 1] += 0.05                   # those windows do reach the last interval
    w = w / w.sum(-1, keepdim=True) * (0.3 + 0.7 * torch.rand(R, 1, generator=g))
    w = w.float()
    if R > 0:
        w[0] = 0.0
    if R > 1:
        w[1, K // 2] = float('nan')
    if R > 2:
        w[2] = 0.0
        w[2, (2 * K) // 3] = 0.75
    return w.contiguous()
