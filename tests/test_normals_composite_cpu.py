"""Volume-composited normals without a GPU: the float64 reference and bound of tests/normal_composite_refs.py calibrated on an fp32 torch
restatement with its own summation order, five seeded faults outside the bound, the C ABI of the composited mode of
ln3d_surface_normals (include/ln3d_normals.h) and the launcher's --normal_map_mode."""
import ctypes as C

import pytest
import torch

import normal_composite_refs as cr
import normal_refs as nr
from render_refs import make_scene
from test_normals_cpu import GRAD_BOUND_ULPS, MARGIN, _normals_args

H, W, BOX = 16, 16, 0.9
CASES = ((2, 24, 21), (65, 40, 22), (128, 40, 23), (256, 14, 24))          # (T, rays, seed): one, two and four passes of the wave


def _case(T, R, seed, half=False):
    inp = make_scene(seed, 1, M=1, H=H, W=W, NP=2, plane_scale=2.0, hidden_gain=12.0 if seed % 2 else 1.0)
    planes = inp['planes'].half() if half else inp['planes']
    coords = nr.sample_points(R * T, seed, H, W, BOX, MARGIN).reshape(R, T, 3)
    ray_plane = torch.arange(R) % 2
    return planes, ray_plane, coords, cr.make_weights(R, T, seed), inp['dec']


_REFS = {}


def _ref(case):
    if case not in _REFS:
        planes, ray_plane, coords, w, dec = _case(*case)
        _REFS[case] = (planes, ray_plane, coords, w, dec, cr.composite64(planes, ray_plane, coords, w, dec, BOX, GRAD_BOUND_ULPS))
    return _REFS[case]


def _share(case, fault=None):
    planes, ray_plane, coords, w, dec, ref = _ref(case)
    got = cr.composite_f32(planes, ray_plane, coords, w, dec, BOX, fault=fault).double()
    err = (got - ref['accum']).abs()
    return torch.where(err == 0, torch.zeros_like(err), err / ref['bound'].clamp(min=1e-300)), ref


def test_omega_is_the_colour_compositing_of_the_marcher():
    """sum_j omega_j n_j = sum_k w_k (n_k + n_{k+1}) / 2 (MipRayMarcher2's midpoints), in float64 on fp32-exact weights; and omega carries
    the stated roundings: fl(0.5 fl(a + b))"""
    g = torch.Generator().manual_seed(3)
    for T in (2, 3, 64, 65, 256):
        w = (torch.rand(7, T - 1, generator=g) * 2.0 ** -3).float()
        n = torch.randn(7, T, 3, generator=g, dtype=torch.float64)
        om = cr.omegas(w)
        assert om.dtype == torch.float32 and om.shape == (7, T)
        mid = (w.double()[..., None] * (n[:, :-1] + n[:, 1:]) / 2).sum(1)
        exact_om = torch.zeros(7, T, dtype=torch.float64)
        exact_om[:, :-1] += 0.5 * w.double()
        exact_om[:, 1:] += 0.5 * w.double()
        assert float(((exact_om[..., None] * n).sum(1) - mid).abs().max()) <= 1e-14
        assert bool(((om.double() - exact_om).abs() <= 2.0 ** -24 * exact_om).all())              # one rounding, of the inner sum
        assert torch.equal(om[:, 0], 0.5 * w[:, 0]) and torch.equal(om[:, -1], 0.5 * w[:, -1])
        if T > 2:
            assert torch.equal(om[:, 1:-1], ((w[:, :-1] + w[:, 1:]) * 0.5))


def test_synthetic_weights_contain_every_listed_shape():
    for T, R, seed in CASES:
        w = cr.make_weights(R, T, seed)
        om = cr.omegas(w)
        assert w.shape == (R, T - 1) and bool((w[0] == 0).all()) and int(torch.isnan(w[1]).sum()) == 1 and int((w[2] != 0).sum()) == 1
        rest = w[3:]
        assert bool((rest >= 0).all()) and bool((rest.double().sum(-1) <= 1 + 1e-6).all()) and bool((rest.sum(-1) > 0).all())
        assert int(torch.isnan(om[1]).sum()) == 2 and int((om[2] > 0).sum()) == 2
        if T >= 65:
            z = rest == 0
            assert bool(z[:, 0].any()) and bool(z[:, -1].any()) and bool((~z[:, 0]).any()) and bool((~z[:, -1]).any())     # leading / trailing zeros, and not
            idx = torch.arange(T - 1)[None].expand_as(z)
            first = torch.where(z, T, idx).amin(1, keepdim=True)
            last = torch.where(z, -1, idx).amax(1, keepdim=True)
            assert bool((z & (idx > first) & (idx < last)).any())                                                         # runs of zeros inside the window


def test_bound_is_calibrated_on_the_fp32_restatement():
    """the whole bound - sum omega_j normal_bound_j plus the summation term of the stated order - against fp32 torch with another order"""
    worst = 0.0
    for case in CASES:
        frac, ref = _share(case)
        T = case[0]
        assert cr.summation_ulps(T) >= (-(-T // 64) + 7) * 2.0 ** -24
        assert frac.shape == (case[1], 3) and bool(torch.isfinite(ref['accum']).all()) and bool(torch.isfinite(ref['bound']).all())
        assert bool((ref['accum'][0] == 0).all()) and bool((ref['bound'][0] == 0).all())                # the all-zero ray: exactly 0, bound 0
        assert bool((frac <= 1).all()), (case, float(frac.max()))
        worst = max(worst, float(frac.max()))
        print(f"[normals-composite] T={T}: fp32 restatement worst {float(frac.max()):.3g} of the bound, "
              f"{int(ref['active'].sum())} / {ref['active'].numel()} samples evaluated")
    assert worst > 1e-3, worst                     # the bound is of the error's own size, not a blanket


def test_float64_reference_on_half_texels_and_floor():
    """binary16 texels are read exactly; a floor removes samples by the stated rule and moves N by at most floor * skipped"""
    planes, ray_plane, coords, w, dec = _case(65, 12, 31, half=True)
    a = cr.composite64(planes, ray_plane, coords, w, dec, BOX, GRAD_BOUND_ULPS)
    b = cr.composite64(planes.float(), ray_plane, coords, w, dec, BOX, GRAD_BOUND_ULPS)
    assert torch.equal(a['accum'], b['accum'])
    floor = float(a['omega'][a['active']].median())
    c = cr.composite64(planes, ray_plane, coords, w, dec, BOX, GRAD_BOUND_ULPS, floor=floor)
    skipped = (a['active'] & ~c['active']).sum(-1)
    assert 0 < int(c['active'].sum()) < int(a['active'].sum()) and bool((c['active'] <= a['active']).all())
    assert bool(((a['accum'] - c['accum']).norm(dim=-1) <= floor * skipped + 1e-12).all())


@pytest.mark.parametrize("fault", cr.FAULTS)
def test_seeded_fault_fails_the_bound(fault):
    worst = 0.0
    for case in CASES:
        if fault == 'first64_only' and case[0] <= 64:
            continue
        frac, _ = _share(case, fault)
        worst = max(worst, float(frac.max()))
        if case[0] > 2 or fault in ('gradients', 'sign'):
            assert bool((frac > 1).any()), (fault, case, float(frac.max()))
    print(f"[normals-composite] fault {fault}: worst {worst:.4g} of the bound")
    assert worst > 100


# ---------------------------------------------------------------- C ABI
def _composite_args(**kw):
    a = _normals_args(mode=1, samples=128, weights=0x10000, coords=0x10000, depth=None)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


COMPOSITE_ROWS = [dict(mode=2), dict(mode=-1), dict(mode=7),
                  dict(samples=0), dict(samples=1), dict(samples=257), dict(samples=-4),
                  dict(weights=None), dict(coords=None), dict(wsum=None), dict(normal=None), dict(planes=None), dict(plane_index=None),
                  dict(weight_floor=-1e-6), dict(weight_floor=float('nan')), dict(weight_floor=float('inf')), dict(weight_floor=-float('inf')),
                  dict(mask_threshold=0.0), dict(space=2), dict(space=1, cams=None), dict(V=0), dict(res=0), dict(box_warp=0.0), dict(H=0)]


def test_composited_mode_abi(hip_lib):
    """both entry points refuse an unknown mode, T outside 2 ... 256, a missing weights / coords and a negative or non-finite floor with
    LN3D_ERR_BAD_ARG before anything is launched (the addresses are fake); the mode-0 argument list with the appended fields zero is
    validated exactly as before, and the mode-1 fields do not leak into it"""
    from ln3diff_amd._lib import NormalsArgs
    names = [f[0] for f in NormalsArgs._fields_]
    assert names[-6:] == ['mode', 'samples', 'weights', 'coords', 'weight_floor', 'accum'] and names[20] == 'points'
    fresh = NormalsArgs()
    assert fresh.mode == 0 and fresh.samples == 0 and fresh.weights is None and fresh.coords is None and fresh.weight_floor == 0.0
    for name in ('ln3d_surface_normals', 'ln3d_surface_normals_f16'):
        fn = getattr(hip_lib, name)
        for kw in COMPOSITE_ROWS:
            assert fn(C.byref(_composite_args(**kw)), None) == -1, (name, kw)
        # mode 0 keeps its validation whatever the appended fields hold: depth is still required, and a zeroed tail changes nothing
        assert fn(C.byref(_normals_args(depth=None)), None) == -1
        assert fn(C.byref(_normals_args(depth=None, samples=128, weights=0x10000, coords=0x10000)), None) == -1
        assert fn(C.byref(_normals_args(cams=None, mode=0)), None) == -1
    assert hip_lib.ln3d_abi_version() == 10


def test_ops_wrapper_checks_before_the_call(hip_lib):
    from ln3diff_amd import ops
    V, M, T = 2, 3, 5
    z = lambda *s: torch.zeros(*s)                                                                      # noqa: E731
    planes, pidx, dec = z(1, 3, 8, 8, 32), torch.zeros(V, dtype=torch.int32), (z(64, 32), z(64), z(4, 64), z(4))
    ok = dict(n_views=V, rays_per_view=M, mode='composited', weights=z(V, M, T - 1), coords=z(V, M, T, 3))
    call = lambda **kw: ops.surface_normals(planes, 8, 8, pidx, dec, 0.9, None, z(V, M), z(V, 3, M), **{**ok, **kw})      # noqa: E731
    with pytest.raises(ValueError, match="normal mode 'volume'"):
        call(mode='volume')
    with pytest.raises(ValueError, match='needs weights'):
        call(weights=None)
    with pytest.raises(ValueError, match='weights has'):
        call(weights=z(V, M, T))
    with pytest.raises(TypeError, match='coords must be a contiguous torch.float32'):
        call(coords=z(V, M, T, 3).double())
    with pytest.raises(TypeError, match='weights must be a contiguous'):
        call(weights=z(V, M, 2 * (T - 1))[..., ::2])
    with pytest.raises(ValueError, match='accum has'):
        call(accum=z(V, 3, M - 1))
    with pytest.raises(ValueError, match='2 ... 256 samples'):
        call(weights=z(V, M, 256), coords=z(V, M, 257, 3))
    with pytest.raises(ValueError, match='writes no points'):
        call(points=z(V, M, 3))
    with pytest.raises(ValueError, match="belong to mode='composited'"):
        call(mode='surface')


# ---------------------------------------------------------------- launcher
@pytest.mark.parametrize('objaverse', [True, False])
def test_launcher_normal_map_mode(objaverse):
    from ln3diff_amd.entry import create_argparser, recorded_args, validate
    parse = lambda s: create_argparser(objaverse).parse_args(s.split())                           # noqa: E731
    with pytest.raises(SystemExit, match='normal_map_mode composited.*save_normal_maps true'):
        validate(parse("--normal_map_mode composited"))
    with pytest.raises(SystemExit, match='normal_map_mode composited.*save_normal_maps true'):
        validate(parse("--normal_map_mode composited --save_normal_maps false"))
    with pytest.raises(SystemExit, match="normal_map_mode volume.*surface.*composited"):
        validate(parse("--normal_map_mode volume --save_normal_maps true"))
    both = parse("--normal_map_mode composited --save_normal_maps true")
    validate(both)
    rec = recorded_args(both)
    assert rec['normal_map_mode'] == 'composited' and rec['save_normal_maps'] is True
    default = parse("")
    validate(default)
    assert default.normal_map_mode == 'surface'
    assert 'normal_map_mode' not in recorded_args(default) and 'save_normal_maps' not in recorded_args(default)
    assert set(vars(default)) - set(recorded_args(default)) >= {'normal_map_mode', 'save_normal_maps', 'export_mesh_normals'}
    surf = parse("--save_normal_maps true --normal_map_mode surface")
    validate(surf)
    assert 'normal_map_mode' not in recorded_args(surf) and recorded_args(surf)['save_normal_maps'] is True
