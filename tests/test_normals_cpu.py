"""Surface normals without a GPU: the float64 reference of tests/normal_refs.py against a central difference of its own sigma, the
calibration of the GPU bound on an fp32 restatement (and five seeded faults outside it), the .obj writer, and the C ABI of
include/ln3d_normals.h."""
import ctypes as C

import numpy as np
import pytest
import torch

import normal_refs as nr
from render_refs import make_scene, make_decoder

H, W, BOX = 16, 24, 0.9
# Calibration: worst |grad_f32 - float64| / (2^-23 * scale) over the scenes of _calibration_cases(), texel_margin >= 0.02; the GPU bound is
# 4 x that (another summation order, hardware exp2 / log2 / rcp, FMA contraction).  Produced by
#     python tests/test_normals_cpu.py
# which printed MEASURED_F32_ULPS = 0.08877   GRAD_BOUND_ULPS = 0.3551.  (The figure is small because the scale is generous: it carries the
# texel-coordinate rounding, ~W ulps, on every tap.)  torch's fp32 matmul sums in an order that depends on the host (threads, vector
# width), so test_gpu_bound_is_calibrated re-measures and accepts HOST_SPREAD around the recorded figure; the bound itself is 4 x the
# recorded figure and nothing else.
MEASURED_F32_ULPS = 0.08877
GRAD_BOUND_ULPS = 4.0 * MEASURED_F32_ULPS
HOST_SPREAD = 0.1                # relative: how far another host's re-measurement may sit from the recorded one
MARGIN = 0.02


def _calibration_cases():
    """(planes [3,H,W,32], pts, dec): f32 and fp16-representable texels, an ordinary decoder and one with hidden_gain 12 (h > 20 in a few percent of the hidden units),
    points inside the box, across its border (some taps padding) and beyond it (all taps padding)"""
    for seed, gain, half in ((11, 1.0, False), (12, 12.0, False), (13, 12.0, True), (14, 1.0, True)):
        inp = make_scene(seed, 1, M=1, H=H, W=W, NP=1, plane_scale=2.0, hidden_gain=gain)
        planes = inp['planes'][0]
        if half:
            planes = planes.half()
        yield planes, nr.sample_points(4096, seed, H, W, BOX, MARGIN), inp['dec']


def _worst_ulps(fault=None):
    worst = 0.0
    for planes, pts, dec in _calibration_cases():
        ref = nr.sigma_and_grad(planes, pts, dec, BOX)
        got = nr.grad_f32(planes, pts, dec, BOX, fault).double()
        err = (got - ref['grad']).abs()
        frac = torch.where(err == 0, torch.zeros_like(err), err / (nr.F32_EPS * ref['scale']).clamp(min=1e-300))
        worst = max(worst, float(frac.max()))
        assert bool((ref['grad'][ref['all_padding']] == 0).all()) and (fault is not None or bool((got[ref['all_padding']] == 0).all()))
    return worst


def test_analytic_gradient_equals_central_difference():
    """float64 analytic gradient vs (sigma(p + d e_a) - sigma(p - d e_a)) / (2 d), d = 1e-6 texels of the finer axis (the points are offset in
    float64, so the reference is evaluated through its double-precision coordinate path: _shifted below).
    Tolerance = truncation + rounding of the difference itself:
      truncation  d^2 / 6 |sigma'''|, sigma''' taken from the SECOND difference of the analytic gradient at a step of 1e-3 texels (inside
                  the same bilinear piece: texel_margin >= 0.02), doubled because that estimate is itself first order;
      rounding    the two float64 sigmas carry n 2^-53 of the absolute sum of their terms (sigma_scale; n = 96, the longest serial
                  chain of the 32- and 64-term sums) each, divided by 2 d."""
    for planes, pts, dec in _calibration_cases():
        pts = pts[:512]
        pl, dec64 = planes.double(), dec
        cs = 2.0 / float(np.float32(BOX))
        d_world = 1e-6 / (cs * max(H, W) / 2)
        e_world = 1e-3 / (cs * max(H, W) / 2)
        base = _ref64(pl, pts.double(), dec64)
        for a in range(3):
            ea = torch.zeros(3, dtype=torch.float64)
            ea[a] = 1.0
            sp, sm = _ref64(pl, pts.double() + d_world * ea, dec64), _ref64(pl, pts.double() - d_world * ea, dec64)
            gp, gm = _ref64(pl, pts.double() + e_world * ea, dec64), _ref64(pl, pts.double() - e_world * ea, dec64)
            fd = (sp['sigma'] - sm['sigma']) / (2 * d_world)
            third = (gp['grad'][:, a] - 2 * base['grad'][:, a] + gm['grad'][:, a]).abs() / e_world ** 2
            tol = 2 * d_world ** 2 / 6 * third + 96 * 2.0 ** -53 * (sp['sigma_scale'] + sm['sigma_scale']) / (2 * d_world)
            err = (fd - base['grad'][:, a]).abs()
            assert bool((err <= tol).all()), (a, float((err / tol.clamp(min=1e-300)).max()))
            assert float((err / tol.clamp(min=1e-300)).max()) > 1e-4          # the tolerance is of the error's own size, not a blanket


def _ref64(planes64, pts64, dec):
    """sigma_and_grad at float64 points: the reference rounds its points to fp32 on entry (they are the kernel's inputs), so the shifted
    points go in through a subclass of its coordinate step"""
    old = nr._texel_coords

    def coords(pts, H_, W_, box_warp, dtype=torch.float64):
        g = pts64 * (2.0 / float(np.float32(box_warp)))
        return torch.stack([torch.stack([((g[:, a] + 1) * W_ - 1) / 2, ((g[:, b] + 1) * H_ - 1) / 2], -1) for a, b in nr.PLANE_AXES], 1)
    nr._texel_coords = coords
    try:
        return nr.sigma_and_grad(planes64, pts64.float(), dec, BOX)
    finally:
        nr._texel_coords = old


def test_gpu_bound_is_calibrated():
    worst = _worst_ulps()
    print(f"[normals] fp32 restatement: worst {worst:.4g} x 2^-23 scale; constants: measured {MEASURED_F32_ULPS}, bound {GRAD_BOUND_ULPS}")
    assert abs(worst - MEASURED_F32_ULPS) <= HOST_SPREAD * MEASURED_F32_ULPS, (worst, MEASURED_F32_ULPS)
    assert GRAD_BOUND_ULPS == 4.0 * MEASURED_F32_ULPS


def test_calibration_points_cover_every_path():
    lin = pad = border = 0
    for planes, pts, dec in _calibration_cases():
        ref = nr.sigma_and_grad(planes, pts, dec, BOX)
        pad += int(ref['all_padding'].sum())
        inside = (pts.abs() <= BOX / 2 - BOX / min(H, W)).all(-1)
        border += int((~inside & ~ref['all_padding']).sum())
        lin += int((nr.grad_f32(planes, pts, dec, BOX, 'no_linear_branch') != nr.grad_f32(planes, pts, dec, BOX)).any(-1).sum())   # some h > 20
        assert float(nr.texel_margin(pts, H, W, BOX).min()) >= MARGIN
    assert pad > 100 and border > 100 and lin > 100, (pad, border, lin)


def test_share_of_points_near_a_texel_centre():
    """what the GPU tests leave out of the ray / vertex comparison (texel_margin < 1e-3): six coordinates, each within 1e-3 of an integer with
    probability 2e-3, so about 1.2 % of points spread over the box - far from the 5 % cap the GPU tests assert"""
    g = torch.Generator().manual_seed(5)
    pts = ((torch.rand(200000, 3, generator=g) - 0.5) * BOX).float()
    share = float((nr.texel_margin(pts, H, W, BOX) < 1e-3).double().mean())
    print(f"[normals] share of box points with texel_margin < 1e-3: {share:.4f}")
    assert 0.009 <= share <= 0.015


@pytest.mark.parametrize("fault", nr.FAULTS)
def test_seeded_fault_lands_outside_the_bound(fault):
    worst = _worst_ulps(fault)
    print(f"[normals] fault {fault}: worst {worst:.4g} x 2^-23 scale against a bound of {GRAD_BOUND_ULPS}")
    assert worst > 100 * GRAD_BOUND_ULPS


# ---------------------------------------------------------------- .obj
OBJ_V = np.array([[0.0, 0.5, -0.25], [1.0, 0.0, 0.0], [0.0, 1.0, 0.125], [0.5, 0.5, 1.0]], np.float32)
OBJ_F = np.array([[0, 1, 2], [0, 2, 3]], np.int64)
OBJ_C = np.array([[1.0, 0.0, 0.5], [0.25, 0.25, 0.25], [0.0, 1.0, 0.0], [0.1, 0.2, 0.3]], np.float32)
OBJ_TODAY = (b"v 0.000000 0.500000 -0.250000 1.0000 0.0000 0.5000\n"
             b"v 1.000000 0.000000 0.000000 0.2500 0.2500 0.2500\n"
             b"v 0.000000 1.000000 0.125000 0.0000 1.0000 0.0000\n"
             b"v 0.500000 0.500000 1.000000 0.1000 0.2000 0.3000\n"
             b"f 1 2 3\n"
             b"f 1 3 4\n")


def test_write_obj_without_normals_is_unchanged(tmp_path):
    from ln3diff_amd.mesh import write_obj
    write_obj(tmp_path / "a.obj", OBJ_V, OBJ_F, OBJ_C)
    assert open(tmp_path / "a.obj", 'rb').read() == OBJ_TODAY
    write_obj(tmp_path / "b.obj", OBJ_V, OBJ_F, OBJ_C, None)
    assert open(tmp_path / "b.obj", 'rb').read() == OBJ_TODAY


def parse_obj(path):
    v, vn, fv, fn = [], [], [], []
    for line in open(path):
        t = line.split()
        if t[0] == 'v':
            v.append([float(x) for x in t[1:4]])
        elif t[0] == 'vn':
            vn.append([float(x) for x in t[1:4]])
        elif t[0] == 'f':
            corners = [c.split('/') for c in t[1:]]
            fv.append([int(c[0]) - 1 for c in corners])
            fn.append([int(c[2]) - 1 for c in corners] if len(corners[0]) == 3 else None)
    return np.array(v).reshape(-1, 3), np.array(vn).reshape(-1, 3), np.array(fv).reshape(-1, 3), fn


def test_write_obj_with_normals_round_trips(tmp_path):
    from ln3diff_amd.mesh import write_obj
    n = np.array([[0, 0, 1], [0.6, 0.8, 0], [0, 0, 0], [-1, 0, 0]], np.float32)
    write_obj(tmp_path / "n.obj", OBJ_V, OBJ_F, OBJ_C, n)
    v, vn, fv, fn = parse_obj(tmp_path / "n.obj")
    assert np.allclose(v, OBJ_V, atol=5e-7) and np.allclose(vn, n, atol=5e-7) and vn.shape == v.shape
    assert np.array_equal(fv, OBJ_F) and all(a == list(b) for a, b in zip(fn, fv.tolist()))


# ---------------------------------------------------------------- C ABI
P_ = C.c_void_p(0x10000)          # fake, never dereferenced: validation comes before any launch
I64, F = C.c_int64, C.c_float
GRAD_OK = (P_, 8, 8, P_, I64(4), P_, P_, P_, P_, F(0.9), P_, P_, None)
GRAD_ROWS = [{0: None}, {3: None}, {5: None}, {6: None}, {7: None}, {8: None}, {10: None}, {11: None},
             {1: 0}, {1: -1}, {2: 0}, {2: -3}, {1: 1 << 15, 2: 1 << 15}, {4: I64(0)}, {4: I64(-1)},
             {9: F(0.0)}, {9: F(-1.0)}, {9: F(float('nan'))}, {9: F(float('inf'))}]


def _normals_args(**kw):
    from ln3diff_amd._lib import NormalsArgs
    a = NormalsArgs()
    for k in ('planes', 'plane_index', 'cams', 'dec_w0', 'dec_b0', 'dec_w1', 'dec_b1', 'depth', 'wsum', 'normal'):
        setattr(a, k, 0x10000)
    a.H, a.W, a.V, a.res, a.box_warp, a.mask_threshold = 8, 8, 1, 4, 0.9, 0.5
    for k, v in kw.items():
        setattr(a, k, v)
    return a


NORMALS_ROWS = [dict(planes=None), dict(plane_index=None), dict(dec_w0=None), dict(dec_b0=None), dict(dec_w1=None), dict(dec_b1=None),
                dict(depth=None), dict(wsum=None), dict(normal=None), dict(cams=None), dict(ray_o=0x10000), dict(ray_d=0x10000),
                dict(cams=None, ray_o=0x10000, ray_d=0x10000, rays_per_view=4, space=1),       # the camera frame needs cams
                dict(cams=None, ray_o=0x10000, ray_d=0x10000, res=0, rays_per_view=0),
                dict(V=0), dict(V=-1), dict(res=0), dict(res=-2), dict(res=1 << 16),
                dict(ray_o=0x10000, ray_d=0x10000, res=1 << 16),                               # M = res * res is an int with explicit rays too
                dict(rays_per_view=-1), dict(rays_per_view=15),
                dict(H=0), dict(H=-1), dict(W=0), dict(W=-8), dict(H=1 << 15, W=1 << 15),
                dict(box_warp=0.0), dict(box_warp=-0.9), dict(box_warp=float('nan')), dict(box_warp=float('inf')),
                dict(mask_threshold=0.0), dict(mask_threshold=-0.5), dict(mask_threshold=1.5), dict(mask_threshold=float('nan')),
                dict(space=2), dict(space=-1)]


def test_normals_abi(hip_lib):
    """the four entry points of include/ln3d_normals.h exist and refuse every missing buffer and every size or scale they index with or
    divide by with LN3D_ERR_BAD_ARG before anything is launched; the ABI number is unchanged"""
    for name in ('ln3d_query_points_grad', 'ln3d_query_points_grad_f16'):
        fn = getattr(hip_lib, name)
        for row in GRAD_ROWS:
            a = list(GRAD_OK)
            for i, v in row.items():
                a[i] = v
            assert fn(*a) == -1, (name, row)
    for name in ('ln3d_surface_normals', 'ln3d_surface_normals_f16'):
        fn = getattr(hip_lib, name)
        assert fn(None, None) == -1
        for kw in NORMALS_ROWS:
            assert fn(C.byref(_normals_args(**kw)), None) == -1, (name, kw)
    assert hip_lib.ln3d_abi_version() == 10


if __name__ == "__main__":
    w = _worst_ulps()
    print(f"MEASURED_F32_ULPS = {w:.4g}   GRAD_BOUND_ULPS = {4 * w:.4g}")
    for f in nr.FAULTS:
        print(f, f"{_worst_ulps(f):.4g}")
