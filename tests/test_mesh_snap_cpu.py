"""The level-set snapping of include/ln3d_meshsnap.h without a GPU:
  - the calibration of the sigma bound of the all-fp32 path (mesh_snap_refs.SIGMA_BOUND_ULPS);
  - the fp32 stand-in of the loop passes every check tests/test_mesh_snap_gpu.py makes, on exactly that test's cases, and every seeded
    fault fails at least one of them;
  - for those cases the left-out shares, computed by the float64 reference alone, are under the caps, and both kinds of rejection (a worse
    candidate, a candidate beyond max_dist) occur among the points whose control flow is compared;
  - what the float64 loop achieves (the figures the feature was proposed with);
  - the two entry points validate on fake addresses before they launch;
  - mesh_snap_iters from every public entry of pipeline down to mesh_from_grid / textured_mesh_from_grid, handed on only when non-zero;
    snap_mesh between the smoothing and the query; the launcher flag; the ValueErrors of snap_mesh and of ops.snap_points."""
import math

import numpy as np
import pytest
import torch

import mesh_snap_refs as R
import normal_refs as nr
from abi_args import BAD_ARG, BIG, with_args as _with

HOST_SPREAD = 0.25               # relative: a maximum over points of an error a few ulps of sigma large moves in steps of a quarter of itself
P0, Q0 = 0x10000, 0x4000000      # two fake device addresses, 64 MiB apart


# ---------------------------------------------------------------- calibration
def _worst_sigma_ulps():
    worst = 0.0
    for planes, pts, dec in R.calibration_cases():
        ref = nr.sigma_and_grad(planes, pts, dec, R.BOX)
        err = (R.sigma_f32(planes, pts, dec, R.BOX).double() - ref['sigma']).abs()
        worst = max(worst, float((err / (R.F32_EPS * ref['sigma_scale'])).max()))
    return worst


def test_sigma_bound_calibration():
    worst = _worst_sigma_ulps()
    print(f"[snap] fp32 sigma stand-in: worst {worst:.4g} x 2^-23 sigma_scale; constants: measured {R.MEASURED_SIGMA_F32_ULPS}, bound {R.SIGMA_BOUND_ULPS}")
    assert abs(worst - R.MEASURED_SIGMA_F32_ULPS) <= HOST_SPREAD * R.MEASURED_SIGMA_F32_ULPS, (worst, R.MEASURED_SIGMA_F32_ULPS)
    assert R.SIGMA_BOUND_ULPS == 4.0 * R.MEASURED_SIGMA_F32_ULPS
    import render_refs as rr
    assert R.SIGMA_BOUND_ULPS < rr.DEC_ULPS / 10                                          # not the bound of the bf16-split query


# ---------------------------------------------------------------- the stand-in, the faults, the caps
def _standin(c, fault=None):
    field = R.field_f32(c['planes'], c['dec'], R.BOX)
    snap = lambda pts, iters, md: R.run_loop(field, pts, c['level'], iters, c['tol'], c['max_step'], md, dtype=torch.float32, fault=fault)   # noqa: E731
    return snap, (lambda x: R.sigma_f32(c['planes'], x, c['dec'], R.BOX))


@pytest.mark.parametrize('P', R.SIZES)
def test_standin_passes_every_gpu_check(P):
    c = R.case(P)
    fails, outs = R.run_all(c, *_standin(c))
    assert fails == []
    assert outs['full']['points'].dtype == torch.float32 and outs['full']['evals'].max() <= R.ITERS + 1


@pytest.mark.parametrize('fault', R.FAULTS)
def test_every_seeded_fault_fails_a_gpu_check(fault):
    """on the two largest cases, which is where the GPU test has enough points of every kind"""
    for P in (257, 4099):
        c = R.case(P)
        fails, _ = R.run_all(c, *_standin(c, fault))
        print(f"[snap] fault {fault} P={P}: {fails}")
        assert fails, (fault, P)


@pytest.mark.parametrize('P', R.SIZES)
def test_left_out_shares_and_rejections_from_the_reference_alone(P):
    c = R.case(P)
    one, full, tight = c['one'], c['full'], c['tight_full']
    shares = [float(one['doubt1'].float().mean()), float(full['doubt'].float().mean()), float(tight['doubt'].float().mean())]
    why = {k: round(float(v.float().mean()), 4) for k, v in full['why'].items()}
    print(f"[snap] P={P} level {c['level']:.4f}: left out {shares[0]:.4f} (one step), {shares[1]:.4f} / {shares[2]:.4f} (control flow); causes {why}")
    assert shares[0] <= R.MAX_ONE_STEP_LEFT_OUT and max(shares[1:]) <= R.MAX_CONTROL_LEFT_OUT
    assert c['points'].shape == (P, 3) and c['points'].dtype == torch.float32
    if P >= 257:                                                                          # both kinds of rejection are among the compared points
        worse = int(((full['n_worse'] > 0) & ~full['doubt']).sum())
        far = int(((tight['n_far'] > 0) & ~tight['doubt']).sum())
        print(f"[snap] P={P}: {worse} compared points reject a worse candidate, {far} one beyond max_dist")
        assert worse >= 4 and far >= 4
        assert int((full['state'] == 2).sum()) > 0 and int((full['state'] == 1).sum()) > 0 and int((full['state'] == 0).sum()) > P // 2
        assert int(one['accept0'].sum()) > P // 2 and int((one['evaluated0'] & ~one['accept0']).sum()) > 0


def test_what_the_float64_loop_achieves():
    """the figures of the proposal, on this file's own case: displaced crossings, 8 iterations"""
    c = R.case(4099)
    near = torch.arange(4099) < 4099 - int(round(4099 * 0.15))
    full = c['full']
    before, after = float(full['initial'][near].median()), float(full['residual'][near].abs().median())
    share = float((full['state'][near] == 0).float().mean())
    print(f"[snap] float64 loop, displaced crossings: median |sigma - level| {before:.4f} -> {after:.2e}, converged {share:.4f}, "
          f"mean evals {float(full['evals'][near].float().mean()):.2f}")
    assert after < before / 20 and share > 0.95
    assert bool((full['residual'].abs() <= full['initial'])[torch.isfinite(full['initial'])].all())          # never worse than it started
    moved = (full['points'].double() - c['points'].double()).norm(dim=-1)
    assert float(moved.max()) <= c['max_dist'] * (1 + 4 * R.F32_EPS)


# ---------------------------------------------------------------- entry points on fake addresses
def _valid():
    # planes H W points_in P w0 b0 w1 b1 box_warp level iters tol max_step max_dist points_out residual state evals stream
    return [P0, 16, 24, P0 + 0x100000, 5, P0 + 0x200000, P0 + 0x210000, P0 + 0x220000, P0 + 0x230000, 0.9, 1.0, 4, 1e-3, 0.01, 0.02,
            Q0, Q0 + 4096, Q0 + 8192, Q0 + 12288, None]


@pytest.mark.parametrize('name', ['ln3d_snap_points', 'ln3d_snap_points_f16'])
def test_snap_entry_points_validate_before_they_launch(hip_lib, name):
    fn, args = getattr(hip_lib, name), _valid()
    for i in (0, 3, 5, 6, 7, 8, 15, 16, 17, 18):
        assert fn(*_with(args, **{'i%d' % i: None})) == BAD_ARG, ('null buffer', i)
    for bad in (0, -1, BIG, 1 << 40):
        assert fn(*_with(args, i4=bad)) == BAD_ARG, ('P', bad)
    for i in (1, 2):
        for bad in (0, -1):
            assert fn(*_with(args, **{'i%d' % i: bad})) == BAD_ARG, ('H / W', i, bad)
    for bad in (-1, 65, 1 << 20):
        assert fn(*_with(args, i11=bad)) == BAD_ARG, ('iters', bad)
    for i in (9, 10, 12, 13, 14):
        for bad in (float('nan'), float('inf'), -float('inf')):
            assert fn(*_with(args, **{'i%d' % i: bad})) == BAD_ARG, ('non-finite', i, bad)
    assert fn(*_with(args, i12=-1e-6)) == BAD_ARG and fn(*_with(args, i13=0.0)) == BAD_ARG and fn(*_with(args, i13=-0.01)) == BAD_ARG
    assert fn(*_with(args, i14=-0.02)) == BAD_ARG and fn(*_with(args, i9=0.0)) == BAD_ARG
    assert fn(*_with(args, i15=args[3])) == BAD_ARG                                        # in and out are one buffer
    for shift in (4, 12 * 5 - 4, -(12 * 5 - 4)):                                           # ... or overlap: P = 5 rows of 12 bytes
        assert fn(*_with(args, i15=args[3] + shift)) == BAD_ARG, shift
    assert b'bad argument' in hip_lib.ln3d_strerror(BAD_ARG)


class _Field:
    """a decoder that records when it is asked for colours"""
    def __init__(self, log):
        self.log = log

    def forward_points(self, pcl, pts, with_grad=False):
        self.log.append(('forward_points', pts[0].clone()))
        return {'rgb': torch.zeros_like(pts), 'normal': torch.zeros_like(pts)}


def test_snapping_sits_between_the_smoothing_and_the_query(monkeypatch):
    from ln3diff_amd import mesh
    log = []
    G = 8
    raw, smoothed, snapped = torch.tensor([[1.0, 2.0, 3.0]]), torch.tensor([[7.0, 0.0, 3.5]]), torch.tensor([[0.25, -0.125, 0.375]])
    faces = torch.zeros(0, 3, dtype=torch.int64)

    def isosurface(sigma, thr, method, *post):
        log.append(('extract_isosurface', post))
        return raw, faces

    def smooth(verts, f, iterations, lam, mu, check=True):
        log.append(('smooth_mesh', verts, iterations))
        return (smoothed if iterations else verts), f

    def snap(decoder, pcl, verts_box, level, iterations, tol=None, max_step=None, max_dist=None):
        log.append(('snap_mesh', verts_box.clone(), tuple(pcl.shape), level, iterations, tol, max_step, max_dist))
        return snapped, {}
    monkeypatch.setattr(mesh, 'extract_isosurface', isosurface)
    monkeypatch.setattr(mesh, 'smooth_mesh', smooth)
    monkeypatch.setattr(mesh, 'snap_mesh', snap)
    d = {'planes_channel_last': torch.zeros(2, 3, 4, 4, 2)}
    cell = 0.9 / (G - 1)
    v = mesh.mesh_from_grid(_Field(log), d, torch.zeros(G ** 3), G, thr=3.5, sample_index=1, smooth_iters=3, snap_iters=5, simplify_cell=2.0)[0]
    assert [e[0] for e in log] == ['extract_isosurface', 'smooth_mesh', 'snap_mesh', 'forward_points']
    assert log[0][1] == ('all', 0, 2.0)                                                   # the extraction is called exactly as before
    box = (smoothed / (G - 1) * 2 - 1) * 0.45                                             # the snap sees the SMOOTHED position in the box
    assert torch.equal(log[2][1], box) and log[2][2] == (1, 3, 4, 4, 2) and log[2][3:6] == (3.5, 5, None)
    assert math.isclose(log[2][7], 2.0 * cell) and math.isclose(log[2][6], 1.0 * cell)   # max(1, simplify_cell) cells, and half of it
    assert torch.equal(log[3][1], snapped)                                                # the query and the result see the SNAPPED position
    assert np.array_equal(v, (mesh.rotation_matrix_x(-90) @ snapped.numpy().T).T.astype(np.float32))
    del log[:]
    out = mesh.textured_mesh_from_grid(_Field(log), d, torch.zeros(G ** 3), G, texture_size=8, snap_iters=2, snap_tol=0.5, snap_max_move=3)
    assert [e[0] for e in log] == ['extract_isosurface', 'smooth_mesh', 'snap_mesh', 'forward_points'] and len(out) == 5
    assert log[2][4:6] == (2, 0.5) and math.isclose(log[2][7], 3 * cell) and math.isclose(log[2][6], 1.5 * cell) and log[2][3] == 10.0
    for off in (dict(), dict(snap_iters=0), dict(snap_iters=None)):                       # off: snap_mesh is not even called
        del log[:]
        mesh.mesh_from_grid(_Field(log), d, torch.zeros(G ** 3), G, **off)
        assert [e[0] for e in log] == ['extract_isosurface', 'smooth_mesh', 'forward_points'] and torch.equal(log[2][1], (raw / (G - 1) * 2 - 1) * 0.45)
    for bad in (dict(snap_iters=65), dict(snap_iters=-1), dict(snap_iters=2.5), dict(snap_iters=True), dict(snap_iters=1, snap_tol=-1.0),
                dict(snap_iters=1, snap_tol=float('nan')), dict(snap_iters=1, snap_max_move=0), dict(snap_iters=1, snap_max_move=float('inf')),
                dict(snap_iters=1, snap_max_move='far')):
        del log[:]
        with pytest.raises(ValueError, match='snap_'):
            mesh.mesh_from_grid(_Field(log), d, torch.zeros(G ** 3), G, **bad)
        assert log == []                                                                  # refused before anything is extracted


def test_the_default_call_launches_nothing_new():
    from ln3diff_amd import mesh

    class NoDecoder:
        def __getattr__(self, name):
            pytest.fail(f"{name} was reached")
    v = torch.rand(5, 3)
    for off in (0, None):
        a, diag = mesh.snap_mesh(NoDecoder(), None, v, 10.0, off)
        assert a is v and diag == {'residual': None, 'state': None, 'evals': None}
    a, diag = mesh.snap_mesh(NoDecoder(), None, v[:0], 10.0, 8)                           # an empty mesh returns empty
    assert a.shape == (0, 3) and diag['state'] is None


def test_wrappers_refuse_bad_arguments(monkeypatch):
    from ln3diff_amd import _lib, mesh, ops

    class NoLibrary:
        def __getattr__(self, name):
            def fail(*a):
                pytest.fail(f"{name} was reached")
            return fail
    monkeypatch.setattr(_lib, 'lib', lambda: NoLibrary())
    v = torch.rand(4, 3)
    for bad in (lambda: mesh.snap_mesh(None, None, v.double(), 1.0, 1), lambda: mesh.snap_mesh(None, None, v.reshape(-1), 1.0, 1),
                lambda: mesh.snap_mesh(None, None, v, 1.0, 65), lambda: mesh.snap_mesh(None, None, v, 1.0, -1),
                lambda: mesh.snap_mesh(None, None, v, 1.0, 1.5), lambda: mesh.snap_mesh(None, None, v, 1.0, 'many'),
                lambda: mesh.snap_mesh(None, None, v, 1.0, 1, tol=-1.0), lambda: mesh.snap_mesh(None, None, v, 1.0, 1, tol=float('inf'))):
        with pytest.raises(ValueError):
            bad()
    assert mesh._snap_args(None) == (0, None, None) and mesh._snap_args(np.int64(3), 0.5, 2) == (3, 0.5, 2.0) and mesh.SNAP_MAX_ITERS == 64
    H, W = 4, 6
    pl, dec = torch.zeros(3, H, W, 32), (torch.zeros(64, 32), torch.zeros(64), torch.zeros(4, 64), torch.zeros(4))
    out, res, st, ev = torch.zeros(4, 3), torch.zeros(4), torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    good = dict(level=1.0, iters=4, tol=1e-3, max_step=0.01, max_dist=0.02)

    def call(planes=pl, pts=v, o=out, r=res, s=st, e=ev, **kw):
        a = dict(good, **kw)
        return ops.snap_points(planes, H, W, pts, dec, 0.9, a['level'], a['iters'], a['tol'], a['max_step'], a['max_dist'], o, r, s, e)
    with pytest.raises(RuntimeError, match="need device tensors"):                        # a host tensor never reaches the library
        call()
    with pytest.raises(RuntimeError, match="need device tensors"):
        call(planes=pl.half())
    with pytest.raises(TypeError, match="float32 or torch.float16"):
        call(planes=pl.double())
    for bad in (lambda: call(pts=v.double()), lambda: call(pts=v[:, :2]), lambda: call(pts=torch.zeros(4, 6)[:, ::2]), lambda: call(pts=v[:0], o=out[:0], r=res[:0], s=st[:0], e=ev[:0]),
                lambda: call(o=out[:3]), lambda: call(o=out.double()), lambda: call(o=v), lambda: call(r=res[:3]), lambda: call(r=res.double()),
                lambda: call(s=st.long()), lambda: call(s=st[:3]), lambda: call(e=ev.long()), lambda: call(e=torch.zeros(8, dtype=torch.int32)[::2]),
                lambda: call(planes=pl[:2]), lambda: call(planes=torch.zeros(3, H, W, 64)[..., ::2]), lambda: call(planes=pl[None]),
                lambda: call(iters=65), lambda: call(iters=-1), lambda: call(iters=2.0), lambda: call(iters=True),
                lambda: call(level=float('nan')), lambda: call(level=1e39), lambda: call(tol=-1e-3), lambda: call(tol=float('inf')),
                lambda: call(max_step=0.0), lambda: call(max_step=-1.0), lambda: call(max_step=float('nan')), lambda: call(max_step=1e-60),
                lambda: call(max_dist=-0.5), lambda: call(max_dist=float('inf')), lambda: call(max_dist='far')):
        with pytest.raises(ValueError):
            bad()


if __name__ == '__main__':
    w = _worst_sigma_ulps()
    print(f"MEASURED_SIGMA_F32_ULPS = {w:.4g}   SIGMA_BOUND_ULPS = {4 * w:.4g}")
