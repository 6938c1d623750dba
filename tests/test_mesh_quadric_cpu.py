"""The quadric-error placement of include/ln3d_meshquadric.h without a GPU:
  - what the float64 reference achieves (the figures the feature was proposed with): creases of a box to 1e-3 cells where the mean is 0.4
    cells off, every cluster inside its cell, and NO gain on a sphere, clean or noisy;
  - the calibration of mesh_quadric_refs.POSITION_BOUND: the fp32 restatement against float64 over every input of the GPU test, times 4;
  - the fp32 restatement passes every check tests/test_mesh_quadric_gpu.py makes on exactly that test's inputs, and each of four seeded
    faults (a missing face, a corner taken twice, lambda from the wrong trace, the plane offset against the origin) fails one;
  - the pair keys of the definition on the hand-made incidence mesh;
  - both entry points validate on fake addresses before they launch;
  - mesh_simplify_placement from every public entry of pipeline down to mesh_from_grid / textured_mesh_from_grid and on to
    extract_isosurface and simplify_mesh, handed on only when it is not 'mean'; the launcher flag; the ValueErrors."""
import numpy as np
import pytest
import torch

import mesh_quadric_refs as R
import mesh_simplify_refs as S
from abi_args import BAD_ARG, BIG, UNSUPPORTED, with_args as _with

HOST_SPREAD = 0.25               # relative: the maximum over clusters of a rounding error moves with the host's float32 / LAPACK details
P0, Q0 = 0x10000, 0x4000000      # two fake device addresses, 64 MiB apart
PLACED = [n for n in R.cases() if n not in R.PAIRS_ONLY]


# ---------------------------------------------------------------- what the reference achieves
@pytest.mark.parametrize('edge,n,cell,nc,mean_min,quad_max', [(6.0, 13, 2.0, 56, 0.37, 2e-3), (50.0, 101, 3.0, 1736, 0.42, 2e-3)])
def test_the_reference_keeps_the_creases_of_a_box(edge, n, cell, nc, mean_min, quad_max):
    v, f, lo, hi = R.grid_box(edge, n)
    assert (len(v), len(f)) == (6 * (n - 1) ** 2 + 2, 12 * (n - 1) ** 2)
    st = S.stages(v, f, cell, (0, 0, 0))
    st['key_unique'] = np.unique(st['key'])
    ref = R.place64(v, f, st, cell)
    d_mean, d_quad = R.box_distance(st['rep'], lo, hi).max(), R.box_distance(ref['rep'], lo, hi).max()
    print(f"[quadric] box edge {edge:g} cell {cell:g}: {st['nc']} clusters, largest distance from the box: mean {d_mean:.4g}, quadric {d_quad:.3g}")
    assert st['nc'] == nc and d_mean >= mean_min and d_quad <= quad_max
    assert ref['placed'].all() and (ref['margin'] > R.POSITION_BOUND).all()               # every cluster placed, inside its cell
    rep32, placed32 = R.place32(v, f, st, cell)
    assert np.array_equal(placed32, ref['placed'])                                        # the fp32 restatement sets the same flags


def test_the_reference_gains_nothing_on_a_sphere():
    """radius 60, 40 962 vertices, cell 3: the face planes of an inscribed mesh lie inside the surface, and the mean averages noise away"""
    v, f = R.icosphere(6, 60.0, (70.3, 70.45, 70.6))
    assert len(v) == 40962
    c = np.array([70.3, 70.45, 70.6])
    out = {}
    for name, verts in (('clean', v), ('noisy', (v + np.random.default_rng(1).normal(0, 0.3, v.shape)).astype(np.float32))):
        st = S.stages(verts, f, 3.0, (0, 0, 0))
        st['key_unique'] = np.unique(st['key'])
        ref = R.place64(verts, f, st, 3.0)
        dist = lambda p: float(np.median(np.abs(np.linalg.norm(p - c, axis=1) - 60.0)))   # noqa: E731
        out[name] = (dist(ref['rep']), dist(st['rep'].astype(np.float64)), float(ref['placed'].mean()))
        print(f"[quadric] sphere r 60 cell 3 {name}: median distance quadric {out[name][0]:.3g}, mean {out[name][1]:.3g}, placed {out[name][2]:.3f}")
    assert out['clean'][0] > out['clean'][1] and out['noisy'][0] > out['noisy'][1]


# ---------------------------------------------------------------- calibration, the stand-in, the faults
def _worst_deviation():
    worst = {}
    for name in PLACED:
        c = R.cases()[name]
        rep, placed = R.place32(c['verts'], c['faces'], c['st'], c['cell'])
        on = (placed != 0) & (c['ref']['placed'] != 0)
        dev = np.abs(rep.astype(np.float64) - c['ref']['x'])[on] / float(np.float32(c['cell']))
        worst[name] = float(dev.max()) if dev.size else 0.0
    return worst


def test_position_bound_calibration():
    worst = _worst_deviation()
    top = max(worst.values())
    print(f"[quadric] fp32 restatement against float64, in cells: {({k: float('%.3g' % v) for k, v in worst.items()})}; constants: measured "
          f"{R.MEASURED_F32_DEVIATION}, bound {R.POSITION_BOUND}")
    assert abs(top - R.MEASURED_F32_DEVIATION) <= HOST_SPREAD * R.MEASURED_F32_DEVIATION, (top, R.MEASURED_F32_DEVIATION)
    assert R.POSITION_BOUND == 4 * R.MEASURED_F32_DEVIATION and R.POSITION_BOUND < 1e-2 / 100            # a real fault moves 1e-2 cells or more


@pytest.mark.parametrize('name', PLACED)
def test_standin_passes_every_gpu_check(name):
    c = R.cases()[name]
    rep, placed = R.place32(c['verts'], c['faces'], c['st'], c['cell'])
    fails, fig = R.check_placement(c, rep, placed, small=name in R.SMALL)
    assert fails == [], (name, fails, fig)


@pytest.mark.parametrize('fault', R.FAULTS)
def test_every_seeded_fault_fails_a_gpu_check(fault):
    caught = {}
    for name in PLACED:
        c = R.cases()[name]
        rep, placed = R.place32(c['verts'], c['faces'], c['st'], c['cell'], fault=fault)
        fails, _ = R.check_placement(c, rep, placed, small=name in R.SMALL)
        if fails:
            caught[name] = fails
    print(f"[quadric] fault {fault}: caught on {sorted(caught)}")
    assert 'box6' in caught or 'incidence' in caught, fault                               # on a small named case, not only on a large one
    assert len(caught) >= 3


def test_named_cases_are_what_they_claim():
    C = R.cases()
    assert (len(C['box6']['verts']), len(C['box6']['faces']), C['box6']['st']['nc']) == (866, 1728, 56) and C['box6']['ref']['placed'].all()
    assert len(C['ico2_c4']['verts']) == 162 and len(C['ico4_c4']['verts']) == 2562
    fan = C['fan3000']
    assert fan['st']['nc'] == 1 and len(fan['faces']) == 3000 and fan['ref']['placed'].tolist() == [1]
    assert np.abs(fan['ref']['x'][0] - [1.2, 1.1, 1.7]).max() < 2e-2                      # the cone's planes meet at its apex
    assert C['zero_area']['ref']['trace'].tolist() == [0.0] and C['zero_area']['ref']['placed'].tolist() == [0]
    cop = C['coplanar']['ref']
    w = np.linalg.eigvalsh(cop['A'][0])
    assert cop['placed'].tolist() == [1] and w[1] < 1e-12 * w[2]                          # rank 1
    far = C['far_wedge']['ref']
    assert far['placed'].tolist() == [0] and far['x'][0, 0] < -0.3 and np.array_equal(far['rep'][0], far['mean'][0])
    for name in R.PAIRS_ONLY:                                                             # why their placements are not compared
        assert C[name]['ref']['doubt'].any()
    for name in PLACED:
        assert float(C[name]['ref']['doubt'].mean()) <= (0.0 if name in R.SMALL else R.MAX_SKIPPED), name


def test_pair_keys_of_the_incidence_mesh():
    c = R.cases()['incidence']
    assert c['st']['cluster'].tolist() == [0, 0, 2, 1, 0] and c['st']['nc'] == 3
    key = R.pairs(c['st']['cfaces'])
    got = sorted((int(k >> 31), int(k & 0x7fffffff)) for k in key if k != R.NONE)
    assert got == c['want'] and int((key == R.NONE).sum()) == 15 - len(c['want'])
    assert key[3:6].tolist() == [(0 << 31) | 1, R.NONE, R.NONE]                           # the collapsed face counts once, at its first corner
    assert key[12:15].tolist() == [(0 << 31) | 4, (2 << 31) | 4, R.NONE]                  # corners 0 and 2 share a cluster
    for name, c in R.cases().items():                                                     # the loop against a vectorised formula
        cf = c['st']['cfaces']
        f = np.arange(len(cf))
        want = np.stack([(cf[:, 0] << 31) | f, np.where(cf[:, 1] != cf[:, 0], (cf[:, 1] << 31) | f, R.NONE),
                         np.where((cf[:, 2] != cf[:, 0]) & (cf[:, 2] != cf[:, 1]), (cf[:, 2] << 31) | f, R.NONE)], -1).reshape(-1)
        assert np.array_equal(R.pairs(cf), want), name
        sk, start = R.rows(R.pairs(cf), c['st']['nc'])
        assert start[0] == 0 and start[-1] == int((sk != R.NONE).sum()) and (np.diff(start) >= 1).all()       # every cluster has a face or none has a vertex


# ---------------------------------------------------------------- entry points on fake addresses
def _pairs_args():
    # cfaces nf nc pair_key stream
    return [P0, 10, 4, Q0, None]


def _place_args():
    # verts nv faces nf sorted_pair_key npairs start nc rep_mean ox oy oz cell cluster_cell_key eps rep_out placed stream
    return [P0, 20, P0 + 0x1000, 10, P0 + 0x2000, 30, P0 + 0x3000, 4, P0 + 0x4000, 0.0, 0.5, -1.0, 2.0, P0 + 0x5000, 1e-3, Q0, Q0 + 0x1000, None]


def test_quadric_pairs_validates_before_it_launches(hip_lib):
    fn, args = hip_lib.ln3d_quadric_pairs, _pairs_args()
    for i in (0, 3):
        assert fn(*_with(args, **{'i%d' % i: None})) == BAD_ARG, ('null buffer', i)
    for i in (1, 2):
        for bad in (0, -1, BIG, 1 << 40):
            assert fn(*_with(args, **{'i%d' % i: bad})) == BAD_ARG, (i, bad)
    assert fn(*_with(args, i2=(1 << 21) + 1)) == UNSUPPORTED


def test_quadric_place_validates_before_it_launches(hip_lib):
    fn, args = hip_lib.ln3d_quadric_place, _place_args()
    for i in (0, 2, 4, 6, 8, 13, 15, 16):
        assert fn(*_with(args, **{'i%d' % i: None})) == BAD_ARG, ('null buffer', i)
    for i in (1, 3, 7):
        for bad in (0, -1, BIG, 1 << 40):
            assert fn(*_with(args, **{'i%d' % i: bad})) == BAD_ARG, ('count', i, bad)
    for bad in (0, -1, 31, 1 << 40):
        assert fn(*_with(args, i5=bad)) == BAD_ARG, ('npairs', bad)                       # below 1 or above 3 nf
    assert fn(*_with(args, i7=21)) == BAD_ARG                                             # nc > nv
    assert fn(*_with(args, i1=1 << 22, i7=(1 << 21) + 1)) == UNSUPPORTED
    for i in (9, 10, 11, 12, 14):
        for bad in (float('nan'), float('inf'), -float('inf')):
            assert fn(*_with(args, **{'i%d' % i: bad})) == BAD_ARG, ('non-finite', i, bad)
    for bad in (0.0, -2.0):
        assert fn(*_with(args, i12=bad)) == BAD_ARG, ('cell', bad)
    for bad in (0.0, -1e-3, 1.0001, 2.0):
        assert fn(*_with(args, i14=bad)) == BAD_ARG, ('eps', bad)
    for shift in (4, 12 * 4 - 4, -(12 * 4 - 4)):                                          # rep_out overlaps rep_mean: nc = 4 rows of 12 bytes
        assert fn(*_with(args, i15=args[8] + shift)) == BAD_ARG, shift
    assert b'bad argument' in hip_lib.ln3d_strerror(BAD_ARG)


class _Field:
    def __init__(self, log):
        self.log = log

    def forward_points(self, pcl, pts, with_grad=False):
        self.log.append(('forward_points', pts[0].clone()))
        return {'rgb': torch.zeros_like(pts), 'normal': torch.zeros_like(pts)}

    def snap_points(self, pcl, pts, level, iters, **kw):
        self.log.append(('snap_points', pts[0].clone()))
        return {'points': pts + 1.0, 'residual': pts[..., 0], 'state': pts[..., 0].int(), 'evals': pts[..., 0].int()}


def test_the_placement_reaches_the_extraction_and_nothing_else_moves(monkeypatch):
    from ln3diff_amd import mesh
    log = []
    G = 8
    raw, faces = torch.tensor([[1.0, 2.0, 3.0]]), torch.zeros(0, 3, dtype=torch.int64)

    def isosurface(sigma, thr, method, *post, **kw):
        log.append(('extract_isosurface', post, kw))
        return raw, faces

    def smooth(verts, f, iterations, lam, mu, check=True):
        log.append(('smooth_mesh', verts.clone(), iterations))
        return verts + 0.5, f
    monkeypatch.setattr(mesh, 'extract_isosurface', isosurface)
    monkeypatch.setattr(mesh, 'smooth_mesh', smooth)
    d = {'planes_channel_last': torch.zeros(2, 3, 4, 4, 2)}
    for off in (dict(), dict(simplify_placement='mean')):                                 # the extraction is called exactly as before
        del log[:]
        mesh.mesh_from_grid(_Field(log), d, torch.zeros(G ** 3), G, simplify_cell=2.0, **off)
        assert log[0] == ('extract_isosurface', ('all', 0, 2.0), {})
    del log[:]
    mesh.mesh_from_grid(_Field(log), d, torch.zeros(G ** 3), G, simplify_cell=2.0, simplify_placement='quadric', smooth_iters=2, snap_iters=3)
    assert [e[0] for e in log] == ['extract_isosurface', 'smooth_mesh', 'snap_points', 'forward_points']      # extract -> smooth -> snap -> query
    assert log[0][1:] == (('all', 0, 2.0), dict(simplify_placement='quadric'))
    assert torch.equal(log[1][1], raw) and torch.equal(log[3][1], log[2][1] + 1.0)        # the query sees what the snap returned
    del log[:]
    out = mesh.textured_mesh_from_grid(_Field(log), d, torch.zeros(G ** 3), G, texture_size=8, simplify_cell=3.0, simplify_placement='quadric')
    assert log[0][1:] == (('all', 0, 3.0), dict(simplify_placement='quadric')) and len(out) == 5
    for bad in ('Quadric', 'qem', None, 1, b'mean'):
        del log[:]
        with pytest.raises(ValueError, match='placement'):
            mesh.mesh_from_grid(_Field(log), d, torch.zeros(G ** 3), G, simplify_cell=2.0, simplify_placement=bad)
        assert log == []                                                                  # refused before anything is extracted


def test_extract_isosurface_hands_the_placement_to_simplify_mesh(monkeypatch):
    from ln3diff_amd import mesh, ops
    seen = []
    e3, ef = torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64)

    def count(sigma, G, thr, counts):
        counts.zero_()
        counts[0] = 1

    def emit(sigma, G, thr, offs, pos, key):
        pos.copy_(torch.tensor([[0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5]]))
        key.copy_(torch.tensor([3, 1, 2]))

    def simplify(verts, faces, cell, origin=None, check=True, **kw):
        seen.append((cell, origin, check, kw))
        return e3, ef
    monkeypatch.setattr(ops, 'mcubes_count', count)
    monkeypatch.setattr(ops, 'mcubes_emit', emit)
    monkeypatch.setattr(mesh, 'simplify_mesh', simplify)
    sigma = torch.zeros(3, 3, 3)
    mesh.extract_isosurface(sigma, 10.0, 'cubes', 'all', 0, 2.0)
    mesh.extract_isosurface(sigma, 10.0, 'cubes', 'all', 0, 2.0, simplify_placement='mean')
    mesh.extract_isosurface(sigma, 10.0, 'cubes', 'all', 0, 2.0, simplify_placement='quadric')
    assert seen == [(2.0, (0.0, 0.0, 0.0), False, {})] * 2 + [(2.0, (0.0, 0.0, 0.0), False, dict(placement='quadric'))]
    with pytest.raises(ValueError, match='placement'):
        mesh.extract_isosurface(sigma, 10.0, simplify_placement='median')
    assert len(seen) == 3


def test_the_default_call_launches_nothing_new(monkeypatch):
    from ln3diff_amd import _lib, mesh, ops

    class NoLibrary:
        def __getattr__(self, name):
            def fail(*a):
                pytest.fail(f"{name} was reached")
            return fail
    monkeypatch.setattr(_lib, 'lib', lambda: NoLibrary())
    v, f = torch.rand(5, 3), torch.tensor([[0, 1, 2], [2, 3, 4]])
    for kw in (dict(), dict(placement='quadric'), dict(placement='quadric', quadric_eps=0.5)):     # no cell: its arguments, whatever the placement
        for cell in (0, None):
            a, b = mesh.simplify_mesh(v, f, cell, **kw)
            assert a is v and b is f
    for bad in (dict(placement='bogus'), dict(placement=None), dict(placement='quadric', quadric_eps=0.0), dict(placement='quadric', quadric_eps=1.5),
                dict(placement='quadric', quadric_eps=float('nan')), dict(placement='mean', quadric_eps='small')):
        with pytest.raises(ValueError, match='placement|quadric_eps'):
            mesh.simplify_mesh(v, f, 2.0, **bad)                                          # before anything is launched
    with pytest.raises(ValueError, match='cell'):
        mesh.simplify_placement(v, f, 0)
    with pytest.raises(ValueError, match='quadric_eps'):
        mesh.simplify_placement(v, f, 2.0, eps=-1.0)
    assert mesh.PLACEMENTS == ('mean', 'quadric') and mesh.QUADRIC_EPS == 1e-3
    # 'mean' reaches none of the two new wrappers: the stages it launches are the ones it always launched
    called = []
    for name in ('quadric_pairs', 'quadric_place'):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: called.append(_n))
    with pytest.raises(RuntimeError, match='need device tensors'):                        # host tensors: refused at the first stage
        mesh.simplify_mesh(v, f, 2.0, placement='mean', check=False)
    assert called == []


def test_wrappers_refuse_bad_buffers(monkeypatch):
    from ln3diff_amd import _lib, ops

    class NoLibrary:
        def __getattr__(self, name):
            def fail(*a):
                pytest.fail(f"{name} was reached")
            return fail
    monkeypatch.setattr(_lib, 'lib', lambda: NoLibrary())
    nv, nf, nc = 6, 4, 3
    verts, faces, cf = torch.rand(nv, 3), torch.zeros(nf, 3, dtype=torch.int64), torch.zeros(nf, 3, dtype=torch.int64)
    key, start, rep, ck = torch.zeros(3 * nf, dtype=torch.int64), torch.zeros(nc + 1, dtype=torch.int64), torch.zeros(nc, 3), torch.zeros(nc, dtype=torch.int64)
    out, placed = torch.zeros(nc, 3), torch.zeros(nc, dtype=torch.int32)
    for bad in (lambda: ops.quadric_pairs(cf.int(), nc, key), lambda: ops.quadric_pairs(cf, nc, key[:-1]), lambda: ops.quadric_pairs(cf[:, :2], nc, key),
                lambda: ops.quadric_pairs(cf + nc, nc, key), lambda: ops.quadric_pairs(cf - 1, nc, key)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError, match="need device tensors"):
        ops.quadric_pairs(cf, nc, key)

    def place(v=verts, f=faces, k=key, s=start, r=rep, c=ck, eps=1e-3, o=out, p=placed, check=True):
        return ops.quadric_place(v, f, k, s, r, (0, 0, 0), 2.0, c, eps, o, p, check=check)
    for bad in (lambda: place(v=verts.double()), lambda: place(f=faces.int()), lambda: place(k=key[:-3]), lambda: place(s=start[:-1]),
                lambda: place(r=rep[:, :2]), lambda: place(c=ck.int()), lambda: place(o=out[:2]), lambda: place(o=out.double()),
                lambda: place(p=placed.long()), lambda: place(p=torch.zeros(2 * nc, dtype=torch.int32)[::2]), lambda: place(eps=0.0),
                lambda: place(eps=1.5), lambda: place(eps=float('nan')), lambda: place(eps='tiny'), lambda: place(f=faces + nv)):        # (a bad start: tests/test_mesh_quadric_gpu.py - a host tensor that passes check_index is refused before it)
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError, match="need device tensors"):
        place()


if __name__ == '__main__':
    w = _worst_deviation()
    print(w)
    print(f"MEASURED_F32_DEVIATION = {max(w.values()):.3g}   POSITION_BOUND = {4 * max(w.values()):.3g}")
