"""The four iso-surface entry points (csrc/mesh.hip: ln3d_mcubes_count / emit, ln3d_mesh_count / emit) called directly and held per cell,
per triangle and per coordinate to the float64 reference of tests/mesh_refs.py (itself checked in tests/test_mesh_refs_cpu.py): all 256
marching-cubes cases (the atlas), arbitrary sign patterns with a partial last block (noise, 1331 cells), corner values equal to the level
(ties), a single cell, empty grids and non-finite values.

counts and tri_key are compared exactly and in emission order.  tri_pos: per coordinate |kernel - float64| <= 4 u |t| |b - a| +
u max(|coord|, 1), u = 2^-24 (mesh_refs.position_bound: two rounded subtractions and a division in t, an exact product with b - a in
{0, 1}, one rounding of the sum); on the tie field every operation is exact and the positions equal the reference's bit for bit.
Measured maxima: profiles/mesh_cells.md."""
import numpy as np
import pytest
import torch

import mesh_refs as R

pytestmark = pytest.mark.gpu

GUARD = 64                                  # triangles beyond ntri that emit must leave alone
METHODS = ('cubes', 'tetra')
FIELDS = {'atlas': (R.atlas_field, 0.0), 'noise': (R.noise_field, 0.0), 'tie': (R.tie_field, 10.0), 'nonfinite': (R.nonfinite_field, 0.0)}
_SENTINEL = np.array([0x7fc0beef], dtype=np.int32).view(np.float32)[0]          # a NaN with a payload no arithmetic produces


def _ops(method):
    from ln3diff_amd import ops
    return {'cubes': (ops.mcubes_count, ops.mcubes_emit), 'tetra': (ops.mesh_count, ops.mesh_emit)}[method]


def _emit(sigma, thr, method):
    """count -> prefix sum -> emit into sentinel-filled buffers with a guard tail: dict(counts [ncell], key [T,3], pos [T,3,3] f32), after
    checking that every slot below T was written and nothing behind it"""
    count, emit = _ops(method)
    sigma = torch.as_tensor(sigma).cuda().contiguous().float()
    G = sigma.shape[0]
    counts = torch.full(((G - 1) ** 3,), -7, dtype=torch.int32, device='cuda')
    count(sigma, G, thr, counts)
    offs = torch.cumsum(counts.long(), 0)
    T = int(offs[-1])
    assert int(counts.min()) >= 0 and T <= 12 * (G - 1) ** 3
    pos = torch.full(((T + GUARD) * 3, 3), float('nan'), device='cuda')
    pos.view(torch.int32).fill_(int(_SENTINEL.view(np.int32)))
    key = torch.full(((T + GUARD) * 3,), -1, dtype=torch.int64, device='cuda')
    emit(sigma, G, thr, offs, pos, key)
    torch.cuda.synchronize()
    pos, key = pos.cpu().numpy(), key.cpu().numpy()
    assert (key[T * 3:] == -1).all() and (pos[T * 3:].view(np.int32) == _SENTINEL.view(np.int32)).all(), 'emit wrote behind its last triangle'
    assert (key[:T * 3] >= 0).all() and not (pos[:T * 3].view(np.int32) == _SENTINEL.view(np.int32)).any(), 'emit left a slot unwritten'
    return dict(counts=counts.cpu().numpy(), key=key[:T * 3].reshape(T, 3), pos=pos[:T * 3].reshape(T, 3, 3))


@pytest.fixture(scope='module')
def ref():
    """(field, method) -> the float64 reference, computed once"""
    table, cache = R.load_mc_table(), {}

    def get(field, method):
        if (field, method) not in cache:
            make, thr = FIELDS[field]
            cache[field, method] = R.ref_cubes(make(), thr, table) if method == 'cubes' else R.ref_tetra(make(), thr)
        return cache[field, method]
    return get


@pytest.fixture(scope='module')
def out(hip_lib):
    """(field, method) -> the kernels' emission, run once"""
    cache = {}

    def get(field, method):
        if (field, method) not in cache:
            make, thr = FIELDS[field]
            cache[field, method] = _emit(make(), thr, method)
        return cache[field, method]
    return get


def _check_positions(name, got, want):
    err = np.abs(got['pos'].astype(np.float64) - want['pos'])
    bound = R.position_bound(want)
    print('%s: %d triangles, max |dpos| %.3e, bound there %.3e, max err / bound %.3f'
          % (name, len(err), err.max(), bound.reshape(-1)[err.argmax()], (err / bound).max()))
    assert (err <= bound).all(), (name, float((err / bound).max()))


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('field', ['atlas', 'noise', 'tie'])
def test_counts_keys_and_positions_per_cell(out, ref, field, method):
    """counts per cell, then every triangle at its offset, corner by corner: the emission order (cells in index order, the table row's or
    the tetrahedra's order inside a cell), the canonical edge orientation of the key and the winding are all in the exact key comparison"""
    got, want = out(field, method), ref(field, method)
    assert got['counts'].shape == want['counts'].shape and np.array_equal(got['counts'], want['counts'])
    assert np.array_equal(got['key'], want['key'])
    _check_positions('%s/%s' % (field, method), got, want)
    if field == 'tie':
        assert np.array_equal(got['pos'].view(np.int32), want['pos'].astype(np.float32).view(np.int32))


@pytest.mark.parametrize('method', METHODS)
def test_single_cell_grids(hip_lib, method):
    """G = 2: one cell, one thread of one block, offsets[cell - 1] never read"""
    table = R.load_mc_table()
    rng = np.random.default_rng(11)
    for case in (0, 255, 1, 128, 0x3c, 0x69, 0x96, 0x7f, 0xa5, 0x1b):
        s = -rng.uniform(0.2, 3.0, (2, 2, 2))
        for c in range(8):
            if (case >> c) & 1:
                s[R.CORNER[c]] = rng.uniform(0.2, 3.0)
        s = s.astype(np.float32)
        want = R.ref_cubes(s, 0.0, table) if method == 'cubes' else R.ref_tetra(s, 0.0)
        got = _emit(s, 0.0, method)
        assert np.array_equal(got['counts'], want['counts']) and np.array_equal(got['key'], want['key']), case
        assert (len(want['key']) == 0) == (case in (0, 255))
        if len(want['key']):
            _check_positions('G=2 case %d %s' % (case, method), got, want)


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('value', [-1.0, 1.0])
def test_empty_grids(hip_lib, method, value):
    from ln3diff_amd.mesh import extract_isosurface
    s = np.full((5, 5, 5), value, dtype=np.float32)
    got = _emit(s, 0.0, method)
    assert (got['counts'] == 0).all() and got['key'].shape == (0, 3)
    v, f = extract_isosurface(torch.from_numpy(s).cuda(), 0.0, method=method)
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and f.dtype == torch.int64


@pytest.mark.parametrize('method', METHODS)
def test_every_copy_of_a_vertex_has_the_same_bits(out, method):
    """extract_isosurface scatters verts[inv] = pos: a race unless the copies written by different cells and call sites are bitwise equal.
    Copies are grouped by the grid edge they lie on, whichever way round its key names the two nodes: one edge, one key, one position."""
    got = out('noise', method)
    G3 = 12 ** 3
    key, bits = got['key'].reshape(-1), got['pos'].reshape(-1, 3).view(np.int32).astype(np.int64)
    edge = np.minimum(key // G3, key % G3) * G3 + np.maximum(key // G3, key % G3)
    order = np.argsort(edge, kind='stable')
    edge, key, bits = edge[order], key[order], bits[order]
    start = np.flatnonzero(np.r_[True, edge[1:] != edge[:-1]])
    assert len(start) < len(edge) / 2                                 # every vertex has several copies
    assert (np.maximum.reduceat(key, start) == np.minimum.reduceat(key, start)).all()
    spread = np.maximum.reduceat(bits, start) - np.minimum.reduceat(bits, start)
    assert (spread == 0).all(), int((spread != 0).any(1).sum())


@pytest.fixture(scope='module')
def welded(out):
    """(field, method) -> extract_isosurface's (verts [Nv,3], faces [Nf,3]) and the sorted vertex keys of the same emission, run once"""
    from ln3diff_amd.mesh import extract_isosurface
    cache = {}

    def get(field, method):
        if (field, method) not in cache:
            make, thr = FIELDS[field]
            v, f = extract_isosurface(torch.from_numpy(make()).cuda(), thr, method=method)
            cache[field, method] = v.cpu().numpy(), f.cpu().numpy(), np.unique(out(field, method)['key'])
        return cache[field, method]
    return get


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('field', ['atlas', 'noise', 'tie'])
def test_extract_isosurface_welds_what_the_reference_welds(welded, ref, field, method):
    wkeys, wfaces, wpos, wbound = R.weld(ref(field, method))
    v, f, uniq = welded(field, method)
    assert v.shape == (len(wkeys), 3) and f.shape == wfaces.shape
    assert f.min() >= 0 and f.max() < len(v)
    assert np.array_equal(uniq, wkeys) and np.array_equal(f, wfaces)          # vertices in key order, faces in emission order
    assert (np.abs(v.astype(np.float64) - wpos) <= wbound).all()


@pytest.mark.parametrize('method', METHODS)
def test_noise_surface_is_closed_and_consistently_wound(welded, method):
    """on the kernels' own output, no reference: arbitrary sign patterns, welding across cell faces and, for the tetrahedra, across face and
    body diagonals - every edge off the grid boundary twice, every edge on it once, no directed edge twice"""
    v, f, uniq = welded('noise', method)
    assert f.max() < len(uniq) == len(v)
    h = R.edge_histogram(uniq[f], 12)
    assert h['boundary'].any() and (h['undirected'][~h['boundary']] == 2).all() and (h['undirected'][h['boundary']] == 1).all()
    assert h['directed_max'] == 1


@pytest.mark.parametrize('method', METHODS)
def test_atlas_blocks_are_closed_with_outward_normals(welded, method):
    """every one of the 255 non-empty cases in its own block: closed, every edge once per direction, positive signed volume"""
    v, f, uniq = welded('atlas', method)
    assert f.max() < len(uniq) == len(v)
    n = R.key_nodes(uniq[f], R.ATLAS_G) // 4
    assert (n == n[:, :1, :1, :]).all()
    blk = (n[:, 0, 0, 0] * 7 + n[:, 0, 0, 1]) * 7 + n[:, 0, 0, 2]
    assert set(blk.tolist()) == set(range(1, 256))
    for k in range(1, 256):
        m = blk == k
        h = R.edge_histogram(uniq[f[m]], R.ATLAS_G)
        assert (h['undirected'] == 2).all() and h['directed_max'] == 1, k
        assert R.signed_volume(v[f[m]]) > 0, k


@pytest.mark.parametrize('method', METHODS)
def test_tie_field_zero_area_faces(welded, ref, method):
    """vertices that land on a grid node (t = 0 or 1) collapse faces; none is dropped by the weld, and the kernels make as many as the
    reference"""
    v, f, _ = welded('tie', method)
    zero = R.zero_area_faces(v[f])
    print('tie/%s: %d faces, %d of zero area, %d vertices' % (method, len(f), zero, len(v)))
    assert zero == R.zero_area_faces(ref('tie', method)['pos']) and zero > 0


@pytest.mark.parametrize('method', METHODS)
def test_input_forms(hip_lib, method):
    """a transposed view and a float16 copy give exactly what their .contiguous().float() form gives"""
    from ln3diff_amd.mesh import extract_isosurface
    s = torch.from_numpy(R.noise_field()).cuda()
    for form in (s.permute(2, 0, 1), s.half(), s.half().permute(1, 2, 0)):
        assert form.dtype != torch.float32 or not form.is_contiguous()
        v0, f0 = extract_isosurface(form.contiguous().float(), 0.0, method=method)
        v1, f1 = extract_isosurface(form, 0.0, method=method)
        assert f0.shape[0] > 1000 and torch.equal(f0, f1) and torch.equal(v0.view(torch.int32), v1.view(torch.int32))


@pytest.mark.parametrize('method', METHODS)
def test_two_calls_are_bitwise_identical(out, method):
    a, b = out('noise', method), _emit(R.noise_field(), 0.0, method)
    assert np.array_equal(a['counts'], b['counts']) and np.array_equal(a['key'], b['key'])
    assert np.array_equal(a['pos'].view(np.int32), b['pos'].view(np.int32))


@pytest.mark.parametrize('method', METHODS)
def test_nonfinite_corners(out, ref, method):
    """include/ln3d.h: NaN and -inf are outside; a crossing between finite values is finite and on its edge even where v[b] - v[a] overflows
    (+-3e38 neighbours); with a +-inf or NaN end it sits on the finite end, with two such ends at the midpoint.  Every triangle holds the
    reference's three vertices (a zero-area triangle has no winding to compare), every vertex the reference's position."""
    got, want = out('nonfinite', method), ref('nonfinite', method)
    assert np.array_equal(got['counts'], want['counts'])
    assert np.isfinite(got['pos']).all()
    n = R.key_nodes(got['key'], 6).astype(np.float64)
    assert (got['pos'] >= n.min(-2)).all() and (got['pos'] <= n.max(-2)).all()           # within its edge
    assert np.array_equal(np.sort(got['key'], 1), np.sort(want['key'], 1))
    o_g, o_w = np.argsort(got['key'], 1), np.argsort(want['key'], 1)
    take = lambda a, o: np.take_along_axis(a, o[..., None], 1)
    err = np.abs(take(got['pos'], o_g).astype(np.float64) - take(want['pos'], o_w))
    bound = take(R.position_bound(want), o_w)
    print('nonfinite/%s: max err / bound %.3f' % (method, (err / bound).max()))
    assert (err <= bound).all()
    m = np.abs(want['winding_margin']) > 400 * R.U if method == 'tetra' else np.ones(len(want['key']), bool)
    assert np.array_equal(got['key'][m], want['key'][m])                                 # the winding wherever it is decided
