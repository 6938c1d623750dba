"""The float64 iso-surface reference (tests/mesh_refs.py) and the marching-cubes table (csrc/mc_table.h) checked on their own, without a
GPU: the table against the sign patterns it has to serve, the reference against closedness, winding and the scikit-image golden, on the
fields that tests/test_mesh_cells_gpu.py then holds the kernels to (profiles/mesh_cells.md)."""
import itertools

import numpy as np
import pytest

import mesh_refs as R
from conftest import golden


@pytest.fixture(scope='module')
def table():
    return R.load_mc_table()


@pytest.fixture(scope='module')
def noise(table):
    s = R.noise_field()
    return s, R.ref_cells(s, 0.0), {'cubes': R.ref_cubes(s, 0.0, table), 'tetra': R.ref_tetra(s, 0.0)}


@pytest.fixture(scope='module')
def atlas(table):
    s = R.atlas_field()
    return s, R.ref_cells(s, 0.0), {'cubes': R.ref_cubes(s, 0.0, table), 'tetra': R.ref_tetra(s, 0.0)}


def _face_of(e, axis, side):
    a, b = R.edge_corners(e)
    return R.CORNER[a][axis] == side and R.CORNER[b][axis] == side


def test_table_rows_use_exactly_the_sign_changing_edges(table):
    tri, cnt = table
    for case in range(256):
        want = {e for e in range(12) if len({(case >> c) & 1 for c in R.edge_corners(e)}) == 2}
        assert {e for t in tri[case] for e in t} == want, case
        assert cnt[case] == len(tri[case]), case
        assert all(len(set(t)) == 3 for t in tri[case]), case


def test_table_rows_are_oriented_surfaces_that_meet_across_cell_faces(table):
    """Without a field: inside a row a directed edge occurs once, and an edge that does not lie in a face of the cell occurs in both
    directions; an edge in a cell face occurs once, and the cell beyond that face - any of the 16 cases that share its four corners -
    has the same edge in the opposite direction.  A row with two ids swapped fails here whatever the rest of the suite covers."""
    tri, _ = table
    on_face = {}
    for case in range(256):
        d = [(t[i], t[(i + 1) % 3]) for t in tri[case] for i in range(3)]
        assert len(set(d)) == len(d), case
        for a, b in d:
            shared = [(ax, s) for ax in range(3) for s in (0, 1) if _face_of(a, ax, s) and _face_of(b, ax, s)]
            assert len(shared) <= 1
            if not shared:
                assert (b, a) in d, (case, a, b)
            else:
                assert (b, a) not in d, (case, a, b)
                on_face.setdefault((case, shared[0]), set()).add((a, b))

    def across(e, ax):                              # the same grid edge seen from the cell on the other side of a face normal to ax
        a, b = R.edge_corners(e)
        return next(f for f in range(12) if R.edge_corners(f) == (a ^ (1 << ax), b ^ (1 << ax)))

    for case, ax in itertools.product(range(256), range(3)):
        hi = [c for c in range(8) if R.CORNER[c][ax] == 1]
        here = {(across(b, ax), across(a, ax)) for a, b in on_face.get((case, (ax, 1)), ())}
        for free in range(16):
            lo = [c for c in range(8) if R.CORNER[c][ax] == 0]
            other = sum(((case >> c) & 1) << (c ^ (1 << ax)) for c in hi) | sum(((free >> i) & 1) << (lo[i] ^ (1 << ax)) for i in range(4))
            assert on_face.get((other, (ax, 0)), set()) == here, (case, ax, other)


def test_atlas_holds_every_case_in_a_closed_outward_block(atlas):
    s, cells, refs = atlas
    assert s.shape == (28, 28, 28)
    centre = cells['case'].reshape(27, 27, 27)[1::4, 1::4, 1::4].reshape(-1)[:256]
    assert centre.tolist() == list(range(256))
    assert len(np.unique(cells['case'])) == 256
    for name, ref in refs.items():
        blk = R.atlas_block_of(ref)
        assert set(blk.tolist()) == set(range(1, 256)), name
        for k in range(1, 256):
            m = blk == k
            h = R.edge_histogram(ref['key'][m], R.ATLAS_G)
            assert (h['undirected'] == 2).all() and h['directed_max'] == 1, (name, k)
            assert R.signed_volume(ref['pos'][m]) > 0, (name, k)


def test_noise_field_holds_every_case_and_both_surfaces_are_closed(noise):
    s, cells, refs = noise
    assert s.shape == (12, 12, 12) and not (s == 0).any()
    assert len(np.unique(cells['case'])) == 256
    for name, ref in refs.items():
        h = R.edge_histogram(ref['key'], 12)
        assert h['boundary'].any() and not h['boundary'].all()
        assert (h['undirected'][~h['boundary']] == 2).all(), name
        assert (h['undirected'][h['boundary']] == 1).all(), name
        assert h['directed_max'] == 1, name


def test_tetrahedra_winding_is_decided_well_away_from_zero(noise, atlas):
    """The kernel takes the sign of normal . dir in float32.  Its error there: a coordinate is within 15 u of float64 (position_bound at
    coordinates below 12; 31 u below 28), an edge vector of length <= 1 within 2 * 15 u + u, a cross-product component (two products of
    such, three roundings) within 127 u, the dot product with |dir_i| <= 1 within 400 u = 2.4e-5 (820 u = 4.9e-5 on the atlas).  The noise
    seed is the one of the first 400 with all 256 cases whose smallest |normal . dir| is largest; both fields stay clear of that error,
    so the float32 and float64 decisions agree on every triangle and the kernel's corner order can be compared exactly."""
    assert np.abs(noise[2]['tetra']['winding_margin']).min() > 400 * R.U
    assert np.abs(atlas[2]['tetra']['winding_margin']).min() > 820 * R.U


@pytest.mark.parametrize('name', ['field', 'sphere'])
def test_reference_replays_the_classic_golden(table, name):
    g = golden('mcubes_classic')
    ref = R.ref_cubes(g[name + '_sigma'], float(g[name + '_level']), table)
    want = g[name + '_tri']
    assert ref['pos'].shape == want.shape
    assert len(np.unique(ref['key'])) == int(g[name + '_nverts'])
    a, b = R.canon(ref['pos']), R.canon(want)
    assert np.abs(a - b).max() < 1e-6, np.abs(a - b).max()            # the golden is stored in float32: half an ulp of 13 is 4.8e-7


def test_golden_reaches_166_cases():
    """what the scikit-image golden alone covers (the reason for the atlas)"""
    g = golden('mcubes_classic')
    seen = set()
    for name in ('field', 'sphere'):
        seen |= set(R.ref_cells(g[name + '_sigma'], float(g[name + '_level']))['case'].tolist())
    assert len(seen) == 166


def test_tie_field_positions_are_exact(table):
    s = R.tie_field()
    assert s.shape == (8, 8, 8) and set(np.unique(s).tolist()) == {9.0, 10.0, 11.0}
    for ref in (R.ref_cubes(s, 10.0, table), R.ref_tetra(s, 10.0)):
        assert set(np.unique(ref['t']).tolist()) == {0.0, 0.5, 1.0}
        assert np.array_equal(ref['pos'] * 2, np.round(ref['pos'] * 2))
        assert np.array_equal(ref['pos'].astype(np.float32).astype(np.float64), ref['pos'])
        assert R.zero_area_faces(ref['pos']) > 0                      # vertices that land on a grid node collapse faces
        faces = R.weld(ref)[1]
        assert len(faces) == len(ref['key'])                          # ... but never two corners on one grid edge: nothing is dropped


def test_nonfinite_rule_of_the_reference(table):
    s = R.nonfinite_field()
    assert np.isinf(s).sum() == 4 and np.isnan(s).sum() == 2
    for ref in (R.ref_cubes(s, 0.0, table), R.ref_tetra(s, 0.0)):
        assert np.isfinite(ref['pos']).all() and (ref['t'] >= 0).all() and (ref['t'] <= 1).all()
        n = R.key_nodes(ref['key'], 6).astype(np.float64)
        assert (ref['pos'] >= n.min(-2)).all() and (ref['pos'] <= n.max(-2)).all()
        ends = s.reshape(-1)[np.stack([ref['key'] // 216, ref['key'] % 216], -1)].astype(np.float64)
        fin = np.isfinite(ends)
        assert (ref['t'][fin[..., 0] & ~fin[..., 1]] == 0).all() and (ref['t'][~fin[..., 0] & fin[..., 1]] == 1).all()
        assert (ref['t'][~fin[..., 0] & ~fin[..., 1]] == 0.5).all() and (~fin[..., 0] & ~fin[..., 1]).any()
        big = fin.all(-1) & (np.abs(ends) > 1e38).all(-1)
        assert big.any() and np.allclose(ref['t'][big], 0.5)


def test_volume_and_histogram_on_a_unit_tetrahedron():
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64)
    f = [(0, 2, 1), (0, 1, 3), (1, 2, 3), (0, 3, 2)]                     # outward
    assert abs(R.signed_volume(p[np.array(f)]) - 1 / 6) < 1e-15
    G = 4
    keys = np.array([0 * G ** 3 + 1, 21 * G ** 3 + 22, 21 * G ** 3 + 25, 21 * G ** 3 + 37])      # any four distinct grid edges
    h = R.edge_histogram(keys[np.array(f)], G)
    assert (h['undirected'] == 2).all() and h['directed_max'] == 1 and len(h['pair']) == 6 and not h['boundary'].any()
    f[3] = (0, 2, 3)                                                     # one face turned over
    assert R.edge_histogram(keys[np.array(f)], G)['directed_max'] == 2
    assert R.edge_histogram(np.array([[0 * G ** 3 + 1, 1 * G ** 3 + 2, 1 * G ** 3 + 5]]), G)['boundary'].all()    # all on x = 0
