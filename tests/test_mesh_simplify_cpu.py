"""The numpy reference of the mesh simplification (tests/mesh_simplify_refs.py) against hand-written answers, its invariants on the iso-surfaces
of the fields of tests/mesh_clean_refs.py, the recorded counts, and seeded faults that the comparisons of tests/test_mesh_simplify_gpu.py must
catch: the reference's own tests, to which tests/test_mesh_simplify_gpu.py holds the package.  Then, still without a GPU, the package's
refusals: a host tensor never reaches the library through the ops wrappers, simplify_mesh refuses bad arguments before any launch, and
the launcher refuses every cell that the library would.  (tests/test_abi_cpu.py has the entry points' own argument validation.)"""
import numpy as np
import pytest
import torch

import mesh_clean_refs as M
import mesh_simplify_refs as S

F32 = np.float32
ZERO = (0.0, 0.0, 0.0)
NAN, INF = float('nan'), float('inf')


# ---------------------------------------------------------------- hand-made meshes, hand-written answers
@pytest.mark.parametrize('n', [4, 3, 2, 1])
def test_two_triangles_in_n_cells(n):
    v, f, cell, want_v, want_f = S.quad(n)
    s = S.stages(v, f, cell, ZERO)
    assert s['nc'] == n and s['degenerate'] == {4: 0, 3: 1, 2: 2, 1: 2}[n] and s['duplicate'] == 0
    assert np.array_equal(S.bits(s['verts']), S.bits(want_v)) and np.array_equal(s['faces'], want_f)
    assert s['verts'].dtype == F32 and s['faces'].dtype == np.int64 and s['verts'].shape[1:] == (3,) and s['faces'].shape[1:] == (3,)
    if n == 3:                                                      # the mean of (0.5, 1.5) and (0.75, 1.25), by hand
        assert s['rep'][1].tolist() == [0.625, 1.375, 0.0] and s['keep_f'].tolist() == [1, 0] and s['fkey'].tolist() == [(1 << 21) | 2, -1]
    if n == 4:                                                      # keys by hand: cells (0,0) (1,0) (0,1) (1,1) -> x << 42 | y << 21
        assert s['key'].tolist() == [0, 1 << 42, 1 << 21, (1 << 42) | (1 << 21)] and s['cluster'].tolist() == [0, 2, 1, 3]
        assert s['fkey'].tolist() == [(1 << 21) | 2, (1 << 42) | (2 << 21) | 3]


def test_opposite_windings_are_duplicates():
    v, f, cell, want_v, want_f = S.opposite_pair()
    s = S.stages(v, f, cell, ZERO)
    assert s['keep_f'].tolist() == [1, 0, 0] and s['duplicate'] == 2 and len(set(s['fkey'].tolist())) == 1
    assert np.array_equal(S.bits(s['verts']), S.bits(want_v)) and np.array_equal(s['faces'], want_f)      # face 0's own corner order


def test_a_vertex_on_a_cell_boundary():
    # a representable cell: 3 * 0.5 = 1.5 exactly; one ulp below falls into cell 2, the boundary and above into cell 3
    x = S.boundary(0.5)
    assert x[1] == 1.5 and S.cell_of(np.stack([x, x, x], 1), ZERO, 0.5)[:, 0].tolist() == [2, 3, 3]
    # cell = 0.1 is not representable: float32(0.1) = 13421773 * 2^-27 > 1/10, and what counts is the float32 quotient, worked out here in
    # exact integer arithmetic: x / c for x = m_x 2^e_x, c = m_c 2^e_c, rounded to nearest even at 24 bits, then floor
    c = F32(0.1)
    x = np.concatenate([S.boundary(0.1), np.array([0.3, 0.7, 1.0, 2.9, 12.3], dtype=F32)])
    got = S.cell_of(np.stack([x, x, x], 1), ZERO, 0.1)[:, 2].tolist()

    def exact_q(xv, cv):
        from fractions import Fraction
        q = Fraction(float(xv)) / Fraction(float(cv))               # both float32 values are exact binary fractions
        e = 0
        while q >= 1 << 24:
            q, e = q / 2, e + 1
        while q < 1 << 23:
            q, e = q * 2, e - 1
        n, r = divmod(q.numerator, q.denominator)
        half = Fraction(r, q.denominator)
        n += 1 if half > Fraction(1, 2) or (half == Fraction(1, 2) and n % 2) else 0
        return (Fraction(n) * Fraction(2) ** e).__floor__()
    assert got == [exact_q(xv, c) for xv in x]
    assert got[:3] == [2, 3, 3] and got[3] == 3 and got[5] == 10   # float32(0.3) / float32(0.1) rounds to exactly 3; float32(1) / float32(0.1) to 10
    # a negative origin and the clamp that makes the kernel total
    assert S.cell_of([[-1.0, -0.5, 0.0]], (-1.0, -1.0, -1.0), 0.5).tolist() == [[0, 1, 2]]
    assert S.cell_of([[-5.0, np.nan, 1e30]], ZERO, 1.0).tolist() == [[0, 0, S.QMAX]]
    assert S.keys(np.array([[S.QMAX + 0.5, 0.25, 7.0]], dtype=F32), ZERO, 1.0).tolist() == [(S.QMAX << 42) | 7]


# ---------------------------------------------------------------- invariants on the fields
def test_the_sweep_covers_every_field():
    assert {(n, m) for n, G, m in S.FIELD_CASES if G is None} == set(M.FIELDS) and len(M.FIELDS) == 4 and ('blob', 'tetra') in M.FIELDS


@pytest.mark.parametrize('cell', S.CELLS)
@pytest.mark.parametrize('name,G,method', S.FIELD_CASES, ids=['%s-%s' % (n, G) + ('' if m == 'cubes' else '-' + m) for n, G, m in S.FIELD_CASES])
def test_invariants_on_fields(name, G, method, cell):
    v, f = S.welded(name, G, method)
    if G is None:
        assert (len(v), len(f)) == (M.FIELDS[name, method]['nv'], M.FIELDS[name, method]['nf'])
    for origin in (ZERO, None):
        s = S.stages(v, f, cell, origin)
        sv, sf = s['verts'], s['faces']
        assert not ((sf[:, 0] == sf[:, 1]) | (sf[:, 1] == sf[:, 2]) | (sf[:, 0] == sf[:, 2])).any()              # no degenerate face
        assert len(np.unique(np.sort(sf, 1), axis=0)) == len(sf)                                                   # no two faces on one vertex set
        assert np.array_equal(np.unique(sf), np.arange(len(sv)))                                                   # every vertex named by a face
        # rep inside its cell's closed box [origin + q cell, origin + (q + 1) cell] (float64), up to 1 ulp
        q = np.stack([s['key'] >> 42, (s['key'] >> 21) & S.QMAX, s['key'] & S.QMAX], 1)
        qc = np.zeros((s['nc'], 3), dtype=np.int64)
        qc[s['cluster']] = q
        o64, c64 = s['origin'].astype(np.float64), float(F32(cell))
        lo, hi = (o64 + qc * c64).astype(F32), (o64 + (qc + 1) * c64).astype(F32)
        assert (s['rep'] >= np.nextafter(lo, F32(-np.inf))).all() and (s['rep'] <= np.nextafter(hi, F32(np.inf))).all()
        # faces in emission order: the survivors are a subsequence of the input, corner order kept
        kept = np.flatnonzero(s['keep_f'])
        assert np.array_equal(S.bits(sv[sf]), S.bits(s['rep'][s['cfaces'][kept]])) and (np.diff(kept) > 0).all()
        assert np.array_equal(s['keep_f'], S.first_by_scan(s['fkey']))                                              # the sort-free statement of `first`
        assert (np.diff(s['key'][np.argsort(s['cluster'], kind='stable')]) >= 0).all()                             # clusters ascend by key
        # idempotence of the face stage: the survivors, put through it again as they are, all survive
        ident = np.arange(len(sv), dtype=np.int64)
        cf2, fk2 = S.cluster_faces(sf, ident)
        assert np.array_equal(cf2, sf) and (fk2 != -1).all() and S.first(*S.sort_keys(fk2)).all()
        assert S.used(cf2, np.ones(len(sf), np.int32), len(sv)).all()
        assert len(sf) == len(f) - s['degenerate'] - s['duplicate']


# ---------------------------------------------------------------- recorded counts
@pytest.mark.parametrize('name,G,cell', list(S.RECORDED))
def test_recorded_counts(name, G, cell):
    rec = S.RECORDED[name, G, cell]
    v, f = S.welded(name, G)
    s = S.stages(v, f, cell, ZERO)
    assert (len(v), len(f)) == rec['before'] and (len(s['verts']), len(s['faces'])) == rec['after'] and s['duplicate'] == rec['duplicate']
    assert 'nc' not in rec or s['nc'] == rec['nc']
    if (name, G) == ('blob', 24):                                   # one cluster that no surviving face names; five components become four
        assert int(s['keep_v'].sum()) == s['nc'] - 1
        ncomp = lambda faces, nv: len(np.unique(M.labels(faces, nv)))                                              # noqa: E731
        assert ncomp(f, len(v)) == 5 and ncomp(s['faces'], len(s['verts'])) == 4


# ---------------------------------------------------------------- seeded faults
def test_a_seeded_fault_in_each_stage_fails_the_comparison():
    # summation in another order, on the 1000-member cluster
    v = S.big_cluster()
    order, start = np.arange(len(v), dtype=np.int64), np.array([0, len(v)], dtype=np.int64)
    rep = S.mean(v, order, start)[0]
    assert not np.array_equal(S.bits(S.mean(v, order[::-1].copy(), start)[0]), S.bits(rep))                           # descending index
    assert not np.array_equal(S.bits(np.array([v[:, a].copy().sum(dtype=F32) for a in range(3)]) / F32(len(v))), S.bits(rep))                              # numpy's pairwise sum
    assert np.array_equal(S.bits(np.cumsum(v, 0, dtype=F32)[-1] / F32(len(v))), S.bits(rep))                       # cumsum is sequential
    assert len(np.unique(S.keys(v, ZERO, 1.0))) == 1
    # floor replaced by truncation, with a negative offset: x - origin is never negative for a vertex the wrapper lets through, so the two
    # differ where the offset is taken out AFTER the rounding - trunc(x / cell) - origin / cell rounds -0.5 towards zero, floor away from it
    v2 = np.array([[-0.5, 0, 0], [0.5, 0, 0], [1.5, 0, 0], [1.5, 1.5, 0]], dtype=F32)
    good = S.cell_of(v2, (-1.0, -1.0, -1.0), 1.0)[:, 0]
    bad = np.trunc(v2[:, 0] / F32(1.0)).astype(np.int64) + 1
    assert good.tolist() == [0, 1, 2, 2] and bad.tolist() == [1, 1, 2, 2] and not np.array_equal(bad, good)
    # keeping the last face instead of the first
    pv, pf, cell, _, want_f = S.opposite_pair()
    s = S.stages(pv, pf, cell, ZERO)
    last = np.zeros_like(s['keep_f'])
    last[s['perm'][-1]] = 1
    assert not np.array_equal(last, s['keep_f'])
    assert not np.array_equal(M.compact(s['rep'], s['cfaces'], s['keep_v'], last)[1], want_f)


# ---------------------------------------------------------------- the package's refusals, without a library
class _NoLibrary:
    def __getattr__(self, name):
        def fail(*a):
            pytest.fail(f"{name} was reached with a host tensor")
        return fail


@pytest.mark.parametrize('check', [True, False])
def test_host_tensors_never_reach_the_library(monkeypatch, check):
    """the new wrappers turn tensors into addresses through ops._p only (and their checks refuse a host tensor themselves): with small CPU
    tensors of the right dtypes, shapes and values each call raises before the (fake) library is touched"""
    from ln3diff_amd import _lib, ops
    monkeypatch.setattr(_lib, 'lib', lambda: _NoLibrary())
    v = torch.rand(4, 3)
    faces = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int64)
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64)                                          # noqa: E731
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)                                          # noqa: E731
    calls = [
        lambda: ops.simplify_keys(v, (0.0, 0.0, 0.0), 1.0, i64(4)),
        lambda: ops.simplify_mean(v, torch.arange(4), torch.tensor([0, 2, 4]), torch.zeros(2, 3), check=check),
        lambda: ops.simplify_faces(faces, torch.tensor([0, 1, 1, 0]), 2, i64(2, 3), i64(2), check=check),
        lambda: ops.simplify_first(i64(2), torch.arange(2), i32(2), check=check),
        lambda: ops.simplify_used(faces, i32(2), i32(4), check=check),
    ]
    for call in calls:
        with pytest.raises(RuntimeError, match="need device tensors"):
            call()
    with pytest.raises(RuntimeError, match="need device tensors"):
        ops.check_index(torch.arange(3), 3, "index")
    # the checks themselves: a value outside its range, a wrong dtype, a wrong shape - ValueError, wherever the tensor lives
    with pytest.raises(ValueError):
        ops.check_index(torch.arange(4), 3, "index")
    with pytest.raises(ValueError):
        ops.check_index(torch.tensor([-1, 0]), 3, "index")
    with pytest.raises(ValueError):
        ops.check_index(torch.arange(3, dtype=torch.int32), 3, "index")
    with pytest.raises(ValueError):
        ops.check_index(torch.arange(3), 3, "index", (4,))
    with pytest.raises(ValueError):
        ops.simplify_faces(faces, torch.tensor([0, 1, 2, 0]), 2, i64(2, 3), i64(2))             # cluster 2 of 2
    with pytest.raises(ValueError):
        ops.simplify_first(i64(2), torch.tensor([0, 2]), i32(2))                                 # perm 2 of 2
    with pytest.raises(ValueError):
        ops.simplify_used(faces, i32(2), i32(3))                                                 # corner 3 of 3 clusters
    with pytest.raises(ValueError):
        ops.simplify_mean(v, torch.tensor([0, 1, 2, 4]), torch.tensor([0, 2, 4]), torch.zeros(2, 3))      # order 4 of 4
    # a buffer that the kernel would write past its end - another dtype, too short, strided - is refused from its metadata, checked or not
    for bad in (lambda: ops.simplify_keys(v, (0.0, 0.0, 0.0), 1.0, i32(4)),
                lambda: ops.simplify_keys(v, (0.0, 0.0, 0.0), 1.0, i64(3)),
                lambda: ops.simplify_keys(v.double(), (0.0, 0.0, 0.0), 1.0, i64(4)),
                lambda: ops.simplify_keys(torch.rand(4, 6)[:, ::2], (0.0, 0.0, 0.0), 1.0, i64(4)),
                lambda: ops.simplify_mean(v, torch.arange(4), torch.tensor([0, 2, 4]), torch.zeros(1, 3), check=check),
                lambda: ops.simplify_mean(v, torch.arange(4), torch.tensor([0, 2, 4]), torch.zeros(2, 3, dtype=torch.float64), check=check),
                lambda: ops.simplify_faces(faces, torch.tensor([0, 1, 1, 0]), 2, i64(1, 3), i64(2), check=check),
                lambda: ops.simplify_faces(faces, torch.tensor([0, 1, 1, 0]), 2, i64(2, 3), i32(2), check=check),
                lambda: ops.simplify_first(i64(2), torch.arange(2), i64(2), check=check),
                lambda: ops.simplify_first(i64(2), torch.arange(2), i32(1), check=check),
                lambda: ops.simplify_used(faces, i32(1), i32(4), check=check),
                lambda: ops.simplify_used(faces, i32(2), i64(4), check=check)):
        with pytest.raises(ValueError):
            bad()


def test_simplify_mesh_refuses_bad_arguments_before_any_launch(monkeypatch):
    from ln3diff_amd import _lib
    from ln3diff_amd.mesh import simplify_mesh, _simplify_cell
    monkeypatch.setattr(_lib, 'lib', lambda: _NoLibrary())
    v = torch.rand(4, 3)
    faces = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int64)
    for cell in (-1.0, NAN, INF, 1e-60, 'two'):
        with pytest.raises(ValueError):
            simplify_mesh(v, faces, cell)
    for cell in (None, 0, 0.0):
        a, b = simplify_mesh(v, faces, cell)
        assert a is v and b is faces and _simplify_cell(cell) == 0.0
    with pytest.raises(ValueError):
        simplify_mesh(v.double(), faces, 1.0)
    with pytest.raises(ValueError):
        simplify_mesh(v.reshape(3, 4), faces, 1.0)
    with pytest.raises(ValueError):
        simplify_mesh(v, faces.int(), 1.0)
    with pytest.raises(ValueError):
        simplify_mesh(v, faces + 2, 1.0)                                                         # index 5 of 4 vertices
    for origin in ((0.0, 0.0), (0.0, NAN, 0.0), (INF, 0.0, 0.0)):
        with pytest.raises(ValueError):
            simplify_mesh(v, faces, 1.0, origin)


def test_launcher_refuses_every_cell_that_simplify_mesh_refuses():
    """validate() alone, before anything is built or sampled: 1e-60 is finite and positive as a double and 0 in float32"""
    from ln3diff_amd.entry import create_argparser, validate
    parse = lambda *flags: create_argparser(True).parse_known_args(list(flags))[0]              # noqa: E731
    for cell in ('1e-60', '-1', 'nan', 'inf'):
        with pytest.raises(SystemExit) as e:
            validate(parse('--mesh_simplify_cell', cell, '--export_mesh', 'true'))
        assert '--mesh_simplify_cell' in str(e.value), cell
    with pytest.raises(SystemExit) as e:
        validate(parse('--mesh_simplify_cell', '2'))
    assert '--export_mesh true' in str(e.value)
    a = parse('--mesh_simplify_cell', '2', '--export_mesh', 'true')
    assert validate(a) == 'edm' and a.mesh_simplify_cell == 2.0 and validate(parse('--mesh_simplify_cell', '0')) == 'edm'
