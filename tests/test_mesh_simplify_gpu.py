"""Mesh simplification on the GPU (include/ln3d_meshsimplify.h): the five entry points called through the C ABI on sentinel-filled, guarded
buffers and held to the numpy reference of tests/mesh_simplify_refs.py with equalities - bit patterns for the representatives, integers
elsewhere; then the seams: simplify_mesh, extract_isosurface, mesh_from_grid, render_video_given_triplane and the launcher flag."""
import json

import numpy as np
import pytest
import torch

import mesh_clean_refs as M
import mesh_simplify_refs as S
from test_mesh_clean_gpu import _buf, _intact
from test_normals_cpu import parse_obj

pytestmark = pytest.mark.gpu

F32 = np.float32
ZERO = (0.0, 0.0, 0.0)


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _same_bits(got, want):
    return np.array_equal(S.bits(got.cpu().numpy() if torch.is_tensor(got) else got), S.bits(want))


def _same_ints(got, want):
    got = got.cpu().numpy()
    return got.shape == np.asarray(want).shape and np.array_equal(got, want)


# ---------------------------------------------------------------- the stages, each on guarded buffers, each against the reference
def _keys(verts, origin, cell, name):
    from ln3diff_amd import ops
    nv = verts.shape[0]
    kw, key = _buf(nv, dtype=torch.int64)
    ops.simplify_keys(verts, origin, cell, key)
    torch.cuda.synchronize()
    _intact(kw, nv, name + ': key')
    assert _same_ints(key, S.keys(verts.cpu().numpy(), origin, cell)), name + ': keys'
    return key


def _mean(verts, order, start, name):
    from ln3diff_amd import ops
    nc = start.shape[0] - 1
    rw, rep = _buf(nc, 3, torch.float32)
    ops.simplify_mean(verts, order, start, rep)
    torch.cuda.synchronize()
    _intact(rw, nc, name + ': rep')
    assert _same_bits(rep, S.mean(verts.cpu().numpy(), order.cpu().numpy(), start.cpu().numpy())), name + ': rep'
    return rep


def _face_stages(faces, cluster, nc, name):
    """ln3d_simplify_faces, torch's stable sort, ln3d_simplify_first, ln3d_simplify_used -> dict of device tensors"""
    from ln3diff_amd import ops
    nf = faces.shape[0]
    f_np, c_np = faces.cpu().numpy(), cluster.cpu().numpy()
    (cw, cfaces), (kw, fkey) = _buf(nf, 3, torch.int64), _buf(nf, dtype=torch.int64)
    ops.simplify_faces(faces, cluster, nc, cfaces, fkey)
    torch.cuda.synchronize()
    _intact(cw, nf, name + ': cfaces')
    _intact(kw, nf, name + ': fkey')
    want_cf, want_key = S.cluster_faces(f_np, c_np)
    assert _same_ints(cfaces, want_cf) and _same_ints(fkey, want_key), name + ': cfaces / fkey'
    sorted_key, perm = torch.sort(fkey, stable=True)
    want_sorted, want_perm = S.sort_keys(want_key)
    assert _same_ints(sorted_key, want_sorted) and _same_ints(perm, want_perm), name + ': the stable sort'
    fw, keep_f = _buf(nf)
    ops.simplify_first(sorted_key, perm, keep_f)
    torch.cuda.synchronize()
    _intact(fw, nf, name + ': keep_f')
    want_keep_f = S.first(want_sorted, want_perm)
    assert _same_ints(keep_f, want_keep_f) and np.array_equal(want_keep_f, S.first_by_scan(want_key)), name + ': keep_f'
    vw, keep_v = _buf(nc)
    ops.simplify_used(cfaces, keep_f, keep_v)
    torch.cuda.synchronize()
    _intact(vw, nc, name + ': keep_v')
    assert _same_ints(keep_v, S.used(want_cf, want_keep_f, nc)), name + ': keep_v'
    return dict(cfaces=cfaces, fkey=fkey, keep_f=keep_f, keep_v=keep_v)


def _clusters(key, name):
    """torch's unique and stable sort between the key and the mean stage, held to the reference's -> (cluster, nc, order, start)"""
    uniq, cluster, members = torch.unique(key, return_inverse=True, return_counts=True)
    nc = uniq.shape[0]
    order = torch.sort(cluster, stable=True)[1]
    start = torch.zeros(nc + 1, dtype=torch.int64, device='cuda')
    start[1:] = torch.cumsum(members, 0)
    want_cluster, want_nc = S.clusters(key.cpu().numpy())
    want_order, want_start = S.csr(want_cluster, want_nc)
    assert nc == want_nc and _same_ints(cluster, want_cluster) and _same_ints(order, want_order) and _same_ints(start, want_start), name
    return cluster, nc, order, start


def _abi(verts, faces, cell, origin, name):
    """the whole through the C ABI, every stage checked -> (verts', faces') numpy, or empty arrays when nothing survives"""
    from ln3diff_amd import ops
    want = S.stages(verts.cpu().numpy(), faces.cpu().numpy(), cell, origin)
    key = _keys(verts, origin, cell, name)
    cluster, nc, order, start = _clusters(key, name)
    rep = _mean(verts, order, start, name)
    st = _face_stages(faces, cluster, nc, name)
    assert _same_bits(rep, want['rep']) and _same_ints(st['keep_f'], want['keep_f']) and _same_ints(st['keep_v'], want['keep_v'])
    vpre, fpre = torch.cumsum(st['keep_v'].long(), 0), torch.cumsum(st['keep_f'].long(), 0)
    nvo, nfo = int(vpre[-1]), int(fpre[-1])
    assert (nvo, nfo) == (len(want['verts']), len(want['faces'])), name
    if nfo == 0:
        assert nvo == 0
        return want['verts'], want['faces']
    (vow, vout), (fow, fout) = _buf(nvo, 3, torch.float32), _buf(nfo, 3, torch.int64)
    ops.mesh_gather(rep, st['cfaces'], st['keep_v'], vpre, st['keep_f'], fpre, vout, fout)
    torch.cuda.synchronize()
    _intact(vow, nvo, name + ': verts_out')
    _intact(fow, nfo, name + ': faces_out')
    assert _same_bits(vout, want['verts']) and _same_ints(fout, want['faces']), name + ': gather'
    return vout.cpu().numpy(), fout.cpu().numpy()


# ---------------------------------------------------------------- keys
@pytest.mark.parametrize('nv', [1, 63, 257])
def test_keys(hip_lib, nv):
    rng = np.random.default_rng(nv)
    for cell, origin in ((0.5, ZERO), (0.5, (-1.5, -0.25, -7.0)), (0.1, ZERO), (0.1, (-0.3, -1.0, -2.5)), (3.0, (-1.0, 0.0, -2.0))):
        c = F32(cell)
        o = np.asarray(origin, dtype=F32)
        v = (rng.random((nv, 3)) * 20 + 0.01).astype(F32) + o                                # normal numbers, nothing below the origin
        k = np.arange(nv, dtype=F32)
        on = o[None] + (k[:, None] % 37) * c                                                  # on a boundary as float32 computes it,
        v[0::3] = on[0::3]
        v[1::3] = np.nextafter(on, F32(np.inf))[1::3]                                         # one ulp above
        v[2::3] = np.maximum(np.nextafter(on, F32(-np.inf)), o)[2::3]                         # and one below (never below the origin)
        tiny = np.finfo(F32).tiny
        v = np.where((v != 0) & (np.abs(v) < tiny), np.copysign(tiny, v), v).astype(F32)      # one ulp from 0 is a denormal: the smallest normal instead
        assert np.isfinite(v).all() and ((v == 0) | (np.abs(v) >= np.finfo(F32).tiny)).all()
        key = _keys(_dev(v, torch.float32), origin, cell, 'keys nv=%d cell=%g' % (nv, cell))
        assert int(key.min()) >= 0
    # the ends of the key's range: q = 2^21 - 1 on one axis and 0 on another, for every assignment of the axes
    for axis in range(3):
        v = np.full((nv, 3), 0.25, dtype=F32)
        v[:, axis] = S.QMAX + 0.5
        v[:, (axis + 1) % 3] = 5.0
        key = _keys(_dev(v, torch.float32), ZERO, 1.0, 'keys: range')
        q = [0, 0, 0]
        q[axis], q[(axis + 1) % 3] = S.QMAX, 5
        assert key.tolist() == [(q[0] << 42) | (q[1] << 21) | q[2]] * nv
    # the same through an offset: origin -(2^21 - 1) cells of 0.5
    o = (-(S.QMAX * 0.5), 0.0, -3.0)
    v = np.array([[0.25, 0.25, -3.0]] * nv, dtype=F32)
    key = _keys(_dev(v, torch.float32), o, 0.5, 'keys: offset')
    assert key.tolist() == [(S.QMAX << 42)] * nv


# ---------------------------------------------------------------- mean
def test_mean_of_a_thousand_members_in_index_order(hip_lib):
    v = S.big_cluster()
    dv = _dev(v, torch.float32)
    key = _keys(dv, ZERO, 1.0, 'big')
    cluster, nc, order, start = _clusters(key, 'big')
    assert nc == 1 and order.tolist() == list(range(len(v)))
    rep = _mean(dv, order, start, 'big')
    # the order is what the bits depend on: the reverse order and a pairwise sum give other bits, and the kernel follows `order`
    rev = S.mean(v, np.arange(len(v))[::-1].copy(), np.array([0, len(v)]))
    assert not _same_bits(rep, rev)
    assert _same_bits(_mean(dv, torch.flip(order, [0]).contiguous(), start, 'big reversed'), rev)
    assert _same_bits(rep, (np.cumsum(v, 0, dtype=F32)[-1] / F32(len(v)))[None])


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_mean_of_many_small_clusters(hip_lib, seed):
    v = S.small_clusters(seed=seed)                                  # the same kind of clusters under another vertex numbering
    dv = _dev(v, torch.float32)
    key = _keys(dv, ZERO, 1.0, 'small')
    cluster, nc, order, start = _clusters(key, 'small')
    sizes = (start[1:] - start[:-1]).cpu().numpy()
    assert nc == 203 and nc % 64 != 0 and sizes.min() >= 1 and sizes.max() <= 8 and len(np.unique(sizes)) == 8
    _mean(dv, order, start, 'small/%d' % seed)
    # one renumbering of the SAME vertices moves no cluster and, members of a cluster being summed in another order, may move bits only
    perm = np.random.default_rng(seed).permutation(len(v))
    dv2 = _dev(v[perm], torch.float32)
    c2, nc2, order2, start2 = _clusters(_keys(dv2, ZERO, 1.0, 'small renumbered'), 'small renumbered')
    assert nc2 == nc and torch.equal(start2, start)
    rep2 = _mean(dv2, order2, start2, 'small renumbered')
    assert rep2.shape == (nc, 3)


# ---------------------------------------------------------------- faces and first
@pytest.mark.parametrize('n', [4, 3, 2, 1])
def test_hand_made_quads(hip_lib, n):
    v, f, cell, want_v, want_f = S.quad(n)
    gv, gf = _abi(_dev(v, torch.float32), _dev(f, torch.int64), cell, ZERO, 'quad %d' % n)
    assert np.array_equal(S.bits(gv), S.bits(want_v)) and np.array_equal(gf, want_f)


def test_hand_made_opposite_windings(hip_lib):
    v, f, cell, want_v, want_f = S.opposite_pair()
    gv, gf = _abi(_dev(v, torch.float32), _dev(f, torch.int64), cell, ZERO, 'opposite')
    assert np.array_equal(S.bits(gv), S.bits(want_v)) and np.array_equal(gf, want_f)


def test_faces_on_random_triples(hip_lib):
    f, nv = M.GRAPHS['random']()
    cluster = np.arange(nv, dtype=np.int64) % 97
    st = _face_stages(_dev(f, torch.int64), _dev(cluster, torch.int64), 97, 'random')
    fkey, keep_f = st['fkey'].cpu().numpy(), st['keep_f'].cpu().numpy()
    cf = st['cfaces'].cpu().numpy()
    alive = fkey != -1
    assert int((~alive).sum()) > 50 and int(alive.sum() - keep_f.sum()) > 20                      # many degenerates, many duplicates
    kept_sets = {tuple(sorted(t)) for t in cf[keep_f != 0].tolist()}
    assert len(kept_sets) == int(keep_f.sum()) == len(np.unique(fkey[alive]))
    # opposite windings among the dropped duplicates: a dropped face whose orientation differs from its survivor's
    first_of = {tuple(sorted(t)): t for t in cf[keep_f != 0].tolist()}
    flipped = sum(1 for t in cf[alive & (keep_f == 0)].tolist()
                  if _winding(tuple(t)) != _winding(tuple(first_of[tuple(sorted(t))])))
    assert flipped > 0


def _winding(t):
    """+1 / -1: the parity of the permutation that sorts a triple of different numbers"""
    a, b, c = t
    return 1 if (a < b) + (b < c) + (c < a) == 2 else -1


def test_all_faces_degenerate_and_a_single_face(hip_lib):
    f, nv = M.GRAPHS['random']()
    st = _face_stages(_dev(f, torch.int64), torch.zeros(nv, dtype=torch.int64, device='cuda'), 1, 'all degenerate')
    assert not st['keep_f'].any() and not st['keep_v'].any() and bool((st['fkey'] == -1).all())
    f, nv = M.GRAPHS['one']()
    st = _face_stages(_dev(f, torch.int64), torch.arange(nv, device='cuda'), nv, 'one face')
    assert st['keep_f'].tolist() == [1] and st['keep_v'].tolist() == [0, 1, 0, 1, 1, 0] and st['fkey'].tolist() == [(1 << 42) | (3 << 21) | 4]
    st = _face_stages(_dev(f, torch.int64), _dev([0, 1, 0, 1, 1, 0], torch.int64), 2, 'one face, collapsed')
    assert st['keep_f'].tolist() == [0] and st['keep_v'].tolist() == [0, 0]


# ---------------------------------------------------------------- the fields through the whole sequence
@pytest.fixture(scope='module')
def field(hip_lib):
    """field, G -> extract_isosurface's unsimplified device mesh (verts, faces), run once"""
    from ln3diff_amd.mesh import extract_isosurface
    cache = {}

    def get(name, G=None, method='cubes'):
        if (name, G, method) not in cache:
            spec = M.FIELDS[name, method]
            sigma = M.blob_field(G) if G else spec['make']()
            cache[name, G, method] = extract_isosurface(torch.from_numpy(sigma).cuda(), spec['thr'], method=method)
        return cache[name, G, method]
    return get


@pytest.mark.parametrize('cell', [1.5, 2.0])
@pytest.mark.parametrize('name,method', list(M.FIELDS))
def test_every_field_through_the_abi_sequence(field, name, method, cell):
    """every entry of mesh_clean_refs.FIELDS, the marching-tetrahedra mesh with its slivers among them"""
    verts, faces = field(name, None, method)
    rv, rf = S.welded(name, None, method)
    assert _same_ints(faces, rf) and (verts.shape[0], faces.shape[0]) == (M.FIELDS[name, method]['nv'], M.FIELDS[name, method]['nf'])
    gv, gf = _abi(verts, faces, cell, ZERO, '%s/%s/%g' % (name, method, cell))
    assert 0 < len(gf) < faces.shape[0]
    _abi(verts, faces, cell, tuple(verts.amin(0).tolist()), 'own origin')


@pytest.mark.parametrize('name,G,cell', list(S.RECORDED) + [('blob', 24, 3.0), ('blob', 24, 1.0)])
def test_fields_through_the_abi_sequence(field, name, G, cell):
    verts, faces = field(name, G if name == 'blob' else None)
    rv, rf = S.welded(name, G)
    assert _same_ints(faces, rf) and verts.shape[0] == len(rv)                 # the device weld is the reference's (tests/test_mesh_cells_gpu.py)
    gv, gf = _abi(verts, faces, cell, ZERO, '%s/%s/%g' % (name, G, cell))
    rec = S.RECORDED.get((name, G, cell))
    if rec:
        assert (verts.shape[0], faces.shape[0]) == rec['before'] and (len(gv), len(gf)) == rec['after']
    _abi(verts, faces, cell, tuple(verts.amin(0).tolist()), 'own origin')      # the origin that simplify_mesh(origin=None) takes


def test_two_runs_give_the_same_bytes(field):
    from ln3diff_amd.mesh import simplify_mesh
    verts, faces = field('noise')
    a, b = simplify_mesh(verts, faces, 2.0), simplify_mesh(verts, faces, 2.0)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and a[1].shape[0] > 0
    v = _dev(S.big_cluster(), torch.float32)
    order, start = torch.arange(v.shape[0], device='cuda'), torch.tensor([0, v.shape[0]], device='cuda')
    assert torch.equal(_mean(v, order, start, 'run 1').view(torch.int32), _mean(v, order, start, 'run 2').view(torch.int32))


# ---------------------------------------------------------------- seams
def test_simplify_mesh(field):
    from ln3diff_amd.mesh import simplify_mesh
    for name, G, cell in (('blob', 24, 2.0), ('noise', None, 2.0), ('blob', 48, 1.5)):
        verts, faces = field(name, G)
        for origin in (None, ZERO, (-1.0, -0.5, -2.0)):
            o = tuple(verts.amin(0).tolist()) if origin is None else origin
            av, af = _abi(verts, faces, cell, o, 'simplify_mesh %s' % name)
            v, f = simplify_mesh(verts, faces, cell, origin)
            assert v.dtype == torch.float32 and f.dtype == torch.int64 and v.is_cuda and f.is_cuda
            assert _same_bits(v, av) and _same_ints(f, af)
    verts, faces = field('blob', 24)
    for off in (0, 0.0, None):
        v, f = simplify_mesh(verts, faces, off)
        assert v is verts and f is faces                                                       # the very same tensors
    # nothing survives: every vertex in one cell / no face at all
    for v, f in (simplify_mesh(verts, faces, 1000.0), simplify_mesh(verts, faces[:0], 2.0), simplify_mesh(verts[:0], faces[:0], 2.0)):
        assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and v.dtype == torch.float32 and f.dtype == torch.int64
        assert v.is_cuda and f.is_cuda
    bad = verts.clone()
    bad[5, 1] = float('nan')
    worse = verts.clone()
    worse[7, 2] = float('inf')
    for args in ((bad, faces, 2.0), (worse, faces, 2.0),                                       # a non-finite vertex
                 (verts, faces, 1e-6),                                                         # 23 grid units are more than 2^21 cells of 1e-6
                 (verts, faces, 2.0, (5.0, 0.0, 0.0)),                                         # vertices below the origin
                 (verts, faces, -2.0), (verts, faces, float('nan')), (verts, faces, float('inf')),
                 (verts, faces, 2.0, (0.0, float('nan'), 0.0)),
                 (verts.double(), faces, 2.0), (verts.reshape(-1), faces, 2.0), (verts, faces.int(), 2.0),
                 (verts[:-1], faces, 2.0)):                                                    # the last vertex is named by a face
        with pytest.raises(ValueError):
            simplify_mesh(*args)
    span = (S.QMAX + 1) * 1e-5                                                                  # exactly too many cells of 1e-5 ...
    wide = torch.tensor([[0.0, 0, 0], [span * 1.01, 0, 0], [0, 1, 0]], device='cuda')
    tri = torch.tensor([[0, 1, 2]], device='cuda')
    with pytest.raises(ValueError):
        simplify_mesh(wide, tri, 1e-5)
    v, f = simplify_mesh(wide * 0.98, tri, 1e-5)                                                # ... and just few enough
    assert v.shape[0] == 3 and f.tolist() == [[0, 2, 1]]


@pytest.mark.parametrize('name', ['blob', 'noise'])
def test_extract_isosurface_simplifies_behind_the_clean_up(field, name):
    from ln3diff_amd.mesh import extract_isosurface
    spec = M.FIELDS[name, 'cubes']
    sigma = torch.from_numpy(spec['make']()).cuda()
    verts, faces = field(name)
    v0, f0 = verts.cpu().numpy(), faces.cpu().numpy()
    for keep in ('all', 'largest'):
        cv, cf = M.clean(v0, f0, keep) if keep != 'all' else (v0, f0)
        want_v, want_f = S.simplify(cv, cf, 2.0, ZERO)
        v, f = extract_isosurface(sigma, spec['thr'], keep=keep, simplify_cell=2.0)
        assert _same_bits(v, want_v) and _same_ints(f, want_f) and 0 < len(want_f) < len(cf), (name, keep)
    v, f = extract_isosurface(sigma, spec['thr'], simplify_cell=0.0)
    assert torch.equal(v.view(torch.int32), verts.view(torch.int32)) and torch.equal(f, faces)
    with pytest.raises(ValueError):
        extract_isosurface(sigma, spec['thr'], simplify_cell=-1.0)


def test_mesh_from_grid_simplifies_before_the_query(hip_lib, tmp_path):
    """colours and normals of a simplified mesh are the field's values at the NEW vertices"""
    from ln3diff_amd.mesh import extract_isosurface, mesh_from_grid, rotation_matrix_x
    from test_normals_gpu import _scene, _triplane, _Seams, _g
    G = M.BLOB_G
    inp = _scene(91, sigma_bias=10.0)
    dec = _Seams(_triplane(inp['dec']))
    pcl = _g(inp['planes'][1:2])
    d = {'planes_channel_last': pcl}
    sigma = torch.from_numpy(M.blob_field()).cuda()
    plain = mesh_from_grid(dec, d, sigma, G, thr=M.BLOB_THR, normals=True)
    assert (len(plain[0]), len(plain[1])) == (222, 424)
    for kw, path in ((dict(simplify_cell=2.0), 's.obj'), (dict(simplify_cell=2.0, keep='largest'), 'sl.obj'), (dict(simplify_cell=3.0, min_faces=9), 'sm.obj')):
        v, f, col, vn = mesh_from_grid(dec, d, sigma, G, thr=M.BLOB_THR, normals=True, path=str(tmp_path / path), **kw)
        gv, gf = extract_isosurface(sigma, M.BLOB_THR, keep=kw.get('keep', 'all'), min_faces=kw.get('min_faces', 0), simplify_cell=kw['simplify_cell'])
        assert 0 < len(f) < 424 and len(v) == gv.shape[0] and np.array_equal(f, gf.cpu().numpy()) and f.dtype == np.int64
        vtx = (gv / (G - 1) * 2 - 1) * 0.45
        q = dec.forward_points(pcl, vtx[None], with_grad=True)
        rot = lambda a: (rotation_matrix_x(-90) @ a.cpu().numpy().T).T.astype(np.float32)      # noqa: E731
        assert np.array_equal(S.bits(v), S.bits(rot(vtx)))
        assert np.array_equal(col, (q['rgb'][0].clamp(0, 1) * 255).to(torch.uint8).cpu().numpy())
        assert np.array_equal(S.bits(vn), S.bits(rot(q['normal'][0])))
        three = mesh_from_grid(dec, d, sigma, G, thr=M.BLOB_THR, **kw)
        assert len(three) == 3 and all(np.array_equal(a, b) for a, b in zip(three, (v, f, col)))
        pv, pvn, pf, _ = parse_obj(tmp_path / path)
        assert (len(pv), len(pvn), len(pf)) == (len(v), len(vn), len(f)) and np.array_equal(pf, f)
    gv, gf = extract_isosurface(sigma, M.BLOB_THR, simplify_cell=2.0)
    assert (gv.shape[0], gf.shape[0]) == S.RECORDED['blob', 24, 2.0]['after']
    # nothing survives: empty arrays of the usual types and an .obj with no records
    out = mesh_from_grid(dec, d, sigma, G, thr=M.BLOB_THR, normals=True, path=str(tmp_path / 'none.obj'), simplify_cell=1000.0)
    assert [a.shape for a in out] == [(0, 3)] * 4 and open(tmp_path / 'none.obj').read() == ''
    # the default arguments reproduce the unsimplified mesh bit for bit
    again = mesh_from_grid(dec, d, sigma, G, thr=M.BLOB_THR, normals=True, simplify_cell=0.0)
    assert all(np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a, b.view(np.int32) if b.dtype == np.float32 else b)
               for a, b in zip(again, plain))
    uv, uf = extract_isosurface(sigma, M.BLOB_THR)
    assert np.array_equal(plain[1], uf.cpu().numpy()) and np.array_equal(S.bits(plain[0]), S.bits(rot((uv / (G - 1) * 2 - 1) * 0.45)))


def test_render_video_given_triplane_mesh_simplify_cell(hip_lib, tmp_path):
    from ln3diff_amd.mesh import extract_isosurface, rotation_matrix_x
    from ln3diff_amd.nsr.triplane import draw_render_noise
    from ln3diff_amd.pipeline import render_video_given_triplane
    from ln3diff_amd.synth import synth_input, orbit_cameras
    from test_normals_gpu import _small_ae
    ae, _ = _small_ae()
    G = 24
    cams = orbit_cameras(1).cuda()
    lat = synth_input('z', (2, 12, 32, 32), 7).cuda()
    j, u = draw_render_noise(2, 16 * 16, 64, generator=torch.Generator().manual_seed(1))
    # the geometry of the default meshes before the box mapping and the rotation: the iso-surface of the same decoded grid; the level is taken
    # from the synthetic sample's own densities so that there is a surface to simplify
    d = {'latent_normalized_2Ddiffusion': lat.clone()}
    d.update(ae(latent=d, behaviour='decode_after_vae_no_render'))
    if d.get('planes_channel_last') is not None:
        d['planes_channel_last'] = ae.decoder.triplane_decoder.cast_planes(d['planes_channel_last'])
    grid = ae(latent=d, grid_size=G, behaviour='triplane_decode_grid')
    thr = float(torch.quantile(grid['sigma'][0].float().flatten(), 0.8))
    run = lambda **kw: render_video_given_triplane(lat.clone(), ae, cams, triplane_scaling_divider=1.0, jitter=j, u_fine=u, resolution=16,
                                                   export_mesh=True, mesh_size=G, mesh_thres=thr, **kw)
    a, b, c = run(), run(mesh_simplify_cell=0.0), run(mesh_simplify_cell=2.0, mesh_path=str(tmp_path / 'm{}.obj'))
    for k in ('image_raw', 'image_depth', 'weights_samples'):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    rot = lambda t: (rotation_matrix_x(-90) @ ((t / (G - 1) * 2 - 1) * 0.45).cpu().numpy().T).T.astype(np.float32)      # noqa: E731
    for i, (ma, mb, mc) in enumerate(zip(a['mesh'], b['mesh'], c['mesh'])):
        assert len(ma) == len(mb) == len(mc) == 3 and all(np.array_equal(x, y) for x, y in zip(ma, mb))          # the default call is unchanged
        gv, gf = extract_isosurface(grid['sigma'][i].reshape(G, G, G), thr)
        assert np.array_equal(ma[1], gf.cpu().numpy()) and (gv.shape[0] == 0 or np.array_equal(S.bits(ma[0]), S.bits(rot(gv))))
        want_v, want_f = S.simplify(gv.cpu().numpy(), gf.cpu().numpy(), 2.0, ZERO) if gf.shape[0] else (np.zeros((0, 3), F32), np.zeros((0, 3), np.int64))
        print('[simplify] sample %d: %d / %d -> %d / %d' % (i, gv.shape[0], gf.shape[0], len(want_v), len(want_f)))
        assert np.array_equal(mc[1], want_f) and mc[0].shape == want_v.shape
        if len(want_v):
            assert np.array_equal(S.bits(mc[0]), S.bits(rot(torch.from_numpy(want_v).cuda())))
    assert 0 < c['mesh'][0][1].shape[0] < a['mesh'][0][1].shape[0]
    pv, _, pf, _ = parse_obj(tmp_path / 'm0.obj')
    assert len(pv) == c['mesh'][0][0].shape[0] and np.array_equal(pf, c['mesh'][0][1])


def test_entry_point_mesh_simplify_flag(hip_lib, tmp_path):
    from ln3diff_amd.entry import create_argparser, run
    base = ("--arch_dit_decoder DiT2-B/2 --num_samples 2 --sample_steps 2 --image_size 32 --num_views 1 --mesh_grid 24 --dit_model_arch DiT-B/2 "
            "--trainer_name sgm_legacy --export_mesh true --mesh_thres 4.7 ")       # the synthetic decoder's densities lie in [4.1, 5.1]: a level inside
    run(create_argparser(True).parse_args((base + f"--logdir {tmp_path / 'plain'}").split()))
    run(create_argparser(True).parse_args((base + f"--mesh_simplify_cell 2 --logdir {tmp_path / 'simple'}").split()))
    plain, simple = json.load(open(tmp_path / 'plain' / 'args.json')), json.load(open(tmp_path / 'simple' / 'args.json'))
    assert 'mesh_simplify_cell' not in plain and simple['mesh_simplify_cell'] == 2.0
    assert {k: v for k, v in simple.items() if k not in ('mesh_simplify_cell', 'logdir')} == {k: v for k, v in plain.items() if k != 'logdir'}
    for i in range(2):
        v0, _, f0, _ = parse_obj(tmp_path / 'plain' / f'mesh_sample{i}.obj')
        v1, _, f1, _ = parse_obj(tmp_path / 'simple' / f'mesh_sample{i}.obj')
        print('[simplify] launcher sample %d: %d / %d -> %d / %d' % (i, len(v0), len(f0), len(v1), len(f1)))
        assert len(f0) > 100 and 0 < len(f1) < len(f0) and len(v1) < len(v0)                     # there is a surface, and it got smaller
        assert len(np.unique(f1)) == len(v1) and len(np.unique(np.sort(f1, 1), axis=0)) == len(f1)
        assert not ((f1[:, 0] == f1[:, 1]) | (f1[:, 1] == f1[:, 2]) | (f1[:, 0] == f1[:, 2])).any()
    off = base.replace("--export_mesh true", "--export_mesh false")
    for flags in (off + "--mesh_simplify_cell 2", base + "--mesh_simplify_cell -1", base + "--mesh_simplify_cell nan", base + "--mesh_simplify_cell inf",
                  base + "--mesh_simplify_cell 1e-60"):                                          # positive, and 0 in the float32 the kernels divide by
        with pytest.raises(SystemExit):
            run(create_argparser(True).parse_args((flags + f" --logdir {tmp_path / 'no'}").split()))
