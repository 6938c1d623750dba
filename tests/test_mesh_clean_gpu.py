"""Mesh clean-up on the GPU (include/ln3d_meshclean.h): the four entry points called through the C ABI on sentinel-filled, guarded buffers
and held to the numpy reference of tests/mesh_clean_refs.py with equalities - labels on graphs built to break a union-find (a long strip,
interleaved strips with loose vertices, a fan whose every hook contends on the hub, random triples with repeated indices, two tetrahedra
that share one vertex, a single face), each under its own numbering and three random ones; labels, counts and the packed `best` on the
iso-surfaces of three fields; the keep masks and the compaction; then the seams: clean_mesh, mesh_from_grid, render_video_given_triplane
and the launcher flags."""
import json

import numpy as np
import pytest
import torch

import mesh_clean_refs as M
from test_normals_cpu import parse_obj

pytestmark = pytest.mark.gpu

GUARD = 64                                   # elements behind every output that a call must leave alone
I32_SENTINEL, I64_SENTINEL = -7, -1
F32_SENTINEL = int(np.array([0x7fc0beef], dtype=np.int32)[0])          # a NaN with a payload no arithmetic produces


def _buf(n, width=None, dtype=torch.int32):
    """(whole, view): a sentinel-filled buffer of n rows plus GUARD rows, and the view of its first n rows that a call is given"""
    shape = (n + GUARD,) if width is None else (n + GUARD, width)
    if dtype == torch.float32:
        whole = torch.empty(shape, dtype=torch.int32, device='cuda').fill_(F32_SENTINEL).view(torch.float32)
    else:
        whole = torch.full(shape, I32_SENTINEL if dtype == torch.int32 else I64_SENTINEL, dtype=dtype, device='cuda')
    return whole, whole[:n]


def _intact(whole, n, what):
    tail = whole[n:]
    if whole.dtype == torch.float32:
        ok = bool((tail.view(torch.int32) == F32_SENTINEL).all())
    else:
        ok = bool((tail == (I32_SENTINEL if whole.dtype == torch.int32 else I64_SENTINEL)).all())
    assert ok, '%s: the guard behind the output was written' % what


def _analyse(faces, nv):
    """ln3d_mesh_components + ln3d_mesh_component_counts on guarded buffers -> dict of device tensors (faces, label, nvert, nface, best)"""
    from ln3diff_amd import ops
    faces = torch.as_tensor(np.ascontiguousarray(faces), dtype=torch.int64).cuda()
    (lw, label), (vw, nvert), (fw, nface), (bw, best) = _buf(nv), _buf(nv), _buf(nv), _buf(1, dtype=torch.int64)
    ops.mesh_components(faces, nv, label)
    ops.mesh_component_counts(faces, label, nvert, nface, best)
    torch.cuda.synchronize()
    for whole, name in ((lw, 'label'), (vw, 'nvert'), (fw, 'nface')):
        _intact(whole, nv, name)
    _intact(bw, 1, 'best')
    return dict(faces=faces, nv=nv, label=label, nvert=nvert, nface=nface, best=best)


def _check_analysis(got, faces, nv, name):
    lab = M.labels(faces, nv)
    nvert, nface, best = M.counts(faces, lab)
    assert torch.equal(got['label'].cpu(), torch.from_numpy(lab)), name + ': labels'
    assert torch.equal(got['nvert'].cpu(), torch.from_numpy(nvert)), name + ': nvert'
    assert torch.equal(got['nface'].cpu(), torch.from_numpy(nface)), name + ': nface'
    assert int(got['best'].item()) == best, (name, hex(int(got['best'].item())), hex(best))
    return lab, nvert, nface, best


# ---------------------------------------------------------------- graphs
@pytest.mark.parametrize('seed', M.RENUMBERINGS)
@pytest.mark.parametrize('graph', list(M.GRAPHS))
def test_labels_counts_and_best_on_graphs(hip_lib, graph, seed):
    f, nv = M.GRAPHS[graph]()
    f = M.renumber(f, nv, seed)
    lab, nvert, nface, best = _check_analysis(_analyse(f, nv), f, nv, '%s/%s' % (graph, seed))
    ncomp = {'strip': 1, 'strips3': 1003, 'fan': 1, 'tetra2': 1, 'one': 4}.get(graph)
    assert ncomp is None or int((lab == np.arange(nv)).sum()) == ncomp
    if graph == 'strips3':                                         # three components of 500 faces: the tie goes to the smallest root
        tied = np.flatnonzero(nface == 500)
        assert len(tied) == 3 and M.best_root(best) == tied[0] and best >> 32 == 500


def test_two_runs_give_the_same_labels(hip_lib):
    f, nv = M.random_triples()
    a, b = _analyse(f, nv), _analyse(f, nv)
    assert torch.equal(a['label'], b['label']) and torch.equal(a['nface'], b['nface']) and torch.equal(a['best'], b['best'])


# ---------------------------------------------------------------- fields
@pytest.fixture(scope='module')
def field(hip_lib):
    """(field, method) -> extract_isosurface's device mesh and its analysis, run once"""
    from ln3diff_amd.mesh import extract_isosurface
    cache = {}

    def get(name, method):
        if (name, method) not in cache:
            spec = M.FIELDS[name, method]
            v, f = extract_isosurface(torch.from_numpy(spec['make']()).cuda(), spec['thr'], method=method)
            cache[name, method] = dict(verts=v, **_analyse(f.cpu().numpy(), v.shape[0]))
        return cache[name, method]
    return get


@pytest.mark.parametrize('name,method', list(M.FIELDS))
def test_labels_counts_and_best_on_fields(field, name, method):
    got = field(name, method)
    pos, wfaces = M.welded(name, method)
    f = got['faces'].cpu().numpy()
    assert np.array_equal(f, wfaces) and got['nv'] == len(pos)              # the device weld is the reference's (tests/test_mesh_cells_gpu.py)
    lab, nvert, nface, best = M.check_figures(name, method, f, got['nv'])    # the recorded figures, the tie rule among them
    _check_analysis(got, f, got['nv'], '%s/%s' % (name, method))
    if name == 'atlas':
        tied = np.flatnonzero(nface == 44)
        assert len(tied) == 25 and 0x7fffffff - (int(got['best'].item()) & 0xffffffff) == tied[0]


def test_mesh_components_view(field):
    from ln3diff_amd.mesh import mesh_components
    got = field('blob', 'cubes')
    label, roots, nvert, nface = mesh_components(got['faces'], got['nv'])
    assert torch.equal(label, got['label']) and label.dtype == torch.int32
    assert roots.tolist() == [0, 6, 79, 162, 216] and nface.tolist() == [8, 248, 56, 104, 8]
    assert int(nvert.sum()) == got['nv'] and nvert.tolist() == np.bincount(got['label'].cpu().numpy())[roots.cpu().numpy()].tolist()
    label, roots, nvert, nface = mesh_components(torch.zeros(0, 3, dtype=torch.long, device='cuda'), 5)
    assert label.tolist() == roots.tolist() == [0, 1, 2, 3, 4] and nvert.tolist() == [1] * 5 and nface.tolist() == [0] * 5


# ---------------------------------------------------------------- mark and gather
def _clean_abi(got, keep, min_faces):
    """ln3d_mesh_mark + prefix sums + ln3d_mesh_gather on guarded buffers, every stage held to the reference -> (verts', faces') numpy"""
    from ln3diff_amd import ops
    faces, verts, nv, nf = got['faces'], got['verts'], got['nv'], got['faces'].shape[0]
    f = faces.cpu().numpy()
    want_v, want_f = M.select(f, got['label'].cpu().numpy(), got['nface'].cpu().numpy(), int(got['best'].item()), keep, min_faces)
    (kvw, keep_v), (kfw, keep_f) = _buf(nv), _buf(nf)
    ops.mesh_mark(faces, got['label'], got['nface'], min_faces, keep == 'largest', got['best'], keep_v, keep_f)
    torch.cuda.synchronize()
    _intact(kvw, nv, 'keep_v')
    _intact(kfw, nf, 'keep_f')
    assert torch.equal(keep_v.cpu(), torch.from_numpy(want_v)) and torch.equal(keep_f.cpu(), torch.from_numpy(want_f))
    assert torch.equal(keep_f, keep_v[faces[:, 0]])
    vpre, fpre = torch.cumsum(keep_v.long(), 0), torch.cumsum(keep_f.long(), 0)
    nvo, nfo = int(vpre[-1]), int(fpre[-1])
    (vow, vout), (fow, fout) = _buf(nvo, 3, torch.float32), _buf(nfo, 3, torch.int64)
    ops.mesh_gather(verts, faces, keep_v, vpre, keep_f, fpre, vout, fout)
    torch.cuda.synchronize()
    _intact(vow, nvo, 'verts_out')
    _intact(fow, nfo, 'faces_out')
    rv, rf = M.compact(verts.cpu().numpy(), f, want_v, want_f)
    vout, fout = vout.cpu().numpy(), fout.cpu().numpy()
    assert np.array_equal(vout.view(np.int32), rv.view(np.int32)) and np.array_equal(fout, rf)      # survivors in order, bits kept
    return vout, fout


@pytest.mark.parametrize('method,big,speck', [('cubes', 248, 8), ('tetra', 768, 24)])
def test_clean_on_the_blob_field(field, method, big, speck):
    from ln3diff_amd.mesh import clean_mesh
    got = field('blob', method)
    verts, faces = got['verts'], got['faces']
    v0, f0 = verts.cpu().numpy(), faces.cpu().numpy()
    lab, nface = got['label'].cpu().numpy(), got['nface'].cpu().numpy()
    root = M.FIELDS['blob', method]['roots'][1]
    for keep, min_faces, kept in (('largest', 0, lab[f0[:, 0]] == root), ('all', 9, nface[lab[f0[:, 0]]] >= 9),
                                  ('all', speck + 1, nface[lab[f0[:, 0]]] > speck), ('largest', speck + 1, lab[f0[:, 0]] == root)):
        va, fa = _clean_abi(got, keep, min_faces)
        v1, f1 = clean_mesh(verts, faces, keep, min_faces)
        assert f1.dtype == torch.int64 and v1.dtype == torch.float32
        v1, f1 = v1.cpu().numpy(), f1.cpu().numpy()
        assert np.array_equal(v1.view(np.int32), va.view(np.int32)) and np.array_equal(f1, fa)
        assert len(f1) == int(kept.sum()) and np.array_equal(v1[f1].view(np.int32), v0[f0[kept]].view(np.int32))     # bit for bit, in order
        assert len(v1) == len(np.unique(f0[kept])) and len(np.unique(f1)) == len(v1)                                    # no vertex left over
    assert len(clean_mesh(verts, faces, 'largest')[1]) == big
    assert len(clean_mesh(verts, faces, min_faces=9)[1]) == len(f0) - (2 * speck if speck < 9 else 0)                 # cubes: the two specks go
    assert len(clean_mesh(verts, faces, min_faces=speck + 1)[1]) == len(f0) - 2 * speck
    ve, fe = clean_mesh(verts, faces, min_faces=10 ** 6)
    assert tuple(ve.shape) == (0, 3) and tuple(fe.shape) == (0, 3) and fe.dtype == torch.int64 and ve.is_cuda
    ve, fe = clean_mesh(verts, faces, 'largest', 10 ** 6)
    assert tuple(ve.shape) == (0, 3) and tuple(fe.shape) == (0, 3)
    vs, fs = clean_mesh(verts, faces, keep='all', min_faces=0)
    assert vs is verts and fs is faces                                                                                  # the very same tensors
    with pytest.raises(ValueError):
        clean_mesh(verts[:-1], faces, 'largest')                                                                        # the last vertex is named by a face


def test_clean_on_the_tie_and_noise_fields(field):
    """atlas: 25 components share the largest face count, the one with the smallest root survives; noise: one large sheet and 24 floaters"""
    from ln3diff_amd.mesh import clean_mesh, extract_isosurface
    got = field('atlas', 'cubes')
    va, fa = _clean_abi(got, 'largest', 0)
    nface = got['nface'].cpu().numpy()
    first = int(np.flatnonzero(nface == 44)[0])
    f0 = got['faces'].cpu().numpy()
    assert len(fa) == 44 and np.array_equal(va[fa].view(np.int32), got['verts'].cpu().numpy()[f0[got['label'].cpu().numpy()[f0[:, 0]] == first]].view(np.int32))
    _clean_abi(got, 'all', 44)
    got = field('noise', 'cubes')
    _, fa = _clean_abi(got, 'largest', 0)
    assert len(fa) == 3931
    spec = M.FIELDS['noise', 'cubes']
    v, f = extract_isosurface(torch.from_numpy(spec['make']()).cuda(), spec['thr'], keep='largest')       # the clean-up behind the weld
    assert torch.equal(f, torch.from_numpy(fa).cuda()) and v.shape[0] == int(got['nvert'][0])


# ---------------------------------------------------------------- seams
def test_mesh_from_grid_cleans_before_the_query(hip_lib, tmp_path):
    """the survivors of a cleaned call carry the bits they have in the uncleaned call: positions, colours and normals"""
    from ln3diff_amd.mesh import mesh_from_grid
    from test_normals_gpu import _scene, _triplane, _Seams, _g
    G = M.BLOB_G
    inp = _scene(91, sigma_bias=10.0)
    dec = _Seams(_triplane(inp['dec']))
    d = {'planes_channel_last': _g(inp['planes'][1:2])}
    sigma = torch.from_numpy(M.blob_field()).cuda()
    v, f, col, vn = mesh_from_grid(dec, d, sigma, G, thr=M.BLOB_THR, normals=True)
    assert (len(v), len(f)) == (222, 424)
    lab = M.labels(f, len(v))
    nface = M.counts(f, lab)[1]
    for kw, mask_v, path in ((dict(keep='largest'), lab == 6, 'big.obj'), (dict(min_faces=9), nface[lab] >= 9, 'nospecks.obj'),
                             (dict(keep='largest', min_faces=57), lab == 6, 'both.obj')):
        mask_f = mask_v[f[:, 0]]
        v1, f1, col1, vn1 = mesh_from_grid(dec, d, sigma, G, thr=M.BLOB_THR, normals=True, path=str(tmp_path / path), **kw)
        assert np.array_equal(v1.view(np.int32), v[mask_v].view(np.int32)) and np.array_equal(col1, col[mask_v])
        assert np.array_equal(vn1.view(np.int32), vn[mask_v].view(np.int32))
        assert np.array_equal(v1[f1].view(np.int32), v[f[mask_f]].view(np.int32)) and f1.dtype == np.int64
        three = mesh_from_grid(dec, d, sigma, G, thr=M.BLOB_THR, **kw)
        assert len(three) == 3 and np.array_equal(three[0], v1) and np.array_equal(three[1], f1) and np.array_equal(three[2], col1)
        pv, pvn, pf, _ = parse_obj(tmp_path / path)
        assert (len(pv), len(pvn), len(pf)) == (int(mask_v.sum()), int(mask_v.sum()), int(mask_f.sum())) and np.array_equal(pf, f1)
    assert int((lab == 6).sum()) < 222 and int((nface[lab] >= 9).sum()) == 222 - int((lab == 0).sum()) - int((lab == 216).sum())
    # nothing survives: empty arrays of the usual types and an .obj with no records
    out = mesh_from_grid(dec, d, sigma, G, thr=M.BLOB_THR, normals=True, path=str(tmp_path / 'none.obj'), min_faces=10 ** 6)
    assert [a.shape for a in out] == [(0, 3)] * 4 and open(tmp_path / 'none.obj').read() == ''
    # the default arguments change nothing
    again = mesh_from_grid(dec, d, sigma, G, thr=M.BLOB_THR, normals=True, keep='all', min_faces=0)
    assert all(np.array_equal(a, b) for a, b in zip(again, (v, f, col, vn)))


def test_render_video_given_triplane_mesh_keep(hip_lib, tmp_path):
    from ln3diff_amd.nsr.triplane import draw_render_noise
    from ln3diff_amd.pipeline import render_video_given_triplane
    from ln3diff_amd.synth import synth_input, orbit_cameras
    from test_normals_gpu import _small_ae
    ae, _ = _small_ae()
    cams = orbit_cameras(1).cuda()
    lat = synth_input('z', (2, 12, 32, 32), 7).cuda()
    j, u = draw_render_noise(2, 16 * 16, 64, generator=torch.Generator().manual_seed(1))
    run = lambda **kw: render_video_given_triplane(lat.clone(), ae, cams, triplane_scaling_divider=1.0, jitter=j, u_fine=u, resolution=16,
                                                   export_mesh=True, mesh_size=24, mesh_thres=4.0, **kw)
    a, b, c = run(), run(mesh_keep='all', mesh_min_faces=0), run(mesh_keep='largest', mesh_path=str(tmp_path / 'm{}.obj'))
    for k in ('image_raw', 'image_depth', 'weights_samples'):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    for ma, mb, mc in zip(a['mesh'], b['mesh'], c['mesh']):
        assert len(ma) == len(mb) == len(mc) == 3 and all(np.array_equal(x, y) for x, y in zip(ma, mb))          # the default call is unchanged
        assert mc[1].shape[0] <= ma[1].shape[0] and mc[0].shape[0] <= ma[0].shape[0]
        if ma[1].shape[0]:
            lab = M.labels(ma[1], len(ma[0]))
            nface, best = M.counts(ma[1], lab)[1:]
            kept = lab[ma[1][:, 0]] == M.best_root(best)
            assert np.array_equal(mc[0][mc[1]].view(np.int32), ma[0][ma[1][kept]].view(np.int32)) and np.array_equal(mc[2], ma[2][lab == M.best_root(best)])
    pv, _, pf, _ = parse_obj(tmp_path / 'm1.obj')
    assert len(pv) == c['mesh'][1][0].shape[0] and len(pf) == c['mesh'][1][1].shape[0]


def test_entry_point_mesh_flags(hip_lib, tmp_path):
    from ln3diff_amd.entry import create_argparser, run
    base = ("--arch_dit_decoder DiT2-B/2 --num_samples 2 --sample_steps 2 --image_size 32 --num_views 1 --mesh_grid 24 --dit_model_arch DiT-B/2 "
            "--trainer_name sgm_legacy --export_mesh true --mesh_thres 4.0 ")
    run(create_argparser(True).parse_args((base + f"--logdir {tmp_path / 'plain'}").split()))
    run(create_argparser(True).parse_args((base + f"--mesh_keep largest --mesh_min_faces 3 --logdir {tmp_path / 'clean'}").split()))
    plain, clean = json.load(open(tmp_path / 'plain' / 'args.json')), json.load(open(tmp_path / 'clean' / 'args.json'))
    assert 'mesh_keep' not in plain and 'mesh_min_faces' not in plain
    assert clean['mesh_keep'] == 'largest' and clean['mesh_min_faces'] == 3
    assert {k: v for k, v in clean.items() if k not in ('mesh_keep', 'mesh_min_faces', 'logdir')} == {k: v for k, v in plain.items() if k != 'logdir'}
    for i in range(2):
        v0, _, f0, _ = parse_obj(tmp_path / 'plain' / f'mesh_sample{i}.obj')
        v1, _, f1, _ = parse_obj(tmp_path / 'clean' / f'mesh_sample{i}.obj')
        assert len(f1) <= len(f0) and len(v1) <= len(v0)
        if len(f0):
            lab = M.labels(f0, len(v0))
            nface, best = M.counts(f0, lab)[1:]
            want = nface[M.best_root(best)] if nface[M.best_root(best)] >= 3 else 0
            assert len(f1) == want and (want == 0 or np.array_equal(v1[f1], v0[f0[lab[f0[:, 0]] == M.best_root(best)]]))
    with pytest.raises(SystemExit):
        run(create_argparser(True).parse_args((base.replace("--export_mesh true", "--export_mesh false") + f"--mesh_keep largest --logdir {tmp_path / 'no'}").split()))
