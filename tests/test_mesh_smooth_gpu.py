"""Mesh smoothing on the GPU (include/ln3d_meshsmooth.h), held to the numpy reference of tests/mesh_smooth_refs.py with equalities -
integers for the adjacency, bit patterns for the coordinates: the three entry points on sentinel-filled buffers with guard rows before and
behind, mesh_adjacency and smooth_mesh on the smallest meshes at which each part of the definition can go wrong, then the seams:
mesh_from_grid, textured_mesh_from_grid, render_video_given_triplane and the launcher flag."""
import json

import numpy as np
import pytest
import torch

import mesh_smooth_refs as R
from test_normals_cpu import parse_obj

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 64                                   # rows before and behind every output that a call must leave alone
SENTINEL = int(np.array([0x7fc0beef], dtype=np.int32)[0])               # as a float: a NaN with a payload no arithmetic produces
CASES = ['tetra', 'sphere258', 'patch6', 'duplicate_faces', 'opposite_windings', 'two_sided_patch', 'three_faces_one_edge', 'face_a_a_b',
         'unreferenced_vertex', 'fan600', 'fan600_two_hubs']


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _buf(n, width=None, dtype=torch.float32):
    """(whole, view): n rows between GUARD rows on either side, every 32-bit word the sentinel; the call is given the view"""
    shape = (n + 2 * GUARD,) if width is None else (n + 2 * GUARD, width)
    words = torch.empty(shape, dtype=dtype, device='cuda')
    words.view(torch.int32).fill_(SENTINEL)
    return words, words[GUARD:GUARD + n]


def _intact(whole, n, what):
    for part in (whole[:GUARD], whole[GUARD + n:]):
        assert bool((part.contiguous().view(torch.int32) == SENTINEL).all()), '%s: a guard row was written' % what


def _same_bits(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    return got.shape == np.asarray(want).shape and np.array_equal(R.bits(got), R.bits(want))


def _same_ints(got, want, dtype):
    got = got.cpu().numpy()
    return got.dtype == dtype and got.shape == np.asarray(want).shape and np.array_equal(got, want)


def test_the_cases_are_all_covered():
    assert sorted(CASES) == sorted(R.cases())


# ---------------------------------------------------------------- the entry points, each on guarded buffers
@pytest.mark.parametrize('name', CASES)
def test_entry_points_on_guarded_buffers(hip_lib, name):
    from ln3diff_amd import ops
    v_np, f_np = R.cases()[name]
    nv, nf = len(v_np), len(f_np)
    verts, faces = _dev(v_np, torch.float32), _dev(f_np, torch.int64)
    kw, key = _buf(3 * nf, dtype=torch.int64)
    ops.smooth_edge_keys(faces, nv, key)
    torch.cuda.synchronize()
    _intact(kw, 3 * nf, name + ': key')
    assert _same_ints(key, R.edge_keys(f_np), np.int64), name + ': key'
    edge, count = torch.unique(key, return_counts=True)
    edge, count = edge[edge >= 0].contiguous(), count[edge >= 0].contiguous()
    want = R.edge_count(f_np)
    assert [(int(k) >> 32, int(k) & 0xffffffff) for k in edge.tolist()] == sorted(want) and count.tolist() == [want[k] for k in sorted(want)]
    ne = edge.shape[0]
    (dw, dkey), (pw, pinned) = _buf(2 * ne, dtype=torch.int64), _buf(nv, dtype=torch.int32)
    pinned.zero_()
    ops.smooth_halfedges(edge, count, nv, dkey, pinned)
    torch.cuda.synchronize()
    _intact(dw, 2 * ne, name + ': dkey')
    _intact(pw, nv, name + ': pinned')
    start_np, nbr_np, pinned_np = R.adjacency(f_np, nv)
    assert _same_ints(pinned, pinned_np, np.int32), name + ': pinned'
    sorted_key = torch.sort(dkey)[0]
    src = np.repeat(np.arange(nv), np.diff(start_np))
    assert _same_ints(sorted_key, (src.astype(np.int64) << 32) | nbr_np.astype(np.int64), np.int64), name + ': dkey'
    start, nbr = _dev(start_np, torch.int64), _dev(nbr_np, torch.int32)
    for factor in (0.5, -0.53, 1.0, -1.0):
        ow, out = _buf(nv, 3)
        ops.smooth_step(verts, start, nbr, pinned.contiguous(), factor, out)
        torch.cuda.synchronize()
        _intact(ow, nv, name + ': verts_out')
        assert _same_bits(out, R.step(v_np, start_np, nbr_np, pinned_np, factor)), (name, factor)
        assert _same_bits(verts, v_np)                                                       # the input is read only
    with pytest.raises(RuntimeError, match='bad argument'):
        ops.smooth_step(verts, start, nbr, pinned.contiguous(), 0.5, verts)                  # in place is refused, not run
    with pytest.raises(RuntimeError, match='bad argument'):
        ops.smooth_step(verts, start, nbr, pinned.contiguous(), float('nan'), torch.empty_like(verts))
    assert _same_bits(verts, v_np)


# ---------------------------------------------------------------- the wrappers against the reference
@pytest.mark.parametrize('name', CASES)
def test_mesh_adjacency_equals_the_reference(hip_lib, name):
    from ln3diff_amd.mesh import mesh_adjacency
    v_np, f_np = R.cases()[name]
    start, nbr, pinned = mesh_adjacency(_dev(f_np, torch.int64), len(v_np))
    want = R.adjacency(f_np, len(v_np))
    assert _same_ints(start, want[0], np.int64) and _same_ints(nbr, want[1], np.int32) and _same_ints(pinned, want[2], np.int32), name


@pytest.mark.parametrize('name', CASES)
def test_smooth_mesh_equals_the_reference_bit_for_bit(hip_lib, name):
    from ln3diff_amd.mesh import smooth_mesh
    v_np, f_np = R.cases()[name]
    verts, faces = _dev(v_np, torch.float32), _dev(f_np, torch.int64)
    pinned = R.adjacency(f_np, len(v_np))[2] != 0
    for lam, mu in R.SETTINGS:
        want = R.expected(name, lam, mu)
        for it in R.ITERATIONS:
            got, gf = smooth_mesh(verts, faces, it, lam, mu)
            assert gf is faces and got.shape == verts.shape and got.dtype == torch.float32 and got.data_ptr() != verts.data_ptr()
            assert _same_bits(got, want[it]), (name, lam, mu, it, int((R.bits(got.cpu().numpy()) != R.bits(want[it])).sum()))
            assert _same_bits(got[torch.from_numpy(pinned).cuda()], v_np[pinned])            # pinned vertices keep their bits
            assert _same_bits(verts, v_np)                                                   # the caller's vertices are not written
    a, b = smooth_mesh(verts, faces, 7)[0], smooth_mesh(verts, faces, 7)[0]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))                             # two runs, identical bits
    if name == 'sphere258':
        assert not _same_bits(a, v_np) and not _same_bits(a, R.expected(name, 1.0, -1.0)[7])  # something moved, and the factors matter


def test_smooth_mesh_edges(hip_lib):
    from ln3diff_amd.mesh import mesh_adjacency, smooth_mesh
    v_np, f_np = R.cases()['sphere258']
    verts, faces = _dev(v_np, torch.float32), _dev(f_np, torch.int64)
    for off in (0, None):
        v, f = smooth_mesh(verts, faces, off)
        assert v is verts and f is faces                                                     # the very same tensors
    for v, f in (smooth_mesh(verts[:0], faces[:0], 3), smooth_mesh(verts, faces[:0], 3)):     # no vertices / no faces: nothing can move
        assert v.is_cuda and f.shape == (0, 3) and f.dtype == torch.int64
    assert smooth_mesh(verts[:0], faces[:0], 3)[0].shape == (0, 3) and _same_bits(smooth_mesh(verts, faces[:0], 3)[0], v_np)
    lonely = torch.tensor([[5, 5, 5], [7, 7, 7]], device='cuda')                             # faces without an edge: nobody has a neighbour
    assert _same_bits(smooth_mesh(verts, lonely, 3)[0], v_np)
    start, nbr, pinned = mesh_adjacency(lonely, 258)
    assert start.tolist() == [0] * 259 and nbr.shape == (0,) and nbr.dtype == torch.int32 and not pinned.any()
    start, nbr, pinned = mesh_adjacency(faces[:0], 4)
    assert start.tolist() == [0] * 5 and nbr.shape == (0,) and pinned.tolist() == [0] * 4
    view = torch.zeros(258, 6, device='cuda')[:, ::2]                                        # a strided view is smoothed as its values
    view.copy_(verts)
    assert _same_bits(smooth_mesh(view, faces, 2)[0], R.expected('sphere258', R.LAM, R.MU)[2])
    bad, worse = verts.clone(), verts.clone()
    bad[5, 1], worse[257, 2] = float('nan'), float('inf')
    for args in ((bad, faces, 2), (worse, faces, 2), (verts.double(), faces, 2), (verts, faces.int(), 2), (verts[:-1], faces, 2),
                 (verts, faces, -1), (verts, faces, 1001), (verts, faces, 1.5), (verts, faces, 2, 0.0), (verts, faces, 2, 1.01),
                 (verts, faces, 2, 0.5, 0.1), (verts, faces, 2, 0.5, -1.5)):
        with pytest.raises(ValueError):
            smooth_mesh(*args)
    with pytest.raises(ValueError):
        mesh_adjacency(faces, 257)


# ---------------------------------------------------------------- seams
@pytest.fixture(scope='module')
def scene(hip_lib):
    """one real tri-plane, its decoder seams and its G = 16 density grid (device): shared, never written"""
    from test_normals_gpu import _scene, _triplane, _Seams, _g
    G = 16
    inp = _scene(91, sigma_bias=10.0)
    dec = _Seams(_triplane(inp['dec']))
    pcl = _g(inp['planes'][1:2])
    sigma = dec.triplane_decode_grid({'planes_channel_last': pcl}, G)['sigma'][0]
    return dict(dec=dec, pcl=pcl, sigma=sigma, G=G)


def _bytes_equal(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_mesh_from_grid_smooths_before_the_query(scene, tmp_path):
    """colours and normals of a smoothed mesh are the field's values at the SMOOTHED positions; the faces are the unsmoothed call's"""
    from ln3diff_amd.mesh import extract_isosurface, mesh_from_grid, rotation_matrix_x
    dec, pcl, sigma, G = scene['dec'], scene['pcl'], scene['sigma'], scene['G']
    d = {'planes_channel_last': pcl}
    for opts in ({}, dict(normals=True), dict(simplify_cell=2.0, keep='largest')):
        plain = mesh_from_grid(dec, d, sigma, G, thr=10.0, **opts)
        assert _bytes_equal(mesh_from_grid(dec, d, sigma, G, thr=10.0, smooth_iters=0, **opts), plain)        # 0 is the call without the keyword
    rot = lambda a: (rotation_matrix_x(-90) @ a.cpu().numpy().T).T.astype(F32)             # noqa: E731
    for smooth, opts in ((dict(smooth_iters=3), dict(simplify_cell=2.0)), (dict(smooth_iters=2, smooth_lambda=0.25, smooth_mu=0.0), {})):
        plain = mesh_from_grid(dec, d, sigma, G, thr=10.0, normals=True, **opts)
        v, f, col, vn = mesh_from_grid(dec, d, sigma, G, thr=10.0, normals=True, path=str(tmp_path / 's.obj'), **smooth, **opts)
        assert len(f) > 20 and np.array_equal(f, plain[1]) and f.dtype == np.int64 and v.shape == plain[0].shape
        gv, gf = extract_isosurface(sigma.reshape(G, G, G), 10.0, **opts)
        assert np.array_equal(gf.cpu().numpy(), f)
        want = R.smooth(gv.cpu().numpy(), f, smooth['smooth_iters'], smooth.get('smooth_lambda', R.LAM), smooth.get('smooth_mu', R.MU))
        assert not np.array_equal(R.bits(want), R.bits(gv.cpu().numpy()))                   # the smoothing moved something
        vtx = (torch.from_numpy(want).cuda() / (G - 1) * 2 - 1) * 0.45
        q = dec.forward_points(pcl, vtx[None], with_grad=True)
        assert np.array_equal(R.bits(v), R.bits(rot(vtx)))                                  # the reference smoothing, mapped and rotated
        assert np.array_equal(col, (q['rgb'][0].clamp(0, 1) * 255).to(torch.uint8).cpu().numpy())
        assert np.array_equal(R.bits(vn), R.bits(rot(q['normal'][0])))
        three = mesh_from_grid(dec, d, sigma, G, thr=10.0, **smooth, **opts)
        assert len(three) == 3 and all(np.array_equal(a, b) for a, b in zip(three, (v, f, col)))
        pv, pvn, pf, _ = parse_obj(tmp_path / 's.obj')
        assert (len(pv), len(pvn)) == (len(v), len(vn)) and np.array_equal(pf, f)
    out = mesh_from_grid(dec, d, sigma, G, thr=10.0, smooth_iters=3, min_faces=10 ** 6)      # nothing survives the clean-up: nothing to smooth
    assert [a.shape for a in out] == [(0, 3)] * 3


def test_textured_mesh_from_grid_bakes_on_the_smoothed_vertices(scene):
    import mesh_bake_refs as BR
    from ln3diff_amd.mesh import atlas_layout, mesh_from_grid, textured_mesh_from_grid
    dec, pcl, sigma, G = scene['dec'], scene['pcl'], scene['sigma'], scene['G']
    d = {'planes_channel_last': pcl}
    opts = dict(simplify_cell=2.0, smooth_iters=3)
    plain = mesh_from_grid(dec, d, sigma, G, thr=10.0, **opts)
    nf = plain[1].shape[0]
    T = 4 * atlas_layout(nf, 8192)[0] + 2
    got = textured_mesh_from_grid(dec, d, sigma, G, thr=10.0, texture_size=T, **opts)
    assert len(got) == 5 and nf > 20 and _bytes_equal(got[:3], plain)
    assert not np.array_equal(got[0], mesh_from_grid(dec, d, sigma, G, thr=10.0, simplify_cell=2.0)[0])
    v = got[0]
    box = np.stack([v[:, 0], -v[:, 2], v[:, 1]], 1)                                        # the rotation (x, y, z) -> (x, z, -y) undone
    pts, owner = BR.points(box, got[1], T)
    rgb = dec.forward_points(pcl, torch.from_numpy(pts).cuda()[None])['rgb'][0]
    assert np.array_equal(got[4].reshape(-1, 3), BR.pack(rgb.cpu().numpy(), owner, 0))
    assert _bytes_equal(textured_mesh_from_grid(dec, d, sigma, G, thr=10.0, texture_size=T, simplify_cell=2.0, smooth_iters=0),
                        textured_mesh_from_grid(dec, d, sigma, G, thr=10.0, texture_size=T, simplify_cell=2.0))


def test_render_video_given_triplane_mesh_smooth_iters(hip_lib):
    from ln3diff_amd.mesh import extract_isosurface, rotation_matrix_x
    from ln3diff_amd.nsr.triplane import draw_render_noise
    from ln3diff_amd.pipeline import render_video_given_triplane
    from ln3diff_amd.synth import synth_input, orbit_cameras
    from test_normals_gpu import _small_ae
    ae, _ = _small_ae()
    G = 16
    cams = orbit_cameras(1).cuda()
    lat = synth_input('z', (2, 12, 32, 32), 7).cuda()
    j, u = draw_render_noise(2, 16 * 16, 64, generator=torch.Generator().manual_seed(1))
    d = {'latent_normalized_2Ddiffusion': lat.clone()}
    d.update(ae(latent=d, behaviour='decode_after_vae_no_render'))
    if d.get('planes_channel_last') is not None:
        d['planes_channel_last'] = ae.decoder.triplane_decoder.cast_planes(d['planes_channel_last'])
    grid = ae(latent=d, grid_size=G, behaviour='triplane_decode_grid')
    thr = float(torch.quantile(grid['sigma'][0].float().flatten(), 0.8))                    # a level inside the synthetic sample's own densities
    run = lambda **kw: render_video_given_triplane(lat.clone(), ae, cams, triplane_scaling_divider=1.0, jitter=j, u_fine=u, resolution=16,
                                                   export_mesh=True, mesh_size=G, mesh_thres=thr, **kw)        # noqa: E731
    a, b, c = run(), run(mesh_smooth_iters=0), run(mesh_smooth_iters=3)
    for k in ('image_raw', 'image_depth', 'weights_samples'):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    rot = lambda t: (rotation_matrix_x(-90) @ ((t / (G - 1) * 2 - 1) * 0.45).cpu().numpy().T).T.astype(F32)      # noqa: E731
    moved = 0
    for i, (ma, mb, mc) in enumerate(zip(a['mesh'], b['mesh'], c['mesh'])):
        assert _bytes_equal(ma, mb) and len(mc) == 3 and np.array_equal(ma[1], mc[1])       # the default call is unchanged; the faces stay
        gv, gf = extract_isosurface(grid['sigma'][i].reshape(G, G, G), thr)
        if gf.shape[0]:
            want = R.smooth(gv.cpu().numpy(), gf.cpu().numpy(), 3)
            assert np.array_equal(R.bits(mc[0]), R.bits(rot(torch.from_numpy(want).cuda())))
            moved += int((R.bits(mc[0]) != R.bits(ma[0])).any())
    assert moved
    with pytest.raises(ValueError, match='smooth_iters'):
        run(mesh_smooth_iters=1001)


def test_entry_point_mesh_smooth_iters(hip_lib, tmp_path):
    from ln3diff_amd.entry import create_argparser, run
    base = ("--arch_dit_decoder DiT2-B/2 --num_samples 2 --sample_steps 2 --image_size 32 --num_views 1 --mesh_grid 16 --dit_model_arch DiT-B/2 "
            "--trainer_name sgm_legacy --export_mesh true --mesh_thres 4.7 ")       # the synthetic decoder's densities lie in [4.1, 5.1]: a level inside
    go = lambda flags, out: run(create_argparser(True).parse_args((base + flags + f" --logdir {tmp_path / out}").split()))        # noqa: E731
    go("", 'plain')
    go("--mesh_smooth_iters 5", 'smooth')
    plain, smooth = json.load(open(tmp_path / 'plain' / 'args.json')), json.load(open(tmp_path / 'smooth' / 'args.json'))
    assert 'mesh_smooth_iters' not in plain and smooth['mesh_smooth_iters'] == 5
    assert {k: v for k, v in smooth.items() if k not in ('mesh_smooth_iters', 'logdir')} == {k: v for k, v in plain.items() if k != 'logdir'}
    changed = 0
    for i in range(2):
        v0, _, f0, _ = parse_obj(tmp_path / 'plain' / f'mesh_sample{i}.obj')
        v1, _, f1, _ = parse_obj(tmp_path / 'smooth' / f'mesh_sample{i}.obj')
        assert len(f0) > 20 and np.array_equal(f0, f1) and np.shape(v0) == np.shape(v1)
        changed += int(not np.array_equal(v0, v1))
    assert changed
    for flags in ("--mesh_smooth_iters 1001", "--mesh_smooth_iters -1"):
        with pytest.raises(SystemExit, match='mesh_smooth_iters'):
            go(flags, 'bad')
    with pytest.raises(SystemExit, match='export_mesh'):
        run(create_argparser(True).parse_args((base.replace("--export_mesh true", "--export_mesh false")
                                               + f"--mesh_smooth_iters 5 --logdir {tmp_path / 'no'}").split()))
