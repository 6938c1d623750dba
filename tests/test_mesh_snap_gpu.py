"""Level-set snapping on the GPU (include/ln3d_meshsnap.h): ln3d_snap_points and its f16 twin against the float64 loop of
tests/mesh_snap_refs.py - the checks are that file's, the ones tests/test_mesh_snap_cpu.py shows an fp32 stand-in to pass and every seeded
fault to fail - on sentinel-tailed buffers, then the seams: Triplane.snap_points, mesh.snap_mesh, mesh_from_grid,
textured_mesh_from_grid, render_video_given_triplane and the launcher flag.

The field's gradient jumps at texel centres and an fp32 loop can decide a close comparison the other way, so per-point comparisons with the
reference are made where the reference ALONE says that nothing is in doubt; the left-out shares are asserted (0.05 for one step, 0.10 for
the control flow).  The invariants - never worse, never farther than max_dist, state 0 <=> |residual| <= tol, residual = the kernel's own
sigma at the returned point minus level, bit for bit - hold for every point."""
import json

import numpy as np
import pytest
import torch

import mesh_snap_refs as R
import normal_refs as nr
from test_normals_cpu import parse_obj

pytestmark = pytest.mark.gpu

H, W, BOX = R.H, R.W, R.BOX
TAIL = 8
INT_SENTINEL = -7


def _g(t):
    return t.cuda().contiguous()


def _snap(planes, dec, pts, level, iters, tol, max_step, max_dist, f16=False):
    """one call on outputs with a NaN (or sentinel) tail behind each -> dict of CPU tensors"""
    from ln3diff_amd import ops
    P = pts.shape[0]
    out = torch.full((3 * P + TAIL,), float('nan'), device='cuda')
    res = torch.full((P + TAIL,), float('nan'), device='cuda')
    st = torch.full((P + TAIL,), INT_SENTINEL, dtype=torch.int32, device='cuda')
    ev = torch.full((P + TAIL,), INT_SENTINEL, dtype=torch.int32, device='cuda')
    ops.snap_points(_g(planes.half() if f16 else planes), H, W, _g(pts), tuple(_g(t) for t in dec), BOX, level, iters, tol, max_step, max_dist,
                    out[:3 * P].view(P, 3), res[:P], st[:P], ev[:P])
    torch.cuda.synchronize()
    out, res, st, ev = out.cpu(), res.cpu(), st.cpu(), ev.cpu()
    assert torch.isnan(out[3 * P:]).all() and torch.isnan(res[P:]).all() and bool((st[P:] == INT_SENTINEL).all()) and bool((ev[P:] == INT_SENTINEL).all()), \
        "the tail behind an output was written"
    return dict(points=out[:3 * P].reshape(P, 3), residual=res[:P], state=st[:P], evals=ev[:P])


def _sigma(planes, dec, pts, f16=False):
    from ln3diff_amd import ops
    P = pts.shape[0]
    sigma, grad = torch.empty(P, device='cuda'), torch.empty(P, 3, device='cuda')
    ops.query_points_grad(_g(planes.half() if f16 else planes), H, W, _g(pts), tuple(_g(t) for t in dec), BOX, sigma, grad)
    return sigma.cpu()


@pytest.mark.parametrize('P', R.SIZES)
def test_snap_points_against_the_float64_loop(hip_lib, P):
    c = R.case(P)
    snap = lambda pts, iters, md, f16=False: _snap(c['planes'], c['dec'], pts, c['level'], iters, c['tol'], c['max_step'], md, f16)   # noqa: E731
    fails, outs = R.run_all(c, snap, lambda pts: _sigma(c['planes'], c['dec'], pts))
    one, full, tight = outs['one'], outs['full'], outs['tight_full']
    ok = ~c['one']['doubt1'] & c['one']['accept0']
    frac = ((one['points'].double() - c['one']['cand']).abs() / c['one']['cand_bound'].clamp(min=1e-300))[ok]
    print(f"[snap] P={P}: one step worst {float(frac.max()) if frac.numel() else 0.0:.3g} of the bound on {int(ok.sum())} accepted points; "
          f"8 iterations: states {[int((full['state'] == k).sum()) for k in range(3)]} (reference {[int((c['full']['state'] == k).sum()) for k in range(3)]}), "
          f"mean evals {float(full['evals'].float().mean()):.2f}, median |residual| {float(outs['zero']['residual'].abs().median()):.4f} -> "
          f"{float(full['residual'].abs().median()):.2e}; tight: states {[int((tight['state'] == k).sum()) for k in range(3)]}")
    assert fails == []
    # binary16 texels: the f16 entry point on the rounded planes = the f32 entry point on their widened values, bit for bit, all four outputs
    planes16 = c['planes'].half().float()
    for iters, md in ((R.ITERS, c['max_dist']), (R.ITERS, c['tight']), (0, c['max_dist'])):
        a = snap(c['points'], iters, md, f16=True)
        b = _snap(planes16, c['dec'], c['points'], c['level'], iters, c['tol'], c['max_step'], md)
        for k in ('points', 'residual', 'state', 'evals'):
            assert torch.equal(R.bits(a[k]), R.bits(b[k])), (iters, k)


def test_non_finite_and_all_padding_points_stall_with_their_bits(hip_lib):
    c = R.case(65)
    nan, inf = float('nan'), float('inf')
    odd = torch.tensor([[nan, 0.0, 0.0], [0.1, inf, 0.0], [0.0, 0.1, -inf], [nan, nan, nan], [5.0, 5.0, 5.0], [-3.0, 0.0, 7.0], [1e30, -1e30, 0.0]])
    pts = torch.cat([odd, c['points'][:20]])
    ref = nr.sigma_and_grad(c['planes'], pts[4:7], c['dec'], BOX)
    assert bool(ref['all_padding'].all()) and abs(float(ref['sigma'][0]) - c['level']) > 2 * c['tol']      # the padding's own sigma is not the level
    for f16 in (False, True):
        got = _snap(c['planes'], c['dec'], pts, c['level'], R.ITERS, c['tol'], c['max_step'], c['max_dist'], f16)
        assert torch.equal(R.bits(got['points'][:7]), R.bits(pts[:7])) and bool((got['evals'][:7] == 1).all()) and bool((got['state'][:7] == 2).all())
        assert bool(torch.isfinite(got['residual']).all())                                  # a plane that a bad coordinate misses contributes its padding
        assert torch.equal(R.bits(got['residual'][3:7]), R.bits(got['residual'][3:4].expand(4)))          # all padding: one value
        zero = _snap(c['planes'], c['dec'], pts, c['level'], 0, c['tol'], c['max_step'], c['max_dist'], f16)
        assert torch.equal(R.bits(zero['points']), R.bits(pts)) and bool((zero['state'][3:7] == 1).all()) and bool((zero['evals'] == 1).all())
        assert bool((got['evals'][7:] >= 1).all()) and bool((got['state'][7:] == 0).any())


# ---------------------------------------------------------------- seams
@pytest.fixture(scope='module')
def scene(hip_lib):
    """one real tri-plane, its decoder seams and its G = 24 density grid (device), as test_mesh_vertex_normals builds them: shared, never written"""
    from test_normals_gpu import _scene, _triplane, _Seams
    G = 24
    inp = _scene(91, sigma_bias=10.0)
    dec = _Seams(_triplane(inp['dec']))
    pcl = _g(inp['planes'][1:2])
    sigma = dec.triplane_decode_grid({'planes_channel_last': pcl}, G)['sigma'][0]
    return dict(dec=dec, pcl=pcl, sigma=sigma, G=G, planes=inp['planes'][1], weights=inp['dec'])


def _bytes_equal(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _box(v):
    """the rotation (x, y, z) -> (x, z, -y) of the returned vertices undone: the box-space points the kernels saw, exactly"""
    return torch.from_numpy(np.stack([v[:, 0], -v[:, 2], v[:, 1]], 1)).float()


def test_triplane_and_snap_mesh_seams(scene):
    from ln3diff_amd.mesh import snap_mesh
    dec, pcl = scene['dec'], scene['pcl']
    c = R.case(257)
    tp = dec.triplane_decoder
    tol = 1e-3 * max(1.0, abs(10.0))                                                      # tol None; 0.01 and 0.02 are the other defaults
    r = tp.snap_points(pcl[0], _g(c['points']), 10.0, 4)
    assert set(r) == {'points', 'residual', 'state', 'evals'} and r['points'].shape == (257, 3) and r['state'].dtype == torch.int32
    want = _snap(scene['planes'], scene['weights'], c['points'], 10.0, 4, tol, 0.01, 0.02)
    for k in r:
        assert torch.equal(R.bits(r[k]), R.bits(want[k])), k
    e = tp.snap_points(pcl[0], _g(c['points'][:0]), 10.0, 4)
    assert e['points'].shape == (0, 3) and e['evals'].shape == (0,)
    s = dec.snap_points(pcl, _g(c['points'])[None], 10.0, 4)
    assert s['points'].shape == (1, 257, 3) and torch.equal(s['points'][0], r['points']) and torch.equal(s['evals'][0], r['evals'])
    v, diag = snap_mesh(dec, pcl, _g(c['points']), 10.0, 4)
    assert torch.equal(v, r['points']) and set(diag) == {'residual', 'state', 'evals'} and torch.equal(diag['state'], r['state'])
    before = tp.plane_precision
    try:                                                                                  # f16 texels as configured: cast_planes, then the f16 entry point
        tp.set_plane_precision('fp16')
        h = tp.snap_points(pcl[0], _g(c['points']), 10.0, 4)
    finally:
        tp.set_plane_precision(before)
    want16 = _snap(scene['planes'], scene['weights'], c['points'], 10.0, 4, tol, 0.01, 0.02, f16=True)
    assert torch.equal(R.bits(h['points']), R.bits(want16['points'])) and not torch.equal(h['points'], r['points'])


@pytest.mark.parametrize('opts', [{}, dict(simplify_cell=2.0, smooth_iters=3, keep='largest')], ids=['plain', 'simplified_smoothed'])
def test_mesh_from_grid_snaps_before_the_query(scene, tmp_path, opts):
    """the vertices of a snapped mesh lie on the level set as the float64 reference sees it, colours and normals are the field's values at the
    SNAPPED positions, and faces, vertex count and order are the unsnapped call's"""
    from ln3diff_amd.mesh import mesh_from_grid, rotation_matrix_x
    dec, pcl, sigma, G = scene['dec'], scene['pcl'], scene['sigma'], scene['G']
    d = {'planes_channel_last': pcl}
    thr, iters = 10.0, 8
    plain = mesh_from_grid(dec, d, sigma, G, thr=thr, normals=True, **opts)
    assert _bytes_equal(mesh_from_grid(dec, d, sigma, G, thr=thr, normals=True, snap_iters=0, **opts), plain)          # 0 is the call without the keyword
    v, f, col, vn = mesh_from_grid(dec, d, sigma, G, thr=thr, normals=True, snap_iters=iters, path=str(tmp_path / 's.obj'), **opts)
    assert len(f) > 100 and np.array_equal(f, plain[1]) and f.dtype == np.int64 and v.shape == plain[0].shape and v.dtype == np.float32
    p0, p1 = _box(plain[0]), _box(v)
    # exactly what one launch on the unsnapped vertices returns, with the documented defaults
    move = max(1.0, opts.get('simplify_cell', 0.0)) * 0.9 / (G - 1)
    tol = 1e-3 * max(1.0, abs(thr))
    want = _snap(scene['planes'], scene['weights'], p0, thr, iters, tol, move / 2, move)
    assert torch.equal(R.bits(want['points']), R.bits(p1))
    # on the level set, by the float64 reference
    s0 = (nr.sigma_and_grad(scene['planes'], p0, scene['weights'], BOX)['sigma'] - thr).abs()
    s1 = (nr.sigma_and_grad(scene['planes'], p1, scene['weights'], BOX)['sigma'] - thr).abs()
    ref = R.run_loop(R.field64(scene['planes'], scene['weights'], BOX), p0, thr, iters, tol, move / 2, move)
    m0, m1, mr = float(s0.median()), float(s1.median()), float(ref['residual'].abs().median())
    print(f"[snap] mesh {opts}: {len(v)} vertices, median |sigma - thr| {m0:.4f} -> {m1:.2e} (float64 loop {mr:.2e}); states "
          f"{[int((want['state'] == k).sum()) for k in range(3)]}, mean evals {float(want['evals'].float().mean()):.2f}")
    assert m0 / m1 >= 0.5 * (m0 / mr) and m1 < m0
    assert float((p1.double() - p0.double()).norm(dim=-1).max()) <= float(np.float32(move)) * (1 + 4 * R.F32_EPS)
    # colours and normals at the snapped positions
    rot = lambda a: (rotation_matrix_x(-90) @ a.cpu().numpy().T).T.astype(np.float32)       # noqa: E731
    q = dec.forward_points(pcl, _g(p1)[None], with_grad=True)
    assert np.array_equal(col, (q['rgb'][0].clamp(0, 1) * 255).to(torch.uint8).cpu().numpy())
    assert np.array_equal(R.bits(torch.from_numpy(vn)), R.bits(torch.from_numpy(rot(q['normal'][0]))))
    three = mesh_from_grid(dec, d, sigma, G, thr=thr, snap_iters=iters, **opts)
    assert len(three) == 3 and all(np.array_equal(a, b) for a, b in zip(three, (v, f, col)))
    pv, pvn, pf, _ = parse_obj(tmp_path / 's.obj')
    assert (len(pv), len(pvn)) == (len(v), len(vn)) and np.array_equal(pf, f)
    out = mesh_from_grid(dec, d, sigma, G, thr=thr, snap_iters=iters, min_faces=10 ** 6)    # nothing survives the clean-up: nothing to snap
    assert [a.shape for a in out] == [(0, 3)] * 3


def test_default_files_are_unchanged_and_the_bake_sees_the_snapped_vertices(scene, tmp_path):
    import mesh_bake_refs as BR
    from ln3diff_amd.mesh import atlas_layout, export_mesh, mesh_from_grid, textured_mesh_from_grid
    dec, pcl, sigma, G = scene['dec'], scene['pcl'], scene['sigma'], scene['G']
    d = {'planes_channel_last': pcl}
    nf = mesh_from_grid(dec, d, sigma, G, thr=10.0, simplify_cell=2.0)[1].shape[0]
    T = 4 * atlas_layout(nf, 8192)[0] + 2
    read = lambda stem: [open(tmp_path / (stem + ext), 'rb').read() for ext in ('.obj', '.mtl', '.png')]       # noqa: E731
    a = textured_mesh_from_grid(dec, d, sigma, G, thr=10.0, texture_size=T, simplify_cell=2.0, path=str(tmp_path / 'a.obj'))
    b = textured_mesh_from_grid(dec, d, sigma, G, thr=10.0, texture_size=T, simplify_cell=2.0, snap_iters=0, path=str(tmp_path / 'b.obj'))
    assert _bytes_equal(a, b)
    fa, fb = read('a'), read('b')
    assert fa[0].replace(b'a.mtl', b'b.mtl') == fb[0] and fa[1].replace(b'a.png', b'b.png') == fb[1] and fa[2] == fb[2]
    mesh_from_grid(dec, d, sigma, G, thr=10.0, path=str(tmp_path / 'p.obj'))
    mesh_from_grid(dec, d, sigma, G, thr=10.0, snap_iters=None, path=str(tmp_path / 'q.obj'))
    assert open(tmp_path / 'p.obj', 'rb').read() == open(tmp_path / 'q.obj', 'rb').read()
    got = textured_mesh_from_grid(dec, d, sigma, G, thr=10.0, texture_size=T, simplify_cell=2.0, snap_iters=8)
    plain = mesh_from_grid(dec, d, sigma, G, thr=10.0, simplify_cell=2.0, snap_iters=8)
    assert len(got) == 5 and nf > 20 and _bytes_equal(got[:3], plain) and np.array_equal(got[1], a[1]) and not np.array_equal(got[0], a[0])
    pts, owner = BR.points(_box(got[0]).numpy(), got[1], T)
    rgb = dec.forward_points(pcl, torch.from_numpy(pts).cuda()[None])['rgb'][0]
    assert np.array_equal(got[4].reshape(-1, 3), BR.pack(rgb.cpu().numpy(), owner, 0))       # the texels are taken on the snapped triangles
    n = export_mesh(dec, d, str(tmp_path / 'e.obj'), grid_size=G, thr=10.0, snap_iters=8, snap_tol=0.05, snap_max_move=0.5)
    assert n == (mesh_from_grid(dec, d, sigma, G, thr=10.0)[0].shape[0], mesh_from_grid(dec, d, sigma, G, thr=10.0)[1].shape[0])
    for bad in (dict(snap_iters=65), dict(snap_iters=1, snap_tol=-1.0), dict(snap_iters=1, snap_max_move=0.0)):
        with pytest.raises(ValueError, match='snap_'):
            mesh_from_grid(dec, d, sigma, G, thr=10.0, **bad)


def test_render_video_given_triplane_mesh_snap_iters(hip_lib):
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
    grid = ae(latent=d, grid_size=G, behaviour='triplane_decode_grid')
    thr = float(torch.quantile(grid['sigma'][0].float().flatten(), 0.8))                    # a level inside the synthetic sample's own densities
    run = lambda **kw: render_video_given_triplane(lat.clone(), ae, cams, triplane_scaling_divider=1.0, jitter=j, u_fine=u, resolution=16,
                                                   export_mesh=True, mesh_size=G, mesh_thres=thr, **kw)        # noqa: E731
    a, b, c = run(), run(mesh_snap_iters=0), run(mesh_snap_iters=6)
    for k in ('image_raw', 'image_depth', 'weights_samples'):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    moved = 0
    for ma, mb, mc in zip(a['mesh'], b['mesh'], c['mesh']):
        assert _bytes_equal(ma, mb) and len(mc) == 3 and np.array_equal(ma[1], mc[1]) and ma[0].shape == mc[0].shape     # the default call is unchanged; the faces stay
        moved += int(ma[0].shape[0] > 0 and not np.array_equal(ma[0], mc[0]))
    assert moved
    with pytest.raises(ValueError, match='snap_iters'):
        run(mesh_snap_iters=65)


def test_entry_point_mesh_snap_iters(hip_lib, tmp_path):
    from ln3diff_amd.entry import create_argparser, run
    base = ("--arch_dit_decoder DiT2-B/2 --num_samples 2 --sample_steps 2 --image_size 32 --num_views 1 --mesh_grid 16 --dit_model_arch DiT-B/2 "
            "--trainer_name sgm_legacy --export_mesh true --mesh_thres 4.7 ")       # the synthetic decoder's densities lie in [4.1, 5.1]: a level inside
    go = lambda flags, out: run(create_argparser(True).parse_args((base + flags + f" --logdir {tmp_path / out}").split()))        # noqa: E731
    go("", 'plain')
    go("--mesh_snap_iters 4", 'snap')
    plain, snap = json.load(open(tmp_path / 'plain' / 'args.json')), json.load(open(tmp_path / 'snap' / 'args.json'))
    assert 'mesh_snap_iters' not in plain and snap['mesh_snap_iters'] == 4
    assert {k: v for k, v in snap.items() if k not in ('mesh_snap_iters', 'logdir')} == {k: v for k, v in plain.items() if k != 'logdir'}
    changed = 0
    for i in range(2):
        v0, _, f0, _ = parse_obj(tmp_path / 'plain' / f'mesh_sample{i}.obj')
        v1, _, f1, _ = parse_obj(tmp_path / 'snap' / f'mesh_sample{i}.obj')
        assert len(f0) > 20 and np.array_equal(f0, f1) and np.shape(v0) == np.shape(v1)
        changed += int(not np.array_equal(v0, v1))
    assert changed
    for flags in ("--mesh_snap_iters 65", "--mesh_snap_iters -1"):
        with pytest.raises(SystemExit, match='mesh_snap_iters'):
            go(flags, 'bad')
    with pytest.raises(SystemExit, match='export_mesh'):
        run(create_argparser(True).parse_args((base.replace("--export_mesh true", "--export_mesh false")
                                               + f"--mesh_snap_iters 4 --logdir {tmp_path / 'no'}").split()))
