"""Texture baking on the GPU (include/ln3d_meshbake.h): the two entry points called through the C ABI on sentinel-filled, guarded buffers
and held to the numpy reference of tests/mesh_bake_refs.py by equality of bits; the whole bake through a stub field (an affine function,
which a bilinear look-up must give back) and through the real point query, f32 and f16 texels; then the seams: textured_mesh_from_grid
against mesh_from_grid, render_video_given_triplane and the launcher flag."""
import json
import os

import numpy as np
import pytest
import torch

import mesh_bake_refs as R
import mesh_clean_refs as M
from test_mesh_bake_cpu import decode_png, parse_textured
from test_normals_cpu import parse_obj

pytestmark = pytest.mark.gpu

GUARD = 64                                   # rows behind every output that a call must leave alone
SENTINEL = {torch.int32: -7, torch.uint8: 0xA5}
F32_SENTINEL = int(np.array([0x7fc0beef], dtype=np.int32)[0])          # a NaN with a payload no arithmetic produces


def _buf(n, width=None, dtype=torch.int32):
    """(whole, view): a sentinel-filled buffer of n rows plus GUARD rows, and the view of its first n rows that a call is given"""
    shape = (n + GUARD,) if width is None else (n + GUARD, width)
    if dtype == torch.float32:
        whole = torch.empty(shape, dtype=torch.int32, device='cuda').fill_(F32_SENTINEL).view(torch.float32)
    else:
        whole = torch.full(shape, SENTINEL[dtype], dtype=dtype, device='cuda')
    return whole, whole[:n]


def _intact(whole, n, what):
    tail = whole[n:]
    ok = bool((tail.view(torch.int32) == F32_SENTINEL).all()) if whole.dtype == torch.float32 else bool((tail == SENTINEL[whole.dtype]).all())
    assert ok, '%s: the guard behind the output was written' % what


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---------------------------------------------------------------- meshes
def _blob12(cell):
    """the G = 12 iso-surface of the suite's blob field in the +-0.45 box, optionally simplified: (verts f32 [nv,3], faces int64 [nf,3]) numpy"""
    from ln3diff_amd.mesh import extract_isosurface, simplify_mesh
    v, f = extract_isosurface(torch.from_numpy(M.blob_field(12)).cuda(), M.BLOB_THR)
    v, f = simplify_mesh(v, f, cell, (0.0, 0.0, 0.0))
    return ((v / 11 * 2 - 1) * 0.45).cpu().numpy(), f.cpu().numpy()


def _case(name):
    """name -> (verts, faces, [sizes])"""
    rng = np.random.default_rng(11)
    if name.startswith('blob'):
        v, f = _blob12(2.0 if name == 'blob12_cell2' else 0.0)
        n = R.layout(len(f), 8192)[0]
        return v, f, [4 * n, 4 * n + 3]
    nf, sizes = {'one_face': (1, [4]), 'border_strip': (4, [11]), 'one_cell_64': (2, [64]), 'exactly_full': (18, [12, 14]), 'odd_last': (7, [29])}[name]
    return R.soup(rng, nf) + (sizes,)


CASES = ['one_face', 'border_strip', 'one_cell_64', 'exactly_full', 'odd_last', 'blob12', 'blob12_cell2']


@pytest.mark.parametrize('name', CASES)
def test_points_and_owner_equal_the_reference(hip_lib, name):
    from ln3diff_amd import mesh
    verts, faces, sizes = _case(name)
    assert len(faces) >= 1 and (name != 'blob12_cell2' or len(faces) < len(_case('blob12')[1]))
    dv, df = torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda()
    for T in sizes:
        n, c = R.layout(len(faces), T)
        want_p, want_o = R.points(verts, faces, T)
        pw, pts = _buf(T * T, 3, torch.float32)
        ow, own = _buf(T * T, None, torch.int32)
        assert hip_lib.ln3d_bake_points(dv.data_ptr(), len(verts), df.data_ptr(), len(faces), T, n, c, pts.data_ptr(), own.data_ptr(), None) == 0
        torch.cuda.synchronize()
        _intact(pw, T * T, 'points')
        _intact(ow, T * T, 'owner')
        assert np.array_equal(own.cpu().numpy(), want_o), (name, T)
        assert np.array_equal(_bits(pts.cpu().numpy()), _bits(want_p)), (name, T, int((_bits(pts.cpu().numpy()) != _bits(want_p)).sum()))
        p2, o2 = mesh.bake_points(dv, df, T)                                           # the wrapper: the same bits
        assert torch.equal(p2.view(torch.int32), pts.view(torch.int32)) and torch.equal(o2, own) and o2.dtype == torch.int32
    if name == 'one_face':
        assert (n, c) == (1, 4) and want_o.reshape(4, 4).tolist() == [[0, 0, 0, 0], [0, 0, 0, -1], [0, 0, -1, -1], [0, -1, -1, -1]]
    if name == 'exactly_full':
        assert len(faces) == 2 * n * n and (want_o.reshape(T, T)[:n * c, :n * c] >= 0).all()


def test_bake_points_refuses_what_it_cannot_lay_out(hip_lib):
    from ln3diff_amd import mesh
    verts, faces, _ = _case('exactly_full')
    dv, df = torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda()
    with pytest.raises(ValueError, match="smallest sufficient size is 12\\b"):
        mesh.bake_points(dv, df, 11)
    with pytest.raises(ValueError, match="outside"):
        mesh.bake_points(dv, df + len(verts), 12)
    with pytest.raises(ValueError):
        mesh.bake_points(dv.double(), df, 12)


def test_pack_equals_the_reference(hip_lib):
    from ln3diff_amd import ops
    one = np.float32(1 / 255)
    vals = np.array([-1, -0.0, 0, np.nextafter(one, np.float32(0)), one, np.nextafter(one, np.float32(1)), 0.5, 1, 2, np.nan, np.inf, -np.inf,
                     0.999999, 254.5 / 255, 1e-30], np.float32)
    P = len(vals)
    rgb = np.stack([vals, np.roll(vals, 1), np.roll(vals, 5)], 1)
    for owner, fill in ((np.arange(P) % 2 - 1, 7), (-(np.arange(P) % 2), 255), (np.full(P, 5), 0), (np.full(P, -1), 0)):
        owner = owner.astype(np.int32)
        tw, tex = _buf(P, 3, torch.uint8)
        d_rgb, d_own = torch.from_numpy(rgb).cuda(), torch.from_numpy(owner).cuda()
        assert hip_lib.ln3d_bake_pack(d_rgb.data_ptr(), d_own.data_ptr(), P, fill, tex.data_ptr(), None) == 0
        torch.cuda.synchronize()
        _intact(tw, P, 'tex')
        assert np.array_equal(tex.cpu().numpy(), R.pack(rgb, owner, fill)), (owner.tolist(), fill)
        t2 = torch.empty(P, 3, dtype=torch.uint8, device='cuda')
        ops.bake_pack(d_rgb, d_own, fill, t2)
        assert torch.equal(t2, tex)
    # the rule of the vertex colours, on the device, for everything but NaN
    ok = ~np.isnan(rgb).any(1)
    dev = (torch.from_numpy(rgb[ok]).cuda().clamp(0, 1) * 255).to(torch.uint8).cpu().numpy()
    assert np.array_equal(R.quantise(rgb[ok]), dev)


# ---------------------------------------------------------------- the whole bake
COEF = np.array([[0.15, -0.10, 0.05], [-0.10, 0.10, 0.10], [0.05, 0.10, -0.10]], np.float32)         # column j: channel j; |coefficient| <= 1
OFFSET = np.array([0.5, 0.45, 0.55], np.float32)


class _AffineField:
    """a decoder whose colour is an affine function of position, evaluated on the device.  A texel that a look-up inside a UV triangle reads
    lies at (1 - s - t) v0 + s v1 + t v2 with s, t >= 0 and s + t <= (c - 2) / (c - 3) <= 2, so within 3 * 0.45 = 1.35 per axis; the
    coefficients of a channel sum to at most 0.3 in magnitude, so the colour stays within 0.5 +- 0.05 +- 0.405, inside (0, 1), and the
    pack's clamp never acts on such a texel."""
    def forward_points(self, planes_channel_last, points, with_grad=False):
        assert points.is_cuda and points.dim() == 3 and points.shape[0] == 1
        coef, off = torch.from_numpy(COEF).to(points.device), torch.from_numpy(OFFSET).to(points.device)
        return {'rgb': (points[..., :, None] * coef).sum(-2) + off}                     # elementwise fp32: no BLAS in between


@pytest.mark.parametrize('name,T', [('odd_last', 29), ('border_strip', 11), ('one_cell_64', 64), ('blob12', None), ('blob12_cell2', None)])
def test_bilinear_lookup_gives_the_field_back(hip_lib, name, T):
    """UV, ownership, points and orientation together: at the corners and at random points of every face, the bilinear look-up of the baked
    texture at the interpolated UV differs from the field at the interpolated position by less than 1/255 (truncation to uint8) + 1e-5
    (fp32 rounding of the points over |p| <= 0.45, and of uv * T, at most 2^-24 T <= 8e-6 of a texel for T <= 128)."""
    from ln3diff_amd import mesh
    verts, faces, sizes = _case(name)
    T = T or sizes[1]
    assert T <= 128
    uv, tex = mesh.bake_texture(_AffineField(), None, torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda(), T, fill=255)
    assert uv.dtype == np.float32 and np.array_equal(uv, R.uvs(len(faces), T)) and tex.shape == (T, T, 3) and tex.dtype == np.uint8
    owner = R.texels(len(faces), T)[0].reshape(T, T)
    assert (tex[owner < 0] == 255).all()
    w = R.bary_samples(np.random.default_rng(5), 12)
    val = tex.astype(np.float64) / 255.0
    worst = 0.0
    for f in range(len(faces)):
        p = w @ uv[f].astype(np.float64) * T
        got = R.lookup(val, p[:, 0], p[:, 1])
        want = (w @ verts[faces[f]].astype(np.float64)) @ COEF.astype(np.float64) + OFFSET.astype(np.float64)
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"[bake] {name} T={T}: {len(faces)} faces, worst |look-up - field| = {worst:.6f} (bound {1 / 255 + 1e-5:.6f})")
    assert worst < 1 / 255 + 1e-5


@pytest.fixture(scope='module')
def scene(hip_lib):
    """one real tri-plane, its decoder seams and the G = 24 level set, simplified to cell 2 (device): shared, never written"""
    from ln3diff_amd.mesh import extract_isosurface
    from test_normals_gpu import _scene, _triplane, _Seams, _g
    G = 24
    inp = _scene(91, sigma_bias=10.0)
    dec = _Seams(_triplane(inp['dec']))
    pcl = _g(inp['planes'][1:2])
    sigma = dec.triplane_decode_grid({'planes_channel_last': pcl}, G)['sigma'][0]
    v, f = extract_isosurface(sigma.reshape(G, G, G), 10.0, simplify_cell=2.0)
    return dict(dec=dec, pcl=pcl, sigma=sigma, G=G, vtx=(v / (G - 1) * 2 - 1) * 0.45, faces=f)


@pytest.mark.parametrize('precision', ['fp32', 'fp16'])
def test_real_field_texels_follow_the_vertex_colour_rule(scene, precision):
    from ln3diff_amd import mesh
    dec, pcl, vtx, faces = scene['dec'], scene['pcl'], scene['vtx'], scene['faces']
    nf = faces.shape[0]
    assert nf > 50
    T = 4 * R.layout(nf, 8192)[0] + 5
    tp = dec.triplane_decoder
    tp.set_plane_precision(precision)
    try:
        uv, tex = mesh.bake_texture(dec, pcl, vtx, faces, T, fill=9)
        pts, owner = mesh.bake_points(vtx, faces, T)
        rgb = dec.forward_points(pcl, pts[None])['rgb'][0]
    finally:
        tp.set_plane_precision('fp32')
    want = (rgb.clamp(0, 1) * 255).to(torch.uint8).cpu().numpy()                        # the line that colours the vertices
    own = owner.cpu().numpy() >= 0
    flat = tex.reshape(-1, 3)
    assert np.array_equal(flat[own], want[own]) and (flat[~own] == 9).all() and 0 < int(own.sum()) < T * T
    assert np.array_equal(owner.cpu().numpy(), R.texels(nf, T)[0]) and uv.shape == (nf, 3, 2)
    assert len(np.unique(flat[own], axis=0)) > 1                                        # a texture, not one colour


# ---------------------------------------------------------------- seams
@pytest.mark.parametrize('opts', [{}, dict(normals=True), dict(simplify_cell=2.0), dict(normals=True, simplify_cell=2.0, keep='largest')])
def test_textured_mesh_from_grid_adds_to_mesh_from_grid(scene, tmp_path, opts):
    from ln3diff_amd.mesh import atlas_layout, mesh_from_grid, textured_mesh_from_grid
    dec, d, sigma, G = scene['dec'], {'planes_channel_last': scene['pcl']}, scene['sigma'], scene['G']
    plain = mesh_from_grid(dec, d, sigma, G, thr=10.0, path=str(tmp_path / 'plain.obj'), **opts)
    nf = plain[1].shape[0]
    T = 4 * atlas_layout(nf, 8192)[0] + 2
    got = textured_mesh_from_grid(dec, d, sigma, G, thr=10.0, path=str(tmp_path / 'tex.obj'), texture_size=T, **opts)
    assert len(got) == len(plain) + 2 and nf > 50
    for a, b in zip(plain, got):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()                 # bit for bit
    uv, tex = got[-2:]
    assert np.array_equal(uv, R.uvs(nf, T)) and tex.shape == (T, T, 3) and tex.dtype == np.uint8
    # the texture is the bake at the BOX-space vertices: (x, y, z) -> (x, z, -y) undone
    v = got[0]
    box = np.stack([v[:, 0], -v[:, 2], v[:, 1]], 1)
    pts, owner = R.points(box, got[1], T)
    rgb = dec.forward_points(scene['pcl'], torch.from_numpy(pts).cuda()[None])['rgb'][0]
    assert np.array_equal(tex.reshape(-1, 3), R.pack(rgb.cpu().numpy(), owner, 0))
    # the three files
    t = parse_textured(tmp_path / 'tex.obj')
    lines = open(tmp_path / 'plain.obj').read().splitlines()
    assert t['v'] == [ln for ln in lines if ln.startswith('v ')] and t['vn'] == [ln for ln in lines if ln.startswith('vn ')]
    assert len(t['vn']) == (len(v) if opts.get('normals') else 0) and t['vt'].shape == (3 * nf, 2)
    assert np.array_equal(t['fv'], got[1]) and np.array_equal(t['ft'], np.arange(3 * nf).reshape(nf, 3))
    assert (t['fn'] is None) if not opts.get('normals') else np.array_equal(t['fn'], got[1])
    assert open(tmp_path / 'tex.mtl').read() == 'newmtl baked\nKd 1 1 1\nmap_Kd tex.png\n'
    assert np.array_equal(decode_png(tmp_path / 'tex.png'), tex[::-1])
    # one cell row too few
    small = 4 * atlas_layout(nf, 8192)[0] - 1
    with pytest.raises(ValueError, match=f"smallest sufficient size is {small + 1}\\b"):
        textured_mesh_from_grid(dec, d, sigma, G, thr=10.0, texture_size=small, **opts)


def test_textured_mesh_from_grid_empty(scene, tmp_path):
    from ln3diff_amd.mesh import textured_mesh_from_grid
    out = textured_mesh_from_grid(scene['dec'], {'planes_channel_last': scene['pcl']}, scene['sigma'], scene['G'], thr=10.0, texture_size=16,
                                  min_faces=10 ** 6, path=str(tmp_path / 'none.obj'))
    assert [a.shape for a in out] == [(0, 3)] * 3 + [(0, 3, 2), (16, 16, 3)] and not out[4].any()
    assert parse_textured(tmp_path / 'none.obj')['order'] == ['mtllib', 'usemtl'] and decode_png(tmp_path / 'none.png').shape == (16, 16, 3)


def test_render_video_given_triplane_mesh_texture_size(hip_lib, tmp_path):
    from ln3diff_amd.nsr.triplane import draw_render_noise
    from ln3diff_amd.pipeline import render_video_given_triplane
    from ln3diff_amd.synth import synth_input, orbit_cameras
    from test_normals_gpu import _small_ae
    ae, _ = _small_ae()
    cams = orbit_cameras(1).cuda()
    lat = synth_input('z', (2, 12, 32, 32), 7).cuda()
    j, u = draw_render_noise(2, 16 * 16, 64, generator=torch.Generator().manual_seed(1))
    # the level is taken from the synthetic sample's own densities so that there is a surface to texture
    d = {'latent_normalized_2Ddiffusion': lat.clone()}
    d.update(ae(latent=d, behaviour='decode_after_vae_no_render'))
    if d.get('planes_channel_last') is not None:
        d['planes_channel_last'] = ae.decoder.triplane_decoder.cast_planes(d['planes_channel_last'])
    thr = float(torch.quantile(ae(latent=d, grid_size=16, behaviour='triplane_decode_grid')['sigma'][0].float().flatten(), 0.8))
    run = lambda **kw: render_video_given_triplane(lat.clone(), ae, cams, triplane_scaling_divider=1.0, jitter=j, u_fine=u, resolution=16,
                                                   export_mesh=True, mesh_size=16, mesh_thres=thr, **kw)      # 16^3: few enough faces for 128 x 128
    a, b = run(), run(mesh_texture_size=0)
    assert set(a) == set(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
    for ma, mb in zip(a['mesh'], b['mesh']):
        assert len(ma) == len(mb) == 3 and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(ma, mb))
    s = run(mesh_simplify_cell=2.0)
    c = run(mesh_simplify_cell=2.0, mesh_texture_size=128, mesh_path=str(tmp_path / 'm{}.obj'))
    for k in ('image_raw', 'image_depth', 'weights_samples'):
        assert torch.equal(a[k], c[k]), k
    for i, (ms, mc) in enumerate(zip(s['mesh'], c['mesh'])):
        assert len(mc) == 5 and all(np.array_equal(x, y) for x, y in zip(ms, mc)) and mc[4].shape == (128, 128, 3)
        t = parse_textured(tmp_path / f'm{i}.obj')
        assert len(t['v']) == len(mc[0]) and np.array_equal(t['fv'], mc[1]) and t['vt'].shape == (3 * len(mc[1]), 2)
        assert t['mtllib'] == [f'mtllib m{i}.mtl'] and open(tmp_path / f'm{i}.mtl').read().endswith(f'map_Kd m{i}.png\n')
        assert np.array_equal(decode_png(tmp_path / f'm{i}.png'), mc[4][::-1])
    assert max(len(m[1]) for m in c['mesh']) > 2                                       # more than the two faces a 4 x 4 texture holds
    with pytest.raises(ValueError, match="smallest sufficient size is"):
        run(mesh_simplify_cell=2.0, mesh_texture_size=4)


# ---------------------------------------------------------------- launcher
def test_entry_point_mesh_texture_size(hip_lib, tmp_path):
    from ln3diff_amd.entry import create_argparser, run
    base = ("--arch_dit_decoder DiT2-B/2 --num_samples 2 --sample_steps 2 --image_size 32 --num_views 1 --mesh_grid 24 --dit_model_arch DiT-B/2 "
            "--trainer_name sgm_legacy --export_mesh true --mesh_thres 4.7 ")       # the synthetic decoder's densities lie in [4.1, 5.1]: a level inside
    go = lambda flags, out: run(create_argparser(True).parse_args((base + flags + f" --logdir {tmp_path / out}").split()))        # noqa: E731
    go("--mesh_simplify_cell 2", 'plain')
    go("--mesh_simplify_cell 2", 'again')
    go("--mesh_simplify_cell 2 --mesh_texture_size 256", 'tex')
    plain, tex = json.load(open(tmp_path / 'plain' / 'args.json')), json.load(open(tmp_path / 'tex' / 'args.json'))
    assert 'mesh_texture_size' not in plain and tex['mesh_texture_size'] == 256
    assert {k: v for k, v in tex.items() if k not in ('mesh_texture_size', 'logdir')} == {k: v for k, v in plain.items() if k != 'logdir'}
    assert sorted(os.listdir(tmp_path / 'plain')) == sorted(os.listdir(tmp_path / 'again'))
    assert not [n for n in os.listdir(tmp_path / 'plain') if n.endswith(('.mtl', '.png'))]
    faces = []
    for i in range(2):
        name = f'mesh_sample{i}'
        assert open(tmp_path / 'plain' / f'{name}.obj', 'rb').read() == open(tmp_path / 'again' / f'{name}.obj', 'rb').read()
        t = parse_textured(tmp_path / 'tex' / f'{name}.obj')
        lines = open(tmp_path / 'plain' / f'{name}.obj').read().splitlines()
        assert t['v'] == [ln for ln in lines if ln.startswith('v ')]                       # the geometry and vertex colours of the untextured export
        _, _, pf, _ = parse_obj(tmp_path / 'plain' / f'{name}.obj')
        assert np.array_equal(t['fv'], pf) and np.array_equal(t['ft'], np.arange(3 * len(pf)).reshape(-1, 3))
        assert open(tmp_path / 'tex' / f'{name}.mtl').read() == f'newmtl baked\nKd 1 1 1\nmap_Kd {name}.png\n'
        assert decode_png(tmp_path / 'tex' / f'{name}.png').shape == (256, 256, 3)
        faces.append(len(pf))
    assert max(faces) > 2                                                              # more than the two faces a 4 x 4 texture holds
    for flags in ("--mesh_texture_size 3", "--mesh_texture_size 9000"):
        with pytest.raises(SystemExit, match='mesh_texture_size'):
            go(flags, 'bad')
    with pytest.raises(SystemExit, match='export_mesh'):
        run(create_argparser(True).parse_args((base.replace("--export_mesh true", "--export_mesh false")
                                               + f"--mesh_texture_size 256 --logdir {tmp_path / 'no'}").split()))
    # a texture too small for the extracted faces fails the export and says what would do
    with pytest.raises(RuntimeError, match="smallest sufficient size is .*--mesh_simplify_cell"):
        go("--mesh_simplify_cell 2 --mesh_texture_size 4", 'small')
