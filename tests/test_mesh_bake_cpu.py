"""The host side of the texture bake (include/ext/ln3d_meshbake.h), without a GPU:
  - mesh.atlas_layout / atlas_uvs equal the reference of tests/mesh_bake_refs.py, at the edges of the capacity too;
  - the property the layout exists for, for every cell size c = 4 ... 13: a bilinear look-up at the corners, the edge midpoints and random
    points of a face's UV triangle has its non-zero taps in texels that face owns (exact arithmetic: dyadic weights, half-integer corners);
  - an affine field baked unquantised at the reference's points comes back from the bilinear look-up to 1e-6;
  - write_png decodes (by an inverse written here, and by Pillow where it imports) to the flipped array; write_obj_textured parses back;
  - mesh_texture_size, from every public entry of pipeline down: 0 calls mesh_from_grid with the four MeshPost keywords only, 64 calls
    textured_mesh_from_grid with texture_size=64 plus the four, and without export_mesh neither is called."""
import struct
import zlib

import numpy as np
import pytest
import torch

import mesh_bake_refs as R


# ---------------------------------------------------------------- layout
@pytest.mark.parametrize('nf,size,want', [(1, 4, (1, 4)), (2, 4, (1, 4)), (1, 64, (1, 64)), (2, 64, (1, 64)), (3, 11, (2, 5)), (4, 11, (2, 5)),
                                          (8, 8, (2, 4)), (9, 12, (3, 4)), (18, 12, (3, 4)), (19, 16, (4, 4)), (131072, 1024, (256, 4)),
                                          (524288, 2048, (512, 4)), (224000, 2048, (335, 6))])
def test_atlas_layout(nf, size, want):
    from ln3diff_amd.mesh import atlas_layout, atlas_uvs
    assert atlas_layout(nf, size) == want == R.layout(nf, size)
    n, c = want
    assert n * n >= -(-nf // 2) and (n == 1 or (n - 1) ** 2 < -(-nf // 2)) and c == size // n
    if nf <= 64:
        uv = atlas_uvs(nf, size)
        assert uv.dtype == np.float32 and uv.shape == (nf, 3, 2) and np.array_equal(uv, R.uvs(nf, size))


def test_atlas_layout_capacity_edge():
    from ln3diff_amd.mesh import atlas_layout, atlas_uvs
    for n in (1, 2, 3, 7, 256):
        full = 2 * n * n
        assert atlas_layout(full, 4 * n) == (n, 4)                                   # exactly full at the smallest cell
        assert atlas_layout(full, 4 * n + 3) == (n, 4 + 3 // n)
        with pytest.raises(ValueError, match=f"smallest sufficient size is {4 * (n + 1)}\\b"):
            atlas_layout(full + 1, max(4 * n, 4))                                    # one face more needs another row of cells
        if n > 1:
            with pytest.raises(ValueError, match=f"smallest sufficient size is {4 * n}\\b"):
                atlas_layout(full, 4 * n - 1)
    assert atlas_layout(131072, 1024) == (256, 4) and atlas_layout(524288, 2048) == (512, 4)
    with pytest.raises(ValueError, match="smallest sufficient size is 1028"):
        atlas_layout(131073, 1024)
    with pytest.raises(ValueError, match="smallest sufficient size is 8196, above the largest texture"):
        atlas_layout(2 * 2048 * 2048 + 1, 8192)
    for bad in (3, 8193, 0, -4, 64.5, True, 'big'):
        with pytest.raises((ValueError, TypeError)):
            atlas_layout(2, bad)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError):
            atlas_layout(bad, 64)
    assert atlas_uvs(0, 64).shape == (0, 3, 2)


def test_uv_corners_are_counter_clockwise_and_inside_their_cell():
    for nf, size in ((5, 11), (2, 64), (8, 8)):
        n, c = R.layout(nf, size)
        num = R.uv_numerators(nf, size)
        e1, e2 = num[:, 1] - num[:, 0], num[:, 2] - num[:, 0]
        assert (e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0] > 0).all()                 # v up: a positive cross product is counter-clockwise
        k = np.arange(nf) // 2
        origin = np.stack([(k % n) * c, (k // n) * c], -1)[:, None]
        assert (num > origin).all() and (num < origin + c).all()


@pytest.mark.parametrize('c', range(4, 14))
def test_bilinear_taps_stay_in_owned_texels(c):
    """nf = 7 on a 2 x 2 grid of cells (the last cell has no odd face), with a border strip of 1 texel"""
    nf, size = 7, 2 * c + 1
    assert R.layout(nf, size) == (2, c)
    owner, _, _ = R.texels(nf, size)
    num = R.uv_numerators(nf, size)
    w = R.bary_samples(np.random.default_rng(c), 200)
    seen = np.zeros(size * size, bool)
    for f in range(nf):
        px, py = w @ num[f, :, 0], w @ num[f, :, 1]
        for x, y in zip(px, py):
            for tx, ty, wt in R.taps(x, y, size):
                assert owner[ty * size + tx] == f, (c, f, x, y, tx, ty, wt)
                seen[ty * size + tx] = True
    # ownership: the two triangles of a cell, nothing in the absent face, the unused cell or the strip
    grid = owner.reshape(size, size)
    assert (grid[2 * c:] == -1).all() and (grid[:, 2 * c:] == -1).all()
    assert sorted(np.unique(owner).tolist()) == [-1] + list(range(nf))
    assert (np.bincount(owner[owner >= 0]) == [c * (c + 1) // 2, c * (c - 1) // 2] * 3 + [c * (c + 1) // 2]).all()
    assert int((grid[c:2 * c, c:2 * c] == -1).sum()) == c * (c - 1) // 2                # the absent odd face of the last cell
    assert not seen[owner < 0].any()


@pytest.mark.parametrize('nf,size', [(1, 4), (4, 11), (2, 64), (8, 8), (7, 29)])
def test_affine_field_comes_back_from_the_lookup(nf, size):
    rng = np.random.default_rng(nf * 100 + size)
    verts, faces = R.soup(rng, nf)
    pts, owner = R.points(verts, faces, size)
    A, b = rng.uniform(-1, 1, (3, 3)), rng.uniform(-1, 1, 3)
    tex = (pts.astype(np.float64) @ A + b).reshape(size, size, 3)
    tex[owner.reshape(size, size) < 0] = 1e6                                          # a tap outside the owned texels would show
    num = R.uv_numerators(nf, size)
    w = R.bary_samples(rng, 50)
    for f in range(nf):
        got = R.lookup(tex, w @ num[f, :, 0], w @ num[f, :, 1])
        want = (w @ verts[faces[f]].astype(np.float64)) @ A + b
        assert np.abs(got - want).max() <= 1e-6, (f, np.abs(got - want).max())
    # the corner texels hold the corners (corner 0 exactly: s = t = 0; the others through v0 + 1 * (v - v0)), unowned texels the origin
    n, c = R.layout(nf, size)
    for f in range(nf):
        for j in range(3):
            x, y = (num[f, j] - 0.5).astype(int)
            assert owner[y * size + x] == f and np.abs(pts[y * size + x] - verts[faces[f, j]]).max() <= (0 if j == 0 else 2.0 ** -23), (f, j)
    assert (pts[owner < 0] == 0).all()


def test_pack_reference_rule():
    one = np.float32(1 / 255)
    x = np.array([-1, -0.0, 0, np.nextafter(one, np.float32(0)), one, np.nextafter(one, np.float32(1)), 0.5, 1, 2, np.nan, np.inf, -np.inf], np.float32)
    near = [int(np.float32(a) * np.float32(255)) for a in x[3:6]]                     # 1 / 255 and its neighbours: one float32 product, truncated
    assert R.quantise(x).tolist() == [0, 0, 0] + near + [127, 255, 255, 0, 255, 0] and near[0] == 0 and near[2] == 1
    t = torch.from_numpy(x[~np.isnan(x)])
    assert np.array_equal(R.quantise(t.numpy()), (t.clamp(0, 1) * 255).to(torch.uint8).numpy())         # the line that colours the vertices


# ---------------------------------------------------------------- files
def decode_png(path):
    """the inverse of mesh.write_png: 8-bit RGB, filter 0 on every row, checksums verified -> [H,W,3] uint8 in FILE order (top row first)"""
    data = open(path, 'rb').read()
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, chunks = 8, []
    while pos < len(data):
        (length,), kind = struct.unpack('>I', data[pos:pos + 4]), data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + length]
        assert struct.unpack('>I', data[pos + 8 + length:pos + 12 + length])[0] == zlib.crc32(kind + body) & 0xffffffff, kind
        chunks.append((kind, body))
        pos += 12 + length
    assert [k for k, _ in chunks][0] == b'IHDR' and chunks[-1] == (b'IEND', b'')
    w, h, depth, colour, comp, filt, lace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(b''.join(b for k, b in chunks if k == b'IDAT')), np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, 3)


@pytest.mark.parametrize('shape', [(1, 1), (4, 4), (5, 3), (64, 64)])
def test_write_png_round_trips(tmp_path, shape):
    from ln3diff_amd.mesh import write_png
    tex = np.random.default_rng(shape[0]).integers(0, 256, shape + (3,), dtype=np.uint8)
    write_png(tmp_path / 't.png', tex)
    assert np.array_equal(decode_png(tmp_path / 't.png'), tex[::-1])                  # the top row of the file is the last row of the array
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        img = Image.open(tmp_path / 't.png')
        assert img.mode == 'RGB' and img.size == (shape[1], shape[0]) and np.array_equal(np.asarray(img), tex[::-1])
    for bad in (tex.astype(np.float32), tex[..., :2], tex[0]):
        with pytest.raises(ValueError):
            write_png(tmp_path / 'bad.png', bad)


def parse_textured(path):
    """-> dict: the lines by record type, and the parsed vt [Nt,2], face vertex / texture / normal indices (0-based; normals None if absent)"""
    lines = open(path).read().splitlines()
    by = lambda k: [ln for ln in lines if ln.split()[0] == k]                         # noqa: E731
    corners = [[c.split('/') for c in ln.split()[1:]] for ln in by('f')]
    pick = lambda i: np.array([[int(c[i]) - 1 for c in f] for f in corners]).reshape(-1, 3)          # noqa: E731
    return dict(order=[ln.split()[0] for ln in lines], v=by('v'), vn=by('vn'), mtllib=by('mtllib'), usemtl=by('usemtl'),
                vt=np.array([[float(x) for x in ln.split()[1:]] for ln in by('vt')]).reshape(-1, 2),
                fv=pick(0), ft=pick(1), fn=pick(2) if corners and len(corners[0][0]) == 3 else None)


@pytest.mark.parametrize('normals', [False, True])
def test_write_obj_textured_parses_back(tmp_path, normals):
    from ln3diff_amd.mesh import atlas_uvs, write_obj, write_obj_textured
    rng = np.random.default_rng(3)
    v = rng.uniform(-1, 1, (6, 3)).astype(np.float32)
    f = np.array([[0, 1, 2], [2, 1, 3], [3, 4, 5], [5, 0, 2], [1, 4, 0]], np.int64)
    col = rng.integers(0, 256, (6, 3)).astype(np.float32) / 255
    n = rng.uniform(-1, 1, (6, 3)).astype(np.float32) if normals else None
    uv = atlas_uvs(len(f), 32)
    write_obj(tmp_path / 'plain.obj', v, f, col, n)
    write_obj_textured(tmp_path / 'tex.obj', v, f, col, uv, n)
    plain = open(tmp_path / 'plain.obj').read().splitlines()
    t = parse_textured(tmp_path / 'tex.obj')
    assert t['v'] == [ln for ln in plain if ln.startswith('v ')] and t['vn'] == [ln for ln in plain if ln.startswith('vn ')]
    assert len(t['v']) == 6 and len(t['vn']) == (6 if normals else 0)
    assert t['order'] == ['mtllib'] + ['v'] * 6 + ['vn'] * len(t['vn']) + ['vt'] * 15 + ['usemtl'] + ['f'] * 5
    assert t['mtllib'] == ['mtllib tex.mtl'] and t['usemtl'] == ['usemtl baked']
    assert np.array_equal(t['fv'], f) and np.array_equal(t['ft'], np.arange(15).reshape(5, 3))
    assert (t['fn'] is None) if not normals else np.array_equal(t['fn'], f)
    assert np.abs(t['vt'] - uv.reshape(-1, 2)).max() <= 5e-9                          # eight decimals
    assert open(tmp_path / 'tex.mtl').read().split('\n') == ['newmtl baked', 'Kd 1 1 1', 'map_Kd tex.png', '']
    # an empty mesh: files without records
    e3, ef = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)
    write_obj_textured(tmp_path / 'none.obj', e3, ef, e3, atlas_uvs(0, 32), e3 if normals else None)
    assert parse_textured(tmp_path / 'none.obj')['order'] == ['mtllib', 'usemtl'] and (tmp_path / 'none.mtl').exists()


# ---------------------------------------------------------------- the option, from every entry down (the recorder idea of test_mesh_options_cpu)
B, V, G, RES = 2, 2, 8, 4
FOUR = dict(normals=False, keep='all', min_faces=0, simplify_cell=0.0)


class _Planes:
    plane_precision = 'fp32'
    neural_rendering_resolution = RES

    def set_plane_precision(self, p):
        self.plane_precision = p

    def cast_planes(self, x):
        return x


class _Decoder:
    triplane_decoder = _Planes()

    def vit_decode_backbone(self, ret_dict, img_size):
        return ret_dict

    def vit_decode_postprocess(self, latent, ret_dict):
        return {'planes_channel_last': torch.zeros(B, 3, 4, 4, 2)}

    def triplane_decode(self, latent, c, return_raw_only=False, **kw):
        r = kw.get('neural_rendering_resolution', RES)
        z = lambda ch: torch.zeros(c.shape[0], ch, r, r)                              # noqa: E731
        return {'image_raw': z(3), 'image_depth': z(1), 'weights_samples': z(1), 'image_mask': z(1)}

    def triplane_decode_grid(self, latent, grid_size):
        return {'sigma': torch.zeros(B, grid_size ** 3, 1)}

    def vae_reparameterization(self, h, sample, eps=None, num_frames=None):
        return {'latent_normalized_2Ddiffusion': torch.zeros(B, 12, 4, 4)}


class _Encoder:
    num_frames = 1

    def forward_frames(self, img):
        return img


def _entries():
    from ln3diff_amd import pipeline as P
    from ln3diff_amd.nsr.script_util import AE
    ae = AE(None, _Decoder(), RES)
    ae.encoder = _Encoder()
    lat = lambda: torch.zeros(B, 12, 4, 4)                                            # noqa: E731
    cams, cond, common = torch.zeros(V, 25), {'crossattn': torch.zeros(1, 1, 1)}, dict(mesh_size=G, resolution=RES)
    t23d, flow, gd = P.T23DPipeline(None, ae), P.FlowMatchingEngine(None, ae, conditioner=lambda img: cond), P.GuidedDiffusionEngine(None, ae, None)
    for eng in (t23d, flow, gd):
        eng.sample = lambda *a, **k: lat()
    return {
        'render_video_given_triplane': lambda e, **kw: P.render_video_given_triplane(lat(), ae, cams, export_mesh=e, **common, **kw),
        'T23DPipeline.eval_cldm': lambda e, **kw: t23d.eval_cldm(cond, cams, num_samples=B, export_mesh=e, **common, **kw),
        'T23DPipeline.render_video_given_triplane': lambda e, **kw: t23d.render_video_given_triplane(lat(), cams, export_mesh=e, **common, **kw),
        'FlowMatchingEngine.eval_cldm': lambda e, **kw: flow.eval_cldm(cond, cams, num_samples=B, export_mesh=e, **common, **kw),
        'FlowMatchingEngine.eval_i23d_and_export': lambda e, **kw: flow.eval_i23d_and_export(None, cams, num_samples=B, export_mesh=e, **common, **kw),
        'FlowMatchingEngine.render_video_given_triplane': lambda e, **kw: flow.render_video_given_triplane(lat(), cams, export_mesh=e, **common, **kw),
        'GuidedDiffusionEngine.eval_cldm': lambda e, **kw: gd.eval_cldm(cond, cams, export_mesh=e, **common, **kw),
        'GuidedDiffusionEngine.eval_ddpm_sample': lambda e, **kw: gd.eval_ddpm_sample(cams, export_mesh=e, **common, **kw),
        'GuidedDiffusionEngine.render_video_given_triplane': lambda e, **kw: gd.render_video_given_triplane(lat(), cams, export_mesh=e, **common, **kw),
        'reconstruct': lambda e, **kw: P.reconstruct(ae, torch.zeros(B, 10, 4, 4), cams, export_mesh=e, **common, **kw),
    }


ENTRIES = ['render_video_given_triplane', 'T23DPipeline.eval_cldm', 'T23DPipeline.render_video_given_triplane', 'FlowMatchingEngine.eval_cldm',
           'FlowMatchingEngine.eval_i23d_and_export', 'FlowMatchingEngine.render_video_given_triplane', 'GuidedDiffusionEngine.eval_cldm',
           'GuidedDiffusionEngine.eval_ddpm_sample', 'GuidedDiffusionEngine.render_video_given_triplane', 'reconstruct']


@pytest.fixture
def recorder(monkeypatch):
    from ln3diff_amd import mesh
    calls = {'plain': [], 'textured': []}
    e3, ef = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)

    def plain(decoder, dec_out, sigma, grid_size, thr=10.0, **kw):
        calls['plain'].append(kw)
        return e3, ef, e3.astype(np.uint8)

    def textured(decoder, dec_out, sigma, grid_size, thr=10.0, **kw):
        calls['textured'].append(kw)
        return e3, ef, e3.astype(np.uint8), np.zeros((0, 3, 2), np.float32), np.zeros((kw['texture_size'],) * 2 + (3,), np.uint8)
    monkeypatch.setattr(mesh, 'mesh_from_grid', plain)
    monkeypatch.setattr(mesh, 'textured_mesh_from_grid', textured)
    return calls


def _strip(kw):
    return {k: v for k, v in kw.items() if k not in ('sample_index', 'path')}


@pytest.mark.parametrize('entry', ENTRIES)
def test_mesh_texture_size_selects_the_function(recorder, entry):
    assert list(_entries()) == ENTRIES
    call = _entries()[entry]
    out = lambda o: o[1] if isinstance(o, tuple) else o                               # noqa: E731
    for given in ({}, dict(mesh_texture_size=0)):
        o = out(call(True, **given))
        assert [_strip(kw) for kw in recorder['plain']] == [FOUR] * B and recorder['textured'] == [] and all(len(m) == 3 for m in o['mesh'])
        assert [kw['sample_index'] for kw in recorder['plain']] == list(range(B))
        del recorder['plain'][:]
    o = out(call(True, mesh_texture_size=64, mesh_keep='largest', mesh_simplify_cell=2.5))
    assert recorder['plain'] == [] and [kw['sample_index'] for kw in recorder['textured']] == list(range(B))
    assert [_strip(kw) for kw in recorder['textured']] == [dict(FOUR, keep='largest', simplify_cell=2.5, texture_size=64)] * B
    assert len(o['mesh']) == B and all(len(m) == 5 and m[4].shape == (64, 64, 3) for m in o['mesh'])
    del recorder['textured'][:]
    o = out(call(False, mesh_texture_size=64))
    assert 'mesh' not in o and recorder == {'plain': [], 'textured': []}
    o = out(call(False, mesh_texture_size='bogus'))                                   # ignored without export_mesh
    assert 'mesh' not in o and recorder == {'plain': [], 'textured': []}


def test_mesh_texture_size_is_not_a_meshpost_field():
    from ln3diff_amd import mesh
    from ln3diff_amd.entry import _MESH_FLAGS, create_argparser, validate
    assert 'texture_size' not in mesh.MeshPost._fields and 'mesh_texture_size' not in _MESH_FLAGS
    with pytest.raises(TypeError, match='mesh_texture_size'):
        mesh.MeshPost.from_kwargs(dict(mesh_texture_size=64))
    parse = lambda s: create_argparser(True).parse_args(s.split())                    # noqa: E731
    assert parse("").mesh_texture_size == 0
    validate(parse("--export_mesh true --mesh_texture_size 256"))
    validate(parse("--export_mesh true --mesh_texture_size 4"))
    validate(parse("--export_mesh true --mesh_texture_size 8192"))
    validate(parse("--mesh_texture_size 0"))
    with pytest.raises(SystemExit, match='export_mesh'):
        validate(parse("--mesh_texture_size 256"))
    for bad in ('3', '9000', '-1'):
        with pytest.raises(SystemExit, match='mesh_texture_size'):
            validate(parse(f"--export_mesh true --mesh_texture_size {bad}"))


def test_bake_wrappers_refuse_bad_buffers_and_host_tensors(monkeypatch):
    from ln3diff_amd import _lib, mesh, ops

    class NoLibrary:
        def __getattr__(self, name):
            def fail(*a):
                pytest.fail(f"{name} was reached")
            return fail
    monkeypatch.setattr(_lib, 'lib', lambda: NoLibrary())
    v = torch.rand(4, 3)
    f = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int64)
    pts, own = torch.zeros(64, 3), torch.zeros(64, dtype=torch.int32)
    rgb, tex = torch.zeros(64, 3), torch.zeros(64, 3, dtype=torch.uint8)
    for check in (True, False):
        with pytest.raises(RuntimeError, match="need device tensors"):
            ops.bake_points(v, f, 8, 1, 8, pts, own, check=check)
    with pytest.raises(RuntimeError, match="need device tensors"):
        ops.bake_pack(rgb, own, 0, tex)
    with pytest.raises(RuntimeError, match="need device tensors"):
        mesh.bake_points(v, f, 8)
    for bad in (lambda: ops.bake_points(v.double(), f, 8, 1, 8, pts, own), lambda: ops.bake_points(v, f.int(), 8, 1, 8, pts, own),
                lambda: ops.bake_points(v, f, 8, 1, 8, pts[:63], own), lambda: ops.bake_points(v, f, 8, 1, 8, pts, own.long()),
                lambda: ops.bake_points(v, f, 8, 1, 8, torch.zeros(64, 6)[:, ::2], own), lambda: ops.bake_points(v, f + 2, 8, 1, 8, pts, own),
                lambda: ops.bake_pack(rgb.double(), own, 0, tex), lambda: ops.bake_pack(rgb, own, 0, tex.int()),
                lambda: ops.bake_pack(rgb[:63], own, 0, tex), lambda: ops.bake_pack(rgb, own.long(), 0, tex),
                lambda: mesh.bake_points(v, f + 2, 8), lambda: mesh.bake_points(v.double(), f, 8), lambda: mesh.bake_points(v, f, 3),
                lambda: mesh.bake_texture(None, None, v, f, 8, fill=256), lambda: mesh.bake_texture(None, None, v, f, 8, fill=-1)):
        with pytest.raises(ValueError):
            bad()
    uv, t = mesh.bake_texture(None, None, v[:0], f[:0], 8, fill=7)                    # an empty mesh: nothing is asked of anybody
    assert uv.shape == (0, 3, 2) and t.shape == (8, 8, 3) and (t == 7).all()
