"""The host side of the texture bake (include/ln3d_meshbake.h), without a GPU:
  - mesh.atlas_layout / atlas_uvs equal the reference of tests/mesh_bake_refs.py, at the edges of the capacity too;
  - the property the layout exists for, for every cell size c = 4 ... 13: a bilinear look-up at the corners, the edge midpoints and random
    points of a face's UV triangle has its non-zero taps in texels that face owns (exact arithmetic: dyadic weights, half-integer corners);
  - an affine field baked unquantised at the reference's points comes back from the bilinear look-up to 1e-6;
  - write_png decodes (by an inverse written here, and by Pillow where it imports) to the flipped array; write_obj_textured parses back;
  - both entry points return LN3D_ERR_BAD_ARG for each null buffer, each zero, negative or oversize count and each bad (T, n, c, nf)
    combination, all on fake addresses that are never dereferenced (validation precedes every launch).
(mesh_texture_size from every public entry of pipeline down, and the launcher flag: tests/test_mesh_options_cpu.py.)"""
import struct
import zlib

import numpy as np
import pytest
import torch

import mesh_bake_refs as R
from abi_args import BAD_ARG, refuses_null_buffers_and_bad_counts, with_args as _with


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


# ---------------------------------------------------------------- entry points on fake addresses
P = 0x10000                                  # a fake device address
# name -> (a valid argument list on fake addresses, indices of its buffers, indices of its int64 counts)
VALID = {
    'ln3d_bake_points': ([P, 9, P, 7, 11, 2, 5, P, P, None], (0, 2, 7, 8), (1, 3)),             # verts nv faces nf T n c points owner stream
    'ln3d_bake_pack': ([P, P, 121, 0, P, None], (0, 1, 4), (2,)),                               # rgb owner P fill tex stream
}


def test_every_entry_point_validates_before_it_launches(hip_lib):
    from ln3diff_amd import _lib
    assert set(VALID) <= set(_lib.PROTOTYPES)
    for name, (args, buffers, counts) in VALID.items():
        assert len(args) == len(_lib.PROTOTYPES[name][1])
        refuses_null_buffers_and_bad_counts(getattr(hip_lib, name), name, args, buffers, counts)
    points, pargs = hip_lib.ln3d_bake_points, VALID['ln3d_bake_points'][0]
    # (T, n, c, nf): T outside [4, 8192]; n < 1; c < 4; n * c > T; nf > 2 n^2 - each with the other values as sane as they can be
    for T, n, c, nf in ((3, 1, 3, 1), (3, 1, 4, 1), (0, 1, 4, 1), (-8, 1, 4, 1), (8193, 1, 4, 1), (16384, 2048, 4, 2), (1 << 30, 1, 4, 1),
                        (11, 0, 5, 1), (11, -2, 5, 1), (11, 2, 3, 7), (11, 2, 0, 7), (11, 2, -5, 7), (11, 2, 6, 7), (11, 3, 4, 7),
                        (8192, 1 << 16, 1 << 16, 7),                                     # n * c overflows an int
                        (11, 2, 5, 9), (4, 1, 4, 3), (64, 1, 64, 3), (8192, 2048, 4, 2 * 2048 * 2048 + 1)):
        assert points(*_with(pargs, i3=nf, i4=T, i5=n, i6=c)) == BAD_ARG, (T, n, c, nf)
    pack, kargs = hip_lib.ln3d_bake_pack, VALID['ln3d_bake_pack'][0]
    for fill in (-1, 256, 1 << 20):
        assert pack(*_with(kargs, i3=fill)) == BAD_ARG, fill
    assert pack(*_with(kargs, i2=8192 * 8192 + 1)) == BAD_ARG
    assert b'bad argument' in hip_lib.ln3d_strerror(BAD_ARG)
