"""The binary mesh export of include/ln3d_meshpack.h without a GPU:
  - the numpy restatement (tests/mesh_pack_refs.py) against the rules it restates, and hand-made meshes through mesh.write_ply /
    mesh.write_glb - with the six packers replaced by the restatement, so that everything the HOST does (headers, JSON, chunks, padding,
    the order of the writes) is the product's - and back through the two readers of that file;
  - every structural rule of a GLB: container lengths, chunk padding, one aligned bufferView per section, counts, min / max equal to the data,
    and the exact JSON of one small asset;
  - seeded faults (fma contraction, rounded colours, big-endian fields, a stride off by one, non-zero pad bytes) that the byte equalities of
    tests/test_mesh_pack_gpu.py must catch, on the inputs those tests use;
  - every new entry point validates its arguments on fake addresses before it launches.  (That a null `normal` is ACCEPTED cannot be shown
    here: an accepted call launches.  The GPU tests run every packer with and without normals.)
  - mesh_format selects the writer of the two mesh functions and nothing else.
(mesh_format from every public entry of pipeline down, and the launcher flag and its refusals: tests/test_mesh_options_cpu.py.)"""
import json
import struct

import numpy as np
import pytest
import torch

import mesh_pack_refs as R
from abi_args import BAD_ARG, BIG, with_args as _with
from test_mesh_bake_cpu import decode_png

P, Q = 0x10000, 0x4000000                    # two fake device addresses, 64 MiB apart


# ---------------------------------------------------------------- the restatement's own rules
def test_the_rules_are_the_ones_the_product_states():
    from ln3diff_amd import mesh
    import mesh_bake_refs
    assert np.array_equal(R.bits(R.ROT_X_M90), R.bits(mesh.rotation_matrix_x(-90)))
    c = R.special_colours()
    assert len(c) == 773 and np.array_equal(R.colour(c), mesh_bake_refs.quantise(c))                        # the rule of ln3d_bake_pack
    ok = ~np.isnan(c)
    assert np.array_equal(R.colour(c[ok]), (torch.from_numpy(c[ok]).clamp(0, 1) * 255).to(torch.uint8).numpy())       # the line that colours the vertices
    assert R.colour(np.float32(np.nan)) == 0 and R.colour(np.float32(-np.inf)) == 0 and R.colour(np.float32(np.inf)) == 255
    assert R.narrow([[0, 1, (1 << 31) - 1], [1 << 32, (1 << 32) + 5, -1]]).tolist() == [[0, 1, 0x7fffffff], [0, 5, 0xffffffff]]
    x = np.array([-np.inf, -1e30, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 1e30, np.inf], np.float32)
    assert (np.diff(R.key(x).astype(np.int64)) > 0).all()                                                   # ascending, -0 below +0
    b = R.bounds(np.array([[0.0, 2, -3], [-0.0, 5, -3], [1, -7, -4]], np.float32))
    assert R.bits(b).tolist() == R.bits(np.array([-0.0, -7, -4, 1, 5, -3], np.float32)).tolist()
    p = np.array([[1, 2, 3]], np.float32)
    assert np.array_equal(R.rotate(R.ROT_X_M90, p), [[1, 3, -2]])                                           # (x, y, z) -> (x, z, -y)


def test_fma_shows_with_a_general_matrix_only():
    """with rotation_matrix_x(-90) the stated order, the fused variant and numpy's matmul give the same bits on 200 000 points of the box;
    with a random matrix the fused variant differs in about 39 % of the values - so the GPU test rotates by a random matrix"""
    rng = np.random.default_rng(5)
    p = rng.uniform(-0.45, 0.45, (200000, 3)).astype(np.float32)
    want = R.rotate(R.ROT_X_M90, p)
    assert np.array_equal(R.bits(want), R.bits(R.rotate(R.ROT_X_M90, p, fma=True)))
    assert np.array_equal(R.bits(want), R.bits((R.ROT_X_M90 @ p.T).T.astype(np.float32)))                   # what mesh_from_grid returns
    M = rng.uniform(-1, 1, (3, 3)).astype(np.float32)
    differ = int((R.bits(R.rotate(M, p)) != R.bits(R.rotate(M, p, fma=True))).sum())
    print('[pack] fma against the stated order, random matrix: %d of %d values differ' % (differ, p.size))
    assert differ > p.size // 10
    exact = (M.astype(np.float64) @ p.astype(np.float64).T).T
    bound = 3 * 2.0 ** -24 * (np.abs(M.astype(np.float64))[None] * np.abs(p.astype(np.float64))[:, None, :]).sum(-1) + 1e-45
    assert (np.abs(R.rotate(M, p) - exact) <= bound).all() and (np.abs(R.rotate(M, p, fma=True) - exact) <= bound).all()


@pytest.mark.parametrize('variant', R.VARIANTS)
def test_every_seeded_fault_changes_bytes(variant):
    """on the inputs of the GPU tests, for the vertex records with and without normals, and for the face records where the fault exists there"""
    hit_v, hit_f, hit_g = [], [], []
    for n in R.SIZES:
        c = R.case(n)
        for normal in (None, c['normal']):
            good = R.ply_body(c['xyz'], normal, c['rgb'], c['faces'], c['R'])
            bad = R.ply_body(c['xyz'], normal, c['rgb'], c['faces'], c['R'], variant=variant)
            assert len(good[0]) == len(bad[0]) and len(good[1]) == len(bad[1])
            hit_v.append(good[0] != bad[0])
            hit_f.append(good[1] != bad[1])
        if variant in ('fma', 'round'):
            good, bad = R.gltf_sections(c['xyz'], c['normal'], c['rgb'], c['faces'], R=c['R']), R.gltf_sections(c['xyz'], c['normal'], c['rgb'], c['faces'], R=c['R'], variant=variant)
            hit_g.append(any(good[k].tobytes() != bad[k].tobytes() for k in good))
    assert any(hit_v), variant
    if variant in ('big_endian', 'stride', 'pad'):
        assert any(hit_f), variant
    if variant == 'pad':                      # wherever the length is no multiple of 4, and nowhere else
        assert hit_v == [(n * s) % 4 != 0 for n in R.SIZES for s in (15, 27)] and hit_f[::2] == [(n * 13) % 4 != 0 for n in R.SIZES]
    if variant == 'stride':
        assert all(h for h, n in zip(hit_v[::2], R.SIZES) if n > 1) and all(h for h, n in zip(hit_f[::2], R.SIZES) if n > 1)
    if hit_g:
        assert hit_g[-1], variant              # n = 1000 holds every special colour and enough rows for a fused sum to differ


# ---------------------------------------------------------------- the writers, with the packers restated
@pytest.fixture
def numpy_packers(monkeypatch):
    """ops.pack_* and ops.position_bounds on HOST tensors, by the restatement: what write_ply and write_glb do around them is the product's"""
    from ln3diff_amd import ops
    calls = []
    arr = lambda t: None if t is None else t.numpy()                                     # noqa: E731
    put = lambda out, a: out.copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).view(out.dtype).reshape(out.shape))   # noqa: E731
    none = np.zeros((0, 3), np.int64)

    def ply_vertices(xyz, normal, rgb, rot9, out):
        calls.append('pack_ply_vertices')
        put(out, np.frombuffer(R.ply_body(arr(xyz), arr(normal), arr(rgb), none, arr(rot9).reshape(3, 3))[0], np.uint8))

    def ply_faces(faces, out):
        calls.append('pack_ply_faces')
        put(out, np.frombuffer(R.ply_body(np.zeros((0, 3), np.float32), None, np.zeros((0, 3), np.float32), arr(faces))[1], np.uint8))

    def gltf_vertices(xyz, normal, rgb, rot9, pos_out, nrm_out, rgba_out):
        calls.append('pack_gltf_vertices')
        s = R.gltf_sections(arr(xyz), arr(normal), arr(rgb), none, R=arr(rot9).reshape(3, 3))
        put(pos_out, s['POSITION']), put(rgba_out, s['COLOR_0'])
        if normal is not None:
            put(nrm_out, s['NORMAL'])

    def gltf_indices(faces, idx_out):
        calls.append('pack_gltf_indices')
        put(idx_out, R.narrow(arr(faces)).reshape(-1))

    def gltf_corners(xyz, normal, faces, uv, rot9, pos_out, nrm_out, uv_out, check=True):
        calls.append('pack_gltf_corners')
        s = R.gltf_sections(arr(xyz), arr(normal), None, arr(faces), uv=arr(uv), R=arr(rot9).reshape(3, 3))
        put(pos_out, s['POSITION']), put(uv_out, s['TEXCOORD_0'])
        if normal is not None:
            put(nrm_out, s['NORMAL'])

    def position_bounds(pos, bounds6):
        calls.append('position_bounds')
        put(bounds6, R.bounds(arr(pos)))
    for name, fn in dict(pack_ply_vertices=ply_vertices, pack_ply_faces=ply_faces, pack_gltf_vertices=gltf_vertices, pack_gltf_indices=gltf_indices,
                         pack_gltf_corners=gltf_corners, position_bounds=position_bounds).items():
        monkeypatch.setattr(ops, name, fn)
    return calls


def _tensors(xyz, normal, rgb, faces, normals):
    t = torch.from_numpy
    return t(xyz), t(faces), t(rgb), (t(normal) if normals else None)


@pytest.mark.parametrize('normals', [False, True])
@pytest.mark.parametrize('name', list(R.hand_made()))
def test_ply_round_trip(tmp_path, numpy_packers, name, normals):
    from ln3diff_amd import mesh
    xyz, normal, rgb, faces = R.hand_made()[name]
    mesh.write_ply(tmp_path / 'm.ply', *_tensors(xyz, normal, rgb, faces, normals), check=False)
    data = open(tmp_path / 'm.ply', 'rb').read()
    assert data == R.ply_file(xyz, normal if normals else None, rgb, faces)                  # the exact bytes of the header's layout
    assert numpy_packers == ['pack_ply_vertices', 'pack_ply_faces']
    p = R.parse_ply(data)
    nv, nf = len(xyz), len(faces)
    assert (p['nv'], p['nf'], p['comments']) == (nv, nf, ['ln3diff_amd'])
    assert p['names'] == ['x', 'y', 'z'] + (['nx', 'ny', 'nz'] if normals else []) + ['red', 'green', 'blue']
    assert np.array_equal(R.bits(p['xyz']), R.bits(R.rotate(R.ROT_X_M90, xyz))) and np.array_equal(p['rgb'], R.colour(rgb))
    assert np.array_equal(p['faces'], faces) and p['faces'].dtype == np.dtype('<i4')
    assert (p['normal'] is None) if not normals else np.array_equal(R.bits(p['normal']), R.bits(R.rotate(R.ROT_X_M90, normal)))
    assert len(data) == len(R.ply_header(nv, nf, normals)) + nv * (27 if normals else 15) + nf * 13


def test_ply_empty_and_refusals(tmp_path, numpy_packers):
    from ln3diff_amd import mesh
    e3, ef = torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64)
    for normals in (False, True):
        mesh.write_ply(tmp_path / 'e.ply', e3, ef, e3, e3 if normals else None, check=False)
        data = open(tmp_path / 'e.ply', 'rb').read()
        assert data == R.ply_header(0, 0, normals) and R.parse_ply(data)['nv'] == 0 and b'element vertex 0\n' in data and b'element face 0\n' in data
    assert numpy_packers == []                                                             # nothing to pack: nothing is launched
    xyz, faces, rgb, normal = _tensors(*R.hand_made()['tetra'], True)
    for bad in (lambda: mesh.write_ply(tmp_path / 'b.ply', xyz.double(), faces, rgb), lambda: mesh.write_ply(tmp_path / 'b.ply', xyz, faces.int(), rgb, check=False),
                lambda: mesh.write_ply(tmp_path / 'b.ply', xyz, faces + 1, rgb), lambda: mesh.write_ply(tmp_path / 'b.ply', xyz, faces - 1, rgb),
                lambda: mesh.write_ply(tmp_path / 'b.ply', xyz, faces, rgb[:3], check=False), lambda: mesh.write_ply(tmp_path / 'b.ply', xyz, faces, rgb, normal[:3], check=False),
                lambda: mesh.write_glb(tmp_path / 'b.glb', xyz, faces + 1, rgb), lambda: mesh.write_glb(tmp_path / 'b.glb', xyz, faces, rgb, uv=np.zeros((4, 3, 2), np.float32), check=False),
                lambda: mesh.write_glb(tmp_path / 'b.glb', xyz, faces, rgb, tex=np.zeros((4, 4, 3), np.uint8), check=False),
                lambda: mesh.write_glb(tmp_path / 'b.glb', xyz, faces, rgb, uv=np.zeros((3, 3, 2), np.float32), tex=np.zeros((4, 4, 3), np.uint8), check=False)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError, match="need device tensors"):                          # in range, but on the host: refused like every other
        mesh.write_ply(tmp_path / 'b.ply', xyz, faces, rgb)
    inf = xyz.clone()
    inf[2, 1] = float('inf')
    with pytest.raises(ValueError, match='not finite'):
        mesh.write_glb(tmp_path / 'b.glb', inf, faces, rgb, check=False)
    assert not (tmp_path / 'b.ply').exists() and not (tmp_path / 'b.glb').exists()          # refused before the file is opened


def _check_glb_structure(data, nsections):
    """what mesh.write_glb promises of every GLB, from the bytes alone -> parse_glb's dict"""
    g = R.parse_glb(data)
    doc = g['json']
    assert len(data) % 4 == 0 and struct.unpack_from('<I', data, 8)[0] == len(data)
    jlen = struct.unpack_from('<I', data, 12)[0]
    assert jlen % 4 == 0 and jlen == len(g['text']) and len(g['text']) - len(g['text'].rstrip(b' ')) < 4           # padded with spaces, no more than needed
    assert len(doc['bufferViews']) == nsections and len(doc['materials']) == 1
    mat = doc['materials'][0]
    assert mat['doubleSided'] is True and mat['pbrMetallicRoughness']['metallicFactor'] == 0 and mat['pbrMetallicRoughness']['roughnessFactor'] == 1
    offset = 0
    for view in doc['bufferViews']:                                                        # every section its own view, packed back to back
        assert view['byteOffset'] == offset and offset % 4 == 0
        offset += (view['byteLength'] + 3) // 4 * 4
    assert offset == doc['buffers'][0]['byteLength'] == len(g['bin']) == struct.unpack_from('<I', data, 20 + jlen)[0]
    pos = doc['accessors'][doc['meshes'][0]['primitives'][0]['attributes']['POSITION']]
    a = g['arrays']['POSITION']
    assert pos['min'] == [float(x) for x in a.min(0)] and pos['max'] == [float(x) for x in a.max(0)]           # exactly the data's
    for k in ('min', 'max'):                                                               # the repr of the float32 widened to double
        assert ('"%s":[%s]' % (k, ','.join(repr(float(np.float32(x))) for x in getattr(a, k)(0)))).encode() in g['text']
    return g


@pytest.mark.parametrize('normals', [False, True])
@pytest.mark.parametrize('name', list(R.hand_made()))
def test_glb_round_trip_untextured(tmp_path, numpy_packers, name, normals):
    from ln3diff_amd import mesh
    xyz, normal, rgb, faces = R.hand_made()[name]
    mesh.write_glb(tmp_path / 'm.glb', *_tensors(xyz, normal, rgb, faces, normals), check=False)
    assert numpy_packers == ['pack_gltf_vertices', 'pack_gltf_indices', 'position_bounds']
    data = open(tmp_path / 'm.glb', 'rb').read()
    g = _check_glb_structure(data, 4 if normals else 3)
    want = R.gltf_sections(xyz, normal if normals else None, rgb, faces)
    assert list(g['arrays']) == list(want) and g['image'] is None
    for k in want:
        assert g['arrays'][k].dtype == want[k].dtype and g['arrays'][k].tobytes() == want[k].tobytes(), k
    doc = g['json']
    prim = doc['meshes'][0]['primitives'][0]
    assert [doc['accessors'][i]['count'] for i in prim['attributes'].values()] == [len(xyz)] * (3 if normals else 2)
    assert doc['accessors'][prim['indices']]['count'] == 3 * len(faces)
    col = doc['accessors'][prim['attributes']['COLOR_0']]
    assert col == {'bufferView': prim['attributes']['COLOR_0'], 'componentType': 5121, 'normalized': True, 'count': len(xyz), 'type': 'VEC4'}
    assert (g['arrays']['COLOR_0'][:, 3] == 255).all() and 'textures' not in doc and 'images' not in doc
    mesh.write_glb(tmp_path / 'again.glb', *_tensors(xyz, normal, rgb, faces, normals), check=False)
    assert open(tmp_path / 'again.glb', 'rb').read() == data                                # two runs, the same bytes


def test_glb_exact_json_of_one_face(tmp_path, numpy_packers):
    from ln3diff_amd import mesh
    xyz, normal, rgb, faces = R.hand_made()['one_face']
    mesh.write_glb(tmp_path / 'm.glb', *_tensors(xyz, normal, rgb, faces, True), check=False)
    g = R.parse_glb(open(tmp_path / 'm.glb', 'rb').read())
    lo, hi = [float(x) for x in g['arrays']['POSITION'].min(0)], [float(x) for x in g['arrays']['POSITION'].max(0)]
    want = ('{"asset":{"version":"2.0","generator":"ln3diff_amd"},"scene":0,"scenes":[{"nodes":[0]}],"nodes":[{"mesh":0}],'
            '"meshes":[{"primitives":[{"attributes":{"POSITION":0,"NORMAL":1,"COLOR_0":2},"indices":3,"material":0,"mode":4}]}],'
            '"materials":[{"pbrMetallicRoughness":{"metallicFactor":0.0,"roughnessFactor":1.0},"doubleSided":true}],'
            '"accessors":[{"bufferView":0,"componentType":5126,"count":3,"type":"VEC3","min":%s,"max":%s},'
            '{"bufferView":1,"componentType":5126,"count":3,"type":"VEC3"},'
            '{"bufferView":2,"componentType":5121,"normalized":true,"count":3,"type":"VEC4"},'
            '{"bufferView":3,"componentType":5125,"count":3,"type":"SCALAR"}],'
            '"bufferViews":[{"buffer":0,"byteOffset":0,"byteLength":36,"target":34962},{"buffer":0,"byteOffset":36,"byteLength":36,"target":34962},'
            '{"buffer":0,"byteOffset":72,"byteLength":12,"target":34962},{"buffer":0,"byteOffset":84,"byteLength":12,"target":34963}],'
            '"buffers":[{"byteLength":96}]}') % (json.dumps(lo, separators=(',', ':')), json.dumps(hi, separators=(',', ':')))
    assert g['text'].rstrip(b' ').decode() == want


@pytest.mark.parametrize('normals', [False, True])
@pytest.mark.parametrize('name', ['tetra', 'five_faces', 'sixty_five'])
def test_glb_round_trip_textured(tmp_path, numpy_packers, name, normals):
    from ln3diff_amd import mesh
    xyz, normal, rgb, faces = R.hand_made()[name]
    nf = len(faces)
    T = 4 * mesh.atlas_layout(nf, 8192)[0] + 1                                              # odd: the PNG's length is then no multiple of 4 for some
    uv = mesh.atlas_uvs(nf, T)
    tex = np.random.default_rng(nf).integers(0, 256, (T, T, 3), dtype=np.uint8)
    mesh.write_glb(tmp_path / 'm.glb', *_tensors(xyz, normal, rgb, faces, normals), uv=uv, tex=tex, check=False)
    assert numpy_packers == ['pack_gltf_corners', 'position_bounds']
    assert sorted(p.name for p in tmp_path.iterdir()) == ['m.glb']                          # no .mtl or .png siblings
    data = open(tmp_path / 'm.glb', 'rb').read()
    g = _check_glb_structure(data, 4 if normals else 3)
    want = R.gltf_sections(xyz, normal if normals else None, rgb, faces, uv=uv)
    assert list(g['arrays']) == list(want) == ['POSITION'] + (['NORMAL'] if normals else []) + ['TEXCOORD_0']
    for k in want:
        assert g['arrays'][k].shape[0] == 3 * nf and g['arrays'][k].tobytes() == want[k].tobytes(), k
    corner = faces.reshape(-1)
    assert np.array_equal(R.bits(g['arrays']['POSITION']), R.bits(R.rotate(R.ROT_X_M90, xyz)[corner]))            # corner 3 i + j holds vertex faces[i][j]
    flat = uv.reshape(-1, 2)
    assert np.array_equal(g['arrays']['TEXCOORD_0'][:, 0], flat[:, 0]) and np.array_equal(g['arrays']['TEXCOORD_0'][:, 1], np.float32(1) - flat[:, 1])
    doc = g['json']
    prim = doc['meshes'][0]['primitives'][0]
    assert 'indices' not in prim and 'COLOR_0' not in prim['attributes']
    assert doc['materials'][0]['pbrMetallicRoughness']['baseColorTexture'] == {'index': 0} and doc['textures'][0]['source'] == 0
    assert g['image'] == mesh.png_bytes(tex)
    mesh.write_png(tmp_path / 't.png', tex)
    assert open(tmp_path / 't.png', 'rb').read() == g['image'] and np.array_equal(decode_png(tmp_path / 't.png'), tex[::-1])


def test_glb_empty_and_too_long(tmp_path, numpy_packers, monkeypatch):
    from ln3diff_amd import mesh
    e3, ef = torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64)
    for kw in ({}, dict(normal=e3), dict(uv=np.zeros((0, 3, 2), np.float32), tex=np.zeros((4, 4, 3), np.uint8))):
        mesh.write_glb(tmp_path / 'e.glb', e3, ef, e3, check=False, **kw)
        g = R.parse_glb(open(tmp_path / 'e.glb', 'rb').read())
        assert g['json'] == {'asset': {'version': '2.0', 'generator': 'ln3diff_amd'}, 'scene': 0, 'scenes': [{}]} and g['bin'] is None
    assert numpy_packers == []
    xyz, normal, rgb, faces = R.hand_made()['tetra']
    mesh.write_glb(tmp_path / 'ok.glb', *_tensors(xyz, normal, rgb, faces, False), check=False)
    size = (tmp_path / 'ok.glb').stat().st_size
    monkeypatch.setattr(mesh, 'GLB_MAX_BYTES', size)                                        # the limit, scaled down: a file of exactly that many bytes
    with pytest.raises(ValueError, match='2\\^32'):
        mesh.write_glb(tmp_path / 'long.glb', *_tensors(xyz, normal, rgb, faces, False), check=False)
    assert not (tmp_path / 'long.glb').exists()
    monkeypatch.setattr(mesh, 'GLB_MAX_BYTES', size + 1)
    mesh.write_glb(tmp_path / 'fits.glb', *_tensors(xyz, normal, rgb, faces, False), check=False)
    assert mesh.MESH_FORMATS == ('obj', 'ply', 'glb')


def test_readers_refuse_broken_files():
    xyz, normal, rgb, faces = R.hand_made()['tetra']
    data = R.ply_file(xyz, None, rgb, faces)
    for bad in (data[:-1], data + b'\0', data.replace(b'binary_little_endian', b'binary_big_endian'), data.replace(b'property float z\n', b'')):
        with pytest.raises((AssertionError, ValueError)):
            R.parse_ply(bad)
    four = bytearray(data)
    four[len(R.ply_header(4, 4, False)) + 4 * 15] = 4                                      # a face that lists four indices
    with pytest.raises(AssertionError):
        R.parse_ply(bytes(four))


# ---------------------------------------------------------------- the ABI
# name -> (a valid argument list on fake addresses, its required buffers, its (input, output) pair that is optional together, its counts,
#          its outputs that must be 4-byte aligned)
VALID = {
    'ln3d_pack_ply_vertices': ([P, P + 4096, P + 8192, P + 12288, 5, Q, None], (0, 2, 3, 5), None, (4,), (5,)),
    'ln3d_pack_ply_faces': ([P, 7, Q, None], (0, 2), None, (1,), (2,)),
    'ln3d_pack_gltf_vertices': ([P, P + 4096, P + 8192, P + 12288, 5, Q, Q + 4096, Q + 8192, None], (0, 2, 3, 5, 7), (1, 6), (4,), (5, 6, 7)),
    'ln3d_pack_gltf_indices': ([P, 7, Q, None], (0, 2), None, (1,), (2,)),
    'ln3d_pack_gltf_corners': ([P, P + 4096, P + 8192, P + 12288, P + 16384, 5, 7, Q, Q + 4096, Q + 8192, None], (0, 2, 3, 4, 7, 9), (1, 8), (5, 6), (7, 8, 9)),
    'ln3d_position_bounds': ([P, 5, Q, None], (0, 2), None, (1,), (2,)),
}


def test_every_pack_entry_point_validates_before_it_launches(hip_lib):
    from ln3diff_amd import _lib
    assert set(VALID) <= set(_lib.PROTOTYPES)
    for name, (args, buffers, pair, counts, aligned) in VALID.items():
        fn = getattr(hip_lib, name)
        assert len(args) == len(_lib.PROTOTYPES[name][1])
        for i in buffers:
            assert fn(*_with(args, **{'i%d' % i: None})) == BAD_ARG, (name, 'null buffer', i)
        if pair is not None:                  # both or neither: one without the other is refused
            for i in pair:
                assert fn(*_with(args, **{'i%d' % i: None})) == BAD_ARG, (name, 'half of the optional pair', i)
        for i in counts:
            for bad in (0, -1, BIG, 1 << 40):
                assert fn(*_with(args, **{'i%d' % i: bad})) == BAD_ARG, (name, 'count', i, bad)
                if pair is not None:          # ... and a null optional pointer does not hide a bad count
                    assert fn(*_with(args, **{'i%d' % i: bad, 'i%d' % pair[0]: None, 'i%d' % pair[1]: None})) == BAD_ARG, (name, 'count', i, bad)
        for i in aligned:
            for shift in (1, 2, 3):
                assert fn(*_with(args, **{'i%d' % i: args[i] + shift})) == BAD_ARG, (name, 'misaligned', i, shift)


def test_pack_wrappers_refuse_bad_buffers_and_host_tensors(monkeypatch):
    from ln3diff_amd import _lib, ops

    class NoLibrary:
        def __getattr__(self, name):
            def fail(*a):
                pytest.fail(f"{name} was reached")
            return fail
    monkeypatch.setattr(_lib, 'lib', lambda: NoLibrary())
    nv, nf = 5, 3
    xyz, rgb, rot = torch.zeros(nv, 3), torch.zeros(nv, 3), torch.zeros(9)
    faces = torch.tensor([[0, 1, 2], [2, 3, 4], [4, 0, 1]], dtype=torch.int64)
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8)                                       # noqa: E731
    pos, nrm, rgba, idx = torch.zeros(nv, 3), torch.zeros(nv, 3), torch.zeros(nv, 4, dtype=torch.uint8), torch.zeros(3 * nf, dtype=torch.int32)
    cpos, cnrm, uv, cuv, b6 = torch.zeros(3 * nf, 3), torch.zeros(3 * nf, 3), torch.zeros(nf, 3, 2), torch.zeros(3 * nf, 2), torch.zeros(6)
    for call in (lambda: ops.pack_ply_vertices(xyz, None, rgb, rot, u8(76)), lambda: ops.pack_ply_vertices(xyz, xyz, rgb, rot, u8(136)),
                 lambda: ops.pack_ply_faces(faces, u8(40)), lambda: ops.pack_gltf_vertices(xyz, None, rgb, rot, pos, None, rgba),
                 lambda: ops.pack_gltf_vertices(xyz, xyz, rgb, rot, pos, nrm, rgba), lambda: ops.pack_gltf_indices(faces, idx),
                 lambda: ops.pack_gltf_corners(xyz, None, faces, uv, rot, cpos, None, cuv, check=False),
                 lambda: ops.pack_gltf_corners(xyz, xyz, faces, uv, rot, cpos, cnrm, cuv), lambda: ops.position_bounds(pos, b6)):
        with pytest.raises(RuntimeError, match="need device tensors"):
            call()
    for bad in (lambda: ops.pack_ply_vertices(xyz, None, rgb, rot, u8(75)), lambda: ops.pack_ply_vertices(xyz, None, rgb, rot, u8(80)),
                lambda: ops.pack_ply_vertices(xyz, xyz, rgb, rot, u8(76)), lambda: ops.pack_ply_vertices(xyz.double(), None, rgb, rot, u8(76)),
                lambda: ops.pack_ply_vertices(xyz, xyz[:4], rgb, rot, u8(136)), lambda: ops.pack_ply_vertices(xyz, None, rgb[:4], rot, u8(76)),
                lambda: ops.pack_ply_vertices(xyz, None, rgb, rot[:8], u8(76)), lambda: ops.pack_ply_vertices(xyz, None, rgb, rot, u8(152)[::2]),
                lambda: ops.pack_ply_vertices(xyz, None, rgb, rot, torch.zeros(19, dtype=torch.int32)),
                lambda: ops.pack_ply_faces(faces.int(), u8(40)), lambda: ops.pack_ply_faces(faces, u8(39)), lambda: ops.pack_ply_faces(faces.reshape(-1), u8(40)),
                lambda: ops.pack_gltf_vertices(xyz, xyz, rgb, rot, pos, None, rgba), lambda: ops.pack_gltf_vertices(xyz, None, rgb, rot, pos, nrm, rgba),
                lambda: ops.pack_gltf_vertices(xyz, None, rgb, rot, pos[:4], None, rgba), lambda: ops.pack_gltf_vertices(xyz, None, rgb, rot, pos, None, rgba[:, :3]),
                lambda: ops.pack_gltf_vertices(xyz, None, rgb, rot, pos, None, rgba.int()), lambda: ops.pack_gltf_indices(faces, idx.long()),
                lambda: ops.pack_gltf_indices(faces, idx[:8]), lambda: ops.pack_gltf_corners(xyz, None, faces + 3, uv, rot, cpos, None, cuv),
                lambda: ops.pack_gltf_corners(xyz, None, faces - 1, uv, rot, cpos, None, cuv), lambda: ops.pack_gltf_corners(xyz, None, faces, uv[:2], rot, cpos, None, cuv, check=False),
                lambda: ops.pack_gltf_corners(xyz, None, faces, uv, rot, cpos[:8], None, cuv, check=False),
                lambda: ops.pack_gltf_corners(xyz, None, faces, uv, rot, cpos, None, cuv[:8], check=False),
                lambda: ops.pack_gltf_corners(xyz, xyz, faces, uv, rot, cpos, None, cuv, check=False), lambda: ops.position_bounds(pos, b6[:5]),
                lambda: ops.position_bounds(pos.double(), b6), lambda: ops.position_bounds(pos.reshape(-1), b6)):
        with pytest.raises(ValueError):
            bad()


class _Field:
    def forward_points(self, pcl, pts, with_grad=False):
        return {'rgb': torch.full_like(pts, 0.5), 'normal': torch.zeros_like(pts)}

    def triplane_decode_grid(self, latent, grid_size):
        return {'sigma': torch.zeros(1, grid_size ** 3, 1)}


def test_the_format_selects_the_writer_and_nothing_else(monkeypatch, tmp_path):
    from ln3diff_amd import mesh
    G = 8
    raw, faces = torch.tensor([[1.0, 2.0, 3.0], [4.0, 2.0, 3.0], [1.0, 5.0, 3.0]]), torch.tensor([[0, 1, 2]])
    log = []
    monkeypatch.setattr(mesh, 'extract_isosurface', lambda sigma, thr, method, *post, **kw: (raw, faces))
    monkeypatch.setattr(mesh, 'bake_texture', lambda dec, pcl, vtx, f, size: (mesh.atlas_uvs(1, size), np.zeros((size, size, 3), np.uint8)))
    for name in ('write_obj', 'write_obj_textured', 'write_png', 'write_ply', 'write_glb'):
        monkeypatch.setattr(mesh, name, lambda path, *a, _n=name, **kw: log.append((_n, str(path), a, kw)))
    d = {'planes_channel_last': torch.zeros(1, 3, 4, 4, 2)}
    sigma = torch.zeros(G ** 3)
    box = (raw / (G - 1) * 2 - 1) * 0.45
    base = mesh.mesh_from_grid(_Field(), d, sigma, G, path='a.xyz')
    assert [e[:2] for e in log] == [('write_obj', 'a.xyz')]
    for fmt in ('obj', 'ply', 'glb'):
        for normals in (False, True):
            del log[:]
            got = mesh.mesh_from_grid(_Field(), d, sigma, G, path='a.xyz', mesh_format=fmt, normals=normals)
            assert len(got) == (4 if normals else 3) and all(np.array_equal(a, b) for a, b in zip(base, got))       # the tuple does not depend on the format
            (name, path, a, kw), = log
            assert (name, path) == ('write_' + fmt, 'a.xyz')                                 # the extension is not interpreted
            if fmt != 'obj':                                                               # the device tensors, not the numpy copies
                assert torch.equal(a[0], box) and a[1] is faces and torch.equal(a[2], torch.full_like(box, 0.5)) and kw == dict(check=False)
                assert (a[3] is None) if not normals else torch.equal(a[3], torch.zeros_like(box))
    del log[:]
    assert len(mesh.mesh_from_grid(_Field(), d, sigma, G, mesh_format='glb')) == 3 and log == []            # no path: nothing is written
    tex = mesh.textured_mesh_from_grid(_Field(), d, sigma, G, texture_size=8, path='t.obj')
    assert [e[0] for e in log] == ['write_obj_textured', 'write_png']
    del log[:]
    got = mesh.textured_mesh_from_grid(_Field(), d, sigma, G, texture_size=8, path='t.obj', mesh_format='glb')
    (name, path, a, kw), = log
    assert (name, path) == ('write_glb', 't.obj') and len(got) == 5 and all(np.array_equal(x, y) for x, y in zip(tex, got))
    assert torch.equal(a[0], box) and a[3] is None and np.array_equal(a[4], got[3]) and np.array_equal(a[5], got[4])
    del log[:]
    for bad in (lambda: mesh.textured_mesh_from_grid(_Field(), d, sigma, G, texture_size=8, path='t.ply', mesh_format='ply'),
                lambda: mesh.mesh_from_grid(_Field(), d, sigma, G, mesh_format='stl'), lambda: mesh.mesh_from_grid(_Field(), d, sigma, G, mesh_format=None),
                lambda: mesh.textured_mesh_from_grid(_Field(), d, sigma, G, texture_size=8, mesh_format='PLY'),
                lambda: mesh.export_mesh(_Field(), d, 'e.obj', grid_size=G, mesh_format='gltf')):
        with pytest.raises(ValueError, match='format'):
            bad()
    assert log == []
    seen = []
    monkeypatch.setattr(mesh, 'mesh_from_grid', lambda *a, **kw: seen.append(kw) or (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), None))
    mesh.export_mesh(_Field(), d, 'e.obj', grid_size=G)
    mesh.export_mesh(_Field(), d, 'e.obj', grid_size=G, mesh_format='obj')
    mesh.export_mesh(_Field(), d, 'e.glb', grid_size=G, mesh_format='glb')
    assert [kw.get('mesh_format') for kw in seen] == [None, 'obj', 'glb']                  # handed on as given: mesh_from_grid has the default
