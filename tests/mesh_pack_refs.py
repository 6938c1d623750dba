"""Plain-numpy restatement of the binary mesh export of include/ln3d_meshpack.h (csrc/meshpack.hip: ln3d_pack_ply_vertices,
ln3d_pack_ply_faces, ln3d_pack_gltf_vertices, ln3d_pack_gltf_indices, ln3d_pack_gltf_corners, ln3d_position_bounds) and two minimal readers
of the files that mesh.write_ply and mesh.write_glb write, which share no code with the writers (struct, json and numpy only).

The three value rules:
  rotate   out[r] = fl(fl(fl(R[r][0] x) + fl(R[r][1] y)) + fl(R[r][2] z)), float32, five roundings, no fused multiply-add;
  colour   (uint8) trunc(min(max(c, 0), 1) * 255), NaN -> 0;
  narrow   the low 32 bits of the int64 index.
ply_body, gltf_sections and bounds are built from them.  VARIANTS seeds the faults a packer could have; the tests show that the
equalities of tests/test_mesh_pack_gpu.py tell each of them from the definition on the inputs those tests use (case)."""
import json
import struct

import numpy as np

SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 257, 1000)        # every phase of the 4-record period, a partial last word, wave and block edges, > 1 block
VARIANTS = ('fma', 'round', 'big_endian', 'stride', 'pad')
ROT_X_M90 = np.array([[1, 0, 0], [0, np.cos(np.radians(-90)), -np.sin(np.radians(-90))], [0, np.sin(np.radians(-90)), np.cos(np.radians(-90))]],
                     dtype=np.float32)                 # mesh.rotation_matrix_x(-90), restated


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------- the value rules
def rotate(R, p, fma=False):
    """R [3,3], p [n,3] float32 -> [n,3] float32 in the stated order.  fma=True is the seeded fault: every product fused into the sum that
    follows it (the float64 product of two float32 is exact, so rounding float64(a * b + c) to float32 is the fused result but for double
    rounding)"""
    R, p = np.asarray(R, np.float32), np.asarray(p, np.float32).reshape(-1, 3)
    out = np.empty_like(p)
    with np.errstate(all='ignore'):
        for r in range(3):
            if fma:
                ab = (R[r, 1].astype(np.float64) * p[:, 1] + (R[r, 0] * p[:, 0]).astype(np.float64)).astype(np.float32)
                out[:, r] = (R[r, 2].astype(np.float64) * p[:, 2] + ab.astype(np.float64)).astype(np.float32)
            else:
                a, b, c = R[r, 0] * p[:, 0], R[r, 1] * p[:, 1], R[r, 2] * p[:, 2]
                ab = a + b
                out[:, r] = ab + c
    return out


def colour(c, rounding=False):
    """float32 [...] -> uint8.  rounding=True is the seeded fault: round to nearest instead of truncating"""
    c = np.asarray(c, np.float32)
    with np.errstate(all='ignore'):
        x = np.fmin(np.fmax(c, np.float32(0)), np.float32(1)) * np.float32(255)          # fmax / fmin return the number when one side is NaN
    return (np.rint(x) if rounding else np.trunc(x)).astype(np.uint8)


def narrow(faces):
    return (np.asarray(faces, np.int64) & 0xffffffff).astype(np.uint32)


def key(x):
    """the order-preserving uint32 key of a float32: ascending with x, -0 below +0"""
    b = bits(x).astype(np.uint32)
    return np.where(b & 0x80000000, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def bounds(pos):
    """pos [n,3] float32 -> float32 [6]: the per-axis minimum, then maximum, in the order of key"""
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    k = key(pos)
    return np.concatenate([pos[k.argmin(0), np.arange(3)], pos[k.argmax(0), np.arange(3)]]).astype(np.float32)


# ---------------------------------------------------------------- the packed bytes
def pad4(data, fill=0):
    return data + bytes([fill]) * (-len(data) % 4)


def ply_body(xyz, normal, rgb, faces, R=ROT_X_M90, variant=None):
    """-> (vertex bytes, face bytes), each padded with zeros to a multiple of 4: what the two PLY packers leave in their buffers"""
    assert variant is None or variant in VARIANTS
    e = '>' if variant == 'big_endian' else '<'
    extra = [('slack', 'u1')] if variant == 'stride' else []
    nv, nf = len(xyz), len(faces)
    fields = [('p', e + 'f4', 3)] + ([('n', e + 'f4', 3)] if normal is not None else []) + [('c', 'u1', 3)] + extra
    v = np.zeros(nv, np.dtype(fields))
    v['p'] = rotate(R, xyz, fma=variant == 'fma')
    if normal is not None:
        v['n'] = rotate(R, normal, fma=variant == 'fma')
    v['c'] = colour(rgb, rounding=variant == 'round')
    f = np.zeros(nf, np.dtype([('k', 'u1'), ('i', e + 'u4', 3)] + extra))
    f['k'], f['i'] = 3, narrow(faces)
    assert v.dtype.itemsize == (27 if normal is not None else 15) + len(extra) and f.dtype.itemsize == 13 + len(extra)
    fill = 0xA5 if variant == 'pad' else 0
    vsize, fsize = nv * (v.dtype.itemsize - len(extra)), nf * 13                          # 'stride': the right length, the wrong period
    return pad4(v.tobytes()[:vsize], fill), pad4(f.tobytes()[:fsize], fill)


def ply_header(nv, nf, normals):
    lines = ['ply', 'format binary_little_endian 1.0', 'comment ln3diff_amd', 'element vertex %d' % nv, 'property float x', 'property float y',
             'property float z'] + (['property float nx', 'property float ny', 'property float nz'] if normals else []) + [
             'property uchar red', 'property uchar green', 'property uchar blue', 'element face %d' % nf,
             'property list uchar int vertex_indices', 'end_header']
    return ''.join(ln + '\n' for ln in lines).encode('ascii')


def ply_file(xyz, normal, rgb, faces, R=ROT_X_M90):
    vb, fb = ply_body(xyz, normal, rgb, faces, R)
    return ply_header(len(xyz), len(faces), normal is not None) + vb[:len(xyz) * (27 if normal is not None else 15)] + fb[:len(faces) * 13]


def gltf_sections(xyz, normal, rgb, faces, uv=None, R=ROT_X_M90, variant=None):
    """-> {name: array} in buffer order.  Without uv: POSITION [nv,3] f32, NORMAL when given, COLOR_0 [nv,4] u8, indices [3 nf] u32.  With
    uv [nf,3,2]: the vertices split per face corner - POSITION [3 nf,3], NORMAL, TEXCOORD_0 [3 nf,2] = (u, 1 - v)."""
    pos = rotate(R, xyz, fma=variant == 'fma')
    nrm = rotate(R, normal, fma=variant == 'fma') if normal is not None else None
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    out = {}
    if uv is None:
        out['POSITION'] = pos
        if nrm is not None:
            out['NORMAL'] = nrm
        out['COLOR_0'] = np.concatenate([colour(rgb, rounding=variant == 'round'), np.full((len(pos), 1), 255, np.uint8)], 1)
        out['indices'] = narrow(faces).reshape(-1)
        return out
    corner = faces.reshape(-1)
    out['POSITION'] = pos[corner]
    if nrm is not None:
        out['NORMAL'] = nrm[corner]
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    out['TEXCOORD_0'] = np.stack([uv[:, 0], np.float32(1) - uv[:, 1]], 1).astype(np.float32)
    return out


# ---------------------------------------------------------------- the inputs of the GPU tests
def special_colours():
    """every k / 255 with both float32 neighbours, then -0.5, 1.5, +-inf and NaN: 773 values"""
    k = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)
    return np.concatenate([np.nextafter(k, np.float32(-1)), k, np.nextafter(k, np.float32(2)),
                           np.array([-0.5, 1.5, np.inf, -np.inf, np.nan], np.float32)]).astype(np.float32)


SPECIAL_ROWS = np.array([[0.0, -0.0, 1e-40], [-1e-45, 1e30, -1e30], [1.1754942e-38, -0.45, 0.45], [-0.0, 0.0, -3e-39]], np.float32)


def case(n, seed=0):
    """n vertices and n faces -> dict(xyz, normal, rgb [n,3] f32, faces [n,3] int64, uv [n,3,2] f32, R [3,3] f32: a general matrix).  The
    special rows (+-0, subnormals, +-1e30) and the special colours rotate with n, so that every size holds some and n = 1000 all."""
    rng = np.random.default_rng(1000 * seed + n)
    xyz = rng.uniform(-0.45, 0.45, (n, 3)).astype(np.float32)
    m = min(n, len(SPECIAL_ROWS))
    xyz[:m] = np.roll(SPECIAL_ROWS, n, 0)[:m]
    normal = rng.normal(size=(n, 3)).astype(np.float32)
    normal /= np.linalg.norm(normal, axis=1, keepdims=True).astype(np.float32)
    normal[n // 2] = 0                                                                    # a vertex where the field has no gradient
    rgb = rng.uniform(-0.1, 1.1, 3 * n).astype(np.float32)
    sc = np.roll(special_colours(), 7 * n)
    rgb[:min(3 * n, len(sc))] = sc[:3 * n]
    faces = rng.integers(0, n, (n, 3)).astype(np.int64)
    faces[0] = (0, n - 1, n // 2)
    uv = rng.uniform(0, 1, (n, 3, 2)).astype(np.float32)
    uv[0, 0], uv[0, 1] = (0.0, 1.0), (1.0, 0.0)
    R = rng.uniform(-1, 1, (3, 3)).astype(np.float32)
    return dict(xyz=xyz, normal=normal, rgb=rgb.reshape(n, 3), faces=faces, uv=uv, R=R)


def hand_made():
    """name -> (xyz, normal, rgb, faces): small meshes in the box with unit normals and colours in and beyond [0, 1]"""
    tet = np.array([[0, 0, 0], [0.4, 0, 0], [0, 0.4, 0], [0, 0, 0.4]], np.float32) - np.float32(0.1)
    tf = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int64)
    n = (tet / np.linalg.norm(tet, axis=1, keepdims=True)).astype(np.float32)
    c = np.array([[0, 0.5, 1], [1.5, -0.5, 0.25], [1 / 255, 2 / 255, 254.999 / 255], [np.nan, 0.999, 0.001]], np.float32)
    out = {'tetra': (tet, n, c, tf), 'one_face': (tet[:3], n[:3], c[:3], tf[:1]), 'five_faces': (tet, n, c, np.concatenate([tf, tf[:1]]))}
    k = case(65, 3)
    out['sixty_five'] = (k['xyz'], k['normal'], k['rgb'], k['faces'])
    return out


# ---------------------------------------------------------------- reader: PLY
PLY_TYPES = {'float': '<f4', 'uchar': 'u1', 'int': '<i4'}


def parse_ply(data):
    """the bytes of a binary little-endian PLY -> dict(comments, nv, nf, names: the vertex property names in order, xyz [nv,3] f32, normal
    [nv,3] f32 or None, rgb [nv,3] u8, faces [nf,3] int32).  The header grammar is checked line by line; every face must list 3 indices;
    the body must end where the file ends."""
    end = data.index(b'end_header\n') + len(b'end_header\n')
    head = data[:end].decode('ascii')
    assert head.endswith('\n') and '\r' not in head
    lines = head[:-1].split('\n')
    assert lines[0] == 'ply' and lines[1] == 'format binary_little_endian 1.0' and lines[-1] == 'end_header'
    elements, comments = [], []
    for ln in lines[2:-1]:
        w = ln.split(' ')
        assert '' not in w, ln
        if w[0] == 'comment':
            comments.append(ln[len('comment '):])
        elif w[0] == 'element':
            assert len(w) == 3 and w[2].isdigit(), ln
            elements.append((w[1], int(w[2]), []))
        elif w[0] == 'property':
            assert elements, ln
            if w[1] == 'list':
                assert len(w) == 5 and w[2] in PLY_TYPES and w[3] in PLY_TYPES, ln
                elements[-1][2].append((w[4], (PLY_TYPES[w[2]], PLY_TYPES[w[3]])))
            else:
                assert len(w) == 3 and w[1] in PLY_TYPES, ln
                elements[-1][2].append((w[2], PLY_TYPES[w[1]]))
        else:
            raise AssertionError('unknown header line %r' % ln)
    assert [e[0] for e in elements] == ['vertex', 'face']
    (_, nv, vprops), (_, nf, fprops) = elements
    vdtype = np.dtype([(name, t) for name, t in vprops])
    assert len(fprops) == 1 and fprops[0][0] == 'vertex_indices' and isinstance(fprops[0][1], tuple)
    fdtype = np.dtype([('n', fprops[0][1][0]), ('i', fprops[0][1][1], 3)])
    assert len(data) == end + nv * vdtype.itemsize + nf * fdtype.itemsize, 'the body does not end where the file ends'
    v = np.frombuffer(data, vdtype, nv, end)
    f = np.frombuffer(data, fdtype, nf, end + nv * vdtype.itemsize)
    assert (f['n'] == 3).all()
    names = [name for name, _ in vprops]
    col = lambda *k: np.stack([v[x] for x in k], 1) if nv else np.zeros((0, len(k)), v[k[0]].dtype)        # noqa: E731
    return dict(comments=comments, nv=nv, nf=nf, names=names, xyz=col('x', 'y', 'z'), normal=col('nx', 'ny', 'nz') if 'nx' in names else None,
                rgb=col('red', 'green', 'blue'), faces=f['i'].reshape(nf, 3))


# ---------------------------------------------------------------- reader: GLB
GLTF_COMPONENT = {5126: '<f4', 5121: 'u1', 5125: '<u4', 5123: '<u2'}
GLTF_WIDTH = {'SCALAR': 1, 'VEC2': 2, 'VEC3': 3, 'VEC4': 4}


def parse_glb(data):
    """the bytes of a GLB -> dict(json: the document, text: the JSON chunk as written, bin: the BIN chunk or None, arrays: {attribute name or
    'indices': array} of the one primitive, image: the bytes of the texture's image or None).  Checks the container (magic, version, total
    length, chunk types, lengths and padding) and, for every accessor, that its bufferView lies in the buffer, starts at a multiple of 4 and
    holds the accessor."""
    magic, version, total = struct.unpack_from('<4sII', data, 0)
    assert magic == b'glTF' and version == 2 and total == len(data) and total % 4 == 0
    jlen, jtype = struct.unpack_from('<I4s', data, 12)
    assert jtype == b'JSON' and jlen % 4 == 0 and 20 + jlen <= total
    text = data[20:20 + jlen]
    doc = json.loads(text.decode('ascii'))
    assert text.rstrip(b' ') == json.dumps(doc, separators=(',', ':')).encode('ascii'), 'the JSON is not in its compact form padded with spaces'
    pos, blob = 20 + jlen, None
    if pos < total:
        blen, btype = struct.unpack_from('<I4s', data, pos)
        assert btype == b'BIN\0' and blen % 4 == 0 and pos + 8 + blen == total
        blob = data[pos + 8:]
    out = dict(json=doc, text=text, bin=blob, arrays={}, image=None)
    assert doc['asset']['version'] == '2.0' and doc['scene'] == 0 and len(doc['scenes']) == 1
    if 'meshes' not in doc:
        assert blob is None and doc['scenes'] == [{}] and set(doc) == {'asset', 'scene', 'scenes'}
        return out
    assert doc['scenes'] == [{'nodes': [0]}] and doc['nodes'] == [{'mesh': 0}] and len(doc['meshes']) == 1 and len(doc['meshes'][0]['primitives']) == 1
    assert len(doc['buffers']) == 1 and set(doc['buffers'][0]) == {'byteLength'} and doc['buffers'][0]['byteLength'] == len(blob)
    last = 0
    for view in doc['bufferViews']:
        assert view['buffer'] == 0 and view['byteOffset'] % 4 == 0 and view['byteOffset'] >= last, view       # in order, aligned, apart
        last = view['byteOffset'] + view['byteLength']
        assert last <= len(blob) and not any(blob[last:(last + 3) // 4 * 4]), 'pad bytes behind a view must be zero'
    assert (last + 3) // 4 * 4 == len(blob)

    def resolve(i):
        acc = doc['accessors'][i]
        view = doc['bufferViews'][acc['bufferView']]
        dt, width = np.dtype(GLTF_COMPONENT[acc['componentType']]), GLTF_WIDTH[acc['type']]
        assert acc['count'] >= 1 and acc.get('byteOffset', 0) == 0 and 'byteStride' not in view
        assert view['byteLength'] == acc['count'] * width * dt.itemsize, (acc, view)
        a = np.frombuffer(blob, dt, acc['count'] * width, view['byteOffset'])
        return (a if width == 1 else a.reshape(acc['count'], width)), acc, view
    prim = doc['meshes'][0]['primitives'][0]
    assert prim['mode'] == 4 and prim['material'] == 0
    for name, i in prim['attributes'].items():
        out['arrays'][name], acc, view = resolve(i)
        assert view['target'] == 34962, name
    if 'indices' in prim:
        out['arrays']['indices'], acc, view = resolve(prim['indices'])
        assert view['target'] == 34963 and acc['componentType'] == 5125 and acc['type'] == 'SCALAR'
    if 'images' in doc:
        (img,) = doc['images']
        view = doc['bufferViews'][img['bufferView']]
        assert img['mimeType'] == 'image/png' and 'target' not in view
        out['image'] = blob[view['byteOffset']:view['byteOffset'] + view['byteLength']]
    return out
