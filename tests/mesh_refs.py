"""Float64 restatement of the iso-surface extractors of csrc/mesh.hip (include/ln3d.h: ln3d_mcubes_count / emit, ln3d_mesh_count / emit),
plain numpy and Python floats, no GPU, and the test fields that tests/test_mesh_refs_cpu.py and tests/test_mesh_cells_gpu.py share.

Conventions (the library's): sigma[x][y][z], corner c of a cell at (c & 1, (c >> 1) & 1, c >> 2), cell = (x (G-1) + y)(G-1) + z, node id
gid = (x G + y) G + z, inside = value > thr (so NaN is outside).  A surface vertex lies on the grid edge between two corners a, b of the cell,
oriented so that gid[a] < gid[b]:  t = (thr - v[a]) / (v[b] - v[a]),  pos = a + t (b - a),  key = gid[a] G^3 + gid[b]; everything in
float64 from the float32 inputs.  Non-finite ends (the rule of include/ln3d.h): an end that is +-inf or NaN pushes the vertex to the other,
finite end (t = 0 or 1); two non-finite ends put it at the midpoint.

Marching tetrahedra: the Kuhn decomposition of the cell around its 0-7 diagonal, tetrahedra in the order TET.  Inside tetrahedron
(c0, c1, c2, c3), `ins` and `outs` are its inside and outside corners in that order:
    1 inside : one triangle (ins0-outs0, ins0-outs1, ins0-outs2)
    3 inside : one triangle (outs0-ins0, outs0-ins1, outs0-ins2)
    2 inside : the quad q0 = ins0-outs0, q1 = ins0-outs1, q2 = ins1-outs1, q3 = ins1-outs0 as triangles (q0, q1, q2), (q0, q2, q3)
and a triangle's last two corners are swapped when its normal (p1 - p0) x (p2 - p0) points against `dir`, the vector from the centroid of
the inside corners to the centroid of the outside corners (normal . dir < 0)."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORNER = [(c & 1, (c >> 1) & 1, c >> 2) for c in range(8)]
TET = ((0, 1, 3, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 6, 7), (0, 4, 5, 7), (0, 1, 5, 7))
G_MAX = 1448                      # gid[a] G^3 + gid[b] < G^6 must stay below 2^63: 1448^6 < 2^63 < 1449^6
U = 2.0 ** -24                    # half an ulp of 1 in float32


def edge_corners(e):
    """table edge id e = axis * 4 + b0 + 2 * b1 -> its two corners: the edge parallel to `axis` whose other two coordinates, in axis order,
    are (b0, b1)"""
    ax, b0, b1 = e >> 2, e & 1, (e >> 1) & 1
    o = [i for i in range(3) if i != ax]
    c = [0, 0, 0]
    c[o[0]], c[o[1]] = b0, b1
    a = c[0] | (c[1] << 1) | (c[2] << 2)
    return a, a | (1 << ax)


def load_mc_table():
    """(tri, count): kMcTri as 256 lists of edge triples and kMcCount as 256 ints, parsed out of ln3diff_amd/csrc/mc_table.h"""
    src = open(os.path.join(ROOT, 'ln3diff_amd', 'csrc', 'mc_table.h')).read()
    body = re.search(r'kMcTri\[256\]\[16\]\s*=\s*\{(.*?)\n\};', src, re.S).group(1)
    rows = re.findall(r'\{([^{}]*)\}', body)
    assert len(rows) == 256
    tri = []
    for r in rows:
        e = [int(x) for x in r.split(',')]
        assert len(e) == 16
        n = e.index(-1)
        assert n % 3 == 0 and all(x == -1 for x in e[n:]) and all(0 <= x < 12 for x in e[:n])
        tri.append([tuple(e[i:i + 3]) for i in range(0, n, 3)])
    cnt = [int(x) for x in re.search(r'kMcCount\[256\]\s*=\s*\{([^}]*)\}', src).group(1).split(',')]
    assert len(cnt) == 256
    return tri, cnt


def ref_cells(sigma, thr):
    """sigma [G,G,G] (read as float32), thr -> dict of per-cell arrays in cell order: v [ncell,8] f32 corner values, gid [ncell,8] int64,
    origin [ncell,3] int64, case [ncell] (bit c = corner c inside), tetra_count [ncell] int32 (triangles of marching tetrahedra), G, thr."""
    s = np.ascontiguousarray(np.asarray(sigma, dtype=np.float32))
    G = s.shape[0]
    assert s.shape == (G, G, G) and 2 <= G <= G_MAX
    thr = np.float32(thr)
    r = np.arange(G - 1, dtype=np.int64)
    origin = np.stack(np.meshgrid(r, r, r, indexing='ij'), -1).reshape(-1, 3)
    off = np.array(CORNER, dtype=np.int64)
    node = origin[:, None, :] + off[None]
    gid = (node[..., 0] * G + node[..., 1]) * G + node[..., 2]
    v = s.reshape(-1)[gid]
    with np.errstate(invalid='ignore'):
        inside = v > thr
    case = (inside.astype(np.int64) << np.arange(8)).sum(1)
    n_in = np.stack([inside[:, list(t)].sum(1) for t in TET], 1)
    tetra_count = np.where(n_in == 2, 2, ((n_in == 1) | (n_in == 3)).astype(np.int64)).sum(1).astype(np.int32)
    return dict(v=v, gid=gid, origin=origin, case=case, tetra_count=tetra_count, G=G, thr=thr)


class _Cell:
    __slots__ = ('v', 'gid', 'o', 'thr', 'G3')

    def vertex(self, a, b):
        """the surface vertex on the cell edge between corners a and b: (key, pos (3 floats), t, |b - a| per axis)"""
        if self.gid[a] > self.gid[b]:
            a, b = b, a
        va, vb, thr = self.v[a], self.v[b], self.thr
        fa, fb = np.isfinite(va), np.isfinite(vb)
        if fa and fb:
            t = (thr - va) / (vb - va)
        else:
            t = 0.0 if fa else (1.0 if fb else 0.5)
        A, B = CORNER[a], CORNER[b]
        pos = tuple(self.o[i] + A[i] + t * (B[i] - A[i]) for i in range(3))
        return self.gid[a] * self.G3 + self.gid[b], pos, t, tuple(abs(B[i] - A[i]) for i in range(3))


def _cells(cells):
    G = cells['G']
    v, gid, origin = cells['v'].astype(np.float64).tolist(), cells['gid'].tolist(), cells['origin'].tolist()
    c = _Cell()
    c.thr, c.G3 = float(cells['thr']), G ** 3
    for i in range(len(v)):
        c.v, c.gid, c.o = v[i], gid[i], origin[i]
        yield i, c


def _pack(cells, counts, tris, margin=None):
    T = len(tris)
    out = dict(G=cells['G'], counts=np.asarray(counts, dtype=np.int32),
               key=np.array([[q[0] for q in t] for t in tris], dtype=np.int64).reshape(T, 3),
               pos=np.array([[q[1] for q in t] for t in tris], dtype=np.float64).reshape(T, 3, 3),
               t=np.array([[q[2] for q in t] for t in tris], dtype=np.float64).reshape(T, 3),
               seg=np.array([[q[3] for q in t] for t in tris], dtype=np.float64).reshape(T, 3, 3))
    if margin is not None:
        out['winding_margin'] = np.asarray(margin, dtype=np.float64)
    return out


def ref_cubes(sigma, thr, table):
    """classic marching cubes over the 256-row `table` = (tri, count) of load_mc_table(): dict(counts [ncell] int32, and per triangle in
    emission order key [T,3] int64, pos [T,3,3] f64, t [T,3] f64, seg [T,3,3] = |b - a| per axis of the edge of every vertex)."""
    tri, cnt = table
    cells = ref_cells(sigma, thr)
    case = cells['case'].tolist()
    counts, tris = [], []
    for i, c in _cells(cells):
        counts.append(cnt[case[i]])
        for t in tri[case[i]]:
            tris.append([c.vertex(*edge_corners(e)) for e in t])
    return _pack(cells, counts, tris)


def ref_tetra(sigma, thr):
    """marching tetrahedra (module docstring): the fields of ref_cubes plus winding_margin [T] = normal . dir of every triangle before the
    swap, in float64 (0 on a zero-area triangle; a value within rounding of 0 elsewhere would make the float32 decision arbitrary)."""
    cells = ref_cells(sigma, thr)
    case = cells['case'].tolist()
    counts, tris, margin = [], [], []
    for i, c in _cells(cells):
        n0 = len(tris)
        if case[i] not in (0, 255):
            for tet in TET:
                ins = [k for k in tet if (case[i] >> k) & 1]
                outs = [k for k in tet if not (case[i] >> k) & 1]
                if len(ins) in (0, 4):
                    continue
                if len(ins) == 1:
                    q = [c.vertex(ins[0], o) for o in outs]
                    faces = [(0, 1, 2)]
                elif len(ins) == 3:
                    q = [c.vertex(outs[0], k) for k in ins]
                    faces = [(0, 1, 2)]
                else:
                    q = [c.vertex(ins[0], outs[0]), c.vertex(ins[0], outs[1]), c.vertex(ins[1], outs[1]), c.vertex(ins[1], outs[0])]
                    faces = [(0, 1, 2), (0, 2, 3)]
                ci = np.mean([CORNER[k] for k in ins], 0)
                co = np.mean([CORNER[k] for k in outs], 0)
                d = co - ci
                for f in faces:
                    p = [np.array(q[j][1]) for j in f]
                    m = float(np.dot(np.cross(p[1] - p[0], p[2] - p[0]), d))
                    margin.append(m)
                    if m < 0:
                        f = (f[0], f[2], f[1])
                    tris.append([q[j] for j in f])
        counts.append(len(tris) - n0)
    out = _pack(cells, counts, tris, margin)
    assert np.array_equal(out['counts'], cells['tetra_count'])
    return out


def position_bound(ref):
    """[T,3,3] bound on |float32 kernel - float64 reference| per coordinate: 4 u |t| |b - a| + u max(|coord|, 1), u = 2^-24.  t is two
    rounded subtractions and one division (3 u |t| to first order, 4 u with the second-order terms), t (b - a) is exact for b - a in
    {0, 1}, and the sum a + t (b - a) is rounded once to a value below G (u |coord|, at least u for the rounding of a value below 1
    when the reference's own coordinate is smaller)."""
    return 4 * U * np.abs(ref['t'])[:, :, None] * ref['seg'] + U * np.maximum(np.abs(ref['pos']), 1.0)


def key_nodes(key, G):
    """vertex keys [...] -> integer node coordinates of both edge ends [..., 2, 3]"""
    key = np.asarray(key, dtype=np.int64)
    g = np.stack([key // G ** 3, key % G ** 3], -1)
    return np.stack([g // (G * G), (g // G) % G, g % G], -1)


def edge_histogram(tris_as_keys, G):
    """tris_as_keys [T,3] int64 (faces as vertex keys) -> dict(pair [E,2] the undirected mesh edges as sorted key pairs, undirected [E] their
    number of uses, directed_max the largest number of uses of one directed edge, boundary [E] bool: both ends of the edge lie on one
    boundary face of the grid (all four grid nodes share a coordinate that is 0 or G - 1))."""
    k = np.asarray(tris_as_keys, dtype=np.int64).reshape(-1, 3)
    e = np.concatenate([k[:, [0, 1]], k[:, [1, 2]], k[:, [2, 0]]])
    if len(e) == 0:
        return dict(pair=e, undirected=np.zeros(0, np.int64), directed_max=0, boundary=np.zeros(0, bool))
    _, dcnt = np.unique(e, axis=0, return_counts=True)
    pair, cnt = np.unique(np.sort(e, 1), axis=0, return_counts=True)
    n = key_nodes(pair, G).reshape(len(pair), 4, 3)
    boundary = ((n == 0).all(1) | (n == G - 1).all(1)).any(1)
    return dict(pair=pair, undirected=cnt, directed_max=int(dcnt.max()), boundary=boundary)


def signed_volume(tris):
    """[T,3,3] -> sum of det(p0, p1, p2) / 6: the enclosed volume of a closed surface with outward normals"""
    t = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    return float(np.linalg.det(t).sum() / 6) if len(t) else 0.0


def zero_area_faces(pos):
    """[T,3,3] -> how many triangles have a cross product that is exactly 0"""
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 3, 3)
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    return int((n == 0).all(1).sum())


def weld(ref):
    """what extract_isosurface does with an emission: (vertex keys [Nv] sorted, faces [Nf,3] of indices into them in emission order without
    the faces that name a vertex twice, positions [Nv,3], position_bound of those [Nv,3])"""
    uniq, first, inv = np.unique(ref['key'].reshape(-1), return_index=True, return_inverse=True)
    faces = inv.reshape(-1, 3)
    ok = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    return uniq, faces[ok], ref['pos'].reshape(-1, 3)[first], position_bound(ref).reshape(-1, 3)[first]


def canon(tri, decimals=4):
    """[T,3,3] triangle soup -> rows of 9 with the smallest vertex first (orientation kept), sorted; `decimals` only decides the order
    (test_mesh_gpu._canon's rule), the values returned are not rounded."""
    t = np.asarray(tri, dtype=np.float64).reshape(-1, 3, 3)
    r = np.round(t, decimals)
    out = np.empty_like(t)
    rr = np.empty_like(t)
    for i in range(len(t)):
        k = min(range(3), key=lambda j: tuple(r[i, j]))
        out[i], rr[i] = np.roll(t[i], -k, axis=0), np.roll(r[i], -k, axis=0)
    order = np.lexsort(rr.reshape(len(t), 9).T[::-1])
    return out.reshape(len(t), 9)[order]


# ------------------------------------------------------------------------------------------------ the shared test fields
ATLAS_G, ATLAS_BLOCKS = 28, 7
NOISE_SEED = 262


def atlas_field(seed=1):
    """G = 28, thr = 0: 7^3 blocks of 4^3 nodes; the central cell of block k < 256 (k = (bx 7 + by) 7 + bz) has its corners set to case k,
    inside magnitudes uniform in [0.2, 3], every other node outside with magnitudes in the same range."""
    rng = np.random.default_rng(seed)
    s = -rng.uniform(0.2, 3.0, (ATLAS_G,) * 3)
    for k in range(256):
        b = (k // 49, (k // 7) % 7, k % 7)
        for c in range(8):
            if (k >> c) & 1:
                x, y, z = (4 * b[i] + 1 + CORNER[c][i] for i in range(3))
                s[x, y, z] = rng.uniform(0.2, 3.0)
    return s.astype(np.float32)


def atlas_block_of(ref):
    """[T] block index k of every triangle of an atlas emission (from its first vertex's lower edge end), after checking that no triangle
    lies in a cell that straddles two blocks"""
    n = key_nodes(ref['key'], ATLAS_G)                     # [T,3,2,3]
    b = n // 4
    assert (b == b[:, :1, :1, :]).all()
    b = b[:, 0, 0]
    return (b[:, 0] * 7 + b[:, 1]) * 7 + b[:, 2]


def noise_field(G=12, seed=NOISE_SEED):
    return np.random.default_rng(seed).standard_normal((G, G, G)).astype(np.float32)


def tie_field(G=8, seed=3):
    """integers in {9, 10, 11}: with thr = 10 every crossing has t in {0, 1/2, 1} and a third of the nodes equal the level"""
    return np.random.default_rng(seed).integers(9, 12, (G, G, G)).astype(np.float32)


def nonfinite_field(G=6, seed=5):
    """a noise field with a few +-inf, NaN and +-3e38 nodes (a crossing between +3e38 and -3e38 overflows v[b] - v[a] in float32)"""
    s = np.random.default_rng(seed).standard_normal((G, G, G)).astype(np.float32)
    s[1, 1, 1], s[1, 1, 2] = np.inf, -np.inf
    s[3, 2, 4], s[4, 4, 1] = np.nan, np.nan
    s[2, 3, 3], s[2, 3, 4] = 3e38, -3e38
    s[4, 2, 2], s[0, 0, 5] = -np.inf, np.inf
    s[5, 5, 5], s[3, 4, 0] = -3e38, 3e38
    return s
