"""The quadric-error placement of include/ln3d_meshquadric.h (csrc/mesh.hip: ln3d_quadric_pairs, ln3d_quadric_place) without a GPU:
the float64 reference of the definition (place64), an fp32 numpy restatement that sums in the kernel's stated order (place32, with the
seeded faults of tests/test_mesh_quadric_cpu.py), the inputs that the CPU and the GPU test share, and the checks both apply (check_placement).
The clusters, cfaces and means are those of tests/mesh_simplify_refs.py.

Definition: face f contributes to cluster k once if one of its corners lies in k; in coordinates local to the float32 mean m_k, with a, b, c
the corners minus m_k, n = (b - a) x (c - a) and d = n . a, the face adds n n^T to A and d n to r; (A + eps trace(A) I) delta = r;
x = m_k + delta is accepted when trace(A) > 0, x is finite and lies in the closed box of the cluster's lattice cell; otherwise the
representative keeps the mean's bits."""
import functools

import numpy as np

import mesh_simplify_refs as S

F32 = np.float32
NONE = np.iinfo(np.int64).max
EPS = 1e-3

# The position bound, per cluster and axis, in units of `cell`: the largest deviation of place32 from place64 over every input of cases()
# (python tests/test_mesh_quadric_cpu.py prints it), times 4 - the kernel may contract products into FMAs and the float64 solve eliminates in
# another order.  A real fault (FAULTS) moves a representative by far more.  profiles/mesh_quadric.md records both numbers.
MEASURED_F32_DEVIATION = 7.54e-6
POSITION_BOUND = 4 * MEASURED_F32_DEVIATION
MAX_SKIPPED = 0.01               # the share of a case's clusters whose flag may go uncompared (x within the bound of a cell face, trace ~ 0)
TINY_TRACE = 1e-30               # a float64 trace below this may be 0 in float32 (squares of normals underflow near 1e-38)
FAULTS = ('missing_face', 'corner_twice', 'wrong_trace', 'offset_from_origin')


# ------------------------------------------------------------------------------------------------ incidence
def pairs(cfaces):
    """-> pair_key [3 nf] int64, from the definition with a loop: corner j of face f counts when its cluster differs from the corners before it"""
    cf = np.asarray(cfaces, dtype=np.int64).reshape(-1, 3)
    key = np.full(3 * len(cf), NONE, dtype=np.int64)
    for f, row in enumerate(cf.tolist()):
        seen = []
        for j, k in enumerate(row):
            if k not in seen:
                seen.append(k)
                key[3 * f + j] = (k << 31) | f
    return key


def rows(pair_key, nc):
    """-> (sorted_key [3 nf], start [nc + 1]): what the caller derives between the two entry points"""
    sk = np.sort(pair_key)
    return sk, np.searchsorted(sk >> 31, np.arange(nc + 1)).astype(np.int64)


def incidence(cfaces, nc):
    """-> (k [np], f [np], start [nc + 1]): the (cluster, face) pairs by cluster, ascending face index inside a cluster"""
    sk, start = rows(pairs(cfaces), nc)
    sk = sk[:start[-1]]
    return sk >> 31, sk & 0x7fffffff, start


def cell_box(cell_key, origin, cell, dtype=np.float64):
    """-> (lo, hi) [nc, 3]: the closed box of every cluster's lattice cell, origin + q cell and origin + (q + 1) cell, rounded once to dtype"""
    key = np.asarray(cell_key, dtype=np.int64)
    q = np.stack([key >> 42, (key >> 21) & S.QMAX, key & S.QMAX], -1).astype(np.float64)
    o, c = np.asarray(origin, dtype=F32).astype(np.float64), float(F32(cell))
    return (o + q * c).astype(dtype), (o + (q + 1) * c).astype(dtype)


# ------------------------------------------------------------------------------------------------ the float64 reference
def _face_terms(verts, faces, k, f, m, dtype):
    """per (cluster, face) pair: n [np, 3] and the local corner a [np, 3] in dtype"""
    v = np.asarray(verts, dtype=F32).astype(dtype)
    m = np.asarray(m, dtype=F32).astype(dtype)[k]
    a, b, c = (v[faces[f, j]] - m for j in range(3))
    return np.cross(b - a, c - a).astype(dtype), a


def place64(verts, faces, st, cell, eps=EPS):
    """st: mesh_simplify_refs.stages(verts, faces, cell, origin) -> dict(x [nc,3] f64: the solution (the mean where trace == 0), placed [nc]
    int32, rep [nc,3] f64: x where placed, else the mean, trace, A [nc,3,3], r [nc,3], margin [nc]: how far inside its cell box x lies on its
    worst axis, in cells (negative: outside), doubt [nc] bool: the clusters whose flag a float32 evaluation may set differently)"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nc = st['nc']
    k, f, _ = incidence(st['cfaces'], nc)
    n, a = _face_terms(verts, faces, k, f, st['rep'], np.float64)
    d = (n * a).sum(1)
    A, r = np.zeros((nc, 3, 3)), np.zeros((nc, 3))
    np.add.at(A, k, n[:, :, None] * n[:, None, :])
    np.add.at(r, k, d[:, None] * n)
    trace = np.trace(A, axis1=1, axis2=2)
    m = st['rep'].astype(np.float64)
    x = m.copy()
    ok = trace > 0
    M = A[ok] + (eps * trace[ok])[:, None, None] * np.eye(3)
    x[ok] = m[ok] + np.linalg.solve(M, r[ok][:, :, None])[:, :, 0]
    lo, hi = cell_box(st['key_unique'], st['origin'], cell)
    margin = np.minimum(x - lo, hi - x).min(1) / float(F32(cell))
    placed = (ok & np.isfinite(x).all(1) & (margin >= 0)).astype(np.int32)
    doubt = (ok & (np.abs(margin) <= POSITION_BOUND)) | (ok & (trace < TINY_TRACE))
    return dict(x=x, placed=placed, rep=np.where(placed[:, None] != 0, x, m), trace=trace, A=A, r=r, margin=margin, doubt=doubt, mean=m)


def energy(ref, x):
    """the quadric energy sum over a cluster's faces of (n . (x - m - a))^2 in float64, from A, r and the constant: -> [nc] minus the
    constant term, so energy(x) - energy(m) is exact enough to compare"""
    dl = np.asarray(x, dtype=np.float64) - ref['mean']
    return np.einsum('ki,kij,kj->k', dl, ref['A'], dl) - 2 * (ref['r'] * dl).sum(1)


# ------------------------------------------------------------------------------------------------ the fp32 restatement
def _butterfly(p):
    """p [nc, 64, C] float32 -> [nc, C]: p_l <- p_l + p_(l xor s) for s = 32 ... 1"""
    lane = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        p = p + p[:, lane ^ s]
    return p[:, 0]


def place32(verts, faces, st, cell, eps=EPS, fault=None):
    """the kernel's arithmetic in numpy float32: 64 partial sums per cluster (partial l takes the faces at positions l, l + 64, ... of the
    cluster's row, one by one), the butterfly, the LDL^T solve, the acceptance test -> (rep [nc,3] float32, placed [nc] int32).  Products are
    rounded where the kernel may fuse them; that difference is inside POSITION_BOUND's margin.  fault: one of FAULTS."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nc = st['nc']
    cf = st['cfaces']
    if fault == 'corner_twice':                                          # every corner counts, so a face with two corners in k is taken twice
        key = ((cf.reshape(-1) << 31) | np.repeat(np.arange(len(cf)), 3)).astype(np.int64)
        sk, start = rows(key, nc)
        k, f = sk >> 31, sk & 0x7fffffff
    else:
        k, f, start = incidence(cf, nc)
    pos = np.arange(len(k)) - start[k]
    if fault == 'missing_face':                                          # the last face of every row is never read
        keep = pos < (start[k + 1] - start[k] - 1)
        k, f, pos = k[keep], f[keep], pos[keep]
    m = st['rep'].astype(F32)
    n, a = _face_terms(verts, faces, k, f, m, F32)
    if fault == 'offset_from_origin':                                    # the plane offset against the origin instead of m_k
        a = a + m[k]
    d = ((n[:, 0] * a[:, 0] + n[:, 1] * a[:, 1]) + n[:, 2] * a[:, 2]).astype(F32)
    term = np.stack([n[:, 0] * n[:, 0], n[:, 0] * n[:, 1], n[:, 0] * n[:, 2], n[:, 1] * n[:, 1], n[:, 1] * n[:, 2], n[:, 2] * n[:, 2],
                     d * n[:, 0], d * n[:, 1], d * n[:, 2]], -1).astype(F32)
    p = np.zeros((nc, 64, 9), dtype=F32)
    lane, rnd = pos % 64, pos // 64
    for i in range(int(rnd.max()) + 1 if len(rnd) else 0):               # a (cluster, lane) occurs at most once per round: += is a plain add
        sel = rnd == i
        p[k[sel], lane[sel]] += term[sel]
    a00, a01, a02, a11, a12, a22, r0, r1, r2 = _butterfly(p).T
    tr = (a00 + a11) + a22
    rep, placed = m.copy(), np.zeros(nc, dtype=np.int32)
    with np.errstate(all='ignore'):
        lam = F32(eps) * (((a00 + a01) + a02) if fault == 'wrong_trace' else tr)        # the first row instead of the diagonal
        d0 = a00 + lam
        l10, l20 = a01 / d0, a02 / d0
        d1 = (a11 + lam) - l10 * a01
        t12 = a12 - l20 * a01
        l21 = t12 / d1
        d2 = ((a22 + lam) - l20 * a02) - l21 * t12
        y1 = r1 - l10 * r0
        y2 = (r2 - l20 * r0) - l21 * y1
        dz = y2 / d2
        dy = y1 / d1 - l21 * dz
        dx = (r0 / d0 - l10 * dy) - l20 * dz
        x = m + np.stack([dx, dy, dz], -1).astype(F32)
        lo, hi = cell_box(st['key_unique'], st['origin'], cell, F32)
        ok = (tr > 0) & np.isfinite(x).all(1) & (x >= lo).all(1) & (x <= hi).all(1)
    rep[ok] = x[ok]
    placed[ok] = 1
    return rep, placed


# ------------------------------------------------------------------------------------------------ the checks both tests apply
def check_placement(case, rep, placed, small=False):
    """rep [nc,3] float32, placed [nc] int32 of one case (from the device, or from place32) -> (failures: a list of strings, figures: a dict).
    Positions within POSITION_BOUND cells of the float64 reference per cluster and axis where the reference places; the mean's bits where it
    does not; placed equal to the reference's flag but for the doubtful clusters, at most MAX_SKIPPED of the case (none when small)."""
    ref, st, cell = case['ref'], case['st'], float(F32(case['cell']))
    rep, placed = np.asarray(rep), np.asarray(placed)
    fails = []
    if rep.dtype != F32 or rep.shape != (st['nc'], 3) or placed.shape != (st['nc'],):
        return [f"shapes {rep.dtype} {rep.shape} {placed.shape}"], {}
    doubt = ref['doubt']
    share = float(doubt.mean())
    if share > (0.0 if small else MAX_SKIPPED):
        fails.append(f"{int(doubt.sum())} of {len(doubt)} clusters are doubtful")
    sure = ~doubt
    if not np.array_equal(placed[sure], ref['placed'][sure]):
        bad = np.nonzero(sure & (placed != ref['placed']))[0]
        fails.append(f"placed differs from the reference at {len(bad)} clusters, first {bad[:5].tolist()}")
    on = sure & (ref['placed'] != 0) & (placed != 0)
    dev = np.abs(rep.astype(np.float64) - ref['x'])[on] / cell
    worst = float(dev.max()) if dev.size else 0.0
    if worst > POSITION_BOUND:
        fails.append(f"position {worst:.3g} cells from the float64 reference, bound {POSITION_BOUND:.3g}")
    off = placed == 0
    if not np.array_equal(S.bits(rep[off]), S.bits(st['rep'][off])):
        fails.append("a refused cluster does not have the mean's bits")
    both = doubt & (placed != 0)                                         # a doubtful cluster is still one of the two answers
    if both.any() and float((np.abs(rep.astype(np.float64) - ref['x'])[both] / cell).max()) > POSITION_BOUND:
        fails.append("a doubtful cluster that was placed is not at the reference's solution")
    return fails, dict(worst=worst, doubtful=int(doubt.sum()), placed=int(placed.sum()), nc=int(st['nc']))


# ------------------------------------------------------------------------------------------------ inputs
def grid_box(edge, n, offset=(1.3, 1.45, 1.6)):
    """the surface of the box [0, edge]^3 + offset with n x n points per side, welded: (verts [nv,3] float32, faces [nf,3] int64,
    lo [3], hi [3] of the box).  n = 13, edge = 6: 866 vertices, 1728 faces."""
    t = np.linspace(0.0, edge, n)
    pts, faces = [], []
    idx = {}

    def vid(p):
        key = tuple(np.round(np.asarray(p) / edge * (n - 1)).astype(int).tolist())
        if key not in idx:
            idx[key] = len(pts)
            pts.append(p)
        return idx[key]
    for ax in range(3):
        for side in (0.0, edge):
            u, w = [(ax + 1) % 3, (ax + 2) % 3]
            for i in range(n - 1):
                for j in range(n - 1):
                    q = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0.0, 0.0, 0.0]
                        p[ax], p[u], p[w] = side, t[i + di], t[j + dj]
                        q.append(vid(p))
                    if side == 0.0:
                        q = q[::-1]
                    faces += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    off = np.asarray(offset, dtype=np.float64)
    return (np.asarray(pts) + off).astype(F32), np.asarray(faces, dtype=np.int64), off, off + edge


def box_distance(p, lo, hi):
    """the distance of points p [n,3] from the SURFACE of the box [lo, hi], float64"""
    p = np.asarray(p, dtype=np.float64)
    c, h = (np.asarray(lo) + np.asarray(hi)) / 2, (np.asarray(hi) - np.asarray(lo)) / 2
    q = np.abs(p - c) - h
    outside = np.linalg.norm(np.maximum(q, 0.0), axis=1)
    inside = np.minimum(q.max(1), 0.0)
    return np.abs(outside + inside)


def icosphere(level, radius=10.0, centre=(20.3, 20.45, 20.6)):
    """-> (verts [10 * 4^level + 2, 3] float32, faces [20 * 4^level, 3] int64): level 2 has 162 vertices, level 4 has 2562"""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                mid[key] = len(v)
                v.append(p / np.linalg.norm(p))
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(v) * radius + np.asarray(centre)).astype(F32), np.asarray(f, dtype=np.int64)


def incidence_mesh():
    """five vertices in three cells of edge 1 at the origin (0, 1, 4 in cell (0,0,0) = cluster 0; 3 in (0,1,0) = cluster 1; 2 in (1,0,0) =
    cluster 2) and the faces that exercise every rule: -> (verts, faces, cell, want: the (cluster, face) pairs)"""
    v = np.array([[0.25, 0.25, 0.5], [0.75, 0.25, 0.25], [1.5, 0.25, 0.5], [0.25, 1.5, 0.75], [0.5, 0.75, 0.125]], dtype=F32)
    f = np.array([[0, 1, 2],      # two corners in one cluster: counts once in 0, once in 2
                  [0, 1, 4],      # fully collapsed: counts once in 0
                  [0, 2, 3],      # three clusters: counts in each
                  [2, 0, 1],      # the repeated cluster in the last two corners
                  [0, 2, 4]],     # the repeated cluster in corners 0 and 2, not adjacent
                 dtype=np.int64)
    want = [(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (2, 0), (2, 2), (2, 3), (2, 4)]
    return v, f, 1.0, want


def heavy_fan(n=3000):
    """a cone of n faces inside one cell of edge 2 at the origin, apex off-centre: one cluster with n faces, all of them collapsed"""
    ang = np.linspace(0.0, 2 * np.pi, n, endpoint=False)
    ring = np.stack([1.0 + 0.7 * np.cos(ang), 0.9 + 0.7 * np.sin(ang), np.full(n, 0.3)], -1)
    v = np.concatenate([[[1.2, 1.1, 1.7]], ring]).astype(F32)
    i = np.arange(n)
    return v, np.stack([np.zeros(n, dtype=np.int64), 1 + i, 1 + (i + 1) % n], -1).astype(np.int64)


def zero_area():
    """faces that name a vertex twice: every normal is exactly 0, so trace == 0 and the mean stays"""
    v = np.array([[0.5, 0.5, 0.5], [1.5, 0.75, 0.25], [0.75, 1.5, 1.25]], dtype=F32)
    return v, np.array([[0, 0, 1], [1, 2, 2], [2, 0, 2]], dtype=np.int64)


def coplanar():
    """a tilted planar patch in one cell of edge 2: rank 1, delta along the normal only (and tiny: the mean lies in the plane), accepted"""
    rng = np.random.default_rng(3)
    xy = 0.3 + 1.4 * rng.random((12, 2))
    v = np.concatenate([xy, (0.4 + 0.25 * xy[:, :1] + 0.125 * xy[:, 1:])], 1).astype(F32)
    return v, np.array([[i, (i + 1) % 12, (i + 5) % 12] for i in range(12)], dtype=np.int64)


def far_wedge():
    """two planar strips in one cell of edge 2 whose planes meet on the line x = -0.5, outside the cell: refused, the mean stays"""
    pts, faces = [], []
    for s, x0 in ((0.3, 0.2), (-0.3, 1.1)):
        b = len(pts)
        for i in range(4):
            for y in (0.3, 1.6):
                x = x0 + 0.2 * i
                pts.append([x, y, 1.0 + s * (x + 0.5)])
        for i in range(3):
            faces += [[b + 2 * i, b + 2 * i + 2, b + 2 * i + 1], [b + 2 * i + 1, b + 2 * i + 2, b + 2 * i + 3]]
    return np.asarray(pts, dtype=F32), np.asarray(faces, dtype=np.int64)


def _soup_faces(nv, nf, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, nv, (nf, 3)).astype(np.int64)


def _case(name, verts, faces, cell, origin, **extra):
    st = S.stages(verts, faces, cell, origin)
    st['key_unique'] = np.unique(st['key'])
    return dict(name=name, verts=np.asarray(verts, dtype=F32), faces=np.asarray(faces, dtype=np.int64).reshape(-1, 3), cell=cell,
                origin=np.asarray(st['origin'], dtype=F32), st=st, ref=place64(verts, faces, st, cell), **extra)


SMALL = ('box6', 'ico2_c1.5', 'ico2_c4', 'incidence', 'fan3000', 'zero_area', 'coplanar', 'far_wedge')          # no cluster may be left out
# mesh_simplify_refs' inputs whose vertices lie ON lattice planes (that is their point): their pair keys are compared, exactly; their
# placements are not, because every cluster's solution sits on a face of its cell
PAIRS_ONLY = ('opposite_pair', 'boundary')


@functools.lru_cache(maxsize=None)
def cases():
    """every input the GPU test runs, by name; computed once and shared (read-only)"""
    out = {}
    v, f, lo, hi = grid_box(6.0, 13)
    out['box6'] = _case('box6', v, f, 2.0, (0, 0, 0), box=(lo, hi))
    for level in (2, 4):
        v, f = icosphere(level)
        for cell in (1.5, 4.0):
            out[f'ico{level}_c{cell:g}'] = _case(f'ico{level}_c{cell:g}', v, f, cell, (0, 0, 0))
    v, f, cell, want = incidence_mesh()
    out['incidence'] = _case('incidence', v, f, cell, (0, 0, 0), want=want)
    v, f = heavy_fan()
    out['fan3000'] = _case('fan3000', v, f, 2.0, (0, 0, 0))
    for name, make in (('zero_area', zero_area), ('coplanar', coplanar), ('far_wedge', far_wedge)):
        v, f = make()
        out[name] = _case(name, v, f, 2.0, (0, 0, 0))
    v, f = S.opposite_pair()[:2]
    out['opposite_pair'] = _case('opposite_pair', v, f, 1.0, None)
    x = S.boundary(0.5)
    v = np.stack([x, np.full(3, 0.25, F32), np.full(3, 0.25, F32)], -1)
    out['boundary'] = _case('boundary', np.concatenate([v, v + F32([0, 0.125, 0.0625])]), [[0, 1, 2], [3, 4, 5], [0, 4, 2], [1, 3, 5]], 0.5, (0, 0, 0))
    v = S.small_clusters()
    out['small_clusters'] = _case('small_clusters', v, _soup_faces(len(v), 2 * len(v), 21), 1.0, (0, 0, 0))
    v = S.big_cluster(1000)
    out['big_cluster'] = _case('big_cluster', v, _soup_faces(1000, 700, 22), 1.0, (0, 0, 0))
    return out
