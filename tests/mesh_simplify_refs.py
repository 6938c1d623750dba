"""Plain-numpy restatement of the mesh simplification of include/ln3d_meshsimplify.h (csrc/mesh.hip: ln3d_simplify_keys, ln3d_simplify_mean,
ln3d_simplify_faces, ln3d_simplify_first, ln3d_simplify_used, then ln3d_mesh_gather), no GPU, written from the definition with loops where the
order matters, and the hand-made meshes that tests/test_mesh_simplify_cpu.py and tests/test_mesh_simplify_gpu.py share.  Every comparison
against it is an equality: bit patterns for the representatives, integers elsewhere.

Definition: a vertex falls into the lattice cell q_a = floor((x_a - origin_a) / cell) per axis, all in float32; key = q_x << 42 | q_y << 21
| q_z; the distinct keys in ascending order are the clusters; a cluster's representative is the float32 sum of its members, added one by one
in ascending vertex index starting from +0, divided by the member count in float32; a face whose clusters are not three different ones is
dropped; of the faces with the same set of three clusters the one with the smallest index survives, with its own corner order; clusters that
no surviving face names are dropped; survivors keep their order and faces are renumbered."""
import functools

import numpy as np

import mesh_clean_refs as M

QMAX = (1 << 21) - 1
F32 = np.float32


def cell_of(x, origin, cell):
    """x [..., 3] float32, origin three float32, cell float32 -> q [..., 3] int64, clamped into [0, QMAX] as the kernel clamps (NaN -> 0)"""
    x, origin, cell = np.asarray(x, dtype=F32), np.asarray(origin, dtype=F32), F32(cell)
    with np.errstate(all='ignore'):
        q = np.floor((x - origin) / cell)                                # float32 throughout: one subtraction, one division, floor
    q = np.where(np.isnan(q), F32(0), np.clip(q, F32(0), F32(QMAX)))
    return q.astype(np.int64)


def keys(verts, origin, cell):
    """-> key [nv] int64"""
    q = cell_of(verts, origin, cell)
    return (q[:, 0] << 42) | (q[:, 1] << 21) | q[:, 2]


def clusters(key):
    """-> (cluster [nv] int64: the rank of key[v] among the distinct keys, nc)"""
    uniq, inv = np.unique(key, return_inverse=True)
    return inv.astype(np.int64).reshape(-1), len(uniq)


def csr(cluster, nc):
    """-> (order [nv] int64: the vertices by cluster, ascending index inside a cluster; start [nc + 1] int64)"""
    order = np.argsort(cluster, kind='stable').astype(np.int64)
    start = np.zeros(nc + 1, dtype=np.int64)
    np.cumsum(np.bincount(cluster, minlength=nc), out=start[1:])
    return order, start


def mean(verts, order, start):
    """-> rep [nc, 3] float32: a loop, because the order of the additions is the definition"""
    verts = np.asarray(verts, dtype=F32)
    nc = len(start) - 1
    rep = np.empty((nc, 3), dtype=F32)
    with np.errstate(all='ignore'):
        for k in range(nc):
            s = np.zeros(3, dtype=F32)                                   # +0
            for v in order[start[k]:start[k + 1]]:
                s = s + verts[v]                                         # float32 + float32, per coordinate
            rep[k] = s / F32(start[k + 1] - start[k])
    return rep


def cluster_faces(faces, cluster):
    """-> (cfaces [nf, 3] int64, fkey [nf] int64: -1 for a face with two equal corners, else its ascending corners packed 21 bits each)"""
    cf = np.asarray(cluster, dtype=np.int64)[np.asarray(faces, dtype=np.int64).reshape(-1, 3)]
    s = np.sort(cf, axis=1)
    dead = (cf[:, 0] == cf[:, 1]) | (cf[:, 1] == cf[:, 2]) | (cf[:, 0] == cf[:, 2])
    return cf, np.where(dead, np.int64(-1), (s[:, 0] << 42) | (s[:, 1] << 21) | s[:, 2])


def sort_keys(fkey):
    """-> (sorted_key, perm): the stable ascending sort that the face-first stage takes"""
    perm = np.argsort(fkey, kind='stable').astype(np.int64)
    return fkey[perm], perm


def first(sorted_key, perm):
    """-> keep_f [nf] int32: 1 at the original index of every run head whose key is not -1"""
    keep = np.zeros(len(perm), dtype=np.int32)
    for i in range(len(perm)):
        if sorted_key[i] != -1 and (i == 0 or sorted_key[i - 1] != sorted_key[i]):
            keep[perm[i]] = 1
    return keep


def first_by_scan(fkey):
    """the same mask without a sort: walk the faces in order and remember the keys seen"""
    seen, keep = set(), np.zeros(len(fkey), dtype=np.int32)
    for f, k in enumerate(fkey.tolist()):
        if k != -1 and k not in seen:
            seen.add(k)
            keep[f] = 1
    return keep


def used(cfaces, keep_f, nc):
    """-> keep_v [nc] int32"""
    keep_v = np.zeros(nc, dtype=np.int32)
    keep_v[cfaces[keep_f != 0].reshape(-1)] = 1
    return keep_v


def stages(verts, faces, cell, origin=None):
    """every intermediate of the whole, as a dict; origin None: the per-axis minimum"""
    verts = np.asarray(verts, dtype=F32)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    origin = verts.min(0) if origin is None else np.asarray(origin, dtype=F32)
    key = keys(verts, origin, cell)
    cluster, nc = clusters(key)
    order, start = csr(cluster, nc)
    rep = mean(verts, order, start)
    cfaces, fkey = cluster_faces(faces, cluster)
    sorted_key, perm = sort_keys(fkey)
    keep_f = first(sorted_key, perm)
    keep_v = used(cfaces, keep_f, nc)
    v, f = M.compact(rep, cfaces, keep_v, keep_f)
    return dict(origin=origin, key=key, cluster=cluster, nc=nc, order=order, start=start, rep=rep, cfaces=cfaces, fkey=fkey,
                sorted_key=sorted_key, perm=perm, keep_f=keep_f, keep_v=keep_v, verts=v, faces=f,
                degenerate=int((fkey == -1).sum()), duplicate=int((fkey != -1).sum() - keep_f.sum()))


def simplify(verts, faces, cell, origin=None):
    """-> (verts' [nv', 3] float32, faces' [nf', 3] int64)"""
    s = stages(verts, faces, cell, origin)
    return s['verts'], s['faces']


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


# ------------------------------------------------------------------------------------------------ hand-made meshes
# Two triangles that share the edge 1 - 2, on the lattice of cell 1 at the origin: (verts, faces, cell, cells they fall into, want verts, want faces)
QUAD_F = [[0, 1, 2], [2, 1, 3]]


def quad(n):
    """the quad 0 1 / 2 3 with its four vertices in 4, 3, 2 or 1 cells"""
    v = {4: [[0.5, 0.5, 0], [1.5, 0.5, 0], [0.5, 1.5, 0], [1.5, 1.5, 0]],            # one vertex per cell: nothing changes but the order
         3: [[0.5, 0.5, 0], [1.5, 0.5, 0], [0.5, 1.5, 0], [0.75, 1.25, 0]],          # 3 joins 2: the second face collapses
         2: [[0.5, 0.5, 0], [1.5, 0.5, 0], [0.25, 0.75, 0], [1.25, 0.75, 0]],        # 2 joins 0, 3 joins 1: both collapse
         1: [[0.5, 0.5, 0], [0.75, 0.5, 0], [0.5, 0.75, 0], [0.75, 0.75, 0]]}[n]
    # clusters ascend by key = (q_x, q_y, q_z): cell (0,0) < (0,1) < (1,0) < (1,1)
    want = {4: ([[0.5, 0.5, 0], [0.5, 1.5, 0], [1.5, 0.5, 0], [1.5, 1.5, 0]], [[0, 2, 1], [1, 2, 3]]),
            3: ([[0.5, 0.5, 0], [0.625, 1.375, 0], [1.5, 0.5, 0]], [[0, 2, 1]]),
            2: ([], []),
            1: ([], [])}[n]
    return (np.array(v, dtype=F32), np.array(QUAD_F, dtype=np.int64), 1.0,
            np.array(want[0], dtype=F32).reshape(-1, 3), np.array(want[1], dtype=np.int64).reshape(-1, 3))


def opposite_pair():
    """two faces on the same three vertices with opposite winding, then a third copy rotated: only face 0 survives, with its own order"""
    v = np.array([[0.5, 0.5, 0.5], [2.5, 0.5, 0.5], [0.5, 2.5, 0.5]], dtype=F32)
    f = np.array([[2, 1, 0], [0, 1, 2], [1, 0, 2]], dtype=np.int64)
    # clusters by key: vertex 0 (0,0,0) -> 0, vertex 2 (0,2,0) -> 1, vertex 1 (2,0,0) -> 2
    return v, f, 1.0, np.array([[0.5, 0.5, 0.5], [0.5, 2.5, 0.5], [2.5, 0.5, 0.5]], dtype=F32), np.array([[1, 2, 0]], dtype=np.int64)


def boundary(cell):
    """vertices exactly on, one ulp below and one ulp above the boundary 3 * cell (as float32 computes it), origin 0: -> (x [3], q [3]) with
    q worked out in exact arithmetic on the float32 values where that is possible (cell = 0.5), by the float32 definition otherwise"""
    c = F32(cell)
    b = F32(3) * c
    x = np.array([np.nextafter(b, F32(0)), b, np.nextafter(b, F32(np.inf))], dtype=F32)
    return x


@functools.lru_cache(maxsize=None)
def big_cluster(n=1000):
    """n vertices in one cell of edge 1 at the origin whose float32 partial sums round at almost every step (24-bit fractions against sums in
    the hundreds), so the order of the additions shows in the bits -> verts [n, 3] float32"""
    rng = np.random.default_rng(5)
    return (rng.random((n, 3)) * 0.999).astype(F32)


def small_clusters(nc=203, seed=9):
    """nc (no multiple of 64) cells of edge 1 along x with 1 to 8 members each, vertices shuffled -> verts [nv, 3] float32"""
    rng = np.random.default_rng(seed)
    members = rng.integers(1, 9, nc)
    cells = np.repeat(np.arange(nc), members)
    v = rng.random((len(cells), 3)) * 0.999
    v[:, 0] += cells
    return v[rng.permutation(len(v))].astype(F32)


# ------------------------------------------------------------------------------------------------ fields
# (field of mesh_clean_refs, G or None for the field's own, cell) -> vertices and faces before and after, clusters, duplicate faces
RECORDED = {
    ('blob', 24, 2.0): dict(before=(222, 424), after=(50, 83), nc=51, duplicate=1),
    ('blob', 48, 1.5): dict(before=(942, 1864), after=(308, 598), duplicate=2),
    ('noise', None, 2.0): dict(before=(2325, 4144), after=(216, 678), duplicate=83),
}
CELLS = (1.0, 1.5, 2.0, 3.0)


@functools.lru_cache(maxsize=None)
def welded(name, G=None, method='cubes'):
    """the reference's welded mesh of a field of mesh_clean_refs.FIELDS (method 'cubes' or 'tetra'; G: the blob field at another grid size,
    marching cubes), float32 vertices in grid units: (verts [nv,3] float32, faces [nf,3] int64)"""
    import mesh_refs as R
    if name == 'blob' and G not in (None, M.BLOB_G):
        assert method == 'cubes'
        _, faces, pos, _ = R.weld(R.ref_cubes(M.blob_field(G), M.BLOB_THR, R.load_mc_table()))
        faces = faces.astype(np.int64)
    else:
        pos, faces = M.welded(name, method)
    return np.asarray(pos).astype(F32), faces


# every entry of mesh_clean_refs.FIELDS (name, None, method), and the blob field at G = 48 on top
FIELD_CASES = [(name, None, method) for name, method in M.FIELDS] + [('blob', 48, 'cubes')]
