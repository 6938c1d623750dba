"""Plain-numpy restatement of the mesh smoothing of include/ln3d_meshsmooth.h (csrc/mesh.hip: ln3d_smooth_edge_keys,
ln3d_smooth_halfedges, ln3d_smooth_step), no GPU, written from the definition - a counter of undirected edges, sets of neighbours, a
sequential float32 loop per vertex - and the hand-made meshes that tests/test_mesh_smooth_cpu.py and tests/test_mesh_smooth_gpu.py share.
Every comparison against it is an equality: bit patterns for the coordinates, integers elsewhere.

Definition (all arithmetic float32): every face contributes its three undirected edges {a, b}, a == b ignored, duplicate faces and opposite
windings contributing again; the neighbours of vertex i are the distinct vertices that share an edge with it, ascending; an edge named exactly
once is a boundary edge and pins both its ends; a pinned vertex and one without a neighbour never move.  One pass with the factor f, per axis,
for a free vertex: s = x[j_1], s = fl(s + x[j_k]) for k = 2 .. d, m = fl(s / fl32(d)), e = fl(m - x_i), x_i' = fl(x_i + fl(f * e)); every
pass reads the previous pass's coordinates only.  One iteration is a pass with lam, then one with mu unless mu == 0."""
import collections
import functools

import numpy as np

F32 = np.float32
LAM, MU = 0.5, -0.53
VARIANTS = ('fma', 'float64', 'descending', 'duplicates', 'in_place')       # the seeded faults of `step`


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def edge_count(faces):
    """-> Counter {(lo, hi): how many face corner pairs name the undirected edge}, a == b left out"""
    n = collections.Counter()
    for a, b, c in np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist():
        for u, v in ((a, b), (b, c), (c, a)):
            if u != v:
                n[min(u, v), max(u, v)] += 1
    return n


def edge_keys(faces):
    """-> key [3 nf] int64, what ln3d_smooth_edge_keys writes: (lo << 32) | hi of corners j and (j + 1) % 3, or -1"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b = f, np.roll(f, -1, axis=1)
    return np.where(a == b, np.int64(-1), (np.minimum(a, b) << 32) | np.maximum(a, b)).reshape(-1)


def adjacency(faces, nv, multiplicity=False):
    """-> (start [nv + 1] int64, nbr [2E] int32, pinned [nv] int32); multiplicity=True lists a neighbour once per naming of the edge
    (the 'duplicates' fault)"""
    rows = [[] for _ in range(nv)]
    pinned = np.zeros(nv, dtype=np.int32)
    for (lo, hi), n in edge_count(faces).items():
        for _ in range(n if multiplicity else 1):
            rows[lo].append(hi)
            rows[hi].append(lo)
        if n == 1:
            pinned[lo] = pinned[hi] = 1
    start = np.zeros(nv + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=start[1:])
    nbr = np.array([j for r in rows for j in sorted(r)], dtype=np.int32)
    return start, nbr, pinned


def step(verts, start, nbr, pinned, factor, variant=None):
    """one pass -> verts' [nv, 3] float32: a loop, because the order of the additions is the definition.  variant: one of VARIANTS, a
    deliberately wrong pass that the comparisons must tell from the right one"""
    assert variant is None or variant in VARIANTS
    x = np.array(verts, dtype=F32)
    out = x if variant == 'in_place' else x.copy()
    f = F32(factor)
    with np.errstate(all='ignore'):
        for i in range(len(x)):
            row = nbr[start[i]:start[i + 1]]
            if pinned[i] or len(row) == 0:
                continue
            if variant == 'descending':
                row = row[::-1]
            if variant == 'float64':
                s = x[row[0]].astype(np.float64)
                for j in row[1:]:
                    s = s + x[j]
                s = s.astype(F32)
            else:
                s = x[row[0]].copy()
                for j in row[1:]:
                    s = s + x[j]                                         # float32 + float32, per coordinate
            m = s / F32(len(row))
            e = m - x[i]
            if variant == 'fma':                                         # the product is exact in float64: one rounding instead of two
                out[i] = (x[i].astype(np.float64) + np.float64(f) * e.astype(np.float64)).astype(F32)
            else:
                fe = f * e
                out[i] = x[i] + fe
    return out


def smooth(verts, faces, iterations, lam=LAM, mu=MU, variant=None, keep=()):
    """-> verts' [nv, 3] float32 after `iterations` iterations; keep: iteration counts whose result is wanted too -> {count: verts'}"""
    verts = np.asarray(verts, dtype=F32)
    start, nbr, pinned = adjacency(faces, len(verts), multiplicity=variant == 'duplicates')
    kept = {}
    for it in range(1, iterations + 1):
        verts = step(verts, start, nbr, pinned, lam, variant)
        if F32(mu) != 0:
            verts = step(verts, start, nbr, pinned, mu, variant)
        if it in keep:
            kept[it] = verts
    return (verts, kept) if keep else verts


def volume(verts, faces):
    """the signed volume of a closed mesh, in float64"""
    v = np.asarray(verts, dtype=np.float64)[np.asarray(faces)]
    return float(np.einsum('ij,ij->i', v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def roughness(verts, faces):
    """the mean squared length of the umbrella residual (neighbour mean - vertex) over the vertices that have a neighbour, in float64"""
    v = np.asarray(verts, dtype=np.float64)
    start, nbr, _ = adjacency(faces, len(v))
    r = [np.sum((v[nbr[start[i]:start[i + 1]]].mean(0) - v[i]) ** 2) for i in range(len(v)) if start[i + 1] > start[i]]
    return float(np.mean(r))


# ------------------------------------------------------------------------------------------------ meshes
TETRA_F = [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]]


@functools.lru_cache(maxsize=None)
def sphere(levels=3):
    """the octahedron subdivided `levels` times onto the unit sphere, outward windings: 3 -> 258 vertices, 512 faces (closed, manifold)"""
    v = [(1.0, 0, 0), (-1.0, 0, 0), (0, 1.0, 0), (0, -1.0, 0), (0, 0, 1.0), (0, 0, -1.0)]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(levels):
        mid, g = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = (np.array(v[a]) + np.array(v[b])) / 2
                v.append(tuple(p / np.linalg.norm(p)))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = g
    return np.array(v, dtype=np.float64), np.array(f, dtype=np.int64)


def patch(n=6):
    """an open n x n grid of vertices, two triangles a square: 6 -> 36 vertices, 50 faces, 20 rim vertices -> (xyz float64, faces, rim)"""
    ij = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing='ij'), -1).reshape(-1, 2)
    xyz = np.concatenate([ij, np.sin(ij[:, :1] * 1.3) * np.cos(ij[:, 1:] * 0.7)], 1).astype(np.float64)
    f = []
    for i in range(n - 1):
        for j in range(n - 1):
            a, b, c, d = i * n + j, (i + 1) * n + j, i * n + j + 1, (i + 1) * n + j + 1
            f += [(a, b, c), (c, b, d)]
    rim = np.array([k for k, (i, j) in enumerate(ij.tolist()) if i in (0, n - 1) or j in (0, n - 1)])
    return xyz, np.array(f, dtype=np.int64), rim


def noisy_sphere():
    """the 258-vertex sphere with 3 % radial noise"""
    v, f = sphere(3)
    return (v * (1 + 0.03 * np.random.default_rng(0).standard_normal(len(v)))[:, None]).astype(F32), f


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (verts [nv,3] float32, faces [nf,3] int64): the smallest meshes at which each part of the definition can go wrong.  The
    connectivity is what matters; the coordinates are seeded random float32 in [0, 191) (grid units of the largest mesh grid), at which
    almost every operation of a pass rounds, so that a different order, width or contraction shows in the bits."""
    s1 = sphere(1)[1]                                                    # 18 vertices, 32 faces, closed
    fan = [[0, 1 + i, 1 + (i + 1) % 600] for i in range(600)]            # the hub has 600 neighbours, every rim vertex 3
    meshes = {
        'tetra': (4, TETRA_F),
        'sphere258': (258, sphere(3)[1]),                                # crosses a block of 256 threads
        'patch6': (36, patch(6)[1]),                                     # open: the rim is pinned
        'duplicate_faces': (18, np.concatenate([s1, s1[3:5], s1[7:8]])),             # edges named 3 and 4 times
        'opposite_windings': (18, np.concatenate([s1, s1[10:12, ::-1]])),
        'two_sided_patch': (36, np.concatenate([patch(6)[1], patch(6)[1][:, ::-1]])),       # every rim edge named twice: nothing is pinned
        'three_faces_one_edge': (5, TETRA_F + [[0, 1, 4]]),              # a fin on the closed tetrahedron: 0, 1, 4 pinned, 2, 3 free
        'face_a_a_b': (20, np.concatenate([s1, [[18, 18, 19], [3, 3, 7], [5, 5, 5]]])),     # 18 - 19 named twice: interior, a pair of free vertices
        'unreferenced_vertex': (7, np.array([0, 1, 3, 4])[np.array(TETRA_F)]),       # 2, 5 and the last vertex have no neighbour
        'fan600': (601, fan),                                            # the rim is a boundary loop: only the hub moves, by a sum of 600
        'fan600_two_hubs': (602, np.array(fan + [[601, 1 + (i + 1) % 600, 1 + i] for i in range(600)])),      # closed: the rim (degree 4) is free
    }
    rng = np.random.default_rng(7)
    return {k: ((rng.random((nv, 3)) * 191).astype(F32), np.asarray(f, dtype=np.int64).reshape(-1, 3)) for k, (nv, f) in meshes.items()}


SETTINGS = ((LAM, MU), (1.0, -1.0), (LAM, 0.0))                          # the defaults, the ends of both ranges, plain Laplacian
ITERATIONS = (1, 2, 7)


@functools.lru_cache(maxsize=None)
def expected(name, lam, mu):
    """{iterations: verts'} for ITERATIONS, computed once per (mesh, setting) and shared; the arrays are not to be written"""
    v, f = cases()[name]
    return smooth(v, f, max(ITERATIONS), lam, mu, keep=ITERATIONS)[1]
