"""Plain-numpy restatement of the mesh clean-up of include/ln3d_meshclean.h (csrc/mesh.hip: ln3d_mesh_components, ln3d_mesh_component_counts,
ln3d_mesh_mark, ln3d_mesh_gather), no GPU, and the graphs and fields that tests/test_mesh_clean_cpu.py and tests/test_mesh_clean_gpu.py share.
Everything is integer work, so every comparison against it is an equality.

Definitions (the header's): two vertices are connected when a face names both; label[v] = the smallest vertex index of v's component; a
vertex that no face names is its own component; nvert[r] / nface[r] = vertices with label r / faces whose first vertex has label r;
best = max over components with a face of (nface << 32) | (0x7fffffff - r); a component survives when nface >= min_faces and, for
keep = 'largest', r is the root packed in best."""
import functools

import numpy as np

import mesh_refs as R


def labels(faces, nv):
    """faces [nf,3] ints in [0, nv) -> label [nv] int32.  Sequential union-find; the smaller root always becomes the parent, so a root is the
    smallest index of its tree."""
    parent = list(range(nv))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r
    for a, b, c in np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist():
        for u, v in ((a, b), (b, c)):
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)
    return np.array([find(v) for v in range(nv)], dtype=np.int32)


def counts(faces, label):
    """-> (nvert [nv] int32, nface [nv] int32, best python int)"""
    faces, nv = np.asarray(faces, dtype=np.int64).reshape(-1, 3), len(label)
    nvert = np.bincount(label, minlength=nv).astype(np.int32)
    nface = np.bincount(label[faces[:, 0]], minlength=nv).astype(np.int32)
    best = max([(int(nface[r]) << 32) | (0x7fffffff - int(r)) for r in np.flatnonzero(nface)], default=0)
    return nvert, nface, best


def best_root(best):
    return 0x7fffffff - (best & 0xffffffff)


def select(faces, label, nface, best, keep='all', min_faces=0):
    """-> (keep_v [nv] int32, keep_f [nf] int32)"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = nface[label].astype(np.int64) >= min_faces
    if keep == 'largest':
        ok &= label == best_root(best)
    else:
        assert keep == 'all'
    keep_v = ok.astype(np.int32)
    return keep_v, keep_v[faces[:, 0]]


def compact(verts, faces, keep_v, keep_f):
    """-> (verts' [nv',3], faces' [nf',3] int64): survivors in their order, faces renumbered"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    new = np.cumsum(keep_v.astype(np.int64)) - 1
    return np.asarray(verts)[keep_v != 0], new[faces[keep_f != 0]]


def clean(verts, faces, keep='all', min_faces=0):
    lab = labels(faces, len(verts))
    _, nface, best = counts(faces, lab)
    return compact(verts, faces, *select(faces, lab, nface, best, keep, min_faces))


def scipy_labels(faces, nv):
    """the same labels from scipy.sparse.csgraph.connected_components (component ids -> the smallest member)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    _, comp = connected_components(coo_matrix((np.ones(len(e), np.int8), (e[:, 0], e[:, 1])), shape=(nv, nv)), directed=False)
    low = np.full(comp.max() + 1, nv, dtype=np.int64)
    np.minimum.at(low, comp, np.arange(nv))
    return low[comp].astype(np.int32)


# ------------------------------------------------------------------------------------------------ graphs: (faces [nf,3] int64, nv)
def strip(n=4096):
    """n triangles (i, i+1, i+2): one component"""
    i = np.arange(n, dtype=np.int64)
    return np.stack([i, i + 1, i + 2], 1), n + 2


def interleaved_strips(m=500, loose=1000):
    """three strips of m triangles on the vertices 3k + s (s = 0, 1, 2) and `loose` vertices that no face names; nv is no multiple of 64"""
    k = np.arange(m, dtype=np.int64)
    f = np.concatenate([np.stack([3 * k + s, 3 * (k + 1) + s, 3 * (k + 2) + s], 1) for s in range(3)])
    nv = 3 * (m + 2) + loose
    assert nv % 64 != 0
    return f, nv


def fan(n=2048):
    """n faces (hub, i, i+1) around the hub nv - 1: every hook contends on the hub, which starts as every rim vertex's largest neighbour"""
    i = np.arange(n, dtype=np.int64)
    return np.stack([np.full(n, n + 1, dtype=np.int64), i, i + 1], 1), n + 2


def random_triples(nf=3000, nv=5000, seed=17):
    """components of mixed sizes; a few faces repeat an index (x, x, y), (x, y, x), (x, x, x)"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, nv, (nf, 3), dtype=np.int64)
    f[0, 1], f[1, 2], f[2, 1], f[2, 2] = f[0, 0], f[1, 0], f[2, 0], f[2, 0]
    return f, nv


def two_tetrahedra():
    """two closed tetrahedra, 0-3 and 3-6, that share vertex 3 only: one component"""
    t = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], dtype=np.int64)
    return np.concatenate([t, t + 3]), 7


def single_face():
    return np.array([[4, 1, 3]], dtype=np.int64), 6


GRAPHS = {'strip': strip, 'strips3': interleaved_strips, 'fan': fan, 'random': random_triples, 'tetra2': two_tetrahedra, 'one': single_face}


def renumber(faces, nv, seed):
    """the same graph under a random permutation of its vertex numbers (seed None: as built)"""
    if seed is None:
        return faces
    return np.random.default_rng(seed).permutation(nv).astype(np.int64)[faces]


RENUMBERINGS = (None, 1, 2, 3)


# ------------------------------------------------------------------------------------------------ fields
BLOB_G, BLOB_THR = 24, 10.0
BLOBS = (((7, 7, 7), 5.3), ((17, 8, 9), 3.2), ((9, 18, 16), 2.1), ((19, 19, 19), 1.5), ((3, 20, 4), 1.5))


def blob_field(G=BLOB_G):
    """sigma = max(-1, max_i 20 (1 - |p - c_i| / r_i)) on the G^3 grid (centres and radii scaled by G / 24), float64 cast to float32: five
    separate blobs at the level 10, two of them specks"""
    s = G / BLOB_G
    g = np.arange(G, dtype=np.float64)
    p = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1)
    sig = np.full((G, G, G), -1.0)
    for c, r in BLOBS:
        sig = np.maximum(sig, 20.0 * (1.0 - np.linalg.norm(p - np.array(c, dtype=np.float64) * s, axis=-1) / (r * s)))
    return sig.astype(np.float32)


# field, method -> (make, thr, expected vertices, faces, roots or their number, faces per root or the largest count and how many share it)
FIELDS = {
    ('blob', 'cubes'): dict(make=blob_field, thr=BLOB_THR, nv=222, nf=424, roots=[0, 6, 79, 162, 216], nface=[8, 248, 56, 104, 8]),
    ('blob', 'tetra'): dict(make=blob_field, thr=BLOB_THR, nv=634, nf=1248, roots=[0, 14, 258, 474, 620], nface=[24, 768, 144, 288, 24]),
    ('atlas', 'cubes'): dict(make=R.atlas_field, thr=0.0, nv=4608, nf=7796, ncomp=355, largest=44, tied=25),
    ('noise', 'cubes'): dict(make=R.noise_field, thr=0.0, nv=2325, nf=4144, ncomp=25, largest=3931, tied=1),
}


@functools.lru_cache(maxsize=None)
def welded(field, method):
    """the reference's welded mesh of a field: (verts [Nv,3] float64 in key order, faces [Nf,3] int64 in emission order), computed once"""
    spec = FIELDS[field, method]
    ref = R.ref_cubes(spec['make'](), spec['thr'], R.load_mc_table()) if method == 'cubes' else R.ref_tetra(spec['make'](), spec['thr'])
    _, faces, pos, _ = R.weld(ref)
    return pos, faces.astype(np.int64)


def check_figures(field, method, faces, nv):
    """assert the recorded figures of FIELDS on a welded mesh; -> (label, nvert, nface, best)"""
    spec = FIELDS[field, method]
    assert (nv, len(faces)) == (spec['nv'], spec['nf']), (nv, len(faces))
    lab = labels(faces, nv)
    nvert, nface, best = counts(faces, lab)
    roots = np.flatnonzero(lab == np.arange(nv))
    if 'roots' in spec:
        assert roots.tolist() == spec['roots'] and nface[roots].tolist() == spec['nface']
    else:
        assert len(roots) == spec['ncomp'] and int(nface.max()) == spec['largest'] and int((nface == nface.max()).sum()) == spec['tied']
    assert best >> 32 == int(nface.max()) and best_root(best) == int(np.flatnonzero(nface == nface.max())[0])      # ties: the smallest root
    return lab, nvert, nface, best
