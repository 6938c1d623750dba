"""Mesh extraction from the sigma grid (the export_mesh branch of render_video_given_triplane,
nsr/train_util_diffusion.py:208-248): iso-surface at sigma = 10 on the G^3 grid, vertices mapped to the +-0.45 box,
coloured by re-querying the tri-plane, rotated -90 degrees about x, written as .obj with per-vertex colours.
The surface is classic marching cubes (what the reference's `mcubes.marching_cubes` is; method='cubes', the default) or marching
tetrahedra (method='tetra'); both run on the GPU in two passes around a prefix sum and weld vertices by grid-edge id.
Opt-in clean-up (no reference counterpart; include/ln3d_meshclean.h): connected components of the welded mesh on the device, then only the
components with at least `min_faces` faces, or only the largest one, are kept - before the colour query, so discarded vertices cost nothing.
Opt-in simplification (no reference counterpart; include/ln3d_meshsimplify.h): vertex clustering on a lattice of `simplify_cell` grid units,
behind the clean-up and before the colour query.  Its representatives are the means of their cells or, opt-in again
(include/ln3d_meshquadric.h), the quadric-error minimisers of the faces that touch the cell, which keep creases and corners.
Opt-in texture baking (no reference counterpart; include/ln3d_meshbake.h): textured_mesh_from_grid adds a per-face texture atlas, UVs,
an .mtl and a .png to what mesh_from_grid makes; mesh_from_grid itself is unchanged.
Opt-in smoothing (no reference counterpart; include/ln3d_meshsmooth.h): Taubin's lambda | mu passes over the extracted (cleaned,
simplified) mesh in grid coordinates, before the box mapping, the colour / normal query and the bake.
Opt-in level-set snapping (no reference counterpart; include/ln3d_meshsnap.h): a damped Newton projection of the box-space vertices
onto sigma = thr, behind the smoothing and before the colour / normal query and the bake.
Opt-in binary export (no reference counterpart; include/ln3d_meshpack.h): mesh_format='ply' / 'glb' writes a binary little-endian
PLY or a binary glTF 2.0 instead of the .obj text; the records and buffer sections are packed on the device from the tensors the colour
query left there, and the host writes whole sections."""
import json
import math
import os
import struct
import zlib
from typing import NamedTuple

import numpy as np
import torch

from . import ops


KEEP_MODES = ('all', 'largest')


class MeshPost(NamedTuple):
    """The opt-in options of an exported mesh, with their defaults: the keywords of mesh_from_grid and textured_mesh_from_grid, which document
    them.  The layers above take them as the keywords of `keyword` (from_kwargs) and hand the record down; mesh_from_record makes a mesh from
    it.  A plain carrier: the values are checked by `check`, which the mesh functions call, so not unless a mesh is made."""
    normals: bool = False
    keep: str = 'all'
    min_faces: int = 0
    simplify_cell: float = 0.0
    simplify_placement: str = 'mean'
    smooth_iters: int = 0
    snap_iters: int = 0
    texture_size: int = 0
    mesh_format: str = 'obj'

    @staticmethod
    def keyword(field):
        """the pipeline keyword of a field: mesh_<field>, except that a field that already begins with mesh_ is its own keyword"""
        return field if field.startswith('mesh_') else 'mesh_' + field

    @classmethod
    def from_kwargs(cls, kw):
        """{keyword(field): value, ...} -> MeshPost; any other key is the TypeError of an unexpected keyword argument"""
        fields = {cls.keyword(f): f for f in cls._fields}
        for k in kw:
            if k not in fields:
                raise TypeError(f"got an unexpected keyword argument {k!r}")
        return cls(**{fields[k]: v for k, v in kw.items()})

    def check(self):
        """every value check of the nine options, before anything is extracted; each ValueError begins with the name of its field"""
        _clean_args(self.keep, self.min_faces)
        _simplify_cell(self.simplify_cell)
        _placement(self.simplify_placement)
        _smooth_args(self.smooth_iters)
        _snap_args(self.snap_iters)
        if self.texture_size != 0:
            _atlas_size(self.texture_size)
        if _mesh_format(self.mesh_format) == 'ply' and self.texture_size != 0:
            raise ValueError("mesh_format 'ply' carries vertex colours only: a textured mesh (texture_size) is written as 'obj' or 'glb'")


def _clean_args(keep, min_faces):
    if keep not in KEEP_MODES:
        raise ValueError(f"keep {keep!r}: expected one of {list(KEEP_MODES)}")
    if int(min_faces) != min_faces or min_faces < 0:
        raise ValueError(f"min_faces {min_faces!r}: expected a non-negative integer")
    return keep, int(min_faces)


def _check_verts(verts):
    if verts.dtype != torch.float32 or verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError(f"verts: expected a float32 [Nv, 3] tensor, got {verts.dtype} {tuple(verts.shape)}")


def _check_faces(faces, nv, check):
    """dtype and shape always; with check also every index in [0, nv) (ops.check_faces: one read-back)"""
    if check:
        ops.check_faces(faces, nv)
    elif faces.dtype != torch.int64 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces: expected an int64 [Nf, 3] tensor, got {faces.dtype} {tuple(faces.shape)}")


def _float32(x):
    """x as the float32 the kernels take, widened to a Python float; NaN when it is not a number"""
    try:
        return float(np.float32(x))
    except (TypeError, ValueError):
        return math.nan


def _empty(dev):
    return torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.long, device=dev)


def _compact(verts, faces, keep_v, keep_f):
    """the rows of verts and faces whose int32 mask is set, faces renumbered (ops.mesh_gather): two prefix sums and one read-back of the two
    surviving counts; no surviving face gives the empty mesh"""
    dev = verts.device
    vpre, fpre = torch.cumsum(keep_v.long(), 0), torch.cumsum(keep_f.long(), 0)
    nv_out, nf_out = torch.stack([vpre[-1], fpre[-1]]).tolist()
    if nf_out == 0:
        return _empty(dev)
    verts_out = torch.empty(nv_out, 3, device=dev)
    faces_out = torch.empty(nf_out, 3, dtype=torch.int64, device=dev)
    ops.mesh_gather(verts, faces, keep_v, vpre, keep_f, fpre, verts_out, faces_out, check=False)
    return verts_out, faces_out


def _label_and_count(faces, nv):
    """faces already through ops.check_faces -> (label, nvert, nface [nv] int32, best int64[1])"""
    dev = faces.device
    label, nvert, nface = (torch.empty(nv, dtype=torch.int32, device=dev) for _ in range(3))
    best = torch.empty(1, dtype=torch.int64, device=dev)
    ops.mesh_components(faces, nv, label, check=False)
    ops.mesh_component_counts(faces, label, nvert, nface, best, check=False)
    return label, nvert, nface, best


@torch.no_grad()
def mesh_components(faces, num_verts):
    """The diagnostic view of the connected components of a mesh: faces [Nf,3] int64 device, num_verts ->
    (label [Nv] int32: the smallest vertex index of every vertex's component, roots [R] int64 ascending: the labels that occur,
    nvert [R], nface [R] int32: vertices and faces of every root's component).  Two vertices are connected when a face names both; a vertex
    that no face names is a component of its own with no face.  Raises ValueError on a face index outside [0, num_verts)."""
    faces = faces.contiguous()
    ops.check_faces(faces, num_verts)
    dev = faces.device
    if num_verts == 0 or faces.shape[0] == 0:
        label = torch.arange(num_verts, dtype=torch.int32, device=dev)
        return label, label.long(), torch.ones_like(label), torch.zeros_like(label)
    label, nvert, nface, _ = _label_and_count(faces, num_verts)
    roots = torch.nonzero(label == torch.arange(num_verts, dtype=torch.int32, device=dev)).reshape(-1)
    return label, roots, nvert[roots], nface[roots]


@torch.no_grad()
def clean_mesh(verts, faces, keep='all', min_faces=0):
    """verts [Nv,3] f32, faces [Nf,3] int64 (device) -> (verts', faces') with only the surviving connected components: a component survives
    when it has at least `min_faces` faces and, for keep='largest', is the one with the most faces (ties: the one that holds the smallest
    vertex index).  Survivors keep their order, vertex coordinates their bits; faces are renumbered.  keep='all', min_faces=0 returns its
    arguments and launches nothing; an empty input, or one of which nothing survives, gives empty tensors.  Labelling, counting, marking
    and gathering are kernels (include/ln3d_meshclean.h); the two prefix sums and the one size read-back are torch's, as in
    extract_isosurface."""
    keep, min_faces = _clean_args(keep, min_faces)
    if keep == 'all' and min_faces == 0:
        return verts, faces
    _check_verts(verts)
    dev = verts.device
    nv, nf = verts.shape[0], faces.shape[0]
    if nv == 0 or nf == 0:
        return _empty(dev)
    verts, faces = verts.contiguous(), faces.contiguous()
    ops.check_faces(faces, nv)
    label, _, nface, best = _label_and_count(faces, nv)
    keep_v = torch.empty(nv, dtype=torch.int32, device=dev)
    keep_f = torch.empty(nf, dtype=torch.int32, device=dev)
    ops.mesh_mark(faces, label, nface, min_faces, keep == 'largest', best, keep_v, keep_f, check=False)
    return _compact(verts, faces, keep_v, keep_f)


SIMPLIFY_MAX_CELLS = 1 << 21                  # lattice cells per axis, and clusters, that a 63-bit key holds (include/ln3d_meshsimplify.h)


def _simplify_cell(cell):
    """cell as the float32 the kernels divide by; None / 0 -> 0.0 (off); ValueError when it is negative, not finite or not a number"""
    if cell is None:
        return 0.0
    try:
        c = float(np.float32(cell))
    except (TypeError, ValueError):
        raise ValueError(f"simplify_cell {cell!r}: expected a positive finite number, or 0 / None for no simplification") from None
    if not math.isfinite(c) or c < 0 or (c == 0 and cell != 0):
        raise ValueError(f"simplify_cell {cell!r}: expected a positive finite number (in float32), or 0 / None for no simplification")
    return c


PLACEMENTS = ('mean', 'quadric')
QUADRIC_EPS = 1e-3                            # the regularisation of the quadric placement, as a share of the trace: a choice, not a measurement


def _placement(placement, eps=QUADRIC_EPS):
    """-> (placement, eps as the float32 the kernel multiplies by); ValueError when placement is not one of PLACEMENTS or eps (in float32)
    lies outside (0, 1]"""
    if not isinstance(placement, str) or placement not in PLACEMENTS:
        raise ValueError(f"simplify_placement {placement!r}: expected one of {list(PLACEMENTS)}")
    e = _float32(eps)
    if not 0.0 < e <= 1.0:
        raise ValueError(f"quadric_eps {eps!r}: expected a number in (0, 1] (in float32)")
    return placement, e


def _simplify_clusters(verts, faces, cell, origin, check):
    """the checks and the first three stages of simplify_mesh, cell > 0 -> None for an empty input, else (verts, faces contiguous, origin as
    three float32, uniq [nc] int64: the clusters' cell keys ascending, rep [nc,3]: the means, cfaces [nf,3], fkey [nf])"""
    _check_verts(verts)
    if origin is not None:
        origin = np.asarray(origin, dtype=np.float32).reshape(-1)
        if origin.shape != (3,) or not np.isfinite(origin).all():
            raise ValueError(f"origin {origin!r}: expected three finite numbers")
    dev = verts.device
    nv, nf = verts.shape[0], faces.shape[0]
    verts, faces = verts.contiguous(), faces.contiguous()
    _check_faces(faces, nv, check)
    if nv == 0 or nf == 0:
        return None
    box = torch.cat([verts.amin(0), verts.amax(0), torch.isfinite(verts).all().float().reshape(1)]).cpu().numpy()      # one read-back
    if not box[6]:
        raise ValueError("verts: a coordinate is not finite")
    lo, hi = box[:3], box[3:6]
    if origin is None:
        origin = lo
    c32 = np.float32(cell)
    with np.errstate(over='ignore', invalid='ignore'):
        qlo, qhi = np.floor((lo - origin) / c32), np.floor((hi - origin) / c32)            # the kernel's arithmetic, monotone in x
    if not (qlo >= 0).all() or not (qhi < SIMPLIFY_MAX_CELLS).all():
        raise ValueError(f"verts span lattice cells {qlo.tolist()} to {qhi.tolist()} at cell {cell}: every axis must stay in [0, 2^21)")
    key = torch.empty(nv, dtype=torch.int64, device=dev)
    ops.simplify_keys(verts, origin, cell, key)
    uniq, cluster, members = torch.unique(key, return_inverse=True, return_counts=True)
    nc = uniq.shape[0]
    order = torch.sort(cluster, stable=True)[1]
    start = torch.zeros(nc + 1, dtype=torch.int64, device=dev)
    torch.cumsum(members, 0, out=start[1:])
    rep = torch.empty(nc, 3, device=dev)
    ops.simplify_mean(verts, order, start, rep, check=False)
    cfaces = torch.empty(nf, 3, dtype=torch.int64, device=dev)
    fkey = torch.empty(nf, dtype=torch.int64, device=dev)
    ops.simplify_faces(faces, cluster, nc, cfaces, fkey, check=False)
    return verts, faces, origin, uniq, rep, cfaces, fkey


def _quadric_place(verts, faces, cfaces, rep, origin, cell, uniq, eps):
    """-> (rep_quadric [nc,3], placed [nc] int32) of include/ln3d_meshquadric.h: the pair keys, their sort, the row pointers
    (searchsorted, as _adjacency) and the placement; two launches, no read-back"""
    dev = verts.device
    nc = rep.shape[0]
    pair_key = torch.empty(3 * faces.shape[0], dtype=torch.int64, device=dev)
    ops.quadric_pairs(cfaces, nc, pair_key, check=False)
    pair_key = torch.sort(pair_key)[0]                                 # distinct keys but for the INT64_MAX entries, which end up last
    start = torch.searchsorted(pair_key >> 31, torch.arange(nc + 1, device=dev))
    out = torch.empty_like(rep)
    placed = torch.empty(nc, dtype=torch.int32, device=dev)
    ops.quadric_place(verts, faces, pair_key, start, rep, origin, cell, uniq, eps, out, placed, check=False)
    return out, placed


@torch.no_grad()
def simplify_mesh(verts, faces, cell, origin=None, check=True, placement='mean', quadric_eps=QUADRIC_EPS):
    """verts [Nv,3] f32, faces [Nf,3] int64 (device) -> (verts', faces'): the mesh simplified by vertex clustering on a lattice of cubic cells
    of edge `cell` whose corner is `origin` (three numbers; None: the per-axis minimum of verts).  The definition (include/
    ln3d_meshsimplify.h; every output is unique, nothing depends on scheduling):
      - a vertex falls into cell q_a = floor((x_a - origin_a) / cell) per axis, in float32;
      - every occupied cell becomes one vertex, the float32 mean of its members summed in ascending vertex index;
      - a face whose corners fall into fewer than three cells is dropped; of the faces that name the same three cells (in any order or
        winding) the one with the smallest index survives, with its own corner order;
      - cells that no surviving face names are dropped; vertices come out in ascending (q_x, q_y, q_z), faces in their input order.
    placement='quadric' (opt-in; include/ln3d_meshquadric.h) changes the second rule only: a cell's vertex is put where the summed
    squared distance to the planes of ALL input faces with a corner in the cell (area-squared weights, collapsing and duplicate faces
    included) is least, solved in float32 about the mean with the regularisation quadric_eps * trace, and accepted when it is finite and
    lies in the closed cell; a cell whose solution is refused keeps the mean's bits.  Faces, vertex count and vertex order are exactly those
    of 'mean'; creases and corners, which the mean chamfers by up to about 0.4 cells, are kept to about 1e-3 cells on a box.  It adds two
    launches and one sort between the mean and the compaction; 'mean' launches nothing new.
    cell None or 0 returns its arguments and launches nothing; an empty input, or one of which nothing survives, gives empty tensors.
    Raises ValueError on a bad dtype or shape, a face index out of range, a non-finite vertex or origin, a cell that is not finite or is
    negative, a mesh that spans 2^21 cells or more on an axis (or reaches below an explicit origin), a placement that is neither 'mean' nor
    'quadric' and a quadric_eps outside (0, 1] - the last two before anything is launched.
    NOT promised: the result can have non-manifold edges and folded-over triangles, under 'mean' convex regions are pulled inward by
    O(cell^2 * curvature), and components that come within a cell of each other can merge.  'quadric' is a feature-preserving option, not a
    better default: on smooth or noisy regions it is NOT closer to the surface than the mean (sphere of radius 60, cell 3: median distance
    0.015 against 0.010; with sigma = 0.3 vertex noise 0.17 against 0.11), folds and non-manifold edges remain, bevels that marching cubes
    already cut at grid resolution are only partly recovered, and quadric_eps trades crease sharpness against noise amplification (its
    default 1e-3 is a choice, not a measurement).  Smoothing is smooth_mesh's.
    The stages are kernels; torch supplies unique (clusters), the stable sorts (members per cluster, duplicate faces), the pair-key sort and
    searchsorted of 'quadric', the prefix sums and the read-backs: the face-index check, the bounds and finiteness of verts, the cluster count
    (inside unique), the surviving counts.
    check=False skips the face-index check and its read-back: for a caller whose faces index verts by construction (extract_isosurface, whose
    faces come out of its own weld and clean-up); dtype and shape are still checked."""
    placement, quadric_eps = _placement(placement, quadric_eps)
    cell = _simplify_cell(cell)
    if cell == 0.0:
        return verts, faces
    dev = verts.device
    front = _simplify_clusters(verts, faces, cell, origin, check)
    if front is None:
        return _empty(dev)
    verts, faces, origin, uniq, rep, cfaces, fkey = front
    nc, nf = rep.shape[0], faces.shape[0]
    if placement == 'quadric':
        rep = _quadric_place(verts, faces, cfaces, rep, origin, cell, uniq, quadric_eps)[0]
    sorted_key, perm = torch.sort(fkey, stable=True)
    keep_f = torch.empty(nf, dtype=torch.int32, device=dev)
    ops.simplify_first(sorted_key, perm, keep_f, check=False)
    keep_v = torch.empty(nc, dtype=torch.int32, device=dev)
    ops.simplify_used(cfaces, keep_f, keep_v, check=False)
    return _compact(rep, cfaces, keep_v, keep_f)


@torch.no_grad()
def simplify_placement(verts, faces, cell, origin=None, eps=QUADRIC_EPS):
    """The diagnostic view of the two placements of simplify_mesh, before the compaction: verts [Nv,3] f32, faces [Nf,3] int64 (device),
    cell > 0 -> (rep_mean [Nc,3] f32, rep_quadric [Nc,3] f32, placed [Nc] int32, cell_key [Nc] int64) for every occupied lattice cell in
    ascending key q_x << 42 | q_y << 21 | q_z.  placed[k] = 1 where the quadric solution was accepted; where it is 0, rep_quadric[k] has
    rep_mean[k]'s bits.  An empty input gives empty tensors.  Raises what simplify_mesh raises, and ValueError for cell None or 0."""
    _, eps = _placement('quadric', eps)
    cell = _simplify_cell(cell)
    if cell == 0.0:
        raise ValueError("cell: expected a positive finite number (there are no clusters without a lattice)")
    dev = verts.device
    front = _simplify_clusters(verts, faces, cell, origin, True)
    if front is None:
        return (torch.zeros(0, 3, device=dev), torch.zeros(0, 3, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                torch.zeros(0, dtype=torch.int64, device=dev))
    verts, faces, origin, uniq, rep, cfaces, _ = front
    quad, placed = _quadric_place(verts, faces, cfaces, rep, origin, cell, uniq, eps)
    return rep, quad, placed, uniq


# ------------------------------------------------------------------ smoothing (include/ln3d_meshsmooth.h)
SMOOTH_MAX_ITERS = 1000
SMOOTH_LAMBDA, SMOOTH_MU = 0.5, -0.53


def _smooth_args(iterations, lam=SMOOTH_LAMBDA, mu=SMOOTH_MU):
    """-> (iterations as an int, None -> 0; lam and mu as the float32 values the kernel multiplies by); ValueError when iterations is no
    integer in [0, 1000], lam (in float32) lies outside (0, 1] or mu outside [-1, 0]"""
    if iterations is None:
        iterations = 0
    try:
        ok = not isinstance(iterations, bool) and int(iterations) == iterations and 0 <= iterations <= SMOOTH_MAX_ITERS
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"smooth_iters {iterations!r}: expected an integer in [0, {SMOOTH_MAX_ITERS}], or None for no smoothing")
    lam32, mu32 = _float32(lam), _float32(mu)
    if not 0.0 < lam32 <= 1.0:
        raise ValueError(f"smooth_lambda {lam!r}: expected a number in (0, 1] (in float32)")
    if not -1.0 <= mu32 <= 0.0:
        raise ValueError(f"smooth_mu {mu!r}: expected a number in [-1, 0] (in float32); 0 is plain Laplacian smoothing")
    return int(iterations), lam32, mu32


def _adjacency(faces, nv):
    """faces [Nf >= 1, 3] int64 contiguous, already through ops.check_faces, nv >= 1 -> (start, nbr, pinned) of mesh_adjacency"""
    dev = faces.device
    nf = faces.shape[0]
    pinned = torch.zeros(nv, dtype=torch.int32, device=dev)
    key = torch.empty(3 * nf, dtype=torch.int64, device=dev)
    ops.smooth_edge_keys(faces, nv, key, check=False)
    edge, count = torch.unique(key, return_counts=True)                # ascending: a -1 (the a == b edges) comes first
    skip = int(edge[0] < 0)                                            # one read-back
    edge, count = edge[skip:], count[skip:]
    ne = edge.shape[0]
    if ne == 0:                                                        # every face is (a, a, a): nobody has a neighbour
        return torch.zeros(nv + 1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev), pinned
    dkey = torch.empty(2 * ne, dtype=torch.int64, device=dev)
    ops.smooth_halfedges(edge, count, nv, dkey, pinned, check=False)
    dkey = torch.sort(dkey)[0]                                         # distinct keys: ascending in (src, dst)
    nbr = (dkey & 0xffffffff).to(torch.int32)
    start = torch.searchsorted(dkey >> 32, torch.arange(nv + 1, device=dev))
    return start, nbr, pinned


@torch.no_grad()
def mesh_adjacency(faces, num_verts):
    """The diagnostic view of what smooth_mesh walks: faces [Nf,3] int64 device, num_verts -> (start [Nv+1] int64, nbr [2E] int32,
    pinned [Nv] int32).  nbr[start[i]:start[i+1]] are the distinct vertices that share an edge with vertex i, ascending (an edge with two equal
    ends is ignored); E is the number of distinct undirected edges.  pinned[i] is 1 when i is an end of a boundary edge - one that exactly one
    face corner pair names, duplicate faces and opposite windings counted.  Raises ValueError on a face index outside [0, num_verts)."""
    faces = faces.contiguous()
    ops.check_faces(faces, num_verts)
    dev = faces.device
    if num_verts == 0 or faces.shape[0] == 0:
        return (torch.zeros(num_verts + 1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                torch.zeros(num_verts, dtype=torch.int32, device=dev))
    return _adjacency(faces, num_verts)


@torch.no_grad()
def smooth_mesh(verts, faces, iterations, lam=SMOOTH_LAMBDA, mu=SMOOTH_MU, check=True):
    """verts [Nv,3] f32, faces [Nf,3] int64 (device) -> (verts', faces): the mesh after `iterations` iterations of Taubin's lambda | mu
    smoothing with uniform weights.  The definition (include/ln3d_meshsmooth.h; all arithmetic float32, every output is unique,
    nothing depends on scheduling):
      - every face contributes its three undirected edges {a, b}; an edge with a == b is ignored; duplicate faces and opposite windings
        contribute the same edge again;
      - the neighbours of vertex i are the DISTINCT vertices that share an edge with it, in ascending index j_1 < ... < j_d;
      - an edge named by exactly one face corner pair is a boundary edge and both its ends are pinned; a pinned vertex never moves, and
        neither does one with d = 0; edges named twice or more, non-manifold ones included, are interior;
      - one pass with the factor f, per axis, for a free vertex: s = x[j_1], then s = fl(s + x[j_k]) for k = 2 .. d; m = fl(s / fl32(d));
        e = fl(m - x_i); x_i' = fl(x_i + fl(f * e)) - every operation rounded once, no fused multiply-add; every pass reads the previous
        pass's coordinates only;
      - one iteration is a pass with lam, then a pass with mu; mu = 0 skips the second pass (plain Laplacian smoothing, which shrinks).
    Faces, vertex count and vertex order are unchanged; `faces` is returned as given.  iterations None or 0 returns its arguments and
    launches nothing, and so does a mesh without vertices or faces (nothing can move).  The adjacency is built once per call
    (mesh_adjacency); each pass is one launch.
    Raises ValueError on a bad dtype or shape, a face index out of range, a non-finite vertex (one read-back), iterations not an integer in
    [0, 1000], lam not in (0, 1] and mu not in [-1, 0].
    NOT promised: the weights are uniform, not cotangent, so vertices also drift along the surface; vertices move off the level set; features
    sharper than the pass band are rounded; the volume is not preserved exactly; boundary loops stay jagged, because they are pinned.
    check=False skips the face-index check and its read-back, for a caller whose faces index verts by construction (_coloured_mesh)."""
    iterations, lam, mu = _smooth_args(iterations, lam, mu)
    if iterations == 0:
        return verts, faces
    _check_verts(verts)
    nv, nf = verts.shape[0], faces.shape[0]
    cverts, cfaces = verts.contiguous(), faces.contiguous()
    _check_faces(cfaces, nv, check)
    if nv == 0 or nf == 0:
        return verts, faces
    if not bool(torch.isfinite(cverts).all()):                          # one read-back
        raise ValueError("verts: a coordinate is not finite")
    start, nbr, pinned = _adjacency(cfaces, nv)
    if nbr.shape[0] == 0:
        return verts, faces
    cur, spare = cverts, [torch.empty_like(cverts), torch.empty_like(cverts)]
    for _ in range(iterations):
        for factor in (lam, mu) if mu != 0.0 else (lam,):
            out = spare[0] if cur is not spare[0] else spare[1]          # never the buffer the pass reads
            ops.smooth_step(cur, start, nbr, pinned, factor, out, check=False)
            cur = out
    return cur, faces


# ------------------------------------------------------------------ level-set snapping (include/ln3d_meshsnap.h)
SNAP_MAX_ITERS = ops.SNAP_MAX_ITERS


def _snap_args(iterations, tol=None, max_move=None):
    """-> (iterations as an int, None -> 0; tol or None; max_move in grid units as a float, or None); ValueError when iterations
    is no integer in [0, 64], tol is given and not a finite number >= 0, or max_move is given and not a finite number > 0"""
    if iterations is None:
        iterations = 0
    try:
        ok = not isinstance(iterations, bool) and int(iterations) == iterations and 0 <= iterations <= SNAP_MAX_ITERS
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"snap_iters {iterations!r}: expected an integer in [0, {SNAP_MAX_ITERS}], or None for no snapping")
    if tol is not None:
        t = _float32(tol)
        if not (math.isfinite(t) and t >= 0):
            raise ValueError(f"snap_tol {tol!r}: expected a finite number >= 0 (in float32), or None for 1e-3 * max(1, |thr|)")
    if max_move is not None:
        m = _float32(max_move)
        if not (math.isfinite(m) and m > 0):
            raise ValueError(f"snap_max_move {max_move!r}: expected a finite number > 0 of grid cells (in float32), or None for max(1, simplify_cell)")
        max_move = m
    return int(iterations), tol, max_move


@torch.no_grad()
def snap_mesh(decoder, planes_channel_last, verts_box, level, iterations, tol=None, max_step=None, max_dist=None):
    """verts_box [Nv,3] f32 (device, box / world coordinates), planes_channel_last [1,3,H,W,32] of ONE sample, decoder: the VAE decoder
    module (its snap_points seam) -> (verts' [Nv,3], {'residual' [Nv] f32, 'state' [Nv] int32, 'evals' [Nv] int32}): every vertex put
    onto sigma = level by at most `iterations` iterations of the damped Newton projection of include/ln3d_meshsnap.h, one fused
    launch with per-lane early exit.  verts' is the best iterate seen (|residual| never exceeds the input's), never farther than max_dist
    from its start, each step at most max_step long (world units); residual = sigma(verts') - level as the kernel evaluates it; state 0 =
    |residual| <= tol, 1 = out of iterations, 2 = stalled.  Vertex count and order never change, so faces stay valid as they are.
    The defaults are choices, not measurements: tol None = 1e-3 * max(1, |level|); max_dist None = 0.02; max_step None = max_dist / 2.
    iterations None or 0, or a mesh without vertices, returns verts_box itself with empty-handed diagnostics (residual None) and launches
    nothing.  Raises ValueError on a bad dtype or shape, iterations not an integer in [0, 64], tol < 0, max_step <= 0, max_dist < 0 or
    any of them not finite.
    NOT promised: only vertices are put on the level set, triangle interiors are not; vertices move independently, so faces can fold or
    flip and thin sheets can collapse onto each other; a vertex may land on a different sheet within max_dist; the field's gradient jumps
    at texel centres, so convergence is not guaranteed - `state` says which vertices did not converge; and snapping partly undoes the
    tangential regularity that smoothing produced."""
    iterations, tol, _ = _snap_args(iterations, tol)
    _check_verts(verts_box)
    if max_dist is None:
        max_dist = 0.02
    if max_step is None:
        max_step = max_dist / 2
    nothing = {'residual': None, 'state': None, 'evals': None}
    if iterations == 0 or verts_box.shape[0] == 0:
        return verts_box, nothing
    r = decoder.snap_points(planes_channel_last, verts_box[None], level, iterations, tol=tol, max_step=max_step, max_dist=max_dist)
    return r['points'][0], {k: r[k][0] for k in nothing}


@torch.no_grad()
def extract_isosurface(sigma, thr=10.0, method='cubes', keep='all', min_faces=0, simplify_cell=0.0, simplify_placement='mean'):
    """sigma [G,G,G] f32 device -> (verts [Nv,3] in grid coordinates, faces [Nf,3] int64).  Faces keep the emission order
    (cells in x-major order, the case table's triangle order inside a cell).  keep / min_faces (opt-in): clean_mesh on the welded result.
    simplify_cell (opt-in, in grid units): simplify_mesh with origin (0, 0, 0) after the weld and after the clean-up, so floaters are judged
    on the full-density mesh.  simplify_placement (opt-in): simplify_mesh's placement, 'mean' or 'quadric'; it changes coordinates only."""
    keep, min_faces = _clean_args(keep, min_faces)
    simplify_cell = _simplify_cell(simplify_cell)
    simplify_placement = _placement(simplify_placement)[0]
    count, emit = {'cubes': (ops.mcubes_count, ops.mcubes_emit), 'tetra': (ops.mesh_count, ops.mesh_emit)}[method]
    G = sigma.shape[0]
    dev = sigma.device
    sigma = sigma.contiguous().float()
    ncell = (G - 1) ** 3
    counts = torch.empty(ncell, dtype=torch.int32, device=dev)
    count(sigma, G, thr, counts)
    offs = torch.cumsum(counts.long(), 0)
    ntri = int(offs[-1])
    if ntri == 0:
        return _empty(dev)
    pos = torch.empty(ntri * 3, 3, device=dev)
    key = torch.empty(ntri * 3, dtype=torch.int64, device=dev)
    emit(sigma, G, thr, offs, pos, key)
    uniq, inv = torch.unique(key, return_inverse=True)                # weld by grid-edge id
    verts = torch.empty(uniq.shape[0], 3, device=dev)
    verts[inv] = pos                                                   # identical bits for every copy of a vertex
    faces = inv.view(ntri, 3)
    ok = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    verts, faces = clean_mesh(verts, faces[ok], keep, min_faces)
    place = dict(placement=simplify_placement) if simplify_placement != 'mean' else {}
    return simplify_mesh(verts, faces, simplify_cell, (0.0, 0.0, 0.0), check=False, **place)      # faces are the weld's own: in range by construction


def rotation_matrix_x(deg):
    a = math.radians(deg)
    return np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]], dtype=np.float32)


def _write_v(fh, v, c):
    for i in range(v.shape[0]):
        fh.write('v %.6f %.6f %.6f %.4f %.4f %.4f\n' % (v[i, 0], v[i, 1], v[i, 2], c[i, 0], c[i, 1], c[i, 2]))


def _write_vn(fh, n):
    for i in range(n.shape[0]):
        fh.write('vn %.6f %.6f %.6f\n' % (n[i, 0], n[i, 1], n[i, 2]))


def write_obj(path, v, f, c, n=None):
    """Wavefront .obj with per-vertex colours (what trimesh.Trimesh(vertex_colors=...).export(path, 'obj') writes).
    n [Nv,3]: per-vertex normals, written as `vn` records behind the vertices, every face corner then names its own vertex's normal
    (`f a//a b//b c//c`).  They are the outward normals -grad sigma / |grad sigma| of the density field (0 0 0 where it has none) and do
    NOT depend on the winding of the faces."""
    with open(path, 'w') as fh:
        _write_v(fh, v, c)
        if n is None:
            for t in f:
                fh.write('f %d %d %d\n' % (t[0] + 1, t[1] + 1, t[2] + 1))
            return
        _write_vn(fh, n)
        for t in f:
            fh.write('f %d//%d %d//%d %d//%d\n' % (t[0] + 1, t[0] + 1, t[1] + 1, t[1] + 1, t[2] + 1, t[2] + 1))


MATERIAL = 'baked'                            # the one material of a textured export


def write_obj_textured(path, v, f, c, uv, n=None):
    """`path` = <stem>.obj with the texture coordinates uv [Nf,3,2] of atlas_uvs, and <stem>.mtl beside it, which names <stem>.png (write_png
    writes that).  The .obj holds, in order: `mtllib <stem>.mtl`; the `v` records of write_obj, byte for byte; its `vn` records when n is
    given; 3 Nf `vt` records, corner j of face i being record 3 i + j + 1 (no two faces share one: every face has its own patch);
    `usemtl baked`; the faces as `f a/t b/t c/t`, or `f a/t/a b/t/b c/t/c` with normals.  The .mtl holds `newmtl baked`, `Kd 1 1 1`,
    `map_Kd <stem>.png`.  An empty mesh writes both files without records."""
    stem = os.path.splitext(str(path))[0]
    name = os.path.basename(stem)
    with open(path, 'w') as fh:
        fh.write('mtllib %s.mtl\n' % name)
        _write_v(fh, v, c)
        if n is not None:
            _write_vn(fh, n)
        for u in np.asarray(uv).reshape(-1, 2):
            fh.write('vt %.8f %.8f\n' % (u[0], u[1]))
        fh.write('usemtl %s\n' % MATERIAL)
        for i, t in enumerate(f):
            a, b, d = t[0] + 1, t[1] + 1, t[2] + 1
            if n is None:
                fh.write('f %d/%d %d/%d %d/%d\n' % (a, 3 * i + 1, b, 3 * i + 2, d, 3 * i + 3))
            else:
                fh.write('f %d/%d/%d %d/%d/%d %d/%d/%d\n' % (a, 3 * i + 1, a, b, 3 * i + 2, b, d, 3 * i + 3, d))
    with open(stem + '.mtl', 'w') as fh:
        fh.write('newmtl %s\nKd 1 1 1\nmap_Kd %s.png\n' % (MATERIAL, name))


def png_bytes(tex):
    """tex [H,W,3] uint8 -> the bytes of an 8-bit RGB PNG (standard library only: one zlib stream, filter 0 on every row).  The rows are
    FLIPPED: the top row of the image is tex[H - 1], because v = 0 is the bottom of a texture and row 0 of the atlas holds v = 0.5 / H."""
    tex = np.ascontiguousarray(tex)
    if tex.dtype != np.uint8 or tex.ndim != 3 or tex.shape[2] != 3 or tex.shape[0] < 1 or tex.shape[1] < 1:
        raise ValueError(f"tex: expected a uint8 [H, W, 3] array, got {tex.dtype} {tex.shape}")
    h, w = tex.shape[:2]
    rows = np.zeros((h, 1 + 3 * w), np.uint8)                           # a filter byte of 0 in front of every row
    rows[:, 1:] = tex[::-1].reshape(h, 3 * w)

    def chunk(kind, data):
        return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0))
            + chunk(b'IDAT', zlib.compress(rows.tobytes(), 6)) + chunk(b'IEND', b''))


def write_png(path, tex):
    """tex [H,W,3] uint8 -> `path`, the PNG of png_bytes"""
    data = png_bytes(tex)
    with open(path, 'wb') as fh:
        fh.write(data)


# ------------------------------------------------------------------ binary export (include/ln3d_meshpack.h)
MESH_FORMATS = ('obj', 'ply', 'glb')
EXPORTER = 'ln3diff_amd'                      # the PLY comment and the glTF generator
GLB_MAX_BYTES = 1 << 32                       # a GLB states its length in 32 bits


def _mesh_format(fmt):
    """-> fmt; ValueError when it is not one of MESH_FORMATS"""
    if not isinstance(fmt, str) or fmt not in MESH_FORMATS:
        raise ValueError(f"mesh_format {fmt!r}: expected one of {list(MESH_FORMATS)}")
    return fmt


def _export_args(verts, faces, rgb, normal, check):
    """the device tensors a binary writer takes, contiguous -> (verts, faces, rgb, normal, rot9 on the device); ValueError on a bad dtype
    or shape and, with check, on a face index out of range (one read-back)"""
    _check_verts(verts)
    nv = verts.shape[0]
    verts, faces = verts.contiguous(), faces.contiguous()
    _check_faces(faces, nv, check)
    for name, t in (('rgb', rgb), ('normal', normal)):
        if t is not None and (t.dim() != 2 or tuple(t.shape) != (nv, 3)):
            raise ValueError(f"{name}: expected a [{nv}, 3] tensor, got {tuple(t.shape)}")
    rgb = rgb.float().contiguous()
    normal = normal.float().contiguous() if normal is not None else None
    rot9 = torch.from_numpy(rotation_matrix_x(-90).reshape(-1)).to(verts.device)
    return verts, faces, rgb, normal, rot9


def _host(t):
    """a packed section on the host, as the bytes a file takes: one copy"""
    return memoryview(t.cpu().numpy()).cast('B')


def _ply_header(nv, nf, normals):
    """the header of write_ply, every line ended by a newline"""
    head = ['ply', 'format binary_little_endian 1.0', 'comment ' + EXPORTER, 'element vertex %d' % nv] + ['property float ' + a for a in 'xyz']
    if normals:
        head += ['property float n' + a for a in 'xyz']
    head += ['property uchar ' + c for c in ('red', 'green', 'blue')] + ['element face %d' % nf, 'property list uchar int vertex_indices', 'end_header']
    return ('\n'.join(head) + '\n').encode('ascii')


@torch.no_grad()
def write_ply(path, verts_box, faces, rgb, normal=None, check=True):
    """A binary little-endian PLY with per-vertex colours, packed on the device (include/ln3d_meshpack.h).  verts_box [Nv,3] f32 in
    box coordinates, faces [Nf,3] int64, rgb [Nv,3] the query's colours, normal [Nv,3] the query's normals or None: DEVICE tensors.  What is
    written: the positions rotation_matrix_x(-90) @ verts_box evaluated as (R0 x + R1 y) + R2 z in float32 without fma, the normals by the
    same rule, the colours as trunc(clamp(c, 0, 1) * 255) - the values mesh_from_grid returns - and the indices as int32.  The header is
    `ply / format binary_little_endian 1.0 / comment ln3diff_amd / element vertex Nv / property float x, y, z [, nx, ny, nz] / property uchar
    red, green, blue / element face Nf / property list uchar int vertex_indices / end_header`; then Nv records of 15 (27) bytes and Nf of 13.
    An empty mesh writes the header alone.  The host formats nothing per element: two launches, two copies, three writes.
    check=False skips the face-index check and its read-back (mesh_from_grid, whose faces are the extraction's own)."""
    verts_box, faces, rgb, normal, rot9 = _export_args(verts_box, faces, rgb, normal, check)
    nv, nf = verts_box.shape[0], faces.shape[0]
    dev = verts_box.device
    vbytes, fbytes = nv * (15 if normal is None else 27), nf * 13
    vbuf = fbuf = None
    if nv:
        vbuf = torch.empty((vbytes + 3) // 4 * 4, dtype=torch.uint8, device=dev)
        ops.pack_ply_vertices(verts_box, normal, rgb, rot9, vbuf)
    if nf:
        fbuf = torch.empty((fbytes + 3) // 4 * 4, dtype=torch.uint8, device=dev)
        ops.pack_ply_faces(faces, fbuf)
    with open(path, 'wb') as fh:
        fh.write(_ply_header(nv, nf, normal is not None))
        if nv:
            fh.write(_host(vbuf)[:vbytes])
        if nf:
            fh.write(_host(fbuf)[:fbytes])


def _glb_json(views, nv_written, bounds, textured, nidx):
    """the JSON of write_glb: views = [(name, byte length)] in buffer order -> (str, total buffer length); the key order is fixed here"""
    F32, U8, U32, ARRAY, ELEMENT = 5126, 5121, 5125, 34962, 34963
    accessors, buffer_views, attributes, offset, indices, image_view = [], [], {}, 0, None, None
    for name, length in views:
        view = {'buffer': 0, 'byteOffset': offset, 'byteLength': length}
        if name != 'image':
            view['target'] = ELEMENT if name == 'indices' else ARRAY
        if name == 'POSITION':
            acc = {'bufferView': len(buffer_views), 'componentType': F32, 'count': nv_written, 'type': 'VEC3',
                   'min': [float(np.float32(b)) for b in bounds[:3]], 'max': [float(np.float32(b)) for b in bounds[3:]]}
        elif name == 'NORMAL':
            acc = {'bufferView': len(buffer_views), 'componentType': F32, 'count': nv_written, 'type': 'VEC3'}
        elif name == 'COLOR_0':
            acc = {'bufferView': len(buffer_views), 'componentType': U8, 'normalized': True, 'count': nv_written, 'type': 'VEC4'}
        elif name == 'TEXCOORD_0':
            acc = {'bufferView': len(buffer_views), 'componentType': F32, 'count': nv_written, 'type': 'VEC2'}
        elif name == 'indices':
            acc = {'bufferView': len(buffer_views), 'componentType': U32, 'count': nidx, 'type': 'SCALAR'}
        else:
            acc = None
        if acc is not None:
            if name == 'indices':
                indices = len(accessors)
            else:
                attributes[name] = len(accessors)
            accessors.append(acc)
        else:
            image_view = len(buffer_views)
        buffer_views.append(view)
        offset += (length + 3) // 4 * 4
    primitive = {'attributes': attributes}
    if indices is not None:
        primitive['indices'] = indices
    primitive.update(material=0, mode=4)
    pbr = {'baseColorTexture': {'index': 0}} if textured else {}
    pbr.update(metallicFactor=0.0, roughnessFactor=1.0)
    doc = {'asset': {'version': '2.0', 'generator': EXPORTER}, 'scene': 0, 'scenes': [{'nodes': [0]}], 'nodes': [{'mesh': 0}],
           'meshes': [{'primitives': [primitive]}], 'materials': [{'pbrMetallicRoughness': pbr, 'doubleSided': True}]}
    if textured:
        doc.update(textures=[{'sampler': 0, 'source': 0}], samplers=[{'magFilter': 9729, 'minFilter': 9729, 'wrapS': 33071, 'wrapT': 33071}],
                   images=[{'bufferView': image_view, 'mimeType': 'image/png'}])
    doc.update(accessors=accessors, bufferViews=buffer_views, buffers=[{'byteLength': offset}])
    return doc, offset


def _write_glb_file(path, doc, sections, bin_length):
    """header, JSON chunk (padded with spaces), BIN chunk (every section padded with zeros to a multiple of 4); no BIN chunk without sections"""
    text = json.dumps(doc, separators=(',', ':')).encode('ascii')
    text += b' ' * (-len(text) % 4)
    total = 12 + 8 + len(text) + ((8 + bin_length) if sections else 0)
    if total >= GLB_MAX_BYTES:
        raise ValueError(f"the GLB would be {total} bytes long: a GLB holds fewer than 2^32")
    with open(path, 'wb') as fh:
        fh.write(struct.pack('<4sII', b'glTF', 2, total) + struct.pack('<I4s', len(text), b'JSON') + text)
        if sections:
            fh.write(struct.pack('<I4s', bin_length, b'BIN\0'))
            for data in sections:
                fh.write(data)
                if len(data) % 4:
                    fh.write(b'\0' * (-len(data) % 4))


@torch.no_grad()
def write_glb(path, verts_box, faces, rgb, normal=None, uv=None, tex=None, check=True):
    """A binary glTF 2.0 asset (.glb) whose buffer is packed on the device (include/ln3d_meshpack.h).  verts_box [Nv,3] f32 in box
    coordinates, faces [Nf,3] int64, rgb [Nv,3] the query's colours, normal [Nv,3] the query's normals or None: DEVICE tensors, with
    write_ply's values.  One scene, one node, one mesh, one primitive in mode 4, one material (metallicFactor 0, roughnessFactor 1,
    doubleSided: the winding of the faces is not promised).  The JSON has a fixed key order and separators, so equal meshes give equal bytes.
    Without a texture the buffer holds POSITION f32 VEC3 [Nv], NORMAL [Nv] when given, COLOR_0 normalized UNSIGNED_BYTE VEC4 [Nv] (alpha
    255) and the indices UNSIGNED_INT [3 Nf], each its own bufferView at a multiple of 4.
    With uv [Nf,3,2] f32 (atlas_uvs) and tex [T,T,3] uint8 (bake_texture), numpy or tensors, the vertices are split per face corner, because
    glTF has one index per vertex and every face owns its UV patch: POSITION [3 Nf], NORMAL [3 Nf] when given, TEXCOORD_0 f32 VEC2 [3 Nf] =
    (u, 1 - v), corner 3 i + j holding vertex faces[i][j]; no indices and no COLOR_0 (glTF would multiply it into the texture); png_bytes(tex)
    is one more bufferView, the image of the material's baseColorTexture.  There are no sibling files.
    POSITION.min / max are the exact extremes of the written positions, as the repr of the float32 values widened to double.  An empty mesh
    writes a valid asset with one empty scene and no buffer.  Raises ValueError on a bad dtype or shape, a face index out of range (check),
    uv without tex or tex without uv, a position that is not finite, and a file of 2^32 bytes or more - all before the file is opened.
    The host formats nothing per element: two or three launches, one copy per section and one write each."""
    if (uv is None) != (tex is None):
        raise ValueError("uv and tex: expected both (a textured asset) or neither")
    verts_box, faces, rgb, normal, rot9 = _export_args(verts_box, faces, rgb, normal, check)
    nv, nf = verts_box.shape[0], faces.shape[0]
    dev = verts_box.device
    textured = uv is not None
    if textured:
        uv = torch.as_tensor(uv).to(dev).contiguous()
        if uv.dtype != torch.float32 or tuple(uv.shape) != (nf, 3, 2):
            raise ValueError(f"uv: expected a float32 [{nf}, 3, 2] array, got {uv.dtype} {tuple(uv.shape)}")
        image = png_bytes(tex.cpu().numpy() if torch.is_tensor(tex) else tex)
    if nv == 0 or nf == 0:
        _write_glb_file(path, {'asset': {'version': '2.0', 'generator': EXPORTER}, 'scene': 0, 'scenes': [{}]}, [], 0)
        return
    n = 3 * nf if textured else nv
    pos = torch.empty(n, 3, device=dev)
    nrm = torch.empty(n, 3, device=dev) if normal is not None else None
    if textured:
        last = torch.empty(n, 2, device=dev)
        ops.pack_gltf_corners(verts_box, normal, faces, uv, rot9, pos, nrm, last, check=False)      # faces: checked above, or the caller's word
    else:
        last = torch.empty(n, 4, dtype=torch.uint8, device=dev)
        idx = torch.empty(3 * nf, dtype=torch.int32, device=dev)
        ops.pack_gltf_vertices(verts_box, normal, rgb, rot9, pos, nrm, last)
        ops.pack_gltf_indices(faces, idx)
    bounds = torch.empty(6, device=dev)
    ops.position_bounds(pos, bounds)
    bounds = bounds.cpu().numpy()                                        # the one read-back the JSON needs
    if not np.isfinite(bounds).all():                                    # any position that is not finite shows in its axis' minimum or maximum
        raise ValueError("verts: a written position is not finite")
    named = [('POSITION', pos)] + ([('NORMAL', nrm)] if nrm is not None else []) + [('TEXCOORD_0' if textured else 'COLOR_0', last)]
    if not textured:
        named.append(('indices', idx))
    sections = [(name, _host(t)) for name, t in named] + ([('image', image)] if textured else [])
    doc, bin_length = _glb_json([(name, len(data)) for name, data in sections], n, bounds, textured, 3 * nf)
    _write_glb_file(path, doc, [data for _, data in sections], bin_length)


# ------------------------------------------------------------------ texture baking (include/ln3d_meshbake.h)
ATLAS_MIN_SIZE, ATLAS_MAX_SIZE, ATLAS_MIN_CELL = 4, 8192, 4


def _atlas_size(size):
    if isinstance(size, bool) or int(size) != size or not ATLAS_MIN_SIZE <= size <= ATLAS_MAX_SIZE:
        raise ValueError(f"texture_size {size!r}: expected an integer in [{ATLAS_MIN_SIZE}, {ATLAS_MAX_SIZE}]")
    return int(size)


def atlas_layout(nf, size):
    """The per-face atlas of nf >= 1 faces in a size x size texture -> (n, c): faces 2k and 2k + 1 share the square cell k of c x c texels
    at ((k % n) * c, (k // n) * c); n is the smallest integer with n * n >= ceil(nf / 2) and c = size // n.  ValueError when c < 4, naming
    the smallest sufficient size, 4 n (capacity: 2 (size // 4)^2 faces)."""
    size = _atlas_size(size)
    if int(nf) != nf or nf < 1:
        raise ValueError(f"nf {nf!r}: expected a positive integer")
    half = (int(nf) + 1) // 2
    n = math.isqrt(half)
    n += n * n < half
    c = size // n
    if c < ATLAS_MIN_CELL:
        need = ATLAS_MIN_CELL * n
        raise ValueError(f"texture size {size} is too small for {nf} faces (it holds {2 * (size // ATLAS_MIN_CELL) ** 2}): the smallest "
                         f"sufficient size is {need}" + ("" if need <= ATLAS_MAX_SIZE else f", above the largest texture, {ATLAS_MAX_SIZE}")
                         + "; a simplified mesh (simplify_cell, --mesh_simplify_cell) has fewer faces")
    return n, c


def atlas_uvs(nf, size):
    """uv [nf,3,2] float32 of the face corners in the atlas of atlas_layout(nf, size), u to the right and v UP from the centre-(0.5, 0.5)
    corner of texel (0, 0).  Cell-local, in texels: the lower (even) face has (0.5, 0.5) (c - 2.5, 0.5) (0.5, c - 2.5), the upper (odd) face
    (c - 0.5, c - 0.5) (2.5, c - 0.5) (c - 0.5, 2.5), both counter-clockwise; uv = (cell origin + corner) / size, one float32 division of an
    exact numerator.  nf = 0 gives an empty array."""
    if nf == 0:
        _atlas_size(size)
        return np.zeros((0, 3, 2), np.float32)
    n, c = atlas_layout(nf, size)
    k = np.arange(nf) // 2
    origin = np.stack([(k % n) * c, (k // n) * c], -1).astype(np.float32)                              # [nf, 2]
    lower = np.array([[0.5, 0.5], [c - 2.5, 0.5], [0.5, c - 2.5]], np.float32)
    upper = np.array([[c - 0.5, c - 0.5], [2.5, c - 0.5], [c - 0.5, 2.5]], np.float32)
    corner = np.where((np.arange(nf) % 2 == 0)[:, None, None], lower[None], upper[None])
    return ((origin[:, None, :] + corner) / np.float32(size)).astype(np.float32)


@torch.no_grad()
def bake_points(verts, faces, size):
    """verts [Nv,3] f32, faces [Nf,3] int64 (device, Nf >= 1) -> (points [size*size,3] f32, owner [size*size] int32): for the texel with flat
    index y * size + x the face that owns it (-1: nobody) and the point on that face's plane that the texel's centre maps to, (0, 0, 0)
    for an unowned texel (ln3d_bake_points; the gutter texels extrapolate the face's affine map).  Raises ValueError on a bad dtype or
    shape, a face index out of range and a size too small for Nf faces (atlas_layout)."""
    _check_verts(verts)
    verts, faces = verts.contiguous(), faces.contiguous()
    n, c = atlas_layout(faces.shape[0], size)
    ops.check_faces(faces, verts.shape[0])
    T = int(size)
    points = torch.empty(T * T, 3, device=verts.device)
    owner = torch.empty(T * T, dtype=torch.int32, device=verts.device)
    ops.bake_points(verts, faces, T, n, c, points, owner, check=False)
    return points, owner


@torch.no_grad()
def bake_texture(decoder, planes_channel_last, verts_box, faces, size, fill=0):
    """The colour of a mesh as a texture: decoder / planes_channel_last [1,3,H,W,C] as mesh_from_grid queries them, verts_box [Nv,3] f32 in
    the box coordinates of that query, faces [Nf,3] int64 (device) -> (uv [Nf,3,2] float32 numpy: atlas_uvs, tex [size,size,3] uint8 numpy:
    row y holds v = (y + 0.5) / size, so row 0 is the BOTTOM).  Every owned texel is forward_points' rgb at bake_points' point, clamped to
    [0, 1], times 255, truncated - the rule of the vertex colours; an unowned texel is `fill` (0 .. 255).  One field sample per texel.  An
    empty mesh gives a texture of `fill` and launches nothing."""
    size = _atlas_size(size)
    if isinstance(fill, bool) or int(fill) != fill or not 0 <= fill <= 255:
        raise ValueError(f"fill {fill!r}: expected an integer in [0, 255]")
    nf = faces.shape[0]
    if nf == 0:
        return atlas_uvs(0, size), np.full((size, size, 3), int(fill), np.uint8)
    points, owner = bake_points(verts_box, faces, size)
    rgb = decoder.forward_points(planes_channel_last, points[None])['rgb'][0].float().contiguous()
    tex = torch.empty(size * size, 3, dtype=torch.uint8, device=points.device)
    ops.bake_pack(rgb, owner, int(fill), tex)
    return atlas_uvs(nf, size), tex.view(size, size, 3).cpu().numpy()


def _coloured_mesh(decoder, dec_out, sigma, grid_size, thr, sample_index, method, post, smooth_tuning=(SMOOTH_LAMBDA, SMOOTH_MU),
                   snap_tuning=(None, None)):
    """the geometry and the colours of _mesh, post: a MeshPost -> (the one sample's planes, the box-space vertices and the faces on the device,
    then verts, faces, colors, vn as mesh_from_grid returns them; vn is None without normals; last the query's own dict, whose 'rgb' and
    'normal' [1,Nv,3] the binary writers take from the device).  smooth_tuning: (lam, mu) of smooth_mesh, which is applied to the extracted
    mesh in grid coordinates, so everything behind it sees the smoothed positions.  snap_tuning: (tol, max_move in grid units) of snap_mesh
    at level = thr, applied to the box-space vertices behind that and before the query."""
    smooth = (post.smooth_iters, *smooth_tuning)
    _smooth_args(*smooth)                                                # a bad value is refused before anything is extracted
    snap_iters, snap_tol, snap_move = _snap_args(post.snap_iters, *snap_tuning)
    sigma = sigma.reshape(grid_size, grid_size, grid_size)
    place = dict(simplify_placement=post.simplify_placement) if post.simplify_placement != 'mean' else {}      # 'mean': the extraction is called as it always was
    verts, faces = extract_isosurface(sigma, thr, method, post.keep, post.min_faces, post.simplify_cell, **place)
    verts, faces = smooth_mesh(verts, faces, *smooth, check=False)       # faces are the extraction's own: in range by construction
    vtx = (verts / (grid_size - 1) * 2 - 1) * 0.45                       # g-objaverse scale
    pcl = dec_out.get('planes_channel_last')
    if pcl is None:
        pcl = decoder.triplane_decoder.to_channel_last(dec_out['latent_after_vit'])        # f32, or f16 under set_plane_precision('fp16')
    pcl = pcl[sample_index:sample_index + 1]
    if snap_iters:                                                       # one grid cell is 0.9 / (grid_size - 1) in the box
        move = (snap_move if snap_move is not None else max(1.0, _simplify_cell(post.simplify_cell))) * 0.9 / (grid_size - 1)
        vtx = snap_mesh(decoder, pcl, vtx.contiguous(), thr, snap_iters, snap_tol, max_step=move / 2, max_dist=move)[0]
    q = decoder.forward_points(pcl, vtx[None], with_grad=post.normals) if vtx.shape[0] else {'rgb': vtx[None], 'normal': vtx[None]}
    colors = (q['rgb'][0].clamp(0, 1) * 255).to(torch.uint8).cpu().numpy()
    v = (rotation_matrix_x(-90) @ vtx.cpu().numpy().T).T.astype(np.float32)
    f = faces.cpu().numpy()
    vn = (rotation_matrix_x(-90) @ q['normal'][0].cpu().numpy().T).T.astype(np.float32) if post.normals else None
    return pcl, vtx, faces, v, f, colors, vn, q


def _mesh(decoder, dec_out, sigma, grid_size, thr, sample_index, path, method, post, smooth_tuning, snap_tuning):
    """the body of mesh_from_grid and textured_mesh_from_grid: post.texture_size != 0 bakes the texture and appends (uv, tex); post.mesh_format
    selects the writer of `path`.  The binary writers get _coloured_mesh's device tensors as they are."""
    post.check()
    pcl, vtx, faces, v, f, colors, vn, q = _coloured_mesh(decoder, dec_out, sigma, grid_size, thr, sample_index, method, post, smooth_tuning, snap_tuning)
    out = (v, f, colors, vn) if post.normals else (v, f, colors)
    uv = tex = None
    if post.texture_size != 0:
        uv, tex = bake_texture(decoder, pcl, vtx, faces, post.texture_size)
        out += (uv, tex)
    normal = q['normal'][0] if post.normals else None
    if not path:
        pass
    elif post.mesh_format == 'ply':
        write_ply(path, vtx, faces, q['rgb'][0], normal, check=False)   # faces are the extraction's own: in range by construction
    elif post.mesh_format == 'glb':
        write_glb(path, vtx, faces, q['rgb'][0], normal, uv, tex, check=False)
    elif tex is None:
        write_obj(path, v, f, colors.astype(np.float32) / 255.0, vn)
    else:
        write_obj_textured(path, v, f, colors.astype(np.float32) / 255.0, uv, vn)
        write_png(os.path.splitext(str(path))[0] + '.png', tex)
    return out


@torch.no_grad()
def mesh_from_grid(decoder, dec_out, sigma, grid_size, thr=10.0, sample_index=0, path=None, method='cubes', smooth_lambda=SMOOTH_LAMBDA,
                   smooth_mu=SMOOTH_MU, snap_tol=None, snap_max_move=None, **post):
    """nsr/train_util_diffusion.py:221-244: iso-surface of the sigma grid at `thr`, vertices mapped to the +-0.45 box, coloured
    by re-querying the tri-plane at the vertices (forward_points), rotated -90 degrees about x.
    Returns (verts [Nv,3] float32 numpy, faces [Nf,3] int64 numpy, colors [Nv,3] uint8 numpy); writes `path` when given.
    normals (opt-in; no reference counterpart): the query that colours the vertices also returns the field's unit outward normal there
    (forward_points(with_grad=True), evaluated in box coordinates and rotated with the mesh); the return value is then the 4-tuple
    (verts, faces, colors, vn [Nv,3] float32 numpy) and the .obj carries `vn` records.
    keep / min_faces (opt-in; no reference counterpart): clean_mesh right after the weld, so only the surviving components are coloured (and
    given normals) and written; what survives has the bits it has in the uncleaned mesh.  Nothing surviving writes an .obj with no records.
    simplify_cell (opt-in, in grid units; no reference counterpart): simplify_mesh behind the clean-up and before the query, so colours and `vn`
    are the field's values AT THE NEW VERTICES and discarded vertices cost nothing.  See simplify_mesh for what clustering does not promise.
    smooth_iters / smooth_lambda / smooth_mu (opt-in; no reference counterpart): smooth_mesh behind the clean-up and the simplification, in
    grid coordinates, before the box mapping and the query, so colours and `vn` are the field's values AT THE SMOOTHED POSITIONS, which lie
    off the level set; faces are unchanged.  0 iterations launches nothing.  See smooth_mesh for what smoothing does not promise.
    snap_iters / snap_tol / snap_max_move (opt-in; no reference counterpart): snap_mesh of the box-space vertices at level = thr, behind
    the smoothing and before the query, so colours and `vn` are the field's values AT THE SNAPPED POSITIONS; faces, vertex count and order
    never change.  snap_iters in [0, 64]; 0 launches nothing.  snap_max_move is the farthest a vertex may end from where it started, in
    grid cells; a Newton step is at most half of it.  The defaults are choices, not measurements: snap_tol None = 1e-3 * max(1, |thr|),
    snap_max_move None = max(1, simplify_cell).  See snap_mesh for what snapping does not promise.
    simplify_placement (opt-in; no reference counterpart): 'quadric' puts every vertex of the simplified mesh where the planes of the faces
    around its cell meet (simplify_mesh's placement) instead of at the mean of the cell, so creases and corners survive; faces, vertex count
    and order are those of 'mean', and smoothing, snapping and the query follow as they do today, at the quadric positions.  Without
    simplify_cell there is nothing to place.  See simplify_mesh for what it does not promise: on smooth regions it is no closer than the mean.
    mesh_format (opt-in; no reference counterpart): what `path` is written as - 'obj' (the default: exactly the text file above), 'ply'
    (write_ply: binary little-endian, vertex colours, normals when asked for) or 'glb' (write_glb: binary glTF 2.0).  The two binary files are
    packed on the device from the tensors the query left there and hold the returned values bit for bit; the returned tuple does not depend
    on the format, and the extension of `path` is not interpreted.  A value that is none of the three is a ValueError before anything is
    extracted.
    **post: normals, keep, min_faces, simplify_cell, simplify_placement, smooth_iters, snap_iters and mesh_format, the fields of MeshPost
    but texture_size (textured_mesh_from_grid's), with MeshPost's defaults; any other keyword is a TypeError."""
    if 'texture_size' in post:
        raise TypeError("mesh_from_grid() got an unexpected keyword argument 'texture_size'")
    return _mesh(decoder, dec_out, sigma, grid_size, thr, sample_index, path, method, MeshPost(**post), (smooth_lambda, smooth_mu), (snap_tol, snap_max_move))


@torch.no_grad()
def textured_mesh_from_grid(decoder, dec_out, sigma, grid_size, thr=10.0, sample_index=0, path=None, method='cubes', texture_size=1024,
                            smooth_lambda=SMOOTH_LAMBDA, smooth_mu=SMOOTH_MU, snap_tol=None, snap_max_move=None, **post):
    """mesh_from_grid plus a baked texture (opt-in; no reference counterpart): the same geometry, vertex colours and `vn`, bit for bit, for
    the same options, then bake_texture of the faces at the box-space vertices (before the rotation, where the field lives) into a
    texture_size x texture_size per-face atlas.  Returns mesh_from_grid's tuple with (uv [Nf,3,2] float32, tex [T,T,3] uint8) appended.
    With `path` = <stem>.obj it writes <stem>.obj and <stem>.mtl (write_obj_textured) and <stem>.png (write_png).  A texture_size too
    small for the extracted face count is a ValueError that names the smallest sufficient size (atlas_layout): simplify_cell is what makes
    a mesh fit a small texture.
    NOT promised: more than half of the atlas is unused; texel density is uniform per face, not per unit area; there is one field sample per
    texel, no supersampling; there is no mip-safe padding beyond the 1 - 1.5 texel gutter; and the colours are the field's values on the
    (possibly simplified, possibly smoothed: smooth_iters / smooth_lambda / smooth_mu are mesh_from_grid's) triangles, which lie off the
    level set by the simplifier's and the smoother's error.  snap_iters / snap_tol / snap_max_move (mesh_from_grid's) put the VERTICES
    back on it before the bake; the interiors of the triangles stay where the flat faces are.  simplify_placement is mesh_from_grid's.
    mesh_format (opt-in): 'glb' writes `path` alone, a binary glTF that embeds the .png and splits the vertices per face corner (write_glb:
    3 Nf vertices, TEXCOORD_0 = (u, 1 - v), no vertex colours); the returned tuple is the same.  'ply' carries vertex colours only: with
    a texture it is a ValueError before anything is extracted.
    **post: mesh_from_grid's."""
    _atlas_size(texture_size)                                            # 0 is no texture in the record: here it is refused like any other bad size
    return _mesh(decoder, dec_out, sigma, grid_size, thr, sample_index, path, method, MeshPost(texture_size=texture_size, **post),
                 (smooth_lambda, smooth_mu), (snap_tol, snap_max_move))


@torch.no_grad()
def mesh_from_record(decoder, dec_out, sigma, grid_size, thr, sample_index, path, post):
    """The mesh of one sample with the options of post, a MeshPost: textured_mesh_from_grid when post.texture_size is not 0, mesh_from_grid
    otherwise (looked up when called).  The whole record is handed on; mesh_from_grid gets every field but texture_size."""
    kw = post._asdict()
    if post.texture_size != 0:
        return textured_mesh_from_grid(decoder, dec_out, sigma, grid_size, thr, sample_index=sample_index, path=path, **kw)
    del kw['texture_size']
    return mesh_from_grid(decoder, dec_out, sigma, grid_size, thr, sample_index=sample_index, path=path, **kw)


@torch.no_grad()
def export_mesh(decoder, dec_out, path, grid_size=192, thr=10.0, sample_index=0, **kw):
    """decoder: the VAE decoder module; dec_out: its vit_decode_postprocess dict.  Writes `path` (.obj, or what mesh_format says), with `vn`
    records when normals; **kw: mesh_from_grid's options and tuning values (normals, keep, min_faces, simplify_cell, simplify_placement,
    smooth_iters, smooth_lambda, smooth_mu, snap_iters, snap_tol, snap_max_move, mesh_format), handed on as they are.
    Returns (number of vertices, number of faces)."""
    pcl = dec_out['planes_channel_last'][sample_index:sample_index + 1]
    grid = decoder.triplane_decode_grid({'planes_channel_last': pcl}, grid_size)
    v, f = mesh_from_grid(decoder, {'planes_channel_last': pcl}, grid['sigma'][0], grid_size, thr, 0, path, **kw)[:2]
    return v.shape[0], f.shape[0]
