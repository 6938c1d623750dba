/* ln3d_meshsmooth.h - entry points of libln3d_hip.so for smoothing an exported mesh: Taubin's lambda | mu scheme with uniform (umbrella)
 * weights, which removes the facets and the noise of the level set without the shrinkage of plain Laplacian smoothing.  There is no
 * reference counterpart; everything here is opt-in and changes no other output.  Same conventions as ln3d_meshclean.h (caller-owned device
 * pointers, stream as void*, 0 or a negative LN3D_ERR_* code, asynchronous on the stream, no allocation, no device-to-host read, one launch
 * per call, no float atomics).  The entry points are additions to ABI 10 of ln3d.h that use no struct and no new constant; they are
 * bound from _lib.PROTOTYPES.
 *
 * The definition (all arithmetic float32; every output is unique, nothing depends on scheduling).  verts [nv, 3] f32, faces [nf, 3] int64:
 *   - edges: every face contributes its three undirected edges {a, b}; an edge with a == b is ignored; duplicate faces and opposite
 *     windings contribute the same undirected edge again;
 *   - neighbours: the neighbours of vertex i are the DISTINCT vertices that share an edge with it, in ascending index j_1 < ... < j_d;
 *   - pinned vertices: an undirected edge named by exactly one face corner pair (multiplicity 1) is a boundary edge and both its ends are
 *     pinned; a pinned vertex never moves, and neither does a vertex with d = 0; edges of multiplicity >= 2, non-manifold ones included,
 *     are interior;
 *   - one pass with the factor f, per axis, for a free vertex:
 *         s = x[j_1], then s = fl(s + x[j_k]) for k = 2 .. d;   m = fl(s / fl32(d));   e = fl(m - x_i);   x_i' = fl(x_i + fl(f * e))
 *     every operation rounded once, no fused multiply-add; a vertex that does not move keeps its bits; every pass reads the previous
 *     pass's coordinates only (two buffers: the output may not overlap the input);
 *   - one iteration is a pass with lambda, then a pass with mu; mu == 0 skips the second pass (plain Laplacian smoothing).
 * Faces, vertex count and vertex order are unchanged; only coordinates move.
 *
 * The split (that of ln3d_meshsimplify.h): the caller supplies the unique with counts of the edge keys, the sort of the half-edge keys and
 * the row pointers (searchsorted or a prefix sum); everything else is a kernel.
 *
 * Arguments are checked before anything touches the device: a null buffer, a count (nf, ne, nv, n_halfedges) below 1 or above 2^31 - 1, a
 * factor that is not finite, or a verts_out that overlaps verts_in returns LN3D_ERR_BAD_ARG.
 *
 * PRECONDITIONS (the Python wrappers check them): every index of faces lies in [0, nv) with nv < 2^31; edge holds keys that
 * ln3d_smooth_edge_keys made from such faces; start [nv + 1] ascends from 0 to n_halfedges and every nbr lies in [0, nv).  The kernels read
 * and write at the indices they find.
 *
 * What the whole does NOT promise: the weights are uniform, not cotangent, so vertices also drift tangentially towards even spacing; the
 * vertices move off the level set; features sharper than the pass band are rounded; the volume is not preserved exactly (Taubin's scheme
 * keeps it to a few per cent where Laplacian smoothing loses half); boundary loops stay as jagged as they were, because they are pinned.
 */
#ifndef LN3D_MESHSMOOTH_H
#define LN3D_MESHSMOOTH_H
#include <stdint.h>
#include "ln3d.h"
#ifdef __cplusplus
extern "C" {
#endif

/* One thread per face.  key[3 f + j] is the undirected edge between corners j and (j + 1) % 3 of face f: (lo << 32) | hi with lo < hi the
 * two vertex indices, or -1 when they are equal.  faces [nf, 3] int64, key [3 nf] int64.  The caller reduces key to its distinct values
 * with their multiplicities and drops -1. */
int ln3d_smooth_edge_keys(const int64_t* faces, int64_t nf, int64_t* key, void* stream);

/* One thread per distinct edge e = (lo << 32) | hi with multiplicity count[e]: dkey[2 e] = (lo << 32) | hi and dkey[2 e + 1] =
 * (hi << 32) | lo, the edge in both directions as (src << 32) | dst; pinned[lo] = pinned[hi] = 1 when count[e] == 1 (plain stores of the
 * same value from many threads).  THE CALLER ZEROES pinned [nv] int32; an end outside [0, nv) is not written.  edge, count [ne] int64,
 * dkey [2 ne] int64.  Sorted ascending, dkey lists every vertex's neighbours in ascending order: nbr is its low word and start[i] the
 * number of entries whose src is below i. */
int ln3d_smooth_halfedges(const int64_t* edge, const int64_t* count, int64_t ne, int64_t nv, int64_t* dkey, int32_t* pinned, void* stream);

/* One pass with `factor`: one thread per vertex walks its row nbr[start[i] .. start[i + 1]) (clipped to [0, n_halfedges)) in order.
 * verts_out[i] is the pass formula above for a free vertex and verts_in[i], bit for bit, for a pinned one or one with an empty row.
 * verts_in, verts_out [nv, 3] f32 that do not overlap, start [nv + 1] int64, nbr [n_halfedges] int32, pinned [nv] int32. */
int ln3d_smooth_step(const float* verts_in, const int64_t* start, const int32_t* nbr, const int32_t* pinned, int64_t nv, int64_t n_halfedges,
                     float factor, float* verts_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
