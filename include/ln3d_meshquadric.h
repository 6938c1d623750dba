/* ln3d_meshquadric.h - entry points of libln3d_hip.so for the opt-in quadric-error placement of the representatives of a mesh simplified by
 * vertex clustering (ln3d_meshsimplify.h): instead of the mean of its members, a cluster's vertex is put where the summed squared distance
 * to the planes of the faces that touch the cluster is least (Lindstrom's rule for clustering simplifiers, in its Tikhonov form), which
 * keeps the creases and corners that the mean chamfers by up to about 0.4 cells.  There is no reference counterpart; everything here is
 * opt-in and changes no other output.  Same conventions as ln3d_meshsmooth.h (caller-owned device pointers, stream as void*, 0 or a negative
 * LN3D_ERR_* code, asynchronous on the stream, no allocation, no device-to-host read, one launch per call, no float atomics).  The entry
 * points are additions to ABI 10 of ln3d.h that use no struct and no new constant; they are bound from _lib.PROTOTYPES.
 *
 * The definition.  Clusters k, cluster[v], cfaces[f][j] and the mean m_k are those of ln3d_meshsimplify.h; ln3d_simplify_mean's output keeps
 * its bits.  verts [nv, 3] f32, faces [nf, 3] int64, cfaces [nf, 3] int64.
 *   - incidence: face f contributes to cluster k ONCE if at least one of its corners lies in k.  Corner j counts only if cfaces[f][j] differs
 *     from cfaces[f][i] for all i < j.  Every input face contributes: the faces that collapse inside one cell (the most informative ones)
 *     and the faces that are later dropped as duplicates too.  The faces of cluster k are taken in ascending face index f_0 < f_1 < ...;
 *   - per contributing face, in coordinates local to m_k: a, b, c = the face's corners minus m_k; n = (b - a) x (c - a), NOT normalised, so
 *     a face weighs with its area squared; d = n . a; the face adds n n^T to A (six distinct entries) and d n to r;
 *   - the order of the sums (part of the definition; all arithmetic float32, products may be fused into the additions that consume them):
 *     64 partial sums p_0 ... p_63, p_l taking the faces f_l, f_(l+64), f_(l+128), ... one by one in that order starting from +0; then six
 *     pairwise steps s = 32, 16, 8, 4, 2, 1 with p_l <- p_l + p_(l xor s); the sum is p_0.  The shape does not depend on the data, on the
 *     scheduling or on the run: two runs return the same bits;
 *   - solve: (A + lambda I) delta = r with lambda = eps * trace(A), by an unpivoted 3 x 3 LDL^T factorisation (the matrix is symmetric
 *     positive definite with a condition number of at most (1 + eps) / eps, so float32 is adequate and no eigen-decomposition is needed);
 *     x = m_k + delta.  This is the Tikhonov form of the truncated pseudo-inverse: along directions that no face plane constrains, delta is 0
 *     and x stays at the mean;
 *   - acceptance: placed[k] = 1 and rep_out[k] = x when trace(A) > 0, every component of x is finite, and x lies in the closed box of the
 *     cluster's lattice cell q on every axis, lo_a <= x_a <= hi_a with lo_a = fma(q_a, cell, origin_a) and hi_a = fma(q_a + 1, cell,
 *     origin_a) (one rounding each); q is unpacked from the cluster's cell key, q_x << 42 | q_y << 21 | q_z.  Otherwise rep_out[k] = m_k bit
 *     for bit and placed[k] = 0.  So a representative is never farther from its members than the mean's bound, the cell diagonal.
 * Faces, vertex count and vertex order of the simplified mesh are those of the mean placement; only coordinates change.
 *
 * The split (that of ln3d_meshsimplify.h): the caller sorts pair_key ascending and derives start[k] = the number of sorted keys whose
 * cluster part (key >> 31) is below k, k = 0 ... nc (searchsorted); everything else is a kernel.
 *
 * Arguments are checked before anything touches the device: a null buffer, a count (nv, nf, nc) below 1 or above 2^31 - 1, npairs below 1 or
 * above 3 nf, nc > nv, a cell that is not finite or not > 0, a non-finite origin, an eps that is not finite or not in (0, 1], or a rep_out
 * that overlaps rep_mean without being the same pointer returns LN3D_ERR_BAD_ARG; nc > 2^21 (a cluster number no longer fits its key)
 * returns LN3D_ERR_UNSUPPORTED.  rep_out == rep_mean (placement in place) is allowed: a cluster reads only its own mean, before it writes.
 *
 * PRECONDITIONS (the Python wrappers check them): every index of faces lies in [0, nv), every index of cfaces in [0, nc); sorted_pair_key
 * holds the keys that ln3d_quadric_pairs made from those cfaces, ascending; start [nc + 1] ascends within [0, npairs].  The kernels read at
 * the indices they find (a sorted key whose cluster part is not the row's cluster, or whose face part is not below nf, is skipped).
 *
 * What the whole does NOT promise: on smooth or noisy regions a quadric representative is NOT closer to the surface than the mean (the face
 * planes of an inscribed mesh lie inside the surface, and the mean averages vertex noise away: on a sphere of radius 60 at cell 3 the median
 * distance to the sphere is 0.015 against the mean's 0.010, with sigma = 0.3 vertex noise 0.17 against 0.11), so this is a feature-preserving
 * option, not a better default; folds and non-manifold edges remain, the faces being the clustering's; bevels that marching cubes already
 * cut at grid resolution are only partly recovered; eps trades crease sharpness (small) against noise amplification (its default 1e-3 is a
 * choice, not a measurement).
 */
#ifndef LN3D_MESHQUADRIC_H
#define LN3D_MESHQUADRIC_H
#include <stdint.h>
#include "ln3d.h"
#ifdef __cplusplus
extern "C" {
#endif

/* One thread per face, integers only.  pair_key[3 f + j] = cfaces[f][j] << 31 | f when corner j counts (see incidence), INT64_MAX otherwise.
 * The key fits because nc <= 2^21 and nf < 2^31.  cfaces [nf, 3] int64, pair_key [3 nf] int64.  Sorted ascending, the keys list every
 * cluster's faces in ascending face index, the INT64_MAX entries behind the last cluster's. */
int ln3d_quadric_pairs(const int64_t* cfaces, int64_t nf, int64_t nc, int64_t* pair_key, void* stream);

/* One wavefront per cluster k walks the row sorted_pair_key[start[k] .. start[k + 1]) (clipped to [0, npairs)), 64 faces at a time, and does
 * the accumulation, the solve and the acceptance test of the definition above.  verts [nv, 3] f32, faces [nf, 3] int64, sorted_pair_key
 * [npairs] int64, start [nc + 1] int64, rep_mean [nc, 3] f32 (ln3d_simplify_mean's output), cluster_cell_key [nc] int64 (the distinct keys
 * of ln3d_simplify_keys in ascending order: cluster k's lattice cell), rep_out [nc, 3] f32, placed [nc] int32.  Every element of rep_out and
 * placed is written. */
int ln3d_quadric_place(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const int64_t* sorted_pair_key, int64_t npairs,
                       const int64_t* start, int64_t nc, const float* rep_mean, float origin_x, float origin_y, float origin_z, float cell,
                       const int64_t* cluster_cell_key, float eps, float* rep_out, int32_t* placed, void* stream);

#ifdef __cplusplus
}
#endif
#endif
