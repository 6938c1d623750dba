/* ln3d_meshsimplify.h - entry points of libln3d_hip.so for simplifying a welded mesh on the device by vertex clustering: vertices are
 * snapped to a uniform lattice of cells, every occupied cell is replaced by one representative, faces that collapse or repeat are dropped.
 * There is no reference counterpart (the reference writes the level set at the grid's full density and leaves reduction to trimesh or
 * MeshLab on the CPU); everything here is opt-in and changes no other output.  Same conventions as ln3d_meshclean.h (caller-owned device
 * pointers, stream as void*, 0 or a negative LN3D_ERR_* code, asynchronous on the stream, no allocation, no device-to-host read, a launch
 * count that does not depend on the data).  The entry points belong to ABI 10 of ln3d.h and, like every other export, are bound from
 * _lib.PROTOTYPES.
 *
 * Arguments are checked before anything touches the device: a null buffer, a count (nv, nf, nc) below 1 or above 2^31 - 1, nc > nv, a
 * cell that is not finite or not > 0, or a non-finite origin returns LN3D_ERR_BAD_ARG; nc > 2^21 (three cluster numbers no longer fit
 * the 63-bit face key) returns LN3D_ERR_UNSUPPORTED from every entry point that takes nc.
 *
 * verts [nv, 3] f32; faces [nf, 3] int64, every index in [0, nv); cluster [nv] int64, every value in [0, nc); order [nv] int64, a
 * permutation of [0, nv); start [nc + 1] int64, ascending from 0 to nv; perm [nf] int64, a permutation of [0, nf); cfaces [nf, 3] int64,
 * every index in [0, nc).  THOSE RANGES ARE PRECONDITIONS: the kernels index with the values they read, and a value outside its range
 * reads or writes outside the caller's buffers.  (The Python wrappers check them.)
 *
 * Every output is unique by definition: integers, or (the representatives) fp32 sums taken in one stated order with correctly rounded
 * operations and no float atomics, so nothing depends on scheduling or on the run.
 *
 * What the whole does NOT promise: clustering can create non-manifold edges; it can fold triangles over; it pulls convex regions inward by
 * O(cell^2 * curvature) (a representative is the mean of points on the surface); and it merges components that come within a cell of
 * each other.  There is no smoothing here.  The mean is the placement of THESE entry points; the opt-in quadric-error placement of the
 * representatives, which keeps creases and corners, is two further entry points in addons/ln3d_meshquadric.h that run between
 * ln3d_simplify_mean and the compaction and change coordinates only.
 */
#ifndef LN3D_MESHSIMPLIFY_H
#define LN3D_MESHSIMPLIFY_H
#include <stdint.h>
#include "ln3d.h"
#ifdef __cplusplus
extern "C" {
#endif

/* key[v] = q_x << 42 | q_y << 21 | q_z with q_a = (int64) floorf((x_a - origin_a) / cell): an fp32 subtraction, a correctly rounded fp32
 * division, floorf - what numpy gives in float32.  q is clamped into [0, 2^21 - 1] (a NaN coordinate gives 0), so the call is total; the
 * caller makes sure that no vertex needs the clamp.  One launch. */
int ln3d_simplify_keys(const float* verts, int64_t nv, float origin_x, float origin_y, float origin_z, float cell, int64_t* key,
                       void* stream);

/* The members of cluster k are the vertices order[start[k]] ... order[start[k + 1] - 1].  rep[k][a] = the fp32 sum of their coordinate a,
 * taken one by one in that order starting from +0, divided (correctly rounded fp32) by the member count as fp32; a cluster without
 * members gets +0 / 0 = NaN.  With order = the stable sort of cluster[] the order is ascending vertex index, which makes the bits unique.
 * One thread per cluster, one launch. */
int ln3d_simplify_mean(const float* verts, const int64_t* order, const int64_t* start, int64_t nv, int64_t nc, float* rep, void* stream);

/* cfaces[f][j] = cluster[faces[f][j]], corner order kept.  fkey[f] = -1 when two corners of cfaces[f] are equal (the face has collapsed);
 * otherwise lo << 42 | mid << 21 | hi of its corners in ascending order, so two faces with the same vertex set have the same key whatever
 * their winding.  One launch. */
int ln3d_simplify_faces(const int64_t* faces, int64_t nf, const int64_t* cluster, int64_t nv, int64_t nc, int64_t* cfaces, int64_t* fkey,
                        void* stream);

/* sorted_key [nf]: fkey in ascending order; perm [nf]: the original index of every sorted position (a STABLE sort, so equal keys keep
 * ascending original indices).  keep_f[perm[i]] = 1 when sorted_key[i] != -1 and (i == 0 or sorted_key[i - 1] != sorted_key[i]), else 0:
 * of the faces with one vertex set only the one with the smallest original index survives.  Every element of keep_f is written.  One
 * launch. */
int ln3d_simplify_first(const int64_t* sorted_key, const int64_t* perm, int64_t nf, int32_t* keep_f, void* stream);

/* keep_v [nc] is zeroed, then keep_v[c] = 1 for every corner c of every face with keep_f != 0 (plain stores of the one value).  Two
 * launches.  keep_v / keep_f and their inclusive prefix sums, rep and cfaces are what ln3d_mesh_gather (ln3d_meshclean.h) compacts. */
int ln3d_simplify_used(const int64_t* cfaces, const int32_t* keep_f, int64_t nf, int64_t nc, int32_t* keep_v, void* stream);

#ifdef __cplusplus
}
#endif
#endif
