/* ln3d_meshclean.h - entry points of libln3d_hip.so for cleaning an extracted mesh on the device: connected components of a welded
 * triangle soup, per-component vertex and face counts, a keep mask (a minimum face count, or the largest component only) and the
 * compaction of the survivors.  There is no reference counterpart (the reference writes every speck of the level set and leaves the
 * clean-up to `trimesh.split` on the CPU); everything here is opt-in and changes no other output.  Same conventions as ln3d.h
 * (caller-owned device pointers, stream as void*, 0 or a negative LN3D_ERR_* code, asynchronous on the stream, no allocation); the ABI
 * number of ln3d.h covers them.
 *
 * Every entry point enqueues a number of launches that does not depend on the data and returns: no device-to-host read, no
 * synchronisation.  Arguments are checked before anything touches the device: a null buffer, nv < 1, nv > 2^31 - 1, nf < 1,
 * nf > 2^31 - 1 (the counts are int32) or a negative min_faces returns LN3D_ERR_BAD_ARG.
 *
 * faces [nf, 3] int64 (what extract_isosurface returns), every index in [0, nv).  THAT RANGE IS A PRECONDITION: the kernels index with
 * the values they read, and an index outside [0, nv) reads or writes outside the caller's buffers.  (The Python wrappers check it.)
 * label, nvert, nface, keep_v [nv] int32; keep_f [nf] int32; best uint64[1].
 *
 * Everything is integer arithmetic and integer atomics: every output is exact and unique by definition, so it does not depend on
 * scheduling or on the run, and on vertex numbering only as far as the definitions below name indices.
 */
#ifndef LN3D_MESHCLEAN_H
#define LN3D_MESHCLEAN_H
#include <stdint.h>
#include "ln3d.h"
#ifdef __cplusplus
extern "C" {
#endif

/* label[v] = the smallest vertex index in the connected component of v.  Two vertices are connected when a face names both (so two
 * surfaces that meet in a single shared vertex are one component); a vertex that no face names is its own component; a face that
 * repeats an index is tolerated and connects what it names.  Union-find on the device: initialise, hook the edges of every face with
 * atomicMin, pointer-jump every vertex to its root - three launches. */
int ln3d_mesh_components(const int64_t* faces, int64_t nf, int64_t nv, int32_t* label, void* stream);

/* label: the output of ln3d_mesh_components over the same faces.  The call zeroes nvert and nface and resets best, then
 * nvert[r] = number of vertices whose label is r, nface[r] = number of faces whose FIRST vertex has label r (both 0 at indices that are
 * not labels), and best[0] = (nface << 32) | (0x7fffffff - r) of the component with the most faces, ties to the smallest label r: the
 * maximum of that 64-bit word over the components that own a face, taken with an integer atomic max, so the tie rule is part of the
 * arithmetic. */
int ln3d_mesh_component_counts(const int64_t* faces, int64_t nf, const int32_t* label, int64_t nv, int32_t* nvert, int32_t* nface,
                               uint64_t* best, void* stream);

/* keep_v[v] = 1 when nface[label[v]] >= min_faces and, if largest_only != 0, label[v] is the label packed in best[0] (read on the
 * device); 0 otherwise.  keep_f[f] = keep_v[faces[f][0]].  The masks are int32 so that the caller can take their prefix sums. */
int ln3d_mesh_mark(const int64_t* faces, int64_t nf, const int32_t* label, const int32_t* nface, int64_t nv, int64_t min_faces,
                   int largest_only, const uint64_t* best, int32_t* keep_v, int32_t* keep_f, void* stream);

/* Compaction.  vprefix [nv], fprefix [nf] int64: the INCLUSIVE prefix sums of keep_v and keep_f, taken by the caller (the convention of
 * the count / emit pairs of ln3d.h).  verts [nv, 3] f32.  Kept vertex v goes to row vprefix[v] - 1 of verts_out, its three coordinates
 * copied bit for bit; kept face f goes to row fprefix[f] - 1 of faces_out with every index i renumbered to vprefix[i] - 1; so vertices
 * and faces keep their relative order.  Nothing outside the first vprefix[nv - 1] rows of verts_out and the first fprefix[nf - 1] rows
 * of faces_out is written.  A kept face names kept vertices only when the masks come from ln3d_mesh_mark. */
int ln3d_mesh_gather(const float* verts, const int64_t* faces, const int32_t* keep_v, const int64_t* vprefix, const int32_t* keep_f,
                     const int64_t* fprefix, int64_t nv, int64_t nf, float* verts_out, int64_t* faces_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
