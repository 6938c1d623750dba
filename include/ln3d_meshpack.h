/* ln3d_meshpack.h - entry points of libln3d_hip.so that assemble the bytes of a binary mesh file on the device: the vertex and face records
 * of a binary little-endian PLY, and the buffer sections of a binary glTF (GLB).  There is no reference counterpart; everything here is
 * opt-in and changes no other output.  Same conventions as ln3d_meshclean.h (caller-owned device pointers, stream as void*, 0 or a negative
 * LN3D_ERR_* code, asynchronous on the stream, no allocation, no device-to-host read, no float atomics).  The entry points are additions to
 * ABI 10 of ln3d.h that use no struct and no new constant; they are bound from _lib.PROTOTYPES.
 *
 * The values (all arithmetic float32; every output byte is unique, nothing depends on scheduling):
 *   - a rotated row: with rot9 the nine floats of a row-major 3 x 3 matrix R and (x, y, z) a row of xyz (or of normal),
 *         out[r] = fl(fl(fl(R[r][0] * x) + fl(R[r][1] * y)) + fl(R[r][2] * z))
 *     every multiply and add rounded once, no fused multiply-add (the convention of ln3d_bake_points and ln3d_smooth_step), so numpy's
 *     float32 operators reproduce the bits.  A zero result has the sign those operations give it;
 *   - a colour byte: (uint8) trunc(min(max(c, 0), 1) * 255), a NaN giving 0: the rule of ln3d_bake_pack;
 *   - an index: the int64 face index narrowed to its low 32 bits.
 * All multi-byte values are little-endian.
 *
 * The PLY records are 15 (27 with normals) and 13 bytes long, so a record does not start on a word.  The packers therefore work BY OUTPUT
 * WORD: one thread produces one aligned 4-byte word, finds the record and the field every one of its four bytes comes from (the pattern
 * repeats every 4 records) and stores the word once, so that a wavefront writes one contiguous run of 256 bytes.  The inputs are read
 * through the caches: 12-byte rows, each re-read by the few neighbouring threads whose words it touches.  `out` holds the byte count
 * rounded UP to a multiple of 4; the pad bytes behind the last record are written as 0 and nothing behind them is written.
 *
 * Arguments are checked before anything touches the device: a null buffer (normal and nrm_out may be null, and must be null together), a
 * count (nv, nf, n) below 1 or above 2^31 - 1, or an output that is not 4-byte aligned returns LN3D_ERR_BAD_ARG.
 *
 * PRECONDITIONS (the Python wrappers check them): the buffers have the stated sizes and do not overlap; for ln3d_pack_gltf_corners every
 * index of faces lies in [0, nv) - a corner whose index does not is written as (0, 0, 0) and its row is not read; for
 * ln3d_position_bounds the positions are finite.
 */
#ifndef LN3D_MESHPACK_H
#define LN3D_MESHPACK_H
#include <stdint.h>
#include "ln3d.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The nv vertex records of a binary PLY: the rotated row of xyz as 3 f32, the rotated row of normal as 3 f32 when normal is not null, the
 * three colour bytes of rgb: 15 or 27 bytes a record, no padding between records.  xyz, normal, rgb [nv, 3] f32, rot9 [9] f32 (device),
 * out [ceil(nv * 15 / 4) * 4] or [ceil(nv * 27 / 4) * 4] bytes, 4-byte aligned. */
int ln3d_pack_ply_vertices(const float* xyz, const float* normal, const float* rgb, const float* rot9, int64_t nv, void* out, void* stream);

/* The nf face records of a binary PLY (`property list uchar int vertex_indices`): the byte 3, then the three indices as int32: 13 bytes a
 * record.  faces [nf, 3] int64, out [ceil(nf * 13 / 4) * 4] bytes, 4-byte aligned. */
int ln3d_pack_ply_faces(const int64_t* faces, int64_t nf, void* out, void* stream);

/* The vertex sections of an untextured GLB: pos_out [nv, 3] f32 <- the rotated rows of xyz; nrm_out [nv, 3] f32 <- the rotated rows of
 * normal (both null, or neither); rgba_out [nv, 4] uint8 <- the three colour bytes of rgb and 255.  One thread per float, and the first nv
 * threads pack one colour word each: every store of a wavefront is one contiguous run. */
int ln3d_pack_gltf_vertices(const float* xyz, const float* normal, const float* rgb, const float* rot9, int64_t nv, float* pos_out,
                            float* nrm_out, void* rgba_out, void* stream);

/* The index section of an untextured GLB: idx_out [3 nf] uint32 <- faces [nf, 3] int64, narrowed. */
int ln3d_pack_gltf_indices(const int64_t* faces, int64_t nf, void* idx_out, void* stream);

/* The vertex sections of a textured GLB, whose vertices are split per face corner: corner c = 3 i + j holds the data of vertex
 * faces[i][j].  pos_out [3 nf, 3] f32 <- the rotated row of xyz at that vertex; nrm_out [3 nf, 3] f32 <- the rotated row of normal there
 * (both null, or neither); uv_out [3 nf, 2] f32 <- (u, fl(1 - v)) of uv [3 nf, 2] f32 (atlas_uvs: v up; glTF: v down).  xyz, normal
 * [nv, 3] f32, faces [nf, 3] int64.  One thread per output float. */
int ln3d_pack_gltf_corners(const float* xyz, const float* normal, const int64_t* faces, const float* uv, const float* rot9, int64_t nv,
                           int64_t nf, float* pos_out, float* nrm_out, float* uv_out, void* stream);

/* bounds6 [6] f32 <- the per-axis minimum (x, y, z), then the per-axis maximum, of pos [n, 3] f32.  Minimum and maximum are taken in the
 * total order of the order-preserving integer key of a float (so -0 lies below +0), which makes the result independent of the order of
 * evaluation: a reduction in the wavefront and the block, then one integer atomic min and max per block and axis on the key.  Three
 * launches: bounds6 is set to the identity keys, reduced into, and turned back into floats in place. */
int ln3d_position_bounds(const float* pos, int64_t n, float* bounds6, void* stream);

#ifdef __cplusplus
}
#endif
#endif
