/* ln3d_meshbake.h - entry points of libln3d_hip.so for baking the colour of an exported mesh into a texture: every face gets its own
 * right-isosceles patch of a T x T atlas, every owned texel is mapped back to a point on its face, the field is evaluated there by the
 * existing point query (ln3d_query_points of ln3d.h / ln3d_planes16.h, which is NOT duplicated here), and the colours are packed to
 * uint8.  There is no reference counterpart (the reference writes one colour per vertex); everything here is opt-in and changes no other
 * output.  Same conventions as ln3d_meshclean.h (caller-owned device pointers, stream as void*, 0 or a negative LN3D_ERR_* code,
 * asynchronous on the stream, no allocation, no device-to-host read, one launch per call, no float atomics).  The entry points are
 * additions to ABI 10 of ln3d.h that use no struct and no new constant; like every other export they are bound from
 * _lib.PROTOTYPES (tests/test_abi_types_cpu.py holds that table to every header).
 *
 * The atlas (pure integer and half-integer arithmetic; ln3diff_amd/mesh.py atlas_layout / atlas_uvs are the host side of it):
 *   - texel (x, y) has its centre at (x + 0.5, y + 0.5); its flat index is y * T + x; 4 <= T <= 8192;
 *   - faces 2k and 2k + 1 share the square cell k of c x c texels whose origin is ((k % n) * c, (k / n) * c); n * n >= ceil(nf / 2),
 *     c >= 4, n * c <= T;
 *   - the cell-local texel (a, b) belongs to the even ("lower") face when a + b <= c - 1, otherwise to the odd ("upper") face;
 *   - the texels of a face >= nf (the absent odd face of the last cell, the cells behind it) and of the border strip beyond n * c belong
 *     to nobody;
 *   - the UV corners of face corners 0, 1, 2, cell-local in texel units: lower (0.5, 0.5) (c - 2.5, 0.5) (0.5, c - 2.5), upper
 *     (c - 0.5, c - 0.5) (2.5, c - 0.5) (c - 0.5, 2.5); both counter-clockwise.  A bilinear look-up anywhere in a face's UV triangle
 *     touches, with non-zero weight, only texels that face owns; the owned texels outside the triangle (the gutter, 1 - 1.5 texels)
 *     carry the same affine map extrapolated, so there is no dilation pass.
 *
 * Arguments are checked before anything touches the device: a null buffer, a count (nv, nf, P) below 1 or above 2^31 - 1, T < 4 or
 * T > 8192, n < 1, c < 4, n * c > T, nf > 2 * n * n, P > 8192 * 8192 or a fill outside [0, 255] returns LN3D_ERR_BAD_ARG.
 *
 * faces [nf, 3] int64 with every index in [0, nv) IS A PRECONDITION: the kernel reads verts at the indices it finds.  (The Python
 * wrapper checks it.)
 *
 * What the whole does NOT promise: more than half of the atlas is unused at the cell sizes of a dense mesh (the two UV triangles cover
 * (c - 3)^2 / c^2 of a cell - 1/16 at c = 4, 1/4 at c = 6, half only from c = 11 - the rest is gutter; the border strip and the spare
 * cells come on top); texel density is uniform per FACE, not per unit area, so a large triangle is sampled as coarsely as a small one is
 * finely; there is one field sample per texel, no supersampling; there is no mip-safe padding beyond the 1 - 1.5 texel gutter, so only
 * the full-resolution level is seam-free; and the colours are the field's values ON THE TRIANGLES, which for a simplified mesh lie off
 * the level set by the simplifier's error.
 */
#ifndef LN3D_MESHBAKE_H
#define LN3D_MESHBAKE_H
#include <stdint.h>
#include "ln3d.h"
#ifdef __cplusplus
extern "C" {
#endif

/* One thread per texel i = y * T + x.  An unowned texel gets owner[i] = -1 and points[i] = (0, 0, 0).  An owned texel gets owner[i] = its
 * face f and, with d = (float)(c - 3), (s, t) = (a / d, b / d) for a lower texel and ((c - 1 - a) / d, (c - 1 - b) / d) for an upper one,
 * v0, v1, v2 = verts[faces[f][0 .. 2]], per axis
 *     points[i] = (v0 + s * (v1 - v0)) + t * (v2 - v0)
 * in which every operation is one correctly rounded fp32 operation (no contraction into an fma), which is what numpy gives in float32. */
int ln3d_bake_points(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, int T, int n, int c, float* points, int32_t* owner,
                     void* stream);

/* tex[i][j] = fill where owner[i] < 0, otherwise (uint8) trunc(min(max(rgb[i][j], 0), 1) * 255), a NaN giving 0: the rule of the vertex
 * colours.  rgb [P, 3] f32, owner [P] int32, tex [P, 3] uint8. */
int ln3d_bake_pack(const float* rgb, const int32_t* owner, int64_t P, int fill, uint8_t* tex, void* stream);

#ifdef __cplusplus
}
#endif
#endif
