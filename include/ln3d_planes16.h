/* ln3d_planes16.h - entry points of libln3d_hip.so for the opt-in fp16 tri-plane texels of the ray-marcher and the point query
 * (Triplane.set_plane_precision('fp16')).  There is no reference counterpart (the reference samples fp32 planes); the fp32 planes of
 * ln3d.h stay the default.  Same conventions as ln3d.h (caller-owned device pointers, stream as void*, 0 or a negative LN3D_ERR_* code,
 * no allocation); the ABI number of ln3d.h covers them.
 *
 * Format: a STORAGE format, not a change of arithmetic.
 *   - layout: channel-last [NP, 3, H, W, 32] like the fp32 planes, every element an IEEE 754 binary16 (1 sign, 5 exponent, 10 mantissa
 *     bits, subnormals kept): a texel of 32 channels is 64 bytes instead of 128, a 256 x 256 tri-plane 12.5 MB instead of 25 MB;
 *   - conversion from f32: round to nearest, ties to even; a value beyond +-65504 (the largest binary16) saturates to +-65504, never
 *     to an infinity (an f32 infinity saturates too: a texel is never infinite); a NaN stays a NaN; values at or below half the
 *     smallest binary16 subnormal round to a zero that keeps the sign.  That is torch's `x.clamp(-65504, 65504).half()`, bit for bit;
 *   - the kernels widen every texel value to f32 (exact) and evaluate the bilinear taps, the plane sum, the decoder and the compositing
 *     exactly as the fp32 entry points do, operation for operation: on planes whose values are representable in binary16 the two
 *     entry points return the same bits.
 */
#ifndef LN3D_PLANES16_H
#define LN3D_PLANES16_H
#include <stdint.h>
#include "ln3d.h"
#ifdef __cplusplus
extern "C" {
#endif

/* planes_nchw [NP, 3 * C, H, W] f32 (the reference's '(n c) h w') -> planes_nhwc_f16 [NP, 3, H, W, C] binary16 by the rule above.
 * C == 32. */
int ln3d_planes_to_channel_last_f16(const float* planes_nchw, void* planes_nhwc_f16, int NP, int C, int H, int W, void* stream);

/* src f32 -> dst binary16 by the rule above, element for element (n elements, any layout): the channel-last f32 planes a decoder wrote,
 * brought to the texel format without a detour through NCHW. */
int ln3d_planes_f32_to_f16(const float* src, void* dst, int64_t n, void* stream);

/* ln3d_render_triplane with a->planes pointing at binary16 channel-last planes [NP, 3, H, W, 32]; every other field, the validation
 * and the scratch are those of ln3d_render_triplane.  Serves the Objaverse 64 + 64 kernel and the generic presets alike. */
int ln3d_render_triplane_f16(const ln3d_render_args* a, void* stream);

/* ln3d_query_points with binary16 channel-last planes [3, H, W, 32]. */
int ln3d_query_points_f16(const void* planes_f16, int H, int W, const float* points, int64_t P, const float* dec_w0, const float* dec_b0,
                          const float* dec_w1, const float* dec_b1, float box_warp, float* sigma, float* rgb, float* scalars, void* stream);

#ifdef __cplusplus
}
#endif
#endif
