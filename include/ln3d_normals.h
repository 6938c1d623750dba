/* ln3d_normals.h - entry points of libln3d_hip.so for surface normals of the tri-plane density field: sigma and its exact gradient at
 * points, and per-ray normals of a finished render: at its expected-depth surface point, or (mode 1 of the same entry points, described
 * behind the argument struct) composited over its samples by the marcher's own weights.  There is no reference counterpart (the
 * reference's `return_surface` is something else and stays refused); everything here is opt-in and changes no other output.  Same
 * conventions as ln3d.h (caller-owned device pointers, stream as void*, 0 or a negative LN3D_ERR_* code, asynchronous on the stream,
 * no allocation); the ABI number of ln3d.h covers them.  No scratch buffer: every workgroup stages the decoder from the caller's
 * weights itself.
 *
 * The field is the one ln3d_query_points evaluates: g = 2 / box_warp * p, projections (x,y) (y,z) (z,x), bilinear taps with zero
 * padding and align_corners = False, mean over the three planes, FC(32 -> 64, gain 1/sqrt 32) - softplus (beta 1, threshold 20) -
 * row 0 of FC(64 -> 4, gain 1/sqrt 64).  The gradient is the derivative of exactly that expression: the bilinear derivative per plane
 * (an out-of-range tap counts as 0, so a border texel pulls towards zero), sigmoid(h) per hidden unit (1 where h > 20), output row 0,
 * and the factor 2 / box_warp: d sigma / d p in world units.  It is discontinuous where a projected coordinate crosses a texel centre;
 * there the kernel returns the derivative of the bilinear piece its own fp32 coordinate falls in.  All arithmetic is fp32 (no bf16
 * split: sigma differs from ln3d_query_points' in the last bits and is the more accurate of the two); binary16 texels are widened
 * inside the multiply-add, and on planes whose values are representable in binary16 the f32 and f16 entry points return the same bits.
 */
#ifndef LN3D_NORMALS_H
#define LN3D_NORMALS_H
#include <stdint.h>
#include "ln3d.h"
#ifdef __cplusplus
extern "C" {
#endif

/* planes [3, H, W, 32] channel-last f32, points [P, 3] -> sigma [P], grad [P, 3] (d sigma / d p).  dec_w1 / dec_b1: at least row 0. */
int ln3d_query_points_grad(const float* planes, int H, int W, const float* points, int64_t P, const float* dec_w0, const float* dec_b0,
                           const float* dec_w1, const float* dec_b1, float box_warp, float* sigma, float* grad, void* stream);
/* the same with binary16 texels (include/ln3d_planes16.h) */
int ln3d_query_points_grad_f16(const void* planes_f16, int H, int W, const float* points, int64_t P, const float* dec_w0,
                               const float* dec_b0, const float* dec_w1, const float* dec_b1, float box_warp, float* sigma, float* grad,
                               void* stream);

typedef struct ln3d_normals_args {
  const void* planes;          /* [NP, 3, H, W, 32] channel-last, f32 or binary16 (the entry point says which) */
  int H, W;
  const int32_t* plane_index;  /* [V] */
  const float* cams;           /* [V, 25] (cam2world 4x4 row-major, intrinsics 3x3); may be NULL with explicit rays and space == 0 */
  int V, res;                  /* camera rays: a res x res image per view, generated exactly as ln3d_render_triplane generates them */
  const float* ray_o;          /* optional explicit rays [V, M, 3] (both or neither); then M = rays_per_view */
  const float* ray_d;
  int rays_per_view;           /* 0 = res * res */
  const float* dec_w0; const float* dec_b0; const float* dec_w1; const float* dec_b1;
  float box_warp;
  const float* depth;          /* [V, M] and */
  const float* wsum;           /* [V, M]: outputs of a finished ln3d_render_triplane call over the same rays.  depth is that call's OUTPUT, i.e.
                                  sum w z clamped to the call's [min, max] sample depth: on a ray whose wsum is just above the threshold the clamp
                                  can lift it, and depth / wsum then lies behind the unclamped expected depth */
  float mask_threshold;        /* in (0, 1]: rays with wsum < mask_threshold (or a NaN wsum) get the zero vector */
  int space;                   /* 0 = world, 1 = camera (the transpose of the view's cam2world rotation is applied; needs cams) */
  float* normal;               /* out [V, 3, M]: -grad sigma / |grad sigma| at p = o + (depth / wsum) d (density falls towards the outside);
                                  0 where |grad sigma| is 0 or not finite */
  float* points;               /* optional out [V, M, 3]: p of every ray with wsum >= mask_threshold, 0 for the others */
  /* ---- appended for the composited mode; all zero = the call above, bit for bit ---- */
  int mode;                    /* 0 = the normal at the expected-depth point (everything above); 1 = volume-composited (below) */
  int samples;                 /* mode 1: T = S + NI sorted samples per ray, 2 ... 256 */
  const float* weights;        /* mode 1: [V, M, T - 1] and */
  const float* coords;         /* mode 1: [V, M, T, 3]: the `weights` / `all_coords` outputs of a finished ln3d_render_triplane call over the same rays */
  float weight_floor;          /* mode 1: finite, >= 0: a sample is evaluated iff its weight omega_j > weight_floor */
  float* accum;                /* mode 1: optional out [V, 3, M]: the un-normalised world-space sum N */
} ln3d_normals_args;

/* mode 1, the volume-composited normal (the Ref-NeRF convention): the per-sample normals are composited by the marcher's own weights
 * exactly as MipRayMarcher2 composites colour, by interval midpoints of the endpoint values,
 *     N = sum_k w_k (n_k + n_{k+1}) / 2 = sum_j omega_j n_j,
 *     omega_0 = 0.5 w_0,  omega_j = 0.5 (w_{j-1} + w_j) for 1 <= j <= T - 2,  omega_{T-1} = 0.5 w_{T-2}   (each operation rounded to fp32),
 *     n_j = -grad sigma / |grad sigma| at coords[ray, j], scaled by the largest component first; 0 where the gradient is 0 or not finite.
 * Sample j is evaluated if and only if omega_j > weight_floor: a zero, negative or NaN omega is never evaluated and contributes exactly
 * 0, so with weight_floor = 0 the result is the exact sum, and with a floor f the omitted mass is at most f times the number of skipped
 * samples (|N| moves by at most that much).  Most samples of a bounded scene carry exactly zero weight; the skip is what makes this
 * affordable.  One wavefront per ray: lane l owns the samples j = l (mod 64) in ascending j, per axis s = fl(s + fl(omega_j n_j)), and
 * the 64 partial sums meet in a fixed butterfly (xor 32, 16, 8, 4, 2, 1): no float atomics, the same bits from run to run.  All of it
 * is fp32, one rounding per operation outside the gradient itself.  The price of that layout: a ray with few weighted samples leaves
 * most of its 64 lanes idle through the gradient evaluation (~600 instructions), so the launch costs about one gradient per PASS that
 * holds any weight, not per weighted sample.
 * Outputs: accum = N (world space); normal = N / |N| (largest component first) where wsum >= mask_threshold and N is finite and not
 * zero, the zero vector otherwise; space == 1 rotates the unit result.  `depth` is not read and may be NULL, `points` is not written,
 * and the rays are not read: M = rays_per_view, or res * res where that is 0; cams only for space == 1.  wsum is the mask and should
 * be that of the render whose picture the normals go with.  LN3D_ERR_BAD_ARG before any launch: a mode other than 0 / 1, samples
 * outside 2 ... 256, a NULL weights / coords, a weight_floor that is negative or not finite.
 * The gradient is that of the UNFILTERED field (a sample the marcher's bbox filter zeroed carries weight 0 and is skipped, nothing
 * else knows about the filter) and jumps at texel centres like every gradient of this header; where the normals along a ray disagree
 * N is short (|N| / wsum < 1), and `normal` is normalised anyway. */

int ln3d_surface_normals(const ln3d_normals_args* a, void* stream);
int ln3d_surface_normals_f16(const ln3d_normals_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
