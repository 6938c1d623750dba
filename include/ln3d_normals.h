/* ln3d_normals.h - entry points of libln3d_hip.so for surface normals of the tri-plane density field: sigma and its exact gradient at
 * points, and per-ray normals at the expected-depth surface point of a finished render.  There is no reference counterpart (the
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
} ln3d_normals_args;

int ln3d_surface_normals(const ln3d_normals_args* a, void* stream);
int ln3d_surface_normals_f16(const ln3d_normals_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
