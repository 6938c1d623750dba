/* ln3d_meshsnap.h - entry points of libln3d_hip.so for putting points (the vertices of an exported mesh) back on a level set of the
 * tri-plane density field: a damped Newton projection along the field's gradient, sigma(p) = level.  Marching-cubes vertices are linear
 * interpolations of grid samples, clustering and smoothing move them further off; this is the step that undoes it before colours, normals
 * and texels are taken.  There is no reference counterpart; everything here is opt-in and changes no other output.  Same conventions as
 * ln3d_normals.h (caller-owned device pointers, stream as void*, 0 or a negative LN3D_ERR_* code, asynchronous on the stream, no
 * allocation, one launch per call, every workgroup stages the decoder from the caller's weights itself).  The entry points are additions
 * to ABI 10 of ln3d.h with scalar and pointer arguments only and no new constant; they are bound from _lib.PROTOTYPES.
 *
 * The field and its gradient are exactly those of ln3d_query_points_grad (ln3d_normals.h): field(p) = (sigma, d sigma / d p in world
 * units), all fp32, one device function for both.  The loop, per point, all arithmetic fp32, every operation outside field() rounded once
 * (no fused multiply-add), sums of three terms taken left to right:
 *
 *     p = in;  (s, g) = field(p);  r = s - level;  f = 1;  evals = 1
 *     repeat at most `iters` times:
 *         g2 = gx*gx + gy*gy + gz*gz
 *         if in, r or g2 is not finite, or g2 == 0:   stalled, stop
 *         if |r| <= tol:                          converged, stop
 *         len = |r| / sqrt(g2);   a = f * min(1, max_step / len);   t = (a * r) / g2
 *         c = p - t * g                                                              (per axis)
 *         if not |c - in| <= max_dist:            f = f / 2, next iteration          (no evaluation; |.| = sqrt of the sum of squares)
 *         (sc, gc) = field(c);  rc = sc - level;  evals += 1
 *         if |rc| < |r|:  p, r, g, f = c, rc, gc, 1      else  f = f / 2
 *     out = p;  residual = r;  state = 0 if |r| <= tol, else 2 if stalled, else 1 (out of iterations)
 *
 * What follows from it:
 *   - out is always the best iterate seen: |residual| never exceeds |sigma(in) - level|;
 *   - no point ends farther than max_dist from where it started (the distance is the fp32 value computed above: a few ulps of slack);
 *   - a Newton step is never longer than max_step, the first one included;
 *   - iters = 0 is a pure evaluation: out has the input's bits, evals = 1, state = 0 or 1;
 *   - a point with a NaN or infinite coordinate, and one whose taps all lie in the padding (gradient exactly 0), stalls with its input
 *     bits (its residual is still the field's value there: planes that such a coordinate misses contribute their padding, 0); state 0
 *     holds if and only if |residual| <= tol, stalled or not;
 *   - residual is the kernel's own sigma at out minus level - what ln3d_query_points_grad returns there, minus level;
 *   - evals counts field evaluations, between 1 and iters + 1; a lane that is done waits only for the slowest lane of its wave.
 *
 * level, max_step and max_dist are in the units of the field and of world space.  Arguments are checked before anything touches the
 * device: a null buffer, P below 1 or above 2^31 - 1, iters outside [0, 64], a level / tol / max_step / max_dist that is not finite,
 * tol < 0, max_step <= 0, max_dist < 0, planes the other entry points refuse, or a points_out that overlaps points_in returns
 * LN3D_ERR_BAD_ARG.
 *
 * What the whole does NOT promise: only the points are put on the level set, not the interiors of the triangles between them; points move
 * independently, so faces can fold or flip and thin sheets can collapse onto each other; a point may land on a different sheet of the
 * level set within max_dist; the gradient jumps where a projected coordinate crosses a texel centre, so convergence is not guaranteed and
 * `state` says which points did not converge; and snapping partly undoes the tangential regularity that smoothing produced.
 */
#ifndef LN3D_MESHSNAP_H
#define LN3D_MESHSNAP_H
#include <stdint.h>
#include "ln3d.h"
#ifdef __cplusplus
extern "C" {
#endif

/* planes [3, H, W, 32] channel-last f32, points_in [P, 3] f32, dec_w0 [64, 32], dec_b0 [64], dec_w1 / dec_b1: at least row 0 ->
 * points_out [P, 3] f32, residual [P] f32, state [P] int32 (0 converged, 1 out of iterations, 2 stalled), evals [P] int32. */
int ln3d_snap_points(const float* planes, int H, int W, const float* points_in, int64_t P, const float* dec_w0, const float* dec_b0,
                     const float* dec_w1, const float* dec_b1, float box_warp, float level, int iters, float tol, float max_step,
                     float max_dist, float* points_out, float* residual, int32_t* state, int32_t* evals, void* stream);
/* the same with binary16 texels (include/ln3d_planes16.h); on planes whose values are representable in binary16 both return the same bits */
int ln3d_snap_points_f16(const void* planes_f16, int H, int W, const float* points_in, int64_t P, const float* dec_w0, const float* dec_b0,
                         const float* dec_w1, const float* dec_b1, float box_warp, float level, int iters, float tol, float max_step,
                         float max_dist, float* points_out, float* residual, int32_t* state, int32_t* evals, void* stream);

#ifdef __cplusplus
}
#endif
#endif
