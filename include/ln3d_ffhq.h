/* ln3d_ffhq.h - entry points of libln3d_hip.so added for the FFHQ VAE decoder class
 * (vit/vit_triplane.py VAE_LDM_V4_vit3D_v3_conv3D_depth2_xformer_mha_PEinit_2d_sincos_uvit_RodinRollOutConv_4x4_lite_mlp_unshuffle_4XC_final:
 * a DINOv2 ViT-B decoder of TriplaneFusionBlockv3 blocks, then RodinConv3D4X_lite_mlp_as_residual, whose two convolutions are both
 * RodinRollOutConv3D_GroupConv, the first over 128-channel planes at 256 x 256).  Same conventions as ln3d.h (caller-owned device
 * pointers, stream as void*, 0 or a negative LN3D_ERR_* code, no allocation); the ABI number of ln3d.h covers them.  Everything else
 * the class runs goes through the ln3d.h / ln3d_shapenet.h kernels.
 */
#ifndef LN3D_FFHQ_H
#define LN3D_FFHQ_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* RodinRollOutConv3D_GroupConv (3 x 3, padding 1, groups = 3) of one object as an implicit GEMM, with the residual step of
 * conv_sr as its epilogue; no im2col matrix is written.  The conv input of plane i at (y, x) is
 * [x_i (C) | rowmean of plane (i+1) % 3 at y (C) | colmean of plane (i+2) % 3 at x (C)], all three parts zero outside the image.
 *   x        [3, H, W, C] channel-last, f32 (x_is_bf16 = 0, rounded to bf16 as ln3d_im2col3x3_rollout does) or bf16 (x_is_bf16 = 1)
 *   rowmean  f32 [3, H, C], colmean f32 [3, W, C] (ln3d_rollout_means of the same planes; rounded to bf16)
 *   w        bf16 [3, Cout, 27*C]: plane i's filters, K index (ky*3 + kx)*3C + k, the K order of ln3d_im2col3x3_rollout
 *   bias     f32 [3, Cout]
 *   base     f32 [3, bh, bw, Cout]: bh == H and bw == W: added as it is; else bilinear-resized to H x W on the fly (align_corners
 *            False, the arithmetic of ln3d_resize_add_lrelu)
 *   out      f32 [3, H, W, Cout] = base + leaky_relu(conv + bias, slope).  out must not overlap x (neighbouring tiles read x's
 *            halo); it may be base when bh == H and bw == W.
 * Products are bf16 x bf16 accumulated in fp32 (v_mfma_f32_32x32x16_bf16).
 * C % 16 == 0 (one MFMA K step), 16 <= C <= 128 (the 10 x 34 pixel tile and its pooled vectors are staged in LDS), Cout % 32 == 0. */
int ln3d_conv3x3_rollout_bf16(const void* x, int x_is_bf16, const float* rowmean, const float* colmean, const void* w_bf16,
                              const float* bias, const float* base, int bh, int bw, float* out, int H, int W, int C, int Cout,
                              float slope, void* stream);

/* ln3d_rollout_means (ln3d_shapenet.h) for bf16 planes x [N, H, W, C]: rowmean[n, y, c] = mean_x x[n, y, x, c],
 * colmean[n, x, c] = mean_y x[n, y, x, c], summed in fp32. */
int ln3d_rollout_means_bf16(const void* x_bf16, float* rowmean, float* colmean, int N, int H, int W, int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif
