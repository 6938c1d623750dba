/* ln3d_encoder.h - entry points of libln3d_hip.so for the multi-view VAE encoder of the released tri-plane VAE
 * (`mv-sd-dit-dynaInp-trilatent`: ldm/modules/diffusionmodules/model.py MVEncoderGSDynamicInp over Encoder, and the posterior of
 * vit/vit_triplane.py vae_encode / vae_reparameterization).  Same conventions as ln3d.h (caller-owned device pointers, stream as
 * void*, 0 or a negative LN3D_ERR_* code, no allocation, no random numbers drawn inside); the ABI number of ln3d.h covers them.
 * Everything else the encoder runs (conv_in, ResnetBlocks, SpatialTransformer3D, norm_out / conv_out) goes through the ln3d.h
 * kernels: ln3d_nchw_to_cl_bf16, ln3d_im2col3x3, ln3d_gemm_bf16, ln3d_groupnorm_swish, ln3d_norm_modulate, ln3d_attention_bf16
 * (the joint attention over all frames of an object: Dh 64, F * H * W keys), ln3d_geglu.
 */
#ifndef LN3D_ENCODER_H
#define LN3D_ENCODER_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Encoder Downsample (model.py:72-91): F.pad(x, (0, 1, 0, 1)) then a 3x3 conv with stride 2 and padding 0 - the zero row / column
 * is on the bottom / right only, unlike ln3d_im2col3x3_strided (padding 1 on every side).  x bf16 channel-last [N, H, W, C],
 * Ho = (H - 2) / 2 + 1, Wo = (W - 2) / 2 + 1 (H, W >= 2), col bf16 [N * Ho * Wo, Kpad]:
 * col[(n*Ho + oy)*Wo + ox, (ky*3 + kx)*C + c] = x[n, 2*oy + ky, 2*ox + kx, c] (0 at or past H / W), columns >= 9C zero.
 * C % 8 == 0, Kpad % 8 == 0, Kpad >= 9C. */
int ln3d_im2col3x3_pad01(const void* x_bf16, void* col_bf16, int N, int H, int W, int C, int Kpad, void* stream);

/* Frame pooling of MVEncoderGSDynamicInp.forward (model.py:614-623): h f32 channel-last [B*F, HW, C] (F consecutive frames per
 * object) -> out f32 NCHW [B, C, HW] = sum over the F frames / F. */
int ln3d_frame_mean(const float* h, float* out, int B, int F, int HW, int C, void* stream);

/* Posterior of the tri-plane VAE, fused from the encoder output to both latent layouts (vit_triplane.py:912-933 vae_encode,
 * :1152-1199 vae_reparameterization, distributions.py:44-88 DiagonalGaussianDistribution(soft_clamp=True)).  C = ldm_embed_dim = 4.
 *   h: f32, element (frame m, pixel p, channel k < 6C) at h[m * s_frame + p * s_pix + k * s_ch]; frames b*F .. b*F+F-1 are averaged
 *      (F = 1: h is the pooled encoder output itself, e.g. NCHW with s_frame = 6C*HW, s_pix = 1, s_ch = HW)
 *   qw [6C, 2C], qb [6C]: superresolution.quant_conv (1x1, groups = 3: output o reads inputs (o / 2C) * 2C ..)
 *   moments [B, 6C, HW] are viewed as [B, 2C, 3, HW]: mean channel (c, n) = moment c*3 + n, logvar (c, n) = moment (C + c)*3 + n
 *   (this view crosses the quant_conv groups, as the reference's reshape does)
 *   logvar = 20 tanh(logvar / 20); std = exp(logvar / 2); var = exp(logvar)
 *   z = eps ? mean + std * eps : mean                      eps: f32 [B, C, 3, HW] or NULL (mode)
 *   log_q = -0.5 ((z - mean) / var)^2 - 0.5 log(2 pi) - logvar;  entropy = logvar + 0.5 (log(2 pi) + 1)
 * Outputs f32: mean, logvar, z, log_q, entropy [B, C, 3, HW] (z is also latent_normalized_2Ddiffusion [B, 3C, H, W]: channel c*3 + n),
 * latent_tok [B, 3*HW, C] (latent_normalized: token n*HW + p). */
int ln3d_mv_posterior(const float* h, int64_t s_frame, int64_t s_pix, int64_t s_ch, const float* qw, const float* qb, const float* eps,
                      float* mean, float* logvar, float* z, float* latent_tok, float* log_q, float* entropy, int B, int F, int HW, int C,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif
