/* ln3d_shapenet.h - entry points of libln3d_hip.so for the ShapeNet VAE decoder class
 * (vit/vit_triplane.py RodinSR_256_fusionv5_ConvQuant_liteSR_dinoInit3DAttn: a DINOv2 ViT-B decoder whose paired blocks add a
 * cross-plane attention, then the roll-out super-resolution convs RodinConv3D4X_lite_mlp_as_residual_lite).  Same conventions as
 * ln3d.h (caller-owned device pointers, stream as void*, 0 or a negative LN3D_ERR_* code, no allocation); the ABI number of ln3d.h
 * covers them.  Everything else the decoder runs (LayerNorm, the GEMMs with their bias / GELU / gate + residual epilogues, the
 * per-plane self-attention, the 3x3 im2col of the in-plane group conv, the posterior) goes through the ln3d.h / ln3d_encoder.h kernels.
 */
#ifndef LN3D_SHAPENET_H
#define LN3D_SHAPENET_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Cross-plane attention of Conv3DCrossAttentionBlockXformerMHANested (xformer_Conv3D_Aware_CrossAttention_xygrid): tokens of B
 * objects x 3 planes x (p x p), row (b*3 + i)*p*p + y*p + x.  The query of plane i at (y, x) attends to 2p keys: row y of plane
 * (i+1) % 3 (tokens (y, j)) and column x of plane (i+2) % 3 (tokens (j, x)), one softmax over all 2p.
 *   qkv f32 [B*3*p*p, ld]: q at columns [0, D), k at [D, 2D), v at [2D, 3D) (the fused [wq ; w_kv] projection), D = H * 64
 *   out bf16 [B*3*p*p, D], head h at columns h*64 ..
 * Each object only reads its own tokens (the reference's batched path re-orders rows across objects when B > 1; B = 1 agrees).
 * 1 <= p <= 32, Dh = 64; B * 3 * p * p * H < 2^31 (else LN3D_ERR_UNSUPPORTED). */
int ln3d_triplane_axis_attention(const float* qkv, int64_t ld, void* out_bf16, int B, int p, int H, float scale, void* stream);

/* decoder_pred output -> the two low-resolution inputs of conv_sr (unpatchify_triplane with patch P, then the short_cut's view):
 *   pred f32 [B, 3*S*S, P*P*C] (token (d, ty, tx), feature (py, px, c))
 *   planes f32 [B, 3, R, R, C] channel-last, R = S*P:  planes[b, d, Y, X, c] = pred[b, d*S*S + (Y/P)*S + X/P, ((Y%P)*P + X%P)*C + c]
 *   mixed bf16 [B, 3, R, R, C]: the short_cut's input x.reshape(B, C, 3, L): mixed[b, e, Y, X, k] = planes[b, (3k+e) / C, Y, X, (3k+e) % C]
 * C % 4 == 0. */
int ln3d_sr_unpatchify(const float* pred, float* planes, void* mixed_bf16, int B, int S, int P, int C, void* stream);

/* Bilinear resize (F.interpolate mode 'bilinear', align_corners False; for up-sampling antialias=True gives the same weights),
 * channel-last f32 [N, h, w, C] -> bf16 [N, Ho, Wo, C].  transpose = 1 writes the transposed image, y[n, Y, X] = resize(x)[n, X, Y]
 * (RodinConv3D4X_lite_mlp_as_residual's x.permute(0, 1, 3, 2) before its interpolate; then Ho must equal Wo).  C % 4 == 0. */
int ln3d_resize_bilinear_cl(const float* x, void* y_bf16, int N, int h, int w, int Ho, int Wo, int C, int transpose, void* stream);

/* out = resize(base) + leaky_relu(t, slope): base f32 [N, h, w, C] bilinear-resized as above to [N, Ho, Wo, C] (h == Ho, w == Wo:
 * base itself), t / out f32 [N, Ho, Wo, C] (out may alias t).  The residual step of conv_sr: x0 = res + act(conv3D_0(x)),
 * x = x0 + act(conv3D_1(x0)).  C % 4 == 0. */
int ln3d_resize_add_lrelu(const float* base, const float* t, float* out, int N, int h, int w, int Ho, int Wo, int C, float slope,
                          void* stream);

/* Row and column means of channel-last planes x f32 [N, H, W, C]: rowmean[n, y, c] = mean_x x[n, y, x, c],
 * colmean[n, x, c] = mean_y x[n, y, x, c] (the two pooled planes of RodinRollOutConv3D_GroupConv). */
int ln3d_rollout_means(const float* x, float* rowmean, float* colmean, int N, int H, int W, int C, void* stream);

/* im2col of RodinRollOutConv3D_GroupConv for plane i of one object, without the rolled-out tensor: the conv input of plane i at
 * (y, x) is [x_i (C) | rowmean of plane (i+1) % 3 at y (C) | colmean of plane (i+2) % 3 at x (C)], zero padded by 1.
 *   x f32 [3, H, W, C], rowmean f32 [3, H, C], colmean f32 [3, W, C] (one object)
 *   col bf16 [H*W, Kpad]: col[y*W + x, (ky*3 + kx)*3C + k] = input(y + ky - 1, x + kx - 1, k), columns >= 27C zero.
 * C % 4 == 0, Kpad % 4 == 0, Kpad >= 27C. */
int ln3d_im2col3x3_rollout(const float* x, const float* rowmean, const float* colmean, void* col_bf16, int plane, int H, int W, int C,
                           int Kpad, void* stream);

#ifdef __cplusplus
}
#endif
#endif
