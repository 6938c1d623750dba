/* ln3d_mx.h - entry points of libln3d_hip.so for the opt-in MX-FP8 path of the T23D DiT (DiT_TriLatent.set_matmul_precision('mxfp8')):
 * the QKV, fc1 and fc2 GEMMs of every block run on the block-scaled MFMA v_mfma_scale_f32_32x32x64_f8f6f4 (gfx950).  There is no
 * reference counterpart (the reference has no fp8 path); the bf16 path of ln3d.h stays the default.  Same conventions as ln3d.h
 * (caller-owned device pointers, stream as void*, 0 or a negative LN3D_ERR_* code, no allocation); the ABI number of ln3d.h covers them.
 *
 * Format: OCP Microscaling v1.0 MXFP8.
 *   - elements: OCP FP8 E4M3 ("e4m3fn": bias 7, no infinities, 0x7F / 0xFF NaN, max normal 448), NOT the MI300 e4m3fnuz encoding;
 *   - every 32 consecutive values along K (a "block") share one E8M0 scale byte s: value = element * 2^(s - 127);
 *   - quantizing a block: amax = max |x|; e = floor(log2(amax)) - 8 (8 = emax of E4M3), clamped to [-127, 127]; an all-zero block
 *     takes e = -127 (byte 0); scale byte = e + 127; element = RNE(x / 2^e) saturated to +-448 (then E4M3 with its subnormals,
 *     sign kept on values that round to zero).  The product x / 2^e is exact in f32 except where it lands in f32 subnormals.
 *   - non-finite values (ln3d_quantize_mx and ln3d_norm_modulate_mx; NOT the GELU_ERF epilogue, see there): amax is taken over the
 *     FINITE elements of a block; a block with no finite non-zero element takes scale byte 0; a NaN or +-Inf element is stored as the
 *     E4M3 NaN code with its sign kept (0x7F / 0xFF); the finite elements of the same block are quantized as if it were not there.
 *     Nothing changes for finite input.  The scaled MFMA reads 0x7F / 0xFF as NaN (measured on MI355X), so one NaN code in a GEMM
 *     operand makes its output row (X) or column (W) NaN and leaves every other element alone.
 * Memory layout of an MXFP8 matrix [R, K] (K % 32 == 0):
 *   q: e4m3 bytes, row r at q + r * ldq (row-major, K contiguous);
 *   s: E8M0 bytes, row-major [R, K / 32]: the scale of elements q[r, 32b .. 32b + 31] is s[r * lds + b].
 * The GEMM reads one 4-byte scale word per row and 128-wide K stage (scales of 4 blocks), so its operands need K % 128 == 0,
 * lds % 4 == 0 and 4-byte aligned scale rows.
 */
#ifndef LN3D_MX_H
#define LN3D_MX_H
#include <stdint.h>
#include "ln3d.h"
#ifdef __cplusplus
extern "C" {
#endif

/* x [R, K] (row stride ldx elements; x_bf16 = 1: raw bfloat16, 0: f32) -> q e4m3 [R, ldq bytes] + s E8M0 [R, lds bytes], the
 * quantizer above, bit for bit.  K % 32 == 0, ldx >= K, ldq >= K, lds >= K / 32.  Used at weight-pack time and as the generic
 * activation path. */
int ln3d_quantize_mx(const void* x, int x_bf16, int64_t ldx, int R, int K, void* q, int64_t ldq, void* s, int64_t lds, void* stream);

/* out = epi( deq(Xq)[M, K] . deq(Wq)[N, K]^T + bias ), fp32 accumulation on v_mfma_scale_f32_32x32x64_f8f6f4 (one scale per lane
 * and MFMA operand: lane l's scale covers K values 32 (l >> 5) + [0, 32) of the 64-wide step, row l & 31).  K % 128 == 0, N % 4 == 0,
 * ldx % 16 == 0, ldw % 16 == 0 (16-byte rows), ldxs / ldws % 4 == 0.  Ragged M and N are fine; only columns < N of rows < M are
 * written, so ldo > N leaves the other columns of out untouched.
 * `epilogue` takes the ln3d.h values:
 *   LN3D_EPI_F32       out0 f32 [M, ldo]
 *   LN3D_EPI_HEADS     out{0,1,2} bf16 split into heads, exactly as ln3d_gemm_bf16 (tokens, tok_pad, heads, head_dim, transpose_mask,
 *                      head_dim_pad; V^T in the attention kernel's key order); no fused qk-norm.  A transposed output permutes
 *                      the tokens inside every group of 16, so transpose_mask != 0 needs tok_pad % 16 == 0
 *   LN3D_EPI_GELU_ERF  erf-GELU, then MXFP8 OUT: out0 e4m3 [M, ldo bytes], out_scale E8M0 [M, ldos]; every 32-column block of a
 *                      row is quantized by the rule above in the epilogue.  N % 32 == 0, ldo % 4 == 0.  FINITE INPUT ASSUMED: the
 *                      non-finite rule is not applied here (it cost fc1 2.5 %, profiles/mx_elements.md).  A NaN pre-activation
 *                      (a NaN code in an operand gives one) is stored as +-448 and ignored by the amax; an Inf takes the block's
 *                      scale to 2^120, so its finite neighbours become 0
 *   LN3D_EPI_GATE_RES  out0 f32 [M, ldo] += gate * (.); optional out1 bf16 copy of the new residual (gate as in ln3d_gemm_bf16)
 */
typedef struct {
  const void* Xq; const void* Xs; int64_t ldx; int64_t ldxs;    /* tokens: e4m3 [M, ldx], scales [M, ldxs] */
  const void* Wq; const void* Ws; int64_t ldw; int64_t ldws;    /* weight (torch.nn.Linear layout): e4m3 [N, ldw], scales [N, ldws] */
  const float* bias;                                            /* [N] or NULL */
  int M, N, K;
  int epilogue;
  void* out0; void* out1; void* out2;
  int64_t ldo;
  void* out_scale; int64_t ldos;                                /* GELU_ERF: E8M0 scales of out0 */
  const float* gate; int gate_rows; int64_t gate_ld;            /* GATE_RES */
  int tokens, tok_pad, heads, head_dim, transpose_mask, head_dim_pad;   /* HEADS */
} ln3d_gemm_mx_args;
int ln3d_gemm_mxfp8(const ln3d_gemm_mx_args* a, void* stream);

/* ln3d_norm_modulate (kind 0 LayerNorm or kind 1 RMSNorm, weight, shift / scale / mod_rows / mod_ld as there) with an MXFP8 output:
 * a->y receives e4m3 [rows, D] (row stride D bytes), y_scale E8M0 [rows, D / 32].  The per-row f32 math is that of
 * ln3d_norm_modulate; each 32-feature block is then quantized by the rule above.  The PixArt tables and rows_in / rows_out are not
 * supported here (NULL / 0).  D % 128 == 0, D <= 1536.  A row whose fp32 statistics are not finite - it holds a NaN or an Inf, or its
 * sum of squares overflows fp32 (|x| beyond ~2^60 at these widths) - is written as the NaN code throughout, with scale bytes 0. */
int ln3d_norm_modulate_mx(const ln3d_norm_args* a, void* y_scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif
