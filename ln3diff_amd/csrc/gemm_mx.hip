// MX-FP8 (OCP MXFP8: e4m3fn elements, one E8M0 scale per 32 values along K) path of the T23D DiT for gfx950 (include/ln3d_mx.h):
// the quantizer, LayerNorm + adaLN modulate with an MXFP8 output, and the GEMM on the block-scaled MFMA
// v_mfma_scale_f32_32x32x64_f8f6f4 with the bf16 GEMM's fused epilogues (gemm_epi.h) plus an erf-GELU epilogue that writes MXFP8.
//
// GEMM design (from gemm_bf16.hip's LDS-DMA ring):
//  * A = weight tile (rows = output features), B = token tile, so the accumulator layout is the bf16 GEMM's and its staged
//    epilogues apply unchanged.  One MFMA multiplies 32 x 32 x 64; the scale lane l passes (byte 0: op_sel 0 after a shift) applies
//    to K values 32 (l >> 5) + [0, 32) of row l & 31, which lanes l and l ^ 32 hold in 16-byte halves (operand map at the K loop).
//  * K stage = 128 K values = one 128-byte row per operand row, staged HBM/L2 -> LDS by global_load_lds_dwordx4 (1 KB = 8 rows per
//    instruction, 16-byte chunk c of row r at chunk c ^ ((r >> 1) & 7): conflict-free ds_read_b128 fragment reads), the 4 scale
//    bytes of every row and stage by global_load_lds_dword (64 rows per instruction) into the same slot.
//  * Tiles of 128 features x 128 tokens, 4 waves of 64 x 64 (2 x 2 MFMA tiles, 8 MFMAs per stage), two 33 KB slots: stage s+1 is
//    in flight while stage s multiplies, stage s+2 is issued into slot s once every wave has read it; two workgroups per CU.
//    Measured at the configs[1] shapes (QKV / fc1 / fc2 in us): 78 / 96 / 81 here; 256 x 128 tiles with three slots (one workgroup
//    per CU) 78 / 103 / 84; 128 x 128 with three slots 110 / 137 / 87; 256 x 256 (8 waves of 64 x 128, two slots) 102 / 109 / 109.
#include "gemm_epi.h"
#include "../../include/ln3d_mx.h"

typedef __attribute__((ext_vector_type(8))) int i32x8;

// ------------------------------------------------------------------------------------------------------------ quantizer helpers
// e = floor(log2(amax)) - 8 clamped to [-127, 127]; 0 and f32-subnormal amax (floor(log2) <= -127) give -127
__device__ __forceinline__ int mx_exp(float amax) {
  const int be = (int)((__float_as_uint(amax) >> 23) & 0xffu);
  return be == 0 ? -127 : max(be - 135, -127);                       // be <= 254: e <= 119, the upper clamp never binds
}
// non-finite rule (ln3d_mx.h): NaN and +-Inf take no part in a block's amax and are stored as the E4M3 NaN code with their sign
__device__ __forceinline__ bool mx_nonfinite(float x) { return __builtin_amdgcn_class(x, 0x207); }      // sNaN | qNaN | -Inf | +Inf
__device__ __forceinline__ float mx_fin_abs(float x) { return mx_nonfinite(x) ? 0.f : fabsf(x); }
// v (already divided by the block scale) -> OCP e4m3fn bits: saturate to 448, round to nearest even, subnormals below 2^-6
__device__ __forceinline__ uint32_t e4m3_rne(float v) {
  const uint32_t sign = (__float_as_uint(v) >> 24) & 0x80u;
  const float a = fminf(fabsf(v), 448.f);
  if (a < 0.015625f) return sign | (uint32_t)__builtin_rintf(a * 512.f);     // subnormal steps of 2^-9 (8 = the smallest normal)
  uint32_t u = __float_as_uint(a);
  u += 0x7ffffu + ((u >> 20) & 1u);                                          // RNE to 3 mantissa bits (448 is representable)
  return sign | (((u >> 23) - 120u) << 3) | ((u >> 20) & 7u);
}
// x / 2^e -> e4m3 bits; the class and the sign of a non-finite x are taken from x itself, not from the scaled value
__device__ __forceinline__ uint32_t e4m3_of(float x, int e) {
  const uint32_t c = e4m3_rne(__builtin_amdgcn_ldexpf(x, -e));
  return mx_nonfinite(x) ? (((__float_as_uint(x) >> 24) & 0x80u) | 0x7fu) : c;
}
__device__ __forceinline__ uint32_t e4m3x4(float a, float b, float c, float d, int e) {
  return e4m3_of(a, e) | (e4m3_of(b, e) << 8) | (e4m3_of(c, e) << 16) | (e4m3_of(d, e) << 24);
}
// the same for finite input only (the GELU epilogue: the class test and the two selects per element cost fc1 2.5 %, profiles/mx_elements.md)
__device__ __forceinline__ uint32_t e4m3x4_finite(float a, float b, float c, float d, int e) {
  return e4m3_rne(__builtin_amdgcn_ldexpf(a, -e)) | (e4m3_rne(__builtin_amdgcn_ldexpf(b, -e)) << 8) |
         (e4m3_rne(__builtin_amdgcn_ldexpf(c, -e)) << 16) | (e4m3_rne(__builtin_amdgcn_ldexpf(d, -e)) << 24);
}

// ------------------------------------------------------------------------------------------------------------ ln3d_quantize_mx
// one thread per 32-value block
template <bool BF16>
__global__ __launch_bounds__(256) void quantize_mx_kernel(const void* x, int64_t ldx, int R, int nb, uint8_t* q, int64_t ldq, uint8_t* s,
                                                          int64_t lds) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= (int64_t)R * nb) return;
  const int r = (int)(id / nb), b = (int)(id - (int64_t)r * nb);
  float v[32];
  if constexpr (BF16) {
    const bf16_t* xr = (const bf16_t*)x + (int64_t)r * ldx + 32 * b;
#pragma unroll
    for (int i = 0; i < 32; ++i) v[i] = bf2f(xr[i]);
  } else {
    const float* xr = (const float*)x + (int64_t)r * ldx + 32 * b;
#pragma unroll
    for (int i = 0; i < 32; ++i) v[i] = xr[i];
  }
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 32; ++i) amax = fmaxf(amax, mx_fin_abs(v[i]));
  const int e = mx_exp(amax);
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = e4m3x4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3], e);
  uint32_t* qr = reinterpret_cast<uint32_t*>(q + (int64_t)r * ldq + 32 * b);
#pragma unroll
  for (int i = 0; i < 8; ++i) qr[i] = w[i];
  s[(int64_t)r * lds + b] = (uint8_t)(e + 127);
}

extern "C" int ln3d_quantize_mx(const void* x, int x_bf16, int64_t ldx, int R, int K, void* q, int64_t ldq, void* s, int64_t lds,
                                void* stream) {
  if (!x || !q || !s || R <= 0 || K <= 0 || (K % 32) != 0 || ldx < K || ldq < K || lds < K / 32) return LN3D_ERR_BAD_ARG;
  if ((ldq % 4) != 0 || ((uintptr_t)q & 3) != 0) return LN3D_ERR_BAD_ARG;                   // 4-byte element stores
  const int nb = K / 32;
  const int64_t n = (int64_t)R * nb;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (x_bf16) hipLaunchKernelGGL((quantize_mx_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, x, ldx, R, nb, (uint8_t*)q, ldq, (uint8_t*)s, lds);
  else hipLaunchKernelGGL((quantize_mx_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, x, ldx, R, nb, (uint8_t*)q, ldq, (uint8_t*)s, lds);
  return ln3d_check_launch();
}

// ------------------------------------------------------------------------------------------------------------ ln3d_norm_modulate_mx
// dit_ops.hip's norm_modulate_kernel with an MXFP8 store: a lane owns 8 consecutive features per 512-column chunk, so the 4 lanes of a
// quad own one 32-feature block (amax over the quad by two xor shuffles); 8 bytes per lane, the scale byte by the quad's first lane.
struct NormMxP {
  const float* x; uint8_t* y; uint8_t* ys; int64_t rows; int D; int kind; float eps; const float* weight;
  const float* shift; const float* scale; int mod_rows; int64_t mod_ld;
};
template <int MV8, bool FULL>
__global__ __launch_bounds__(256) void norm_modulate_mx_kernel(NormMxP p) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.rows) return;                                           // wave-uniform
  const float* xr = p.x + row * p.D;
  float4 v[MV8][2], sc[MV8][2], sh[MV8][2];
  bool ok[MV8];
#pragma unroll
  for (int i = 0; i < MV8; ++i) {
    ok[i] = FULL ? (i * 512 < p.D) : (i * 512 + lane * 8 < p.D);
#pragma unroll
    for (int k = 0; k < 2; ++k)
      v[i][k] = ok[i] ? *reinterpret_cast<const float4*>(xr + i * 512 + lane * 8 + 4 * k) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (p.scale) {
    const int64_t mrow = (row / p.mod_rows) * p.mod_ld;
#pragma unroll
    for (int i = 0; i < MV8; ++i)
      if (ok[i]) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int d = i * 512 + lane * 8 + 4 * k;
          sc[i][k] = *reinterpret_cast<const float4*>(p.scale + mrow + d);
          sh[i][k] = *reinterpret_cast<const float4*>(p.shift + mrow + d);
        }
      }
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MV8; ++i)
#pragma unroll
    for (int k = 0; k < 2; ++k) s += (v[i][k].x + v[i][k].y) + (v[i][k].z + v[i][k].w);
  float mean = 0.f, var;
  if (p.kind == 0) {
    mean = wave_sum_dpp(s) / p.D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MV8; ++i)
      if (ok[i]) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const float a = v[i][k].x - mean, b = v[i][k].y - mean, c = v[i][k].z - mean, d = v[i][k].w - mean;
          q += (a * a + b * b) + (c * c + d * d);
        }
      }
    var = wave_sum_dpp(q) / p.D;
  } else {
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MV8; ++i)
#pragma unroll
      for (int k = 0; k < 2; ++k)
        q += (v[i][k].x * v[i][k].x + v[i][k].y * v[i][k].y) + (v[i][k].z * v[i][k].z + v[i][k].w * v[i][k].w);
    var = wave_sum_dpp(q) / p.D;
  }
  // a row whose statistics are not finite (a NaN or Inf element, or squares that overflow f32) is NaN throughout: rsqrtf(Inf) = 0 would
  // turn the finite elements of an RMSNorm row that holds an Inf into zeros
  const float rstd = mx_nonfinite(var) ? __builtin_nanf("") : rsqrtf(var + p.eps);
#pragma unroll
  for (int i = 0; i < MV8; ++i) {
    if (FULL && !ok[i]) continue;                                       // wave-uniform
    float4 o[2];
    float amax = 0.f;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int d = i * 512 + lane * 8 + 4 * k;
      o[k] = make_float4((v[i][k].x - mean) * rstd, (v[i][k].y - mean) * rstd, (v[i][k].z - mean) * rstd, (v[i][k].w - mean) * rstd);
      if (p.weight && ok[i]) {
        const float4 w = *reinterpret_cast<const float4*>(p.weight + d);
        o[k].x *= w.x; o[k].y *= w.y; o[k].z *= w.z; o[k].w *= w.w;
      }
      if (p.scale && ok[i]) {
        o[k].x = o[k].x * (1.f + sc[i][k].x) + sh[i][k].x; o[k].y = o[k].y * (1.f + sc[i][k].y) + sh[i][k].y;
        o[k].z = o[k].z * (1.f + sc[i][k].z) + sh[i][k].z; o[k].w = o[k].w * (1.f + sc[i][k].w) + sh[i][k].w;
      }
      amax = fmaxf(amax, fmaxf(fmaxf(mx_fin_abs(o[k].x), mx_fin_abs(o[k].y)), fmaxf(mx_fin_abs(o[k].z), mx_fin_abs(o[k].w))));
    }
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));                        // a quad = one 32-feature block (D % 128 == 0: whole quads
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));                        // are in or out together)
    const int e = mx_exp(amax);
    if (ok[i]) {
      const int d0 = i * 512 + lane * 8;
      uint2 w;
      w.x = e4m3x4(o[0].x, o[0].y, o[0].z, o[0].w, e);
      w.y = e4m3x4(o[1].x, o[1].y, o[1].z, o[1].w, e);
      *reinterpret_cast<uint2*>(p.y + row * p.D + d0) = w;
      if ((lane & 3) == 0) p.ys[row * (p.D / 32) + d0 / 32] = (uint8_t)(e + 127);
    }
  }
}

extern "C" int ln3d_norm_modulate_mx(const ln3d_norm_args* a, void* y_scale, void* stream) {
  constexpr int MVG = 3;                                                // 512-feature chunks per lane set: widths up to 1536
  if (!a || !a->x || !a->y || !y_scale || a->D % 128 != 0 || a->D > 512 * MVG || a->rows <= 0) return LN3D_ERR_BAD_ARG;
  if ((a->scale == nullptr) != (a->shift == nullptr)) return LN3D_ERR_BAD_ARG;
  if (a->scale && (a->mod_ld % 4) != 0) return LN3D_ERR_BAD_ARG;
  if (a->scale_table || a->shift_table) return LN3D_ERR_BAD_ARG;        // the PixArt tables are not on this path
  if ((a->rows_in > 0 && a->rows_in != a->rows) || (a->rows_out > 0 && a->rows_out != (a->rows_in > 0 ? a->rows_in : a->rows)))
    return LN3D_ERR_BAD_ARG;
  if (((uintptr_t)a->y & 7) != 0) return LN3D_ERR_BAD_ARG;               // 8-byte element stores
  NormMxP p;
  p.x = a->x; p.y = (uint8_t*)a->y; p.ys = (uint8_t*)y_scale; p.rows = a->rows; p.D = a->D; p.kind = a->kind; p.eps = a->eps;
  p.weight = a->weight; p.shift = a->shift; p.scale = a->scale; p.mod_rows = a->mod_rows > 0 ? a->mod_rows : 1; p.mod_ld = a->mod_ld;
  const dim3 grid((unsigned)((a->rows + 3) / 4));
  if (a->D % 512 == 0 && a->D <= 1024) hipLaunchKernelGGL((norm_modulate_mx_kernel<2, true>), grid, dim3(256), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL((norm_modulate_mx_kernel<MVG, false>), grid, dim3(256), 0, (hipStream_t)stream, p);
  return ln3d_check_launch();
}

// ------------------------------------------------------------------------------------------------------------ ln3d_gemm_mxfp8
struct MxP {
  GemmP g;                                   // epilogue parameters (g.X / g.W unused)
  const uint8_t* Xq; const uint8_t* Xs; int64_t ldx, ldxs;
  const uint8_t* Wq; const uint8_t* Ws; int64_t ldw, ldws;
  uint8_t* os; int64_t ldos;                 // GELU_ERF: scales of the e4m3 output
};

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
// LDS-DMA of one dword per lane (LDS destination = M0 + lane * 4), per-lane 64-bit source; see lds_dma16_v in common.h
__device__ __forceinline__ void lds_dma4_v(const void* vaddr, uint32_t lds) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" ::"v"(vaddr), "s"(lds) : "memory", "m0");
}
#pragma clang diagnostic pop

// erf-GELU with an MXFP8 output, straight from the accumulators: acc[i][j] is one 32-feature block (= one MX block) of 32 tokens, a
// lane holds 16 of its features and lane l ^ 32 the other 16
// Finite input assumed (ln3d_mx.h): a NaN accumulator is stored as +-448 and skipped by the amax, an Inf zeroes its block's neighbours.
template <int NJ>
__device__ __forceinline__ void gelu_mx_epilogue(const MxP& p, f32x16 (&acc)[2][NJ], int fw0, int tw0, int lane) {
  const int l31 = lane & 31, hi = lane >> 5;
  const GemmP& g = p.g;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int fblk = fw0 + 32 * i;
    if (fblk >= g.N) continue;                                          // wave-uniform; N % 32 == 0
    float4 b[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      b[q] = g.bias ? *reinterpret_cast<const float4*>(g.bias + fblk + 8 * q + 4 * hi) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int tok = tw0 + 32 * j + l31;
      float v[16];
      float amax = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        v[4 * q + 0] = acc[i][j][4 * q + 0] + b[q].x; v[4 * q + 1] = acc[i][j][4 * q + 1] + b[q].y;
        v[4 * q + 2] = acc[i][j][4 * q + 2] + b[q].z; v[4 * q + 3] = acc[i][j][4 * q + 3] + b[q].w;
        gelu_erf2(v[4 * q + 0], v[4 * q + 1]); gelu_erf2(v[4 * q + 2], v[4 * q + 3]);
#pragma unroll
        for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fabsf(v[4 * q + e]));
      }
      amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
      const int e = mx_exp(amax);
      if (tok < g.M) {
        uint8_t* orow = (uint8_t*)g.out0 + (int64_t)tok * g.ldo + fblk;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *reinterpret_cast<uint32_t*>(orow + 8 * q + 4 * hi) = e4m3x4_finite(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3], e);
        if (hi == 0) p.os[(int64_t)tok * p.ldos + fblk / 32] = (uint8_t)(e + 127);
      }
    }
  }
}

// MX_NJ = 2 token blocks of 32 per wave (the wave owns 64 x 64); MX_ROWS = operand rows of a stage
constexpr int MX_NJ = 2, MX_BF = 128, MX_BT = 128, MX_ROWS = MX_BF + MX_BT, MX_STAGEB = MX_ROWS * 128 + MX_ROWS * 4, MX_LDS = 2 * MX_STAGEB;

template <int EPI>
__global__ __launch_bounds__(256, 2) void gemm_mx_kernel(MxP p) {
  constexpr int NW = 4, NJ = MX_NJ, BF = MX_BF, BT = MX_BT, ROWS = MX_ROWS;
  constexpr int OPB = ROWS * 128;                      // operand bytes of a stage
  constexpr int STAGEB = MX_STAGEB;                    // + one scale word per row
  constexpr int NPW = ROWS / 8 / NW;                   // 1 KB operand pieces per wave and stage
  constexpr int NSP = ROWS / 64;                       // scale pieces (64 rows x 4 B) per stage
  static_assert(ROWS % (8 * NW) == 0 && ROWS % 64 == 0 && NSP <= NW, "DMA pieces divide over the waves");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const GemmP& g = p.g;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wf = wid >> 1, wt = wid & 1;
  const int l31 = lane & 31, hi = lane >> 5;
  const int nft = (g.N + BF - 1) / BF;
  const int ft = blockIdx.x % nft, tt = blockIdx.x / nft;
  const int f0 = ft * BF, t0 = tt * BT;

  // per-lane DMA sources (rows past M / N clamped to the last row: their results are never stored)
  const uint8_t* src[NPW];
#pragma unroll
  for (int q = 0; q < NPW; ++q) {
    const int rt = 8 * (wid * NPW + q) + (lane >> 3);
    const int chunk = (lane & 7) ^ ((rt >> 1) & 7);
    src[q] = rt < BF ? p.Wq + (int64_t)min(f0 + rt, g.N - 1) * p.ldw + chunk * 16
                     : p.Xq + (int64_t)min(t0 + rt - BF, g.M - 1) * p.ldx + chunk * 16;
  }
  const int sp = wid < NSP ? wid : NSP - 1;            // every wave issues one scale piece (the surplus ones repeat the last):
  const uint8_t* ssrc;                                 // a uniform DMA count per wave keeps the vmcnt waits compile-time
  {
    const int rt = 64 * sp + lane;
    ssrc = rt < BF ? p.Ws + (int64_t)min(f0 + rt, g.N - 1) * p.ldws : p.Xs + (int64_t)min(t0 + rt - BF, g.M - 1) * p.ldxs;
  }
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_void_t*)smem;
  auto issue = [&](int s, int slot) __attribute__((always_inline)) {
    const uint32_t base = lds0 + slot * STAGEB;
#pragma unroll
    for (int q = 0; q < NPW; ++q) lds_dma16_v(src[q] + (int64_t)s * 128, base + (wid * NPW + q) * 1024);
    lds_dma4_v(ssrc + (int64_t)s * 4, base + OPB + sp * 256);
  };

  f32x16 acc[2][NJ];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int key = (l31 >> 1) & 7;
  const int a_row = (wf * 64 + l31) * 128, b_row = (BF + wt * 32 * NJ + l31) * 128;
  const int a_sc = OPB + (wf * 64 + l31) * 4, b_sc = OPB + (BF + wt * 32 * NJ + l31) * 4;
  const int ns = g.K / 128;
  issue(0, 0);
  if (ns > 1) issue(1, 1);
  int slot = 0;
  for (int s = 0; s < ns; ++s) {
    if (s + 1 < ns) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPW + 1) : "memory");     // stage s landed (s+1 still in flight)
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0xC07F);                                                  // lgkmcnt(0)
    __builtin_amdgcn_s_barrier();            // every wave's pieces of stage s landed
    const char* base = smem + slot * STAGEB;
    uint32_t sa[2], sb[NJ];
#pragma unroll
    for (int i = 0; i < 2; ++i) sa[i] = *reinterpret_cast<const uint32_t*>(base + a_sc + i * 128);
#pragma unroll
    for (int j = 0; j < NJ; ++j) sb[j] = *reinterpret_cast<const uint32_t*>(base + b_sc + j * 128);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      // operand map of the 32x32x64 form (measured with exact integers, tests/test_mxfp8_gpu.py): lane half h holds k = 16h + [0, 16)
      // in bytes 0-15 and k = 32 + 16h + [0, 16) in bytes 16-31 of the 64-wide step, and its scale applies to k = 32h + [0, 32).  So
      // half h reads 16-byte chunks 4 ks + h and 4 ks + 2 + h of its row, and passes the scale of K block 2 ks + h.
      const int c0 = 4 * ks + hi, c1 = c0 + 2;
      const int sh = 8 * (2 * ks + hi);
      i32x8 fa[2], fb[NJ];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const uint4 lo = *reinterpret_cast<const uint4*>(base + a_row + i * 4096 + ((c0 ^ key) << 4));
        const uint4 up = *reinterpret_cast<const uint4*>(base + a_row + i * 4096 + ((c1 ^ key) << 4));
        fa[i] = i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)up.x, (int)up.y, (int)up.z, (int)up.w};
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const uint4 lo = *reinterpret_cast<const uint4*>(base + b_row + j * 4096 + ((c0 ^ key) << 4));
        const uint4 up = *reinterpret_cast<const uint4*>(base + b_row + j * 4096 + ((c1 ^ key) << 4));
        fb[j] = i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)up.x, (int)up.y, (int)up.z, (int)up.w};
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fa[i], fb[j], acc[i][j], 0, 0, 0, (int)(sa[i] >> sh), 0,
                                                                      (int)(sb[j] >> sh));
    }
    if (s + 2 < ns) {                        // stage s+2 goes into the slot just read, once every wave is done with it
      __builtin_amdgcn_s_waitcnt(0xC07F);
      __builtin_amdgcn_s_barrier();
      issue(s + 2, slot);
    }
    slot ^= 1;
  }

  const int fw0 = f0 + wf * 64, tw0 = t0 + wt * 32 * NJ;
  if constexpr (EPI == LN3D_EPI_GELU_ERF) {
    gelu_mx_epilogue<NJ>(p, acc, fw0, tw0, lane);
    return;
  } else {
    __builtin_amdgcn_s_barrier();                      // ring retired: every wave stages its epilogue in its own 8 KB of it
    if (fw0 >= g.N) return;
    float4 pre[8];
    RunEpi<EPI> re;
    bool direct = false;
    if constexpr (EPI == LN3D_EPI_HEADS) {
      // a wave row (64 features, heads * head_dim % 64 == 0 checked by the launcher) lies inside one of q / k / v: V^T straight from
      // the accumulators (32 consecutive tokens per feature and store instruction), q / k through the staged, row-contiguous epilogue
      const int which = fw0 / (g.heads * g.head_dim);
      direct = ((g.transpose_mask >> which) & 1) || g.tokens < 32;
    }
    if (direct) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int tok = tw0 + j * 32 + l31;
        if (tok >= g.M) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int fb = fw0 + i * 32 + 8 * q + 4 * hi;
            if (fb < g.N) epilogue4<EPI>(g, tok, fb, acc[i][j][4 * q + 0], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]);
          }
      }
      return;
    }
    staged_epilogue<EPI, 2, NJ, true, false>(g, acc, smem + wid * 8192, fw0, tw0, lane, pre, re, false);
  }
}

template <int EPI>
static int run_mx(const MxP& p, hipStream_t s) {
  static_assert(MX_LDS * 2 <= 163840 && MX_LDS >= 4 * 8192, "two workgroups per CU; the ring holds the epilogue staging");
  static AttrOnce attr_once;
  if (attr_once.need())
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_mx_kernel<EPI>), hipFuncAttributeMaxDynamicSharedMemorySize, MX_LDS);
  const int nft = (p.g.N + MX_BF - 1) / MX_BF, ntt = (p.g.M + MX_BT - 1) / MX_BT;
  hipLaunchKernelGGL((gemm_mx_kernel<EPI>), dim3(nft * ntt), dim3(256), MX_LDS, s, p);
  return ln3d_check_launch();
}

extern "C" int ln3d_gemm_mxfp8(const ln3d_gemm_mx_args* a, void* stream) {
  if (!a || !a->Xq || !a->Xs || !a->Wq || !a->Ws || !a->out0) return LN3D_ERR_BAD_ARG;
  if (a->M <= 0 || a->N <= 0 || a->K <= 0 || (a->K % 128) != 0 || (a->N % 4) != 0) return LN3D_ERR_BAD_ARG;
  if (a->ldx < a->K || a->ldw < a->K || (a->ldx % 16) != 0 || (a->ldw % 16) != 0 || ((uintptr_t)a->Xq & 15) != 0 || ((uintptr_t)a->Wq & 15) != 0)
    return LN3D_ERR_BAD_ARG;
  if (a->ldxs < a->K / 32 || a->ldws < a->K / 32 || (a->ldxs % 4) != 0 || (a->ldws % 4) != 0 || ((uintptr_t)a->Xs & 3) != 0 ||
      ((uintptr_t)a->Ws & 3) != 0)
    return LN3D_ERR_BAD_ARG;
  if (a->bias && ((uintptr_t)a->bias & 15) != 0) return LN3D_ERR_BAD_ARG;
  MxP p;
  GemmP& g = p.g;
  g.X = nullptr; g.W = nullptr; g.bias = a->bias;
  g.ldx = 0; g.ldw = 0; g.ldo = a->ldo;
  g.M = a->M; g.N = a->N; g.K = a->K;
  g.out0 = a->out0; g.out1 = a->out1; g.out2 = a->out2;
  g.gate = a->gate; g.gate_rows = a->gate_rows > 0 ? a->gate_rows : 1; g.gate_ld = a->gate_ld;
  g.tokens = a->tokens; g.tok_pad = a->tok_pad; g.heads = a->heads; g.head_dim = a->head_dim; g.transpose_mask = a->transpose_mask;
  g.head_dim_pad = a->head_dim_pad > 0 ? a->head_dim_pad : a->head_dim;
  g.ctx_keys = 0; g.ctx_pad = 0; g.ctx_scale_log2 = 0.f;
  g.hn0 = nullptr; g.hn1 = nullptr; g.hn_eps = 0.f;
  g.rb = nullptr; g.rb_ld = 0;
  p.Xq = (const uint8_t*)a->Xq; p.Xs = (const uint8_t*)a->Xs; p.ldx = a->ldx; p.ldxs = a->ldxs;
  p.Wq = (const uint8_t*)a->Wq; p.Ws = (const uint8_t*)a->Ws; p.ldw = a->ldw; p.ldws = a->ldws;
  p.os = (uint8_t*)a->out_scale; p.ldos = a->ldos;
  hipStream_t s = (hipStream_t)stream;
  switch (a->epilogue) {
    case LN3D_EPI_F32:
      if (a->ldo < a->N || (a->ldo % 4) != 0) return LN3D_ERR_BAD_ARG;
      return run_mx<LN3D_EPI_F32>(p, s);
    case LN3D_EPI_GELU_ERF:
      if (!a->out_scale || (a->N % 32) != 0 || a->ldo < a->N || (a->ldo % 4) != 0 || ((uintptr_t)a->out0 & 3) != 0 || a->ldos < a->N / 32)
        return LN3D_ERR_BAD_ARG;
      return run_mx<LN3D_EPI_GELU_ERF>(p, s);
    case LN3D_EPI_GATE_RES:
      if (a->ldo < a->N || (a->ldo % 4) != 0) return LN3D_ERR_BAD_ARG;
      if (a->gate && ((a->gate_ld % 4) != 0 || ((uintptr_t)a->gate & 15) != 0 || a->gate_rows <= 0)) return LN3D_ERR_BAD_ARG;
      return run_mx<LN3D_EPI_GATE_RES>(p, s);
    case LN3D_EPI_HEADS:
      if (!a->out1 || !a->out2 || a->tokens <= 0 || a->heads <= 0 || a->head_dim <= 0 || (a->head_dim % 8) != 0 || a->tok_pad < a->tokens ||
          g.head_dim_pad < a->head_dim || ((a->heads * a->head_dim) % 64) != 0 || a->N != 3 * a->heads * a->head_dim || (a->M % a->tokens) != 0)
        return LN3D_ERR_BAD_ARG;
      // a transposed output stores token t of a 16-group at t with bits 2 and 3 swapped: a row that ends inside a group would be overrun
      if ((a->transpose_mask & 7) != 0 && (a->tok_pad % 16) != 0) return LN3D_ERR_BAD_ARG;
      return run_mx<LN3D_EPI_HEADS>(p, s);
    default: return LN3D_ERR_UNSUPPORTED;
  }
}
