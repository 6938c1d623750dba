// Which kernel a shape gets: the bf16 GEMM's tile table and the two dispatch decisions (ln3d_gemm_bf16, ln3d_attention_bf16) as pure
// functions of a handful of integers.  Host only - no HIP header - so that a plain host compile can print and test them without a GPU
// (tests/test_kernel_plan_cpu.py); gemm_bf16.hip and attention.hip launch what these functions return and decide nothing themselves.
#pragma once
#include <stdint.h>
#include "../../include/ln3d.h"

// ------------------------------------------------------------------------------------------------ bf16 GEMM tiles
enum Ln3dTileKind { LN3D_TILE_STAGED, LN3D_TILE_RING, LN3D_TILE_PERSISTENT };   // gemm_bf16_kernel / _ring64_kernel / _p4_kernel
enum Ln3dTileRow {                     // rows of ln3d_gemm_tiles, in its order
  LN3D_TILE_S128, LN3D_TILE_256x256, LN3D_TILE_384x192, LN3D_TILE_256x192, LN3D_TILE_128x384, LN3D_TILE_128x192, LN3D_TILE_256x256_W4,
  LN3D_TILE_256x256_P4, LN3D_GEMM_TILE_ROWS
};
static constexpr unsigned ln3d_epi_bit(int epi) { return epi >= 0 && epi < 32 ? 1u << epi : 0u; }
constexpr unsigned LN3D_EPIS_PLAIN = ln3d_epi_bit(LN3D_EPI_F32) | ln3d_epi_bit(LN3D_EPI_BF16) | ln3d_epi_bit(LN3D_EPI_GELU_ERF) |
                                     ln3d_epi_bit(LN3D_EPI_GELU_TANH) | ln3d_epi_bit(LN3D_EPI_SILU) | ln3d_epi_bit(LN3D_EPI_GATE_RES) |
                                     ln3d_epi_bit(LN3D_EPI_HEADS) | ln3d_epi_bit(LN3D_EPI_F32_SILU) | ln3d_epi_bit(LN3D_EPI_QUICK_GELU);
constexpr unsigned LN3D_EPIS_CROSS = ln3d_epi_bit(LN3D_EPI_CROSS_ATTN);

struct Ln3dGemmTile {
  int id;              // LN3D_GEMM_TILE=x<id> forces it (s = 0)
  const char* name;
  int kind;
  int nw, wgt, ni, nj; // waves, waves along tokens, 32-wide MFMA tiles per wave along features / tokens: the kernel's template parameters
  int bf, bt;          // features x tokens per tile = 32 ni (nw / wgt) x 32 nj wgt
  float speed;         // relative throughput in the cost estimate (measured at K = 1024: the L2 -> LDS fill is the limiter, so it
                       // follows the tile's flop / byte); 0 = not a candidate of the estimate, only taken by a rule of its own
  bool head_row;       // a wave row is ONE 64-wide head (ring, ni = 2): the staged, head-aware, normalising LN3D_EPI_HEADS epilogue
  unsigned epis;       // epilogues it is instantiated for (bits 1 << LN3D_EPI_*)
};
// The estimate walks its candidates in this order and the first of equal cost wins.  r2's 384x192 / 8-wave variant (11) was measured
// slower and is gone.
constexpr Ln3dGemmTile ln3d_gemm_tiles[LN3D_GEMM_TILE_ROWS] = {
    {0, "128x128 register-staged", LN3D_TILE_STAGED, 4, 2, 2, 2, 128, 128, 0.f, false, LN3D_EPIS_PLAIN},
    {7, "256x256 ring, 8 waves", LN3D_TILE_RING, 8, 4, 4, 2, 256, 256, 1.0f, false, LN3D_EPIS_PLAIN},
    {12, "384x192 ring, 12 waves (3 per SIMD)", LN3D_TILE_RING, 12, 2, 2, 3, 384, 192, 1.0f, true, LN3D_EPIS_PLAIN},
    {9, "256x192 ring, 8 waves", LN3D_TILE_RING, 8, 2, 2, 3, 256, 192, 0.95f, true, LN3D_EPIS_PLAIN | LN3D_EPIS_CROSS},
    {8, "128x384 ring, 8 waves", LN3D_TILE_RING, 8, 4, 2, 3, 128, 384, 0.945f, true, LN3D_EPIS_PLAIN},
    // 4 waves, 80 KB: two workgroups per CU (the half-batch GEMMs)
    {14, "128x192 ring, 4 waves", LN3D_TILE_RING, 4, 2, 2, 3, 128, 192, 0.f, true, LN3D_EPIS_PLAIN | LN3D_EPIS_CROSS},
    // ONE wave per SIMD, 128 x 128 per wave, the 16 accumulator tiles in AGPRs (hipcc allocates them there by itself: only MFMAs touch
    // them inside the K loop).  Instantiated for the epilogues that have long-K users.
    {13, "256x256 ring, 4 waves", LN3D_TILE_RING, 4, 2, 4, 4, 256, 256, 0.f, false,
     ln3d_epi_bit(LN3D_EPI_GATE_RES) | ln3d_epi_bit(LN3D_EPI_BF16) | ln3d_epi_bit(LN3D_EPI_F32)},
    // r6: the persistent form of 13 (plain bf16 / erf-GELU epilogues, interior tiles only)
    {16, "256x256 persistent, 4 waves", LN3D_TILE_PERSISTENT, 4, 2, 4, 4, 256, 256, 0.f, false,
     ln3d_epi_bit(LN3D_EPI_BF16) | ln3d_epi_bit(LN3D_EPI_GELU_ERF)},
};
static constexpr bool ln3d_gemm_tiles_consistent() {
  for (int r = 0; r < LN3D_GEMM_TILE_ROWS; ++r) {
    const Ln3dGemmTile& t = ln3d_gemm_tiles[r];
    if (t.bf != 32 * t.ni * (t.nw / t.wgt) || t.bt != 32 * t.nj * t.wgt) return false;
    if (t.head_row != (t.kind == LN3D_TILE_RING && t.ni == 2)) return false;
  }
  return ln3d_gemm_tiles[LN3D_TILE_S128].id == 0 && ln3d_gemm_tiles[LN3D_TILE_256x256].id == 7 && ln3d_gemm_tiles[LN3D_TILE_384x192].id == 12 &&
         ln3d_gemm_tiles[LN3D_TILE_256x192].id == 9 && ln3d_gemm_tiles[LN3D_TILE_128x384].id == 8 && ln3d_gemm_tiles[LN3D_TILE_128x192].id == 14 &&
         ln3d_gemm_tiles[LN3D_TILE_256x256_W4].id == 13 && ln3d_gemm_tiles[LN3D_TILE_256x256_P4].id == 16;
}
static_assert(ln3d_gemm_tiles_consistent(), "tile sizes follow from the template parameters; Ln3dTileRow names the rows in order");

static constexpr int64_t ln3d_tiles_of(const Ln3dGemmTile& t, int M, int N) { return (int64_t)((N + t.bf - 1) / t.bf) * ((M + t.bt - 1) / t.bt); }
// the persistent kernel has interior tiles only and eight compile-time K-stage positions in a loop unrolled by two
static constexpr bool ln3d_persistent_shape_ok(int M, int N, int K) {
  return (M % ln3d_gemm_tiles[LN3D_TILE_256x256_P4].bt) == 0 && (N % ln3d_gemm_tiles[LN3D_TILE_256x256_P4].bf) == 0 && (K % 128) == 0 && K >= 512;
}

// The tile the heuristics want before the instantiation / alignment fall-backs (ln3d_plan_gemm resolves those).
// Small problems (per-sample adaLN / timestep GEMMs, the conv decoder's 32/64 channels) take the 128x128 kernel.  Otherwise the
// candidate with the least estimated time: rounds of one tile per CU x tile area / relative throughput.  DiT-L/2 at 12288 tokens:
// N = 4096 -> 256x256 (3 full rounds), N = 3072 -> 384x192 with 12 waves (2 full rounds), N = 1024 -> 256x192 (1 full round).
static constexpr int ln3d_pick_gemm_tile(int M, int N, int K, int epi, bool head_stageable, int cus) {
  if (!(M >= 1536 && N >= 128)) return LN3D_TILE_S128;
  int best = LN3D_TILE_128x384;
  float best_cost = 1e30f;
  int64_t best_tiles = 0;
  for (int r = 0; r < LN3D_GEMM_TILE_ROWS; ++r) {
    const Ln3dGemmTile& t = ln3d_gemm_tiles[r];
    // a stageable head split only takes tiles with the head-contiguous staged epilogue; at the I23D shapes (65536 x 3072) 256x256
    // costs 550 us against 500 (384x192)
    if (t.speed <= 0.f || (head_stageable && !t.head_row)) continue;
    const int64_t tiles = ln3d_tiles_of(t, M, N);
    const float cost = (float)((tiles + cus - 1) / cus) * (float)(t.bf * t.bt) / t.speed;
    if (cost < best_cost) { best_cost = cost; best = r; best_tiles = tiles; }
  }
  // Under-filled launch (the best 8-wave tiling leaves half the CUs idle - the conditional half of a CFG batch, M = 6144 x
  // N = 1024: 128 tiles of 256x192): 128x192 tiles with 4 waves double the tile count.  r3: 22.5 us vs 27.0 (GATE_RES), 15.7 vs 21.1
  // (plain); at full M the two tie (35.9 vs 36.2), so it is only taken here.
  if (best_tiles * 2 <= cus && ln3d_tiles_of(ln3d_gemm_tiles[LN3D_TILE_128x192], M, N) > best_tiles) best = LN3D_TILE_128x192;
  // r5: long K loops over several rounds of 256x256 tiles (the I23D family's fc2: 49152 x 1024 x 4096, 3 rounds) run faster with ONE
  // wave per SIMD holding 128 x 128 (a third fewer LDS fragment bytes per flop): 372 - 379 us against 412, 500 against 538 at M = 65536,
  // bit-identical output.  With 16 K stages (K = 1024) the exposed prologue / epilogue of a lone wave costs more than the loop gains
  // (fc1 111 vs 98 us), and below two rounds the tile count decides (T23D fc2 takes 256x192) - profiles/r5_gemm_x13.log, r5_gemm_x15.log.
  // In situ (same-box A/B of the configs[2] line, temporary switch removed): 11.60 -> 11.70 samples/s, golden check unchanged.
  if (best == LN3D_TILE_256x256 && K >= 2048 && best_tiles >= 2 * (int64_t)cus && (ln3d_gemm_tiles[LN3D_TILE_256x256_W4].epis & ln3d_epi_bit(epi)))
    best = LN3D_TILE_256x256_W4;
  // r6: the persistent one-wave-per-SIMD kernel for its epilogues when every CU gets >= 2 whole 256 x 256 tiles and the last round is
  // >= 85 % full (DiT-L/2 fc1: 768 tiles = 3 rounds; I23D fc1: 12).  Sustained (3000-launch loops, profiles/r6_gemm.md):
  // fc1 + GELU 102.8 -> 99.0 us, plain 94.0 -> 87.2, I23D fc1 + GELU 411.6 -> 398.0.
  if ((ln3d_gemm_tiles[LN3D_TILE_256x256_P4].epis & ln3d_epi_bit(epi)) && ln3d_persistent_shape_ok(M, N, K)) {
    const int64_t t = ln3d_tiles_of(ln3d_gemm_tiles[LN3D_TILE_256x256_P4], M, N), rounds = (t + cus - 1) / cus;
    if (t >= 2 * (int64_t)cus && t * 100 >= rounds * cus * 85) best = LN3D_TILE_256x256_P4;
  }
  return best;
}

// The row of ln3d_gemm_tiles that ln3d_gemm_bf16 launches.  head_stageable: LN3D_EPI_HEADS whose head split the staged epilogue can
// serve; out_aligned: ldo % 8 == 0 and out0 / bias (if any) 16-byte aligned, the persistent kernel's stores and bias DMA;
// forced: the parsed LN3D_GEMM_TILE id, negative = none.  LN3D_EPI_CROSS_ATTN geometry (N % 256 == 0, tokens % 192 == 0) is the
// caller's to validate.
static constexpr int ln3d_plan_gemm(int M, int N, int K, int epi, bool head_stageable, bool out_aligned, int cus, int forced) {
  if (epi == LN3D_EPI_CROSS_ATTN) {
    // 256x192 tiles (8 waves); when they would leave half the chip idle, 128x192 tiles with 4 waves (2 heads per tile) unless the
    // switch forces the former.  No other forced id has a cross-attention instantiation to select.
    const Ln3dGemmTile& wide = ln3d_gemm_tiles[LN3D_TILE_256x192];
    return (ln3d_tiles_of(wide, M, N) * 2 <= cus && forced != wide.id) ? LN3D_TILE_128x192 : LN3D_TILE_256x192;
  }
  int row = LN3D_TILE_S128;          // what an unknown forced id runs
  if (forced < 0) row = ln3d_pick_gemm_tile(M, N, K, epi, head_stageable, cus);
  else
    for (int r = 0; r < LN3D_GEMM_TILE_ROWS; ++r)
      if (ln3d_gemm_tiles[r].id == forced) row = r;
  // a tile without this epilogue, or a persistent launch the shape or the alignment refuses, runs as the 8-wave 256x256 ring
  const Ln3dGemmTile& t = ln3d_gemm_tiles[row];
  if (!(t.epis & ln3d_epi_bit(epi))) return LN3D_TILE_256x256;
  if (t.kind == LN3D_TILE_PERSISTENT && !(ln3d_persistent_shape_ok(M, N, K) && out_aligned)) return LN3D_TILE_256x256;
  return row;
}

// ------------------------------------------------------------------------------------------------ attention
enum Ln3dAttnKernel {
  LN3D_ATTN_SHORT,          // attn_short_kernel: Dh 64, <= 128 keys, causal
  LN3D_ATTN_KRES,           // attn_kres_kernel: Dh 64, K of a head resident beside the V^T ring
  LN3D_ATTN_STREAM,         // attn_stream_kernel: Dh 64, unpadded keys in blocks of 256
  LN3D_ATTN_RING64_OCC4,    // attn_kernel<64, 4>
  LN3D_ATTN_RING64_OCC2,    // attn_kernel<64, 2>
  LN3D_ATTN_RING80,         // attn_kernel<80, 2>: the U-Net's 80-wide heads
  LN3D_ATTN_RING80_T72,     // attn_kernel<80, 2, 72>: DiT-XL/2's 72-wide heads stored 80 wide
  LN3D_ATTN_RING128,        // attn_kernel<128, 2>
  LN3D_ATTN_RING128_T72,    // attn_kernel<128, 2, 72>: DiT-XL/2's stored 128 wide
  LN3D_ATTN_KERNELS
};

// The kernel ln3d_attention_bf16 launches (>= 0), or the LN3D_ERR_* it returns.  BH = B * H.
static constexpr int ln3d_plan_attention(int Dh, int Dh_true, int Nq, int Nq_pad, int Nk, int Nk_pad, int BH, bool causal, int cus) {
  if (Nk <= 0 || Nq <= 0 || Nk_pad % 64 != 0 || Nk_pad < Nk || Nq_pad < Nq) return LN3D_ERR_BAD_ARG;
  // causal masking exists in the short-sequence kernel only (its one user is the 77-token CLIP text tower)
  if (causal && !(Dh == 64 && Nk <= 128)) return LN3D_ERR_UNSUPPORTED;
  if (Dh == 64) {
    if (Dh_true != 0 && Dh_true != 64) return LN3D_ERR_UNSUPPORTED;             // compact heads: the padded kernels only
    // The short-sequence kernel serves the causal text tower; for the non-causal 77-key cross-attention it measures 2 us
    // faster in isolation but slower inside the sampling loop than the ring kernel (and the DiT runs that attention inside
    // the query-projection GEMM anyway, LN3D_EPI_CROSS_ATTN), so the ring kernel serves it.
    if (causal) return LN3D_ATTN_SHORT;
    if ((Nk & 255) == 0 && Nk_pad == Nk) {
      // K-resident kernel: K of a head fits beside the V^T ring (Nk <= 768) and there is a head for every CU, so that one
      // workgroup per head walks all its query blocks (fewer heads: the query blocks of a head are shared out - attn_stream)
      if (Nk >= 512 && Nk <= 768 && (Nq & 255) == 0 && Nq_pad == Nq && BH >= cus) return LN3D_ATTN_KRES;
      return LN3D_ATTN_STREAM;
    }
    return Nk > 128 ? LN3D_ATTN_RING64_OCC4 : LN3D_ATTN_RING64_OCC2;
  }
  if (Dh == 80 || Dh == 128) {             // r6: 65 - 80 wide heads may be stored 80 wide instead of 128
    if (Dh_true == 0 || Dh_true == Dh) return Dh == 80 ? LN3D_ATTN_RING80 : LN3D_ATTN_RING128;
    if (Dh_true == 72) return Dh == 80 ? LN3D_ATTN_RING80_T72 : LN3D_ATTN_RING128_T72;
  }
  return LN3D_ERR_UNSUPPORTED;
}
