// bf16 GEMM with fused epilogues for gfx950 (CDNA4): out[m,n] = epi(sum_k X[m,k] W[n,k] + bias[n]).
//
// Design (MI355X-first):
//  * MFMA v_mfma_f32_32x32x16_bf16, 64-lane wavefronts.  The MFMA "A" operand is the WEIGHT tile
//    (rows = output features) and the "B" operand the TOKEN tile, so the fp32 accumulator fragment
//    of a lane holds 4 consecutive output FEATURES of one token ( row = (r&3)+8(r>>2)+4(lane>>5),
//    col = lane&31 ): per-feature bias / per-(sample,feature) gates are 4-wide vector loads, and the
//    accumulators double as the B operand of a following product (LN3D_EPI_CROSS_ATTN).
//  * Large problems: LDS-DMA ring kernels (gemm_bf16_ring64_kernel below: 256x256 / 384x192 / 256x192 / 128x384 tiles,
//    K stages of 64 = full cache lines, epilogue through LDS with 16-byte stores).
//  * Small problems: 128(features) x 128(tokens) x 64(K) block tile, 4 waves as 2x2, each wave 64x64 = 2x2 MFMA tiles
//    (64 accumulator VGPRs).  Both operands are K-contiguous in HBM ([rows, K] row-major), staged
//    HBM -> VGPR (global_load_dwordx4, 8 lanes cover one 128-B row segment) -> LDS rows padded to
//    144 B, which makes the ds_read_b128 fragment reads bank-conflict free (16 distinct rows of a
//    b128 lane-group land on 16 distinct 16-B slots: 144*r mod 256).  Double-buffered LDS, the next
//    tile's global loads are issued before the MFMA block of the current tile (latency hidden under
//    16 MFMAs/wave), one barrier per K-tile.
//  * Epilogues fused: bias, GELU(erf/tanh/quick), SiLU, gate*out+residual (adaLN-zero gating into the fp32
//    residual stream, optional bf16 copy), head split with V^T emission for the attention kernel,
//    cross-attention over a short cached context.
#include <stdlib.h>
#include "common.h"
#include "../../include/ln3d.h"
#include "kernel_plan.h"

#define BMF 128  // features per block
#define BTK 128  // tokens per block
#define BK 64
#define ROWB 144                      // LDS bytes per tile row (128 + 16 pad)
#define TILEB (128 * ROWB)            // 18432
#define GEMM_LDS (4 * TILEB)          // 2 buffers x (W tile + X tile)

#include "gemm_epi.h"

template <int EPI>
__global__ __launch_bounds__(256) void gemm_bf16_kernel(GemmP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wf = wid >> 1, wt = wid & 1;
  const int l31 = lane & 31, hi = lane >> 5;

  const int nft = (p.N + BMF - 1) / BMF;
  const int ft = blockIdx.x % nft, tt = blockIdx.x / nft;
  const int f0 = ft * BMF, t0 = tt * BTK;

  // staging map: 8 lanes x 16 B cover one 128-B row segment; 32 rows per pass, 4 passes
  const int c = tid & 7, r0 = tid >> 3;
  const bf16_t* wsrc[4]; const bf16_t* xsrc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int rf = f0 + r0 + 32 * i; rf = rf < p.N ? rf : p.N - 1;
    int rt = t0 + r0 + 32 * i; rt = rt < p.M ? rt : p.M - 1;
    wsrc[i] = p.W + (int64_t)rf * p.ldw + c * 8;
    xsrc[i] = p.X + (int64_t)rt * p.ldx + c * 8;
  }
  const int st_off = r0 * ROWB + c * 16;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  uint4 ra[4], rb[4];
  const int nk = p.K / BK;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ra[i] = *reinterpret_cast<const uint4*>(wsrc[i]);
    rb[i] = *reinterpret_cast<const uint4*>(xsrc[i]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    *reinterpret_cast<uint4*>(smem + st_off + i * 32 * ROWB) = ra[i];
    *reinterpret_cast<uint4*>(smem + TILEB + st_off + i * 32 * ROWB) = rb[i];
  }
  __syncthreads();

  const int a_off = (wf * 64 + l31) * ROWB + hi * 16;
  const int b_off = TILEB + (wt * 64 + l31) * ROWB + hi * 16;

  auto mma_tile = [&](const char* base) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = *reinterpret_cast<const bf16x8*>(base + a_off + i * 32 * ROWB + ks * 32);
        b[i] = *reinterpret_cast<const bf16x8*>(base + b_off + i * 32 * ROWB + ks * 32);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  };

  for (int kt = 0; kt + 1 < nk; ++kt) {
    const int buf = kt & 1;
    const int koff = (kt + 1) * BK;
    // explicit scalars (not arrays): keeps the in-flight tile in VGPRs across the sched_barrier
    const uint4 na0 = *reinterpret_cast<const uint4*>(wsrc[0] + koff);
    const uint4 na1 = *reinterpret_cast<const uint4*>(wsrc[1] + koff);
    const uint4 na2 = *reinterpret_cast<const uint4*>(wsrc[2] + koff);
    const uint4 na3 = *reinterpret_cast<const uint4*>(wsrc[3] + koff);
    const uint4 nx0 = *reinterpret_cast<const uint4*>(xsrc[0] + koff);
    const uint4 nx1 = *reinterpret_cast<const uint4*>(xsrc[1] + koff);
    const uint4 nx2 = *reinterpret_cast<const uint4*>(xsrc[2] + koff);
    const uint4 nx3 = *reinterpret_cast<const uint4*>(xsrc[3] + koff);
    __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ahead of the MFMA block (hipcc sinks it otherwise)
    mma_tile(smem + buf * 2 * TILEB);
    __builtin_amdgcn_sched_barrier(0);
    char* nb = smem + (buf ^ 1) * 2 * TILEB + st_off;
    *reinterpret_cast<uint4*>(nb + 0 * 32 * ROWB) = na0;
    *reinterpret_cast<uint4*>(nb + 1 * 32 * ROWB) = na1;
    *reinterpret_cast<uint4*>(nb + 2 * 32 * ROWB) = na2;
    *reinterpret_cast<uint4*>(nb + 3 * 32 * ROWB) = na3;
    *reinterpret_cast<uint4*>(nb + TILEB + 0 * 32 * ROWB) = nx0;
    *reinterpret_cast<uint4*>(nb + TILEB + 1 * 32 * ROWB) = nx1;
    *reinterpret_cast<uint4*>(nb + TILEB + 2 * 32 * ROWB) = nx2;
    *reinterpret_cast<uint4*>(nb + TILEB + 3 * 32 * ROWB) = nx3;
    __syncthreads();
  }
  mma_tile(smem + ((nk - 1) & 1) * 2 * TILEB);

#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int tok = t0 + wt * 64 + j * 32 + l31;
    if (tok >= p.M) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int fb = f0 + wf * 64 + i * 32 + 8 * g + 4 * hi;
        if (fb < p.N)
          epilogue4<EPI>(p, tok, fb, acc[i][j][4 * g + 0], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]);
      }
    }
  }
}

// =================================================================================================


// ------------------------------------------------------------------------------------------------------------------
// LDS-DMA ring kernel for the large GEMMs: NW waves as (NW/WGT) x WGT, wave tile 32*NI features x 32*NJ tokens.
//  * Operand tiles go HBM/L2 -> LDS with global_load_lds_dwordx4 (no VGPR staging); K stages of 64 so that an LDS row is a
//    full 128-byte cache line of the operand (64-byte rows fetch every line twice: +11..20 % measured); two 64 KB slots.
//    16-byte chunk c of row r is stored at chunk c ^ ((r >> 1) & 7) (applied to the DMA *source* address, the LDS side of
//    a DMA is lane-linear): ds_read_b128 fragment reads are bank-conflict free without padding.
//  * A stage is 4 K-substeps of 16 with two fragment register sets: substep k multiplies while substep k+1 is read; the one
//    barrier of the stage sits before substep 3, behind which the first fragments of stage s+1 are read and the DMAs of
//    stage s+2 are issued into the slot that was just retired; reads and DMA issues are slotted one per MFMA
//    (sched_barrier pins the interleave) and the second wave of the SIMD covers the issue latency.
//  * Measured limiter is the L2 -> LDS fill (~11-12 TB/s chip-wide whatever the schedule), so the tile shapes maximise
//    flop per filled byte within 256 VGPRs at 2 waves/SIMD: 256x256 (128 flop/B), 256x192 (110), 128x384 (96).
//  * Workgroup -> tile map is XCD-aware (block b runs on XCD b % 8): an XCD owns ntt/8 token panels and walks the
//    feature tiles in groups of 4, so concurrently running tiles share 4 W panels and its own X panels.
//  * Epilogue through LDS (staged_epilogue) except V^T tiles.
template <int EPI, int NW, int WGT, int NI, int NJ>
__global__ __launch_bounds__(NW * 64, (NW == 4 && NI * NJ <= 6) ? 2 : NW / 4) void gemm_bf16_ring64_kernel(GemmP p) {
  constexpr int WGF = NW / WGT, BF = 32 * NI * WGF, BT = 32 * NJ * WGT;
  constexpr int WB = BF * 128, STAGEB = (BF + BT) * 128, NPW = (BF + BT) / 8 / NW;
  static_assert((BF + BT) / 8 % NW == 0, "DMA instructions must divide evenly over the waves");
  constexpr int NM = NI * NJ, NR = NI + NJ;
  static_assert(NM >= NR, "one fragment read per MFMA slot");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wf = wid / WGT, wt = wid % WGT;
  const int l31 = lane & 31, hi = lane >> 5;

  const int nft = (p.N + BF - 1) / BF, ntt = (p.M + BT - 1) / BT;
  const int ntiles = nft * ntt;
  int ft, tt;
  {
    const int b = blockIdx.x, xcd = b & 7, slot = b >> 3;
    if ((ntt & 7) == 0 && (nft & 3) == 0) {
      const int rows = ntt >> 3;
      const int g = slot / (rows * 4), rem = slot - g * rows * 4;
      ft = g * 4 + (rem & 3);
      tt = xcd * rows + (rem >> 2);
    } else {
      const int q = ntiles >> 3, r = ntiles & 7;
      const int tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
      ft = tile % nft; tt = tile / nft;
    }
  }
  const int f0 = ft * BF, t0 = tt * BT;

  // DMA instruction = 8 rows x 128 B -> 1 KB of the slot (W row groups first, then X row groups).  Every wave owns NPWW row
  // groups of the W tile and NPWX of the X tile, so the operand (and with it the wave-uniform base pointer) of instruction q is
  // known at compile time: the source is base (SGPR pair) + a 32-bit lane offset - one VGPR per instruction.
  constexpr int NPWW = BF / 8 / NW, NPWX = BT / 8 / NW;
  static_assert(BF / 8 % NW == 0 && BT / 8 % NW == 0 && NPWW + NPWX == NPW, "row groups of both operands divide evenly over the waves");
  const int r8 = lane >> 3;
  const char* const Wb = reinterpret_cast<const char*>(p.W + (int64_t)f0 * p.ldw);
  const char* const Xb = reinterpret_cast<const char*>(p.X + (int64_t)t0 * p.ldx);
  uint32_t soff[NPW];
#pragma unroll
  for (int q = 0; q < NPW; ++q) {
    const int rt = 8 * (q < NPWW ? wid * NPWW + q : wid * NPWX + (q - NPWW)) + r8;          // row inside its own tile
    const int chunk = (lane & 7) ^ ((rt >> 1) & 7);
    if (q < NPWW) {
      int r = f0 + rt; r = r < p.N ? r : p.N - 1;
      soff[q] = (uint32_t)(((int64_t)(r - f0) * p.ldw + chunk * 8) * 2);
    } else {
      int r = t0 + rt; r = r < p.M ? r : p.M - 1;
      soff[q] = (uint32_t)(((int64_t)(r - t0) * p.ldx + chunk * 8) * 2);
    }
  }
  const int dW0 = wid * NPWW * 1024, dX0 = WB + wid * NPWX * 1024;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_void_t*)smem;
#define Y_ISSUE1(s, q)                                                                                        \
  lds_dma16_s(((q) < NPWW ? Wb : Xb) + (int64_t)(s) * 128, soff[q],                                           \
              lds0 + ((s) & 1) * STAGEB + ((q) < NPWW ? dW0 + (q) * 1024 : dX0 + ((q) - NPWW) * 1024))

  const int key = (l31 >> 1) & 7;
  const int a_row = (wf * 32 * NI + l31) * 128;
  const int b_row = WB + (wt * 32 * NJ + l31) * 128;
#define Y_RDA(s, ks, i) (*reinterpret_cast<const bf16x8*>(smem + ((s) & 1) * STAGEB + a_row + (i) * 4096 + (((2 * (ks) + hi) ^ key) << 4)))
#define Y_RDB(s, ks, j) (*reinterpret_cast<const bf16x8*>(smem + ((s) & 1) * STAGEB + b_row + (j) * 4096 + (((2 * (ks) + hi) ^ key) << 4)))

  f32x16 acc[NI][NJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  bf16x8 a0[NI], b0[NJ], a1[NI], b1[NJ];
  const int ns = p.K / 64;

  // CROSS_ATTN: the K rows of this tile's sample and 4 heads go into the LDS above the ring now (40 KB at 77 keys), long
  // before the epilogue needs them.  Row r of head hh at XK + hh*XKH + r*128, 16-byte chunk c at c ^ ((r >> 1) & 7).
  constexpr int XK = 2 * STAGEB, XKH = 96 * 128;
  if constexpr (EPI == LN3D_EPI_CROSS_ATTN) {
    static_assert(NI == 2 && NJ == 3 && WGT == 2 && (NW == 8 || NW == 4), "one head (64 features) per wave row: 256x192 (8 waves) or 128x192 (4 waves) tile");
    const int bsmp = t0 / p.tokens;
    const int nrows8 = (p.ctx_keys + 7) >> 3;                      // DMA instructions (8 rows each) per head
    const bf16_t* kc = (const bf16_t*)p.out1 + ((int64_t)bsmp * p.heads + (f0 >> 6)) * p.ctx_pad * 64;
    for (int idx = wid; idx < WGF * nrows8; idx += NW) {
      const int hh = idx / nrows8, j = idx - hh * nrows8;
      const int r = 8 * j + (lane >> 3);
      const bf16_t* src_k = kc + ((int64_t)hh * p.ctx_pad + r) * 64 + (((lane & 7) ^ ((r >> 1) & 7)) << 3);
      lds_dma16_v(src_k, lds0 + XK + hh * XKH + j * 1024);
    }
  }

#pragma unroll
  for (int q = 0; q < NPW; ++q) Y_ISSUE1(0, q);
  if (ns > 1) { _Pragma("unroll") for (int q = 0; q < NPW; ++q) Y_ISSUE1(1, q); }
  if (ns > 1) { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPW) : "memory"); }          // stage 0 landed
  else { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int i = 0; i < NI; ++i) a0[i] = Y_RDA(0, 0, i);
#pragma unroll
  for (int j = 0; j < NJ; ++j) b0[j] = Y_RDB(0, 0, j);

#define Y_MMA(FA, FB, n) acc[(n) / NJ][(n) % NJ] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(FA[(n) / NJ], FB[(n) % NJ], acc[(n) / NJ][(n) % NJ], 0, 0, 0)
  // D1 (half, rounded up) of a stage's NPW DMA instructions are issued in the last substep of stage s (right behind the
  // barrier that retires their slot), the other NPW - D1 in the first two substeps of stage s+1 (LATE slots apart): the texture
  // path accepts a 1 KB piece every ~16 cycles and a wave that finds its queue full stalls with its MFMAs behind it.
  constexpr int D1 = (NPW + 1) / 2;
  constexpr int NLATE = NPW - D1;
  // substep: multiply (CA, CB) while (s2, ks2) is read into (NA, NB); LATE0 >= 0: late DMA pieces [LATE0, LATE1) of stage sd
#define Y_PHASE(CA, CB, NA, NB, s2, ks2, LATE, sd, L0, L1)                                                \
  _Pragma("unroll") for (int n = 0; n < NM; ++n) {                                                        \
    Y_MMA(CA, CB, n);                                                                                     \
    if (n < NI) NA[n] = Y_RDA(s2, ks2, n);                                                                \
    else if (n < NR) NB[n - NI] = Y_RDB(s2, ks2, n - NI);                                                 \
    if (LATE) {                                                                                           \
      _Pragma("unroll") for (int d = (L0); d < (L1); ++d)                                                 \
          if ((d - (L0)) * NM / ((L1) - (L0) > 0 ? (L1) - (L0) : 1) == n) Y_ISSUE1(sd, d);                \
    }                                                                                                     \
    __builtin_amdgcn_sched_barrier(0);                                                                    \
  }
  // The stage's one barrier sits behind the FIRST MFMA of the last substep: every wave has read the last fragments of slot
  // s & 1 (lgkmcnt(0): they were issued at least two MFMAs earlier) and its own DMAs of stage s+1 have landed (vmcnt(0): the
  // only ones in flight); the fragment reads of stage s+1 and the first D1 DMAs of stage s+2 fill the remaining NM-1 slots.
  static_assert(NM - 1 >= NR, "one fragment read per MFMA slot behind the barrier");
  constexpr int LH = D1 + (NLATE + 1) / 2;             // late pieces [D1, LH) in the first substep, [LH, NPW) in the second
#define Y_STAGE(s, PREV, FILL, MORE)                                                                      \
  {                                                                                                       \
    Y_PHASE(a0, b0, a1, b1, s, 1, (PREV) && NLATE > 0, (s) + 1, D1, LH);                                  \
    Y_PHASE(a1, b1, a0, b0, s, 2, (PREV) && NLATE > 0, (s) + 1, LH, NPW);                                 \
    Y_PHASE(a0, b0, a1, b1, s, 3, false, 0, 0, 0);                                                        \
    _Pragma("unroll") for (int n = 0; n < NM; ++n) {                                                      \
      Y_MMA(a1, b1, n);                                                                                   \
      if (MORE && n == 0) {                                                                               \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                  \
        __builtin_amdgcn_s_waitcnt(0xC07F);                                                               \
        __builtin_amdgcn_s_barrier();                                                                     \
      }                                                                                                   \
      if (MORE) {                                                                                         \
        if (n >= 1 && n - 1 < NI) a0[n - 1] = Y_RDA((s) + 1, 0, n - 1);                                   \
        else if (n >= 1 && n - 1 < NR) b0[n - 1 - NI] = Y_RDB((s) + 1, 0, n - 1 - NI);                    \
      }                                                                                                   \
      if (FILL) {                                                                                         \
        _Pragma("unroll") for (int d = 0; d < D1; ++d)                                                    \
            if (1 + d * (NM - 1) / D1 == n) Y_ISSUE1((s) + 2, d);                                         \
      }                                                                                                   \
      __builtin_amdgcn_sched_barrier(0);                                                                  \
    }                                                                                                     \
  }
  // Nothing but LDS reads may be pending when the K loop is entered: a kernel-argument s_load still counted on lgkmcnt makes
  // hipcc answer the loop head's fragment dependency with lgkmcnt(0) on EVERY iteration (mixed event types cannot be counted).
  __builtin_amdgcn_s_waitcnt(0xC07F);
  int s = 0;
  if (ns >= 3) {
    Y_STAGE(0, false, true, true);
    for (s = 1; s + 2 < ns; ++s) Y_STAGE(s, true, true, true);
    Y_STAGE(s, true, false, true);
    ++s;
  } else if (ns == 2) {
    Y_STAGE(0, false, false, true);
    s = 1;
  }
  // GATE_RES, interior tile: block 0's residual quads (8 rows x 16 B per lane) and its bias / gate rows are requested here, one K stage
  // before the accumulators are final - the epilogue then starts on data that has arrived instead of on an L2 / fabric round trip
  constexpr bool kPre = EPI == LN3D_EPI_GATE_RES && NW <= 8 && NI % 2 == 0 && NI * NJ <= 6;
  float4 xpre[8];
  RunEpi<EPI> re_pre;
  bool have_pre = false;
  if constexpr (kPre) {
    const int fw0 = f0 + wf * 32 * NI, tw0 = t0 + wt * 32 * NJ;
    const bool full = (tw0 + 32 * NJ <= p.M) && (fw0 + 32 * NI <= p.N) && !((p.gate || p.rb) && p.gate_rows < 32);
    if (__builtin_amdgcn_readfirstlane(full ? 1 : 0)) {
      have_pre = true;
      const int rrow = lane >> 4, rc = lane & 15;
      re_pre.init(p, fw0 + 4 * rc, __builtin_amdgcn_readfirstlane(tw0), 0, 0, 0);
      const float* base = (const float*)p.out0 + (int64_t)(tw0 + rrow) * p.ldo + fw0 + 4 * rc;
#pragma unroll
      for (int it = 0; it < 8; ++it) xpre[it] = *reinterpret_cast<const float4*>(base + (int64_t)(4 * it) * p.ldo);
    }
  }
  Y_STAGE(s, false, false, false);

  if constexpr (EPI == LN3D_EPI_CROSS_ATTN) {
    // acc[i][j] = q^T of head (f0/64 + wf): features (rows) x the wave's 96 tokens (columns, lane & 31 within block j).
    // Same swapped products and lane-local softmax as csrc/attention.hip; q is consumed straight from the accumulators
    // (bf16-rounded like the stored q of the unfused path): the B operand of k-step s is accumulator half s of feature
    // block s/2, whose row order inside a 16-group is [0-3, 8-11, 4-7, 12-15] - the order the K cache stores its dims in.
    const int bsmp = t0 / p.tokens;
    const int nkb = (p.ctx_keys + 63) >> 6, nkt = (p.ctx_keys + 31) >> 5;
    __builtin_amdgcn_s_barrier();                     // ring retired: V^T tiles of the 4 heads go to its start
    {
      const bf16_t* vc = (const bf16_t*)p.out2 + ((int64_t)bsmp * p.heads + (f0 >> 6)) * 64 * p.ctx_pad;
      for (int idx = wid; idx < WGF * nkb * 8; idx += NW) {       // (head, key block, 8 pieces of 8 rows)
        const int hh = idx / (nkb * 8), rem = idx - hh * nkb * 8, kb = rem >> 3, j = rem & 7;
        const int vrow = 8 * j + (lane >> 3);
        const bf16_t* src_v = vc + ((int64_t)hh * 64 + vrow) * p.ctx_pad + kb * 64 + (((lane & 7) ^ ((vrow >> 1) & 7)) << 3);
        lds_dma16_v(src_v, lds0 + (hh * 2 + kb) * 8192 + j * 1024);
      }
    }
    const int kkey = (l31 >> 1) & 7;
    const char* kbase = smem + XK + wf * XKH + l31 * 128;
    float inv[NJ];
    uint32_t pk[NJ][24];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      f32x16 st[3];
#pragma unroll
      for (int kt = 0; kt < 3; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) st[kt][r] = 0.f;
#pragma unroll
      for (int sd = 0; sd < 4; ++sd) {
        union { uint32_t u[4]; bf16x8 v; } qb;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
          qb.u[jj] = pack2bf(acc[sd >> 1][j][8 * (sd & 1) + 2 * jj], acc[sd >> 1][j][8 * (sd & 1) + 2 * jj + 1]);
#pragma unroll
        for (int kt = 0; kt < 3; ++kt)
          if (kt < nkt) {
            const bf16x8 kf = *reinterpret_cast<const bf16x8*>(kbase + kt * 32 * 128 + (((2 * sd + hi) ^ kkey) << 4));
            st[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qb.v, st[kt], 0, 0, 0);
          }
      }
      float mx = -3.0e38f;
#pragma unroll
      for (int kt = 0; kt < 3; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kt * 32 + 4 * hi + (r & 3) + 8 * (r >> 2);
          st[kt][r] = key < p.ctx_keys ? st[kt][r] : -3.0e38f;
          mx = fmaxf(mx, st[kt][r]);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m = mx * p.ctx_scale_log2;
      float psum = 0.f;
#pragma unroll
      for (int kt = 0; kt < 3; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float pv = __builtin_amdgcn_exp2f(fmaf(st[kt][r], p.ctx_scale_log2, -m));
          st[kt][r] = pv;
          psum += pv;
        }
      inv[j] = 1.0f / (psum + __shfl_xor(psum, 32, 64));
      // P (bf16 pairs) parks in the accumulator registers of token block j, which are dead now: key step ks of 16 keys ->
      // 4 dwords at acc[ks >> 2][j][4 * (ks & 3) ...]
#pragma unroll
      for (int ks = 0; ks < 6; ++ks)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
          pk[j][4 * ks + jj] = pack2bf(st[ks >> 1][8 * (ks & 1) + 2 * jj], st[ks >> 1][8 * (ks & 1) + 2 * jj + 1]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's V^T pieces landed
    __builtin_amdgcn_s_barrier();                      // ... and everybody else's
    const char* vbase = smem + (wf * 2) * 8192 + l31 * 128;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      f32x16 oa[2];
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oa[dt][r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 6; ++ks)
        if (ks < 2 * nkt) {
          union { uint32_t u[4]; bf16x8 v; } pb;
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) pb.u[jj] = pk[j][4 * ks + jj];
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) {
            const bf16x8 vf = *reinterpret_cast<const bf16x8*>(vbase + (ks >> 2) * 8192 + dt * 32 * 128 + (((2 * (ks & 3) + hi) ^ kkey) << 4));
            oa[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pb.v, oa[dt], 0, 0, 0);
          }
        }
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[dt][j][r] = oa[dt][r] * inv[j];
    }
    // acc now holds O^T of the head in the accumulator layout of a plain GEMM tile: the staged epilogue writes it as bf16
  }
  bool direct = false;
  if constexpr (EPI == LN3D_EPI_HEADS) {
    direct = (p.transpose_mask != 0) && (f0 + BF > 2 * p.heads * p.head_dim);
    // A wave row that is exactly one head of a transposed target (V^T) goes through LDS transposed: each store instruction
    // then writes 16 rows x 64 contiguous bytes of V^T instead of 64 scattered 2-byte elements.
    if constexpr (NI == 2) {
      const int dm = p.heads * p.head_dim;
      // r4: any head size that is a multiple of 8 with heads * head_dim a multiple of 64 (DiT-XL/2: 72 in 128-wide rows) - a wave
      // row of 64 features then lies inside ONE of q / k / v, and an 8-feature chunk inside one head; the (head, dim) of a lane's
      // chunk / feature row is computed once per run (it was the 64-wide heads' shift before; XL/2 took the direct path with
      // 2-byte scattered V^T stores: 142 us for its QKV GEMM).
      if ((p.head_dim & 7) == 0 && (dm & 63) == 0 && (p.tokens & 31) == 0 && (p.M % p.tokens) == 0 && (p.N % 64) == 0) {
        const int fw0 = f0 + wf * 64;
        const int which = fw0 / dm;                                   // wave-uniform
        const bool tr = fw0 < p.N && ((p.transpose_mask >> which) & 1);
        const int HD = p.head_dim, DP = p.head_dim_pad;
        __builtin_amdgcn_s_barrier();                                 // ring retired (all waves take this branch)
        if (tr) {
          char* stg = smem + wid * 8192;
          bf16_t* dst = (bf16_t*)(which == 0 ? p.out0 : (which == 1 ? p.out1 : p.out2));
          const int fr = lane >> 2, c = lane & 3;
          int64_t vrow[4];                                            // (head * DP + dim) of the lane's 4 feature rows
#pragma unroll
          for (int it = 0; it < 4; ++it) {
            const int fr_ = fw0 - which * dm + 16 * it + fr;
            const int hh_ = fr_ / HD;
            vrow[it] = (int64_t)hh_ * DP + (fr_ - hh_ * HD);
          }
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            const int tb = __builtin_amdgcn_readfirstlane(t0 + wt * 32 * NJ + j * 32);
            if (tb >= p.M) break;
            const int tp = (l31 & ~12) | ((l31 & 4) << 1) | ((l31 & 8) >> 1);     // key order of the attention kernel
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
              for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                  *reinterpret_cast<float*>(stg + (i * 32 + 8 * g + 4 * hi + e) * 128 + tp * 4) = acc[i][j][4 * g + e];
            const int b = tb / p.tokens, t = tb - b * p.tokens;
#pragma unroll
            for (int it = 0; it < 4; ++it) {
              const int f = 16 * it + fr;
              const float bv = p.bias ? p.bias[fw0 + f] : 0.f;
              const float4 v0 = *reinterpret_cast<const float4*>(stg + f * 128 + c * 32);
              const float4 v1 = *reinterpret_cast<const float4*>(stg + f * 128 + c * 32 + 16);
              uint4 o;
              o.x = pack2bf(v0.x + bv, v0.y + bv); o.y = pack2bf(v0.z + bv, v0.w + bv);
              o.z = pack2bf(v1.x + bv, v1.y + bv); o.w = pack2bf(v1.z + bv, v1.w + bv);
              *reinterpret_cast<uint4*>(dst + ((int64_t)b * p.heads * DP + vrow[it]) * p.tok_pad + t + 8 * c) = o;
            }
          }
        } else if (fw0 < p.N) {
          // q / k: [B, heads, tok_pad, 64] - the wave's 32 tokens x 64 features of one head are 4 KB of CONTIGUOUS memory:
          // stage as usual (row = token), come back with 8 features per lane and store 16 bytes per lane, 1 KB per instruction
          char* stg = smem + wid * 8192;
          bf16_t* dst = (bf16_t*)(which == 0 ? p.out0 : (which == 1 ? p.out1 : p.out2));
          const int r8 = lane >> 3, c8 = lane & 7;
          const int fc_ = fw0 - which * dm + 8 * c8;                  // the lane's 8-feature chunk: inside one head
          const int h = fc_ / HD, d8 = fc_ - h * HD;
          float4 b0 = make_float4(0.f, 0.f, 0.f, 0.f), b1 = b0;
          if (p.bias) { b0 = *reinterpret_cast<const float4*>(p.bias + fw0 + 8 * c8); b1 = *reinterpret_cast<const float4*>(p.bias + fw0 + 8 * c8 + 4); }
          // fused qk_norm: the 8 lanes c8 = 0..7 of a row hold the 64 features of one (token, head)
          const float* nw = (HD == 64 && DP == 64) ? (which == 0 ? p.hn0 : (which == 1 ? p.hn1 : nullptr)) : nullptr;   // the DPP reduction below is the 64-wide heads'
          float4 n0 = make_float4(1.f, 1.f, 1.f, 1.f), n1 = n0;
          if (nw) { n0 = *reinterpret_cast<const float4*>(nw + 8 * c8); n1 = *reinterpret_cast<const float4*>(nw + 8 * c8 + 4); }
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            const int tb = __builtin_amdgcn_readfirstlane(t0 + wt * 32 * NJ + j * 32);
            if (tb >= p.M) break;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
              for (int g = 0; g < 4; ++g) {
                const int c = i * 8 + 2 * g + hi;
                *reinterpret_cast<float4*>(stg + l31 * 256 + ((c ^ (l31 & 15)) << 4)) =
                    make_float4(acc[i][j][4 * g + 0], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]);
              }
            const int b = tb / p.tokens, t = tb - b * p.tokens;
#pragma unroll
            for (int it = 0; it < 4; ++it) {
              const int row = 8 * it + r8;
              float4 v0 = *reinterpret_cast<const float4*>(stg + row * 256 + (((2 * c8) ^ (row & 15)) << 4));
              float4 v1 = *reinterpret_cast<const float4*>(stg + row * 256 + (((2 * c8 + 1) ^ (row & 15)) << 4));
              v0.x += b0.x; v0.y += b0.y; v0.z += b0.z; v0.w += b0.w; v1.x += b1.x; v1.y += b1.y; v1.z += b1.z; v1.w += b1.w;
              if (nw) {                                            // wave-uniform
                float ss = (v0.x * v0.x + v0.y * v0.y) + (v0.z * v0.z + v0.w * v0.w) + (v1.x * v1.x + v1.y * v1.y) + (v1.z * v1.z + v1.w * v1.w);
                ss += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(ss), 0xB1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
                ss += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(ss), 0x4E, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
                ss += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(ss), 0x141, 0xf, 0xf, false));   // row_half_mirror
                const float rs = rsqrtf(ss * (1.0f / 64.0f) + p.hn_eps);
                v0.x *= rs * n0.x; v0.y *= rs * n0.y; v0.z *= rs * n0.z; v0.w *= rs * n0.w;
                v1.x *= rs * n1.x; v1.y *= rs * n1.y; v1.z *= rs * n1.z; v1.w *= rs * n1.w;
              }
              uint4 o;
              o.x = pack2bf(v0.x, v0.y); o.y = pack2bf(v0.z, v0.w);
              o.z = pack2bf(v1.x, v1.y); o.w = pack2bf(v1.z, v1.w);
              *reinterpret_cast<uint4*>(dst + (((int64_t)b * p.heads + h) * p.tok_pad + t + row) * DP + d8) = o;
            }
          }
        }
        return;
      }
    }
  }
  if (direct) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int tok = t0 + wt * 32 * NJ + j * 32 + l31;
      if (tok >= p.M) continue;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int fb = f0 + wf * 32 * NI + i * 32 + 8 * g + 4 * hi;
          if (fb < p.N)
            epilogue4<EPI>(p, tok, fb, acc[i][j][4 * g + 0], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]);
        }
      }
    }
    return;
  }
  __builtin_amdgcn_s_barrier();
  staged_epilogue<EPI, NI, NJ, (NW <= 8), kPre>(p, acc, smem + wid * 8192, f0 + wf * 32 * NI, t0 + wt * 32 * NJ, lane, xpre, re_pre, have_pre);
}


// ------------------------------------------------------------------------------------------------------------------
// r6: PERSISTENT one-wave-per-SIMD kernel ("p4", cfg 16).  256f x 256t tiles, 4 waves x (128f x 128t) with the 256 accumulators in
// AGPRs (the cfg-13 K loop: 64 MFMAs, 32 ds_read_b128, 16 LDS-DMA pieces per K stage of 64), ONE workgroup per CU walking its tiles.
// Why (profiles/r6_gemm.md): at K = 1024 a tile's loop is 33.8 k cycles (97 % of its MFMA bound), and the epilogue of a non-persistent
// kernel - 100 MB of bf16 written by all CUs at once with the matrix pipe idle - costs 22 - 30 us of a ~105 us fc1 launch.  The store
// path of a CU takes ~12 B / cycle for 16-byte-per-lane stores whatever the HBM does, so the stores have to run UNDER a K loop:
//  * the epilogue only computes: accumulators -> (+ bias, GELU) -> bf16, the 4-feature quads of lanes l and l + 32 exchanged with
//    v_permlane32_swap so that a lane holds 8 consecutive features of its token (one 16-byte store, no LDS staging - the ring already
//    belongs to the next tile), the packed tile parked in 128 VGPRs;
//  * the parked tile is stored from inside the NEXT tile's K loop, 3 stores in the third substep of eight stages (the first five and
//    the last three, which are compile-time positions); the vector-memory counter retires in order, so those stages' rendezvous is
//    `vmcnt(3)` - every DMA piece is older than the stores - and the stores have a whole stage to land before the next `vmcnt(0)`;
//  * the next tile's first two K stages (and its bias row, a 1 KB LDS image) are DMA'd while this tile's last two stages multiply;
//  * every tile runs the same code (the last tile "prefetches" itself: 128 KB of wasted fill per workgroup, no second code path).
// Requires M % 256 == 0, N % 256 == 0, K % 128 == 0, K >= 512 (interior tiles only: the launcher falls back otherwise).
template <int EPI>
__global__ __launch_bounds__(256, 1) void gemm_bf16_p4_kernel(GemmP p) {
  constexpr int NI = 4, NJ = 4, NM = 16, NR = 8;
  constexpr int BF = 256, BT = 256, WB = BF * 128, STAGEB = (BF + BT) * 128, NPW = 16;
  constexpr int BIASB = 2 * STAGEB;                         // two 1 KB bias images (tile parity) above the ring
  constexpr int D1 = 8, LH = 12;                            // DMA pieces of a stage: [0, D1) behind the barrier two stages ahead, [D1, LH) / [LH, NPW) in the next stage's first two substeps
  static_assert(EPI == LN3D_EPI_BF16 || EPI == LN3D_EPI_GELU_ERF, "p4 epilogues");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wf = wid >> 1, wt = wid & 1;
  const int l31 = lane & 31, hi = lane >> 5;
  const int nft = p.N / BF, ntt = p.M / BT, ntiles = nft * ntt;
  const int G = gridDim.x;
  auto tile_of = [&](int b, int& ft, int& tt) __attribute__((always_inline)) {
    const int xcd = b & 7, slot = b >> 3;
    if ((ntt & 7) == 0 && (nft & 3) == 0) {                 // an XCD owns ntt/8 token panels and walks the feature tiles in groups of 4
      const int rows = ntt >> 3;
      const int g = slot / (rows * 4), rem = slot - g * rows * 4;
      ft = g * 4 + (rem & 3);
      tt = xcd * rows + (rem >> 2);
    } else {
      const int q = ntiles >> 3, r = ntiles & 7;
      const int tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
      ft = tile % nft; tt = tile / nft;
    }
  };
  // lane offsets of the wave's 16 DMA pieces (8 W row groups, 8 X row groups): the same for every tile (interior tiles only)
  const int r8 = lane >> 3;
  // piece q covers rows 8 (8 wid + (q & 7)) + r8 of its operand tile: the (q & 7) term rides on the scalar base (8 rows = 8 ld bytes * 2),
  // the swizzle chunk only depends on ((row >> 1) & 7) = ((4 (q & 7) + (r8 >> 1)) & 7): pieces of equal parity share the lane offset
  uint32_t soff[2][2];                                      // [operand][q & 1]
#pragma unroll
  for (int o = 0; o < 2; ++o)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int rt = 8 * (wid * 8 + h) + r8;
      const int chunk = (lane & 7) ^ ((rt >> 1) & 7);
      soff[o][h] = (uint32_t)(((int64_t)(8 * wid * 8 + r8) * (o == 0 ? p.ldw : p.ldx) + chunk * 8) * 2);
    }
  const int64_t ld8w = 8 * p.ldw * 2, ld8x = 8 * p.ldx * 2;   // bytes per 8 rows
  const int dW0 = wid * 8 * 1024, dX0 = WB + wid * 8 * 1024;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_void_t*)smem;
#define P_ISSUE(WP, XP, slot, q) lds_dma16_s(((q) < 8 ? (WP) + ((q) & 7) * ld8w : (XP) + ((q) & 7) * ld8x), soff[(q) >> 3][(q) & 1], lds0 + (slot) * STAGEB + ((q) < 8 ? dW0 + (q) * 1024 : dX0 + ((q) - 8) * 1024))
  const int key = (l31 >> 1) & 7;
  const int a_row = (wf * 128 + l31) * 128;
  const int b_row = WB + (wt * 128 + l31) * 128;
#define P_RDA(slot, ks, i) (*reinterpret_cast<const bf16x8*>(smem + (slot) * STAGEB + a_row + (i) * 4096 + (((2 * (ks) + hi) ^ key) << 4)))
#define P_RDB(slot, ks, j) (*reinterpret_cast<const bf16x8*>(smem + (slot) * STAGEB + b_row + (j) * 4096 + (((2 * (ks) + hi) ^ key) << 4)))
#define P_MMA(FA, FB, n) acc[(n) / NJ][(n) % NJ] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(FA[(n) / NJ], FB[(n) % NJ], acc[(n) / NJ][(n) % NJ], 0, 0, 0)
#define P_MMA0(FA, FB, n) acc[(n) / NJ][(n) % NJ] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(FA[(n) / NJ], FB[(n) % NJ], kZero16, 0, 0, 0)
  const f32x16 kZero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  // parked output of the previous tile: entry (j, i, m) = 8 features [32 i + 16 m + 8 hi, + 8) of token 32 j + l31 of the wave's sub-tile
  uint4 pend[24];                                            // token blocks 1 .. 3 (block 0 is stored from the epilogue: 128 parked VGPRs spilled)
  char* pbase = nullptr;                                     // lane address of entry (0, 0, 0) in the previous tile's output
  bool have = false;                                         // wave-uniform
  const int64_t jstride = (int64_t)32 * p.ldo * 2;
#define P_STORE(j, k) *reinterpret_cast<uint4*>(pbase + (j) * jstride + ((k) >> 1) * 64 + ((k) & 1) * 32) = pend[((j) - 1) * 8 + (k)]
#define P_STOREQ(q) P_STORE(1 + (q) / 8, (q) % 8)          // parked entry q = 0..23
  // substep: multiply (af, CB) while the next substep (rslot, ks2) is read: the token fragments into the other set NB (slots 1, 2, 4, 5),
  // the weight fragments IN PLACE - af[i] is last used by MFMA 4 i + 3 and next by MFMA 4 i of the following substep, 13 slots later, so
  // one register set serves (16 VGPRs that the parked output tile needs).  LATE: DMA pieces [L0, L1) of the NEXT stage into the other
  // slot; SJ >= 0: parked stores 3 SJ .. 3 SJ + 2, one behind every fourth MFMA; ZERO: the tile's first substep multiplies into C = 0;
  // SYNC: the stage's rendezvous sits behind the first MFMA (the reads then come from the other slot, which it publishes)
#define P_PHASE(CB, NB, rslot, ks2, RD, LATE, WL, XL, dslot, L0, L1, SJ, ZERO, SYNC, FILL, WF, XF, fslot)  \
  _Pragma("unroll") for (int n = 0; n < NM; ++n) {                                                        \
    if (ZERO) { P_MMA0(af, CB, n); } else { P_MMA(af, CB, n); }                                           \
    if ((SYNC) && n == 0) {                                                                               \
      if ((SJ) >= 0 && have) { asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); }                         \
      else { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }                                           \
      __builtin_amdgcn_s_waitcnt(0xC07F);                                                                 \
      __builtin_amdgcn_s_barrier();                                                                       \
    }                                                                                                     \
    if (RD) {                                                                                             \
      if ((n & 3) == 3) af[n >> 2] = P_RDA(rslot, ks2, n >> 2);                                           \
      else if (n == 1 || n == 2) NB[n - 1] = P_RDB(rslot, ks2, n - 1);                                    \
      else if (n == 4 || n == 5) NB[n - 2] = P_RDB(rslot, ks2, n - 2);                                    \
    }                                                                                                     \
    if (LATE) {                                                                                           \
      _Pragma("unroll") for (int d = (L0); d < (L1); ++d)                                                 \
          if ((d - (L0)) * NM / ((L1) - (L0)) == n) P_ISSUE(WL, XL, dslot, d);                            \
    }                                                                                                     \
    if (FILL) {                                                                                           \
      _Pragma("unroll") for (int d = 0; d < D1; ++d)                                                      \
          if (1 + d * (NM - 1) / D1 == n) P_ISSUE(WF, XF, fslot, d);                                      \
    }                                                                                                     \
    if (!(SYNC) && (SJ) >= 0 && (n & 3) == 1 && n < 12) { if (have) P_STOREQ(3 * ((SJ) < 0 ? 0 : (SJ)) + (n >> 2)); } \
    __builtin_amdgcn_sched_barrier(0);                                                                    \
  }
  // One K stage on `slot`.  LATE: pieces [D1, NPW) of the next stage (sources WL / XL) go into the other slot during the first two
  // substeps; the third substep carries the parked stores of group SJ (if any).  Behind the first MFMA of the last substep: own DMAs
  // of the next stage landed - vmcnt(3) when this stage issued stores (they are the 3 youngest operations; the counter retires in
  // order), else vmcnt(0) -, own fragment reads retired, barrier; then the first fragments of the next stage are read (PRE) and pieces
  // [0, D1) of the stage after it (sources WF / XF) go into THIS slot, which the barrier just retired.
#define P_STAGE(slot, LATE, WL, XL, WF, XF, SJ, ZERO, PRE)                                                \
  {                                                                                                       \
    P_PHASE(b0, b1, slot, 1, true, LATE, WL, XL, (slot) ^ 1, D1, LH, -1, ZERO, false, false, WF, XF, slot);      \
    P_PHASE(b1, b0, slot, 2, true, LATE, WL, XL, (slot) ^ 1, LH, NPW, -1, false, false, false, WF, XF, slot);    \
    P_PHASE(b0, b1, slot, 3, true, false, WL, XL, (slot) ^ 1, 0, 1, SJ, false, false, false, WF, XF, slot);      \
    P_PHASE(b1, b0, (slot) ^ 1, 0, PRE, false, WL, XL, (slot) ^ 1, 0, 1, SJ, false, true, true, WF, XF, slot);   \
  }

  f32x16 acc[NI][NJ];
  bf16x8 af[NI], b0[NJ], b1[NJ];
  const int ns = p.K / 64;
  const int64_t ldw2 = p.ldw * 2, ldx2 = p.ldx * 2;

  int vb = blockIdx.x, ft, tt;
  tile_of(vb, ft, tt);
  const char* Wc = reinterpret_cast<const char*>(p.W) + (int64_t)ft * BF * ldw2;
  const char* Xc = reinterpret_cast<const char*>(p.X) + (int64_t)tt * BT * ldx2;
  int par = 0;                                              // bias image of the current tile
  // prologue: both stages of the first tile and its bias row, landed before the loop
#pragma unroll
  for (int q = 0; q < NPW; ++q) P_ISSUE(Wc, Xc, 0, q);
#pragma unroll
  for (int q = 0; q < NPW; ++q) P_ISSUE(Wc + 128, Xc + 128, 1, q);
  const uint32_t boff = (uint32_t)lane * 16;
  if (p.bias) { if (wid == 0) lds_dma16_s(p.bias + ft * BF, boff, lds0 + BIASB); }
  else if (wid < 2) *reinterpret_cast<float4*>(smem + BIASB + wid * 1024 + lane * 16) = make_float4(0.f, 0.f, 0.f, 0.f);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_s_waitcnt(0xC07F);                        // nothing but LDS reads pending inside the loop (kernel-argument s_loads retired)

  for (;;) {
    const int vbn = vb + G;
    const bool has_next = vbn < ntiles;
    int ftn, ttn;
    tile_of(has_next ? vbn : vb, ftn, ttn);
    const char* Wn = reinterpret_cast<const char*>(p.W) + (int64_t)ftn * BF * ldw2;
    const char* Xn = reinterpret_cast<const char*>(p.X) + (int64_t)ttn * BT * ldx2;
    // first fragments of this tile (its stage 0 landed and was published by the previous tile's last rendezvous / the prologue): read
    // here rather than under the last stage, so that 32 VGPRs are not live across the epilogue (they spilled)
#pragma unroll
    for (int i = 0; i < NI; ++i) af[i] = P_RDA(0, 0, i);
#pragma unroll
    for (int j = 0; j < NJ; ++j) b0[j] = P_RDB(0, 0, j);
    // stages 0 .. 4 and ns - 3 .. ns - 1 are compile-time positions: each carries 3 of the previous tile's 24 parked stores
    P_STAGE(0, false, Wc, Xc, Wc + 2 * 128, Xc + 2 * 128, 0, true, true);                                          // s = 0: C = 0
    P_STAGE(1, true, Wc + 2 * 128, Xc + 2 * 128, Wc + 3 * 128, Xc + 3 * 128, 1, false, true);
    P_STAGE(0, true, Wc + 3 * 128, Xc + 3 * 128, Wc + 4 * 128, Xc + 4 * 128, 2, false, true);
    P_STAGE(1, true, Wc + 4 * 128, Xc + 4 * 128, Wc + 5 * 128, Xc + 5 * 128, 3, false, true);
    P_STAGE(0, true, Wc + 5 * 128, Xc + 5 * 128, Wc + 6 * 128, Xc + 6 * 128, 4, false, true);
    for (int s = 5; s + 3 < ns; s += 2) {
      P_STAGE(1, true, Wc + (s + 1) * 128, Xc + (s + 1) * 128, Wc + (s + 2) * 128, Xc + (s + 2) * 128, -1, false, true);  // s odd
      P_STAGE(0, true, Wc + (s + 2) * 128, Xc + (s + 2) * 128, Wc + (s + 3) * 128, Xc + (s + 3) * 128, -1, false, true);  // s + 1
    }
    P_STAGE(1, true, Wc + (ns - 2) * 128, Xc + (ns - 2) * 128, Wc + (ns - 1) * 128, Xc + (ns - 1) * 128, 5, false, true);  // s = ns - 3
    P_STAGE(0, true, Wc + (ns - 1) * 128, Xc + (ns - 1) * 128, Wn, Xn, 6, false, true);                            // s = ns - 2: fills the next tile's stage 0
    P_STAGE(1, true, Wn, Xn, Wn + 128, Xn + 128, 7, false, false);                                                  // s = ns - 1: ... and its stage 1; a0 / b0 = its first fragments
#pragma unroll
    for (int d = D1; d < NPW; ++d) P_ISSUE(Wn + 128, Xn + 128, 1, d);                                        // rest of the next tile's stage 1
    if (p.bias && wid == 0) lds_dma16_s(p.bias + ftn * BF, boff, lds0 + BIASB + (par ^ 1) * 1024);

    // ---- epilogue: accumulators -> parked bf16 tile (registers only).  Bias is always added from the LDS image (zeros when the
    // launch has none: a runtime test inside the unrolled block made hipcc round-trip all 256 accumulators through AGPR writes)
    {
      const float* bl = reinterpret_cast<const float*>(smem + BIASB + par * 1024) + wf * 128 + 4 * hi;
      char* const nbase = reinterpret_cast<char*>((bf16_t*)p.out0 + (int64_t)(tt * BT + wt * 128 + l31) * p.ldo + ft * BF + wf * 128 + 8 * hi);
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        ln3d_f32x2 bq[2][4];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          const float4 bA = *reinterpret_cast<const float4*>(bl + i * 32 + 16 * m), bB = *reinterpret_cast<const float4*>(bl + i * 32 + 16 * m + 8);
          bq[m][0] = ln3d_f32x2{bA.x, bA.y}; bq[m][1] = ln3d_f32x2{bA.z, bA.w}; bq[m][2] = ln3d_f32x2{bB.x, bB.y}; bq[m][3] = ln3d_f32x2{bB.z, bB.w};
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
#pragma unroll
          for (int m = 0; m < 2; ++m) {
            ln3d_f32x2 v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = ln3d_f32x2{acc[i][j][8 * m + 2 * e], acc[i][j][8 * m + 2 * e + 1]} + bq[m][e];
            if constexpr (EPI == LN3D_EPI_GELU_ERF) {
#pragma unroll
              for (int e = 0; e < 4; ++e) { float g0 = v[e].x, g1 = v[e].y; gelu_erf2(g0, g1); v[e] = ln3d_f32x2{g0, g1}; }
            }
            // lanes l / l + 32 exchange quads: lower lanes end up with features [16m, 16m + 8), upper lanes with [16m + 8, 16m + 16)
            const uint32_t x0 = pack2bf(v[0].x, v[0].y), x1 = pack2bf(v[1].x, v[1].y), y0 = pack2bf(v[2].x, v[2].y), y1 = pack2bf(v[3].x, v[3].y);
            const auto r0 = __builtin_amdgcn_permlane32_swap(x0, y0, false, false);
            const auto r1 = __builtin_amdgcn_permlane32_swap(x1, y1, false, false);
            if (j == 0) *reinterpret_cast<uint4*>(nbase + i * 64 + m * 32) = make_uint4(r0[0], r1[0], r0[1], r1[1]);
            else pend[(j - 1) * 8 + i * 2 + m] = make_uint4(r0[0], r1[0], r0[1], r1[1]);
          }
          __builtin_amdgcn_sched_barrier(0);           // one accumulator tile at a time: without it hipcc hoists the AGPR reads of the whole block and spills
        }
      }
      pbase = nbase;
      have = true;
    }
    if (!has_next) break;
    vb = vbn; ft = ftn; tt = ttn; Wc = Wn; Xc = Xn; par ^= 1;
  }
  // the last tile's output; the self-prefetch of the last tile must not outlive the workgroup's LDS
#pragma unroll
  for (int j = 1; j < NJ; ++j)
#pragma unroll
    for (int k = 0; k < 8; ++k) P_STORE(j, k);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#undef P_ISSUE
#undef P_RDA
#undef P_RDB
#undef P_MMA
#undef P_STORE
#undef P_STOREQ
#undef P_MMA0
#undef P_PHASE
#undef P_STAGE
}

template <int EPI>
static int launch_p4(const GemmP& p, hipStream_t s) {
  constexpr int LDSB = 2 * (256 + 256) * 128 + 2048;
  static_assert(LDSB <= 163840, "ring + bias images");
  static AttrOnce attr_once;
  if (attr_once.need())
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_bf16_p4_kernel<EPI>), hipFuncAttributeMaxDynamicSharedMemorySize, LDSB);
  const int ntiles = (p.N / 256) * (p.M / 256), cus = ln3d_device_cus();
  hipLaunchKernelGGL((gemm_bf16_p4_kernel<EPI>), dim3(ntiles < cus ? ntiles : cus), dim3(256), LDSB, s, p);
  return ln3d_check_launch();
}

template <int EPI, int NW, int WGT, int NI, int NJ>
static int launch_ring64(const GemmP& p, hipStream_t s) {
  constexpr int BF = 32 * NI * (NW / WGT), BT = 32 * NJ * WGT;
  constexpr int LDSB = 2 * (BF + BT) * 128 + (EPI == LN3D_EPI_CROSS_ATTN ? (NW / WGT) * 96 * 128 : 0);
  static_assert(2 * (BF + BT) * 128 >= NW * 8192 && LDSB <= 163840, "staging regions live in the ring");
  static AttrOnce attr_once;
  if (attr_once.need()) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_bf16_ring64_kernel<EPI, NW, WGT, NI, NJ>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, LDSB);
  }
  const int nft = (p.N + BF - 1) / BF, ntt = (p.M + BT - 1) / BT;
  hipLaunchKernelGGL((gemm_bf16_ring64_kernel<EPI, NW, WGT, NI, NJ>), dim3(nft * ntt), dim3(NW * 64), LDSB, s, p);
  return ln3d_check_launch();
}

template <int EPI>
static int launch(const GemmP& p, hipStream_t s) {
  static AttrOnce attr_once;
  if (attr_once.need()) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_bf16_kernel<EPI>),
                        hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS);
  }
  const int nft = (p.N + BMF - 1) / BMF, ntt = (p.M + BTK - 1) / BTK;
  hipLaunchKernelGGL(gemm_bf16_kernel<EPI>, dim3(nft * ntt), dim3(256), GEMM_LDS, s, p);
  return ln3d_check_launch();
}

// The launch of one row of ln3d_gemm_tiles (csrc/kernel_plan.h): kernel and template parameters come from the row.  ln3d_plan_gemm only
// returns rows that are instantiated for the epilogue, so the refusal below is never reached; it keeps the other epilogues' kernels
// from being instantiated.
template <int EPI, int ROW>
static int launch_tile(const GemmP& p, hipStream_t s) {
  constexpr Ln3dGemmTile t = ln3d_gemm_tiles[ROW];
  if constexpr (!(t.epis & ln3d_epi_bit(EPI))) return LN3D_ERR_UNSUPPORTED;
  else if constexpr (t.kind == LN3D_TILE_STAGED) return launch<EPI>(p, s);
  else if constexpr (t.kind == LN3D_TILE_PERSISTENT) return launch_p4<EPI>(p, s);
  else return launch_ring64<EPI, t.nw, t.wgt, t.ni, t.nj>(p, s);
}
template <int EPI>
static int run_tile(const GemmP& p, hipStream_t s, int row) {
  static_assert(LN3D_GEMM_TILE_ROWS == 8, "one case per row");
  switch (row) {
    case LN3D_TILE_256x256: return launch_tile<EPI, LN3D_TILE_256x256>(p, s);
    case LN3D_TILE_128x384: return launch_tile<EPI, LN3D_TILE_128x384>(p, s);
    case LN3D_TILE_256x192: return launch_tile<EPI, LN3D_TILE_256x192>(p, s);
    case LN3D_TILE_384x192: return launch_tile<EPI, LN3D_TILE_384x192>(p, s);
    case LN3D_TILE_128x192: return launch_tile<EPI, LN3D_TILE_128x192>(p, s);
    case LN3D_TILE_256x256_P4: return launch_tile<EPI, LN3D_TILE_256x256_P4>(p, s);
    case LN3D_TILE_256x256_W4: return launch_tile<EPI, LN3D_TILE_256x256_W4>(p, s);
    default: return launch_tile<EPI, LN3D_TILE_S128>(p, s);
  }
}

// LN3D_GEMM_TILE (measurement switch, read once per process): s = the 128x128 register-staged kernel, x<id> = that row of the tile
// table (an id the table does not have runs the 128x128 kernel), anything else = unforced
static int g_gemm_forced = -2;           // environment switch, parsed once (ln3d_reload_env() re-reads it)
static int forced_tile() {
  if (g_gemm_forced == -2) {
    const char* e = getenv("LN3D_GEMM_TILE");
    g_gemm_forced = !e ? -1 : (e[0] == 's' ? 0 : (e[0] == 'x' ? atoi(e + 1) : -1));
  }
  return g_gemm_forced;
}
extern "C" void ln3d_gemm_reload_env(void) { g_gemm_forced = -2; }

extern "C" int ln3d_gemm_heads_norm_fusable(int M, int N, int tokens, int head_dim, int head_dim_pad) {
  if (head_dim_pad <= 0) head_dim_pad = head_dim;
  if (!(head_dim == 64 && head_dim_pad == 64 && tokens > 0 && (tokens & 31) == 0 && (M % tokens) == 0 && (N % 64) == 0)) return 0;
  // neither K nor the output alignment enters the plan of a LN3D_EPI_HEADS launch
  return ln3d_gemm_tiles[ln3d_plan_gemm(M, N, 0, LN3D_EPI_HEADS, true, true, ln3d_device_cus(), forced_tile())].head_row ? 1 : 0;
}

extern "C" int ln3d_gemm_bf16(const ln3d_gemm_args* a, void* stream) {
  if (!a || !a->X || !a->W || !a->out0) return LN3D_ERR_BAD_ARG;
  if (a->M <= 0 || a->N <= 0 || a->K <= 0 || (a->K % BK) != 0 || (a->N % 4) != 0) return LN3D_ERR_BAD_ARG;
  if ((a->ldx % 8) != 0 || (a->ldw % 8) != 0) return LN3D_ERR_BAD_ARG;
  if (a->epilogue == LN3D_EPI_GATE_RES) {
    // the epilogue reads float4 quads at gate / res_bias + sample * ld + feature: 16-byte aligned rows, and a per-sample row needs
    // gate_rows (rows per sample) - with it left at 0 every TOKEN would index a row of a [samples, N] buffer
    if (a->gate && ((a->gate_ld % 4) != 0 || ((uintptr_t)a->gate & 15) != 0)) return LN3D_ERR_BAD_ARG;
    if (a->res_bias && ((a->res_bias_ld % 4) != 0 || ((uintptr_t)a->res_bias & 15) != 0)) return LN3D_ERR_BAD_ARG;
    if ((a->gate || a->res_bias) && a->gate_rows <= 0) return LN3D_ERR_BAD_ARG;
  }
  GemmP p;
  p.X = (const bf16_t*)a->X; p.W = (const bf16_t*)a->W; p.bias = a->bias;
  p.ldx = a->ldx; p.ldw = a->ldw; p.ldo = a->ldo;
  p.M = a->M; p.N = a->N; p.K = a->K;
  p.out0 = a->out0; p.out1 = a->out1; p.out2 = a->out2;
  p.gate = a->gate; p.gate_rows = a->gate_rows > 0 ? a->gate_rows : 1; p.gate_ld = a->gate_ld;
  p.tokens = a->tokens; p.tok_pad = a->tok_pad; p.heads = a->heads; p.head_dim = a->head_dim;
  p.transpose_mask = a->transpose_mask;
  p.head_dim_pad = a->head_dim_pad > 0 ? a->head_dim_pad : a->head_dim;
  p.ctx_keys = a->ctx_keys; p.ctx_pad = a->ctx_pad; p.ctx_scale_log2 = a->ctx_scale * 1.4426950408889634f;
  p.hn0 = a->head_norm0; p.hn1 = a->head_norm1; p.hn_eps = a->head_norm_eps;
  p.rb = a->epilogue == LN3D_EPI_GATE_RES ? a->res_bias : nullptr; p.rb_ld = a->res_bias_ld;
  hipStream_t s = (hipStream_t)stream;
  // head split: the head_row tiles have the staged, head-aware epilogue (any head size that is a multiple of 8 with
  // heads * head_dim a multiple of 64)
  const bool head_staged = a->epilogue == LN3D_EPI_HEADS && a->head_dim > 0 && (a->head_dim & 7) == 0 && a->heads > 0 &&
                           ((a->heads * a->head_dim) & 63) == 0 && a->tokens > 0 && (a->tokens & 31) == 0 && (a->M % a->tokens) == 0 &&
                           (a->N % 64) == 0;
  const bool out_aligned = (a->ldo % 8) == 0 && ((uintptr_t)a->out0 & 15) == 0 && (!a->bias || ((uintptr_t)a->bias & 15) == 0);
  const int row = ln3d_plan_gemm(a->M, a->N, a->K, a->epilogue, head_staged, out_aligned, ln3d_device_cus(), forced_tile());
  switch (a->epilogue) {
    case LN3D_EPI_F32: return run_tile<LN3D_EPI_F32>(p, s, row);
    case LN3D_EPI_BF16: return run_tile<LN3D_EPI_BF16>(p, s, row);
    case LN3D_EPI_GELU_ERF: return run_tile<LN3D_EPI_GELU_ERF>(p, s, row);
    case LN3D_EPI_GELU_TANH: return run_tile<LN3D_EPI_GELU_TANH>(p, s, row);
    case LN3D_EPI_SILU: return run_tile<LN3D_EPI_SILU>(p, s, row);
    case LN3D_EPI_QUICK_GELU: return run_tile<LN3D_EPI_QUICK_GELU>(p, s, row);
    case LN3D_EPI_CROSS_ATTN:
      if (!a->out1 || !a->out2 || a->bias || a->head_dim != 64 || a->heads <= 0 || a->N != a->heads * 64 || a->tokens <= 0 ||
          (a->tokens % 192) != 0 || (a->M % a->tokens) != 0 || a->ctx_keys <= 0 || a->ctx_keys > 96 || a->ctx_pad < a->ctx_keys ||
          (a->ctx_pad % 64) != 0 || (a->N % 256) != 0)
        return LN3D_ERR_BAD_ARG;
      return run_tile<LN3D_EPI_CROSS_ATTN>(p, s, row);
    case LN3D_EPI_GATE_RES: return run_tile<LN3D_EPI_GATE_RES>(p, s, row);
    case LN3D_EPI_F32_SILU:
      if (!a->out1) return LN3D_ERR_BAD_ARG;
      return run_tile<LN3D_EPI_F32_SILU>(p, s, row);
    case LN3D_EPI_HEADS:
      if (a->tokens <= 0 || a->heads <= 0 || a->head_dim <= 0 || (a->head_dim % 4) != 0 || a->tok_pad < a->tokens)
        return LN3D_ERR_BAD_ARG;
      if ((a->head_norm0 || a->head_norm1) &&
          !(ln3d_gemm_tiles[row].head_row && a->head_dim == 64 && p.head_dim_pad == 64 && (a->tokens & 31) == 0 &&
            (a->M % a->tokens) == 0 && (a->N % 64) == 0))
        return LN3D_ERR_UNSUPPORTED;                  // only the head-aligned staged epilogue normalises
      return run_tile<LN3D_EPI_HEADS>(p, s, row);
    default: return LN3D_ERR_UNSUPPORTED;
  }
}
