// Shared by the bf16 and MX-FP8 GEMMs (gemm_bf16.hip, gemm_mx.hip): the kernel parameter block and the fused epilogues that
// run on a 32x32 MFMA accumulator tile.  Both MFMA families (v_mfma_f32_32x32x16_bf16 and v_mfma_scale_f32_32x32x64_f8f6f4)
// hand their fp32 results over in the same C/D layout: row (feature) = (r&3) + 8(r>>2) + 4(lane>>5), column (token) = lane&31.
#pragma once
#include "common.h"
#include "../../include/ln3d.h"

struct GemmP {
  const bf16_t* X; const bf16_t* W; const float* bias;
  int64_t ldx, ldw, ldo;
  int M, N, K;
  void* out0; void* out1; void* out2;
  const float* gate; int gate_rows; int64_t gate_ld;
  int tokens, tok_pad, heads, head_dim, transpose_mask, head_dim_pad;
  int ctx_keys, ctx_pad; float ctx_scale_log2;
  const float* hn0; const float* hn1; float hn_eps;   // HEADS: fused qk_norm weights (outputs 0 / 1) or NULL
  const float* rb; int64_t rb_ld;                      // GATE_RES: per-sample row added after gating (sample = row / gate_rows) or NULL
};

template <int EPI>
__device__ __forceinline__ void epilogue4(const GemmP& p, int tok, int fb, float v0, float v1, float v2, float v3) {
  // 4 consecutive features fb..fb+3 of token `tok` (all in range, fb % 4 == 0)
  if (p.bias) {
    const float4 b = *reinterpret_cast<const float4*>(p.bias + fb);
    v0 += b.x; v1 += b.y; v2 += b.z; v3 += b.w;
  }
  if constexpr (EPI == LN3D_EPI_F32) {
    *reinterpret_cast<float4*>((float*)p.out0 + (int64_t)tok * p.ldo + fb) = make_float4(v0, v1, v2, v3);
  } else if constexpr (EPI == LN3D_EPI_BF16 || EPI == LN3D_EPI_GELU_ERF || EPI == LN3D_EPI_GELU_TANH ||
                       EPI == LN3D_EPI_SILU || EPI == LN3D_EPI_QUICK_GELU || EPI == LN3D_EPI_CROSS_ATTN) {
    if constexpr (EPI == LN3D_EPI_QUICK_GELU) { v0 = quick_gelu(v0); v1 = quick_gelu(v1); v2 = quick_gelu(v2); v3 = quick_gelu(v3); }
    if constexpr (EPI == LN3D_EPI_GELU_ERF) { gelu_erf2(v0, v1); gelu_erf2(v2, v3); }
    if constexpr (EPI == LN3D_EPI_GELU_TANH) { v0 = gelu_tanh(v0); v1 = gelu_tanh(v1); v2 = gelu_tanh(v2); v3 = gelu_tanh(v3); }
    if constexpr (EPI == LN3D_EPI_SILU) { v0 = silu(v0); v1 = silu(v1); v2 = silu(v2); v3 = silu(v3); }
    uint2 o; o.x = pack2bf(v0, v1); o.y = pack2bf(v2, v3);
    *reinterpret_cast<uint2*>((bf16_t*)p.out0 + (int64_t)tok * p.ldo + fb) = o;
  } else if constexpr (EPI == LN3D_EPI_F32_SILU) {
    *reinterpret_cast<float4*>((float*)p.out0 + (int64_t)tok * p.ldo + fb) = make_float4(v0, v1, v2, v3);
    uint2 o; o.x = pack2bf(silu(v0), silu(v1)); o.y = pack2bf(silu(v2), silu(v3));
    *reinterpret_cast<uint2*>((bf16_t*)p.out1 + (int64_t)tok * p.ldo + fb) = o;
  } else if constexpr (EPI == LN3D_EPI_GATE_RES) {
    if (p.gate) {
      const float4 g = *reinterpret_cast<const float4*>(p.gate + (int64_t)(tok / p.gate_rows) * p.gate_ld + fb);
      v0 *= g.x; v1 *= g.y; v2 *= g.z; v3 *= g.w;
    }
    if (p.rb) {
      const float4 r = *reinterpret_cast<const float4*>(p.rb + (int64_t)(tok / p.gate_rows) * p.rb_ld + fb);
      v0 += r.x; v1 += r.y; v2 += r.z; v3 += r.w;
    }
    float4* xp = reinterpret_cast<float4*>((float*)p.out0 + (int64_t)tok * p.ldo + fb);
    float4 x = *xp;
    x.x += v0; x.y += v1; x.z += v2; x.w += v3;
    *xp = x;
    if (p.out1) {
      uint2 o; o.x = pack2bf(x.x, x.y); o.y = pack2bf(x.z, x.w);
      *reinterpret_cast<uint2*>((bf16_t*)p.out1 + (int64_t)tok * p.ldo + fb) = o;
    }
  } else if constexpr (EPI == LN3D_EPI_HEADS) {
    const int dm = p.heads * p.head_dim;
    const int which = fb / dm;
    const int rem = fb - which * dm;
    const int h = rem / p.head_dim, d = rem - h * p.head_dim;
    const int b = tok / p.tokens, t = tok - b * p.tokens;
    bf16_t* dst = (bf16_t*)(which == 0 ? p.out0 : (which == 1 ? p.out1 : p.out2));
    const int64_t bh = (int64_t)b * p.heads + h;
    if (!((p.transpose_mask >> which) & 1)) {
      uint2 o; o.x = pack2bf(v0, v1); o.y = pack2bf(v2, v3);
      *reinterpret_cast<uint2*>(dst + (bh * p.tok_pad + t) * p.head_dim_pad + d) = o;
    } else {
      // V^T: tokens of every 16-group stored in the order [0-3, 8-11, 4-7, 12-15] (bits 2 and 3 of t swapped) - the
      // order in which the attention kernel's S^T accumulator hands P to the PV MFMA (csrc/attention.hip)
      const int tp = (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1);
      bf16_t* q = dst + (bh * p.head_dim_pad + d) * p.tok_pad + tp;
      q[0] = f2bf(v0); q[p.tok_pad] = f2bf(v1); q[2 * (int64_t)p.tok_pad] = f2bf(v2); q[3 * (int64_t)p.tok_pad] = f2bf(v3);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Epilogue of the LDS-DMA kernels.  A lane's accumulator quad is 4 consecutive features of ONE token and lanes 0-31 are 32
// different tokens, so storing straight from the accumulators writes 16-byte pieces scattered over 32 output rows per
// instruction (measured: ~1.5 TB/s, a third of a K = 1024 GEMM).  Instead every wave transposes its own sub-tile through a
// private 8 KB fp32 LDS region (the ring is free after the main loop), 32 tokens x 64 features at a time, and comes back
// with 16 consecutive lanes holding the 64 consecutive features of one token: each store instruction then writes four
// complete 128-byte (bf16) / 256-byte (f32) row segments and the bias / gate / residual traffic is row-contiguous too.
// 256-byte staging rows, 16-byte chunk c of row r stored at chunk c ^ (r & 15): conflict-free ds_write_b128 (8-lane
// groups = 8 rows) and ds_read_b128 (16-lane groups) without padding.  DS operations of one wave execute in order, so
// no barrier is needed beyond the caller's one that retires the ring.
// Per-lane context of the staged epilogue: the lane keeps one feature quad fb and walks 32 consecutive tokens, so
// everything that depends on fb (bias, head / dim split) or on the run's first token (sample index, gate rows, base
// pointers) is computed once per run instead of once per store: the head-split epilogue spent more time in integer
// divisions and 64-bit multiplies than in stores before this.
template <int EPI>
struct RunEpi {
  float4 bias;
  bool generic;            // a sample shorter than the run (or a transposed target): per-element path
  // HEADS
  bf16_t* hbase; int64_t hwrap; int hrows_left; int hstride;
  // GATE_RES
  float4 g0, g1; int grows_left;
  float4 r0, r1;            // res_bias rows of the run's first sample / the next one

  __device__ __forceinline__ void init_feature(const GemmP& p, int fb, int& which, int& h, int& d) const {
    const int dm = p.heads * p.head_dim;
    which = fb / dm;
    const int rem = fb - which * dm;
    h = rem / p.head_dim; d = rem - h * p.head_dim;
  }
  __device__ __forceinline__ void init(const GemmP& p, int fb, int tb, int which, int h, int d) {
    bias = p.bias ? *reinterpret_cast<const float4*>(p.bias + fb) : make_float4(0.f, 0.f, 0.f, 0.f);
    generic = false;
    if constexpr (EPI == LN3D_EPI_HEADS) {
      generic = p.tokens < 32 || ((p.transpose_mask >> which) & 1);
      const int b0 = tb / p.tokens, t0 = tb - b0 * p.tokens;
      bf16_t* dst = (bf16_t*)(which == 0 ? p.out0 : (which == 1 ? p.out1 : p.out2));
      hbase = dst + (((int64_t)b0 * p.heads + h) * p.tok_pad + t0) * p.head_dim_pad + d;
      hwrap = ((int64_t)p.heads * p.tok_pad - p.tokens) * p.head_dim_pad;
      hrows_left = p.tokens - t0;
      hstride = p.head_dim_pad;
    }
    if constexpr (EPI == LN3D_EPI_GATE_RES) {
      g0 = g1 = make_float4(1.f, 1.f, 1.f, 1.f);
      r0 = r1 = make_float4(0.f, 0.f, 0.f, 0.f);
      grows_left = 1 << 30;
      if (p.gate || p.rb) {
        generic = p.gate_rows < 32;
        const int s0 = tb / p.gate_rows;
        grows_left = p.gate_rows - (tb - s0 * p.gate_rows);
        const bool two = grows_left < 32 && tb + grows_left < p.M;
        if (p.gate) {
          g0 = *reinterpret_cast<const float4*>(p.gate + (int64_t)s0 * p.gate_ld + fb);
          if (two) g1 = *reinterpret_cast<const float4*>(p.gate + (int64_t)(s0 + 1) * p.gate_ld + fb);
        }
        if (p.rb) {
          r0 = *reinterpret_cast<const float4*>(p.rb + (int64_t)s0 * p.rb_ld + fb);
          if (two) r1 = *reinterpret_cast<const float4*>(p.rb + (int64_t)(s0 + 1) * p.rb_ld + fb);
        }
      }
    }
  }
  // GATE_RES with the residual quad already in registers (staged_epilogue prefetches the 8 rows of a block in one batch)
  __device__ __forceinline__ void apply_res(const GemmP& p, int tb, int row, int fb, float4 v, float4 x) const {
    const float4 g = row >= grows_left ? g1 : g0;
    const float4 r = row >= grows_left ? r1 : r0;
    x.x += (v.x + bias.x) * g.x + r.x; x.y += (v.y + bias.y) * g.y + r.y; x.z += (v.z + bias.z) * g.z + r.z; x.w += (v.w + bias.w) * g.w + r.w;
    *reinterpret_cast<float4*>((float*)p.out0 + (int64_t)(tb + row) * p.ldo + fb) = x;
    if (p.out1) {
      uint2 o; o.x = pack2bf(x.x, x.y); o.y = pack2bf(x.z, x.w);
      *reinterpret_cast<uint2*>((bf16_t*)p.out1 + (int64_t)(tb + row) * p.ldo + fb) = o;
    }
  }
  __device__ __forceinline__ void apply(const GemmP& p, int tb, int row, int fb, float4 v) const {
    if constexpr (EPI == LN3D_EPI_HEADS) {
      if (generic) { epilogue4<EPI>(p, tb + row, fb, v.x, v.y, v.z, v.w); return; }
      uint2 o; o.x = pack2bf(v.x + bias.x, v.y + bias.y); o.y = pack2bf(v.z + bias.z, v.w + bias.w);
      *reinterpret_cast<uint2*>(hbase + (int64_t)row * hstride + (row >= hrows_left ? hwrap : 0)) = o;
    } else if constexpr (EPI == LN3D_EPI_GATE_RES) {
      if (generic) { epilogue4<EPI>(p, tb + row, fb, v.x, v.y, v.z, v.w); return; }
      const float4 g = row >= grows_left ? g1 : g0;
      const float4 r = row >= grows_left ? r1 : r0;
      float4* xp = reinterpret_cast<float4*>((float*)p.out0 + (int64_t)(tb + row) * p.ldo + fb);
      float4 x = *xp;
      x.x += (v.x + bias.x) * g.x + r.x; x.y += (v.y + bias.y) * g.y + r.y; x.z += (v.z + bias.z) * g.z + r.z; x.w += (v.w + bias.w) * g.w + r.w;
      *xp = x;
      if (p.out1) {
        uint2 o; o.x = pack2bf(x.x, x.y); o.y = pack2bf(x.z, x.w);
        *reinterpret_cast<uint2*>((bf16_t*)p.out1 + (int64_t)(tb + row) * p.ldo + fb) = o;
      }
    } else if constexpr (EPI == LN3D_EPI_GELU_ERF || EPI == LN3D_EPI_GELU_TANH || EPI == LN3D_EPI_SILU || EPI == LN3D_EPI_QUICK_GELU) {
      uint2 o; o.x = pack2bf(v.x, v.y); o.y = pack2bf(v.z, v.w);     // bias + activation were applied before staging
      *reinterpret_cast<uint2*>((bf16_t*)p.out0 + (int64_t)(tb + row) * p.ldo + fb) = o;
    } else {
      float v0 = v.x + bias.x, v1 = v.y + bias.y, v2 = v.z + bias.z, v3 = v.w + bias.w;
      const int64_t off = (int64_t)(tb + row) * p.ldo + fb;
      if constexpr (EPI == LN3D_EPI_F32 || EPI == LN3D_EPI_F32_SILU)
        *reinterpret_cast<float4*>((float*)p.out0 + off) = make_float4(v0, v1, v2, v3);
      if constexpr (EPI == LN3D_EPI_GELU_ERF) { gelu_erf2(v0, v1); gelu_erf2(v2, v3); }
      if constexpr (EPI == LN3D_EPI_GELU_TANH) { v0 = gelu_tanh(v0); v1 = gelu_tanh(v1); v2 = gelu_tanh(v2); v3 = gelu_tanh(v3); }
      if constexpr (EPI == LN3D_EPI_SILU || EPI == LN3D_EPI_F32_SILU) { v0 = silu(v0); v1 = silu(v1); v2 = silu(v2); v3 = silu(v3); }
      if constexpr (EPI == LN3D_EPI_QUICK_GELU) { v0 = quick_gelu(v0); v1 = quick_gelu(v1); v2 = quick_gelu(v2); v3 = quick_gelu(v3); }
      if constexpr (EPI != LN3D_EPI_F32) {
        uint2 o; o.x = pack2bf(v0, v1); o.y = pack2bf(v2, v3);
        *reinterpret_cast<uint2*>((bf16_t*)(EPI == LN3D_EPI_F32_SILU ? p.out1 : p.out0) + off) = o;
      }
    }
  }
};

// `pre` / `pre_re`: GATE_RES interior tiles - the residual batch and the bias / gate rows of block 0, requested by the caller in
// front of the LAST K stage so that their L2 / fabric round trip runs under that stage's MFMAs (r5); null = fetched here.
template <int EPI, int NI, int NJ, bool DBUF = true, bool PRE = false>
__device__ __forceinline__ void staged_epilogue(const GemmP& p, f32x16 (&acc)[NI][NJ], char* stg, int fw0, int tw0, int lane,
                                                const float4 (&pre)[8], const RunEpi<EPI>& pre_re, bool have_pre) {
  constexpr bool kPreAct = EPI == LN3D_EPI_GELU_ERF || EPI == LN3D_EPI_GELU_TANH || EPI == LN3D_EPI_SILU || EPI == LN3D_EPI_QUICK_GELU;
  constexpr bool kBf16Out = kPreAct || EPI == LN3D_EPI_BF16 || EPI == LN3D_EPI_CROSS_ATTN;
  const bool wide = kBf16Out && (p.N & 7) == 0 && (p.ldo & 7) == 0;
  const int l31 = lane & 31, hi = lane >> 5;
  const int rrow = lane >> 4, rc = lane & 15;
  // GATE_RES: the fp32 residual rows of a 32-token block (8 quads per lane) are fetched as ONE batch, a block ahead of their
  // use when the register budget allows (DBUF).  r2 read each quad right before its own store: out0 is both loaded and stored,
  // so hipcc kept every load behind the previous row's store - 24 dependent round trips to L2 / the fabric per wave
  // (global_load, s_waitcnt vmcnt(0), global_store, ...), measured as +10 us on the attention-projection GEMM.
  constexpr int NBLK = (NI / 2) * NJ;
  float4 xres[2][DBUF ? 8 : 1];
  auto prefetch_res = [&](int blk, float4 (&xr)[DBUF ? 8 : 1]) __attribute__((always_inline)) {
    const int fb_ = fw0 + (blk / NJ) * 64 + 4 * rc;
    const int tb_ = tw0 + (blk % NJ) * 32;
#pragma unroll
    for (int it = 0; it < (DBUF ? 8 : 1); ++it) {
      const int row = 4 * it + rrow;
      xr[it] = (tb_ + row < p.M && fb_ < p.N) ? *reinterpret_cast<const float4*>((const float*)p.out0 + (int64_t)(tb_ + row) * p.ldo + fb_)
                                             : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  if constexpr (EPI == LN3D_EPI_GATE_RES && DBUF) {
   if constexpr (NI % 2 == 0) {
    // Interior tiles (every tile of the DiT shapes): branch-free, so that hipcc's counted vmcnt waits let block b+1's batch
    // stay in flight while block b is stored (behind exec-masked range checks it falls back to vmcnt(0) per block).
    const bool full = (tw0 + 32 * NJ <= p.M) && (fw0 + 32 * NI <= p.N) && !((p.gate || p.rb) && p.gate_rows < 32);
    if (__builtin_amdgcn_readfirstlane(full ? 1 : 0)) {
      auto fetch = [&](int blk, float4 (&xr)[8]) __attribute__((always_inline)) {
        const float* base = (const float*)p.out0 + (int64_t)(tw0 + (blk % NJ) * 32 + rrow) * p.ldo + fw0 + (blk / NJ) * 64 + 4 * rc;
#pragma unroll
        for (int it = 0; it < 8; ++it) xr[it] = *reinterpret_cast<const float4*>(base + (int64_t)(4 * it) * p.ldo);
      };
      constexpr bool TWO = NI * NJ <= 6;                 // 128 accumulators (256x256 tile) leave room for one batch only
      // bias / gate quads of a block are requested BEFORE its residual batch: whatever wait hipcc puts behind them (they
      // sit in conditionals) then covers only the previous batch, which the block being stored needs anyway
      auto blk_fb = [&](int blk) __attribute__((always_inline)) { return fw0 + (blk / NJ) * 64 + 4 * rc; };
      auto blk_tb = [&](int blk) __attribute__((always_inline)) { return __builtin_amdgcn_readfirstlane(tw0 + (blk % NJ) * 32); };
      RunEpi<EPI> re_cur, re_nxt;
      if (PRE && have_pre) {             // have_pre is wave-uniform and implied by `full` (same predicate at the call site)
        re_cur = pre_re;
#pragma unroll
        for (int it = 0; it < 8; ++it) xres[0][it] = pre[it];
      } else {
        re_cur.init(p, blk_fb(0), blk_tb(0), 0, 0, 0);
        fetch(0, xres[0]);
      }
#pragma unroll
      for (int blk = 0; blk < NBLK; ++blk) {
        const int ih = blk / NJ, j = blk % NJ;
        const int fb = blk_fb(blk);
        const int tb = blk_tb(blk);
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int c = ii * 8 + 2 * g + hi;
            *reinterpret_cast<float4*>(stg + l31 * 256 + ((c ^ (l31 & 15)) << 4)) =
                make_float4(acc[2 * ih + ii][j][4 * g + 0], acc[2 * ih + ii][j][4 * g + 1], acc[2 * ih + ii][j][4 * g + 2], acc[2 * ih + ii][j][4 * g + 3]);
          }
        if constexpr (TWO) {
          if (blk + 1 < NBLK) { re_nxt.init(p, blk_fb(blk + 1), blk_tb(blk + 1), 0, 0, 0); fetch(blk + 1, xres[(blk + 1) & 1]); }
        }
#pragma unroll
        for (int it = 0; it < 8; ++it) {
          const int row = 4 * it + rrow;
          const float4 v = *reinterpret_cast<const float4*>(stg + row * 256 + ((rc ^ (row & 15)) << 4));
          re_cur.apply_res(p, tb, row, fb, v, xres[TWO ? (blk & 1) : 0][it]);
        }
        if constexpr (TWO) re_cur = re_nxt;
        else if (blk + 1 < NBLK) { re_cur.init(p, blk_fb(blk + 1), blk_tb(blk + 1), 0, 0, 0); fetch(blk + 1, xres[0]); }
      }
      return;
    }
   }
    prefetch_res(0, xres[0]);
  }
#pragma unroll
  for (int ih = 0; ih < NI / 2; ++ih) {
    const int fb = fw0 + ih * 64 + 4 * rc;
    const bool fok = fb < p.N;
    RunEpi<EPI> re;
    int which = 0, h = 0, d = 0;
    if constexpr (EPI == LN3D_EPI_HEADS) { if (fok) re.init_feature(p, fb, which, h, d); }
    float4 wb0 = make_float4(0.f, 0.f, 0.f, 0.f), wb1 = wb0;
    if (wide && !kPreAct && p.bias) {
      const int f8 = fw0 + ih * 64 + 8 * (lane & 7);
      if (f8 < p.N) { wb0 = *reinterpret_cast<const float4*>(p.bias + f8); wb1 = *reinterpret_cast<const float4*>(p.bias + f8 + 4); }
    }
    float4 pre_bias[2][4];
    if constexpr (kPreAct) {
#pragma unroll
      for (int ii = 0; ii < 2; ++ii)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int fa = fw0 + ih * 64 + ii * 32 + 8 * g + 4 * hi;      // the accumulator quad's features
          pre_bias[ii][g] = (p.bias && fa < p.N) ? *reinterpret_cast<const float4*>(p.bias + fa) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int tb = __builtin_amdgcn_readfirstlane(tw0 + j * 32);
      if (fok && tb < p.M) re.init(p, fb, tb, which, h, d);
#pragma unroll
      for (int ii = 0; ii < 2; ++ii)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int c = ii * 8 + 2 * g + hi;
          float v0 = acc[2 * ih + ii][j][4 * g + 0], v1 = acc[2 * ih + ii][j][4 * g + 1], v2 = acc[2 * ih + ii][j][4 * g + 2],
                v3 = acc[2 * ih + ii][j][4 * g + 3];
          if constexpr (kPreAct) {
            // bias + activation here, on the accumulator quads (all independent: full ILP), not on the read-back side
            // where every lane walks a dependent chain per row
            const float4 b = pre_bias[ii][g];
            v0 += b.x; v1 += b.y; v2 += b.z; v3 += b.w;
            if constexpr (EPI == LN3D_EPI_GELU_ERF) { gelu_erf2(v0, v1); gelu_erf2(v2, v3); }
            if constexpr (EPI == LN3D_EPI_GELU_TANH) { v0 = gelu_tanh(v0); v1 = gelu_tanh(v1); v2 = gelu_tanh(v2); v3 = gelu_tanh(v3); }
            if constexpr (EPI == LN3D_EPI_SILU) { v0 = silu(v0); v1 = silu(v1); v2 = silu(v2); v3 = silu(v3); }
            if constexpr (EPI == LN3D_EPI_QUICK_GELU) { v0 = quick_gelu(v0); v1 = quick_gelu(v1); v2 = quick_gelu(v2); v3 = quick_gelu(v3); }
          }
          *reinterpret_cast<float4*>(stg + l31 * 256 + ((c ^ (l31 & 15)) << 4)) = make_float4(v0, v1, v2, v3);
        }
      if (wide) {
        // bf16 outputs: 8 features (two staged chunks) per lane -> 16-byte stores, 8 lanes per 128-byte row segment; the
        // 8-byte-per-lane form of the generic path costs ~15 % of a K = 1024 GEMM on this part
        const int r8 = lane >> 3, c8 = lane & 7;
        const int f8 = fw0 + ih * 64 + 8 * c8;
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          const int row = 8 * it + r8;
          float4 v0 = *reinterpret_cast<const float4*>(stg + row * 256 + (((2 * c8) ^ (row & 15)) << 4));
          float4 v1 = *reinterpret_cast<const float4*>(stg + row * 256 + (((2 * c8 + 1) ^ (row & 15)) << 4));
          if constexpr (!kPreAct) {
            v0.x += wb0.x; v0.y += wb0.y; v0.z += wb0.z; v0.w += wb0.w;
            v1.x += wb1.x; v1.y += wb1.y; v1.z += wb1.z; v1.w += wb1.w;
          }
          uint4 o;
          o.x = pack2bf(v0.x, v0.y); o.y = pack2bf(v0.z, v0.w); o.z = pack2bf(v1.x, v1.y); o.w = pack2bf(v1.z, v1.w);
          if (tb + row < p.M && f8 < p.N) {
            typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
            u32x4_t ov = {o.x, o.y, o.z, o.w};
            u32x4_t* dstp = reinterpret_cast<u32x4_t*>((bf16_t*)p.out0 + (int64_t)(tb + row) * p.ldo + f8);
            // plain store, NOT nontemporal: the next kernel reads these activations, and in the pipeline a streaming store
            // sends them past the 256 MB memory-side cache (same-box A/B of the whole bench line, r4: 2.62 -> 2.65 samples/s)
            *dstp = ov;
          }
        }
      } else if constexpr (EPI == LN3D_EPI_GATE_RES) {
        constexpr int DB = DBUF ? 1 : 0;
        const int blk = ih * NJ + j;                     // compile-time after unrolling
        if constexpr (DBUF) {
          if (blk + 1 < NBLK) prefetch_res(blk + 1, xres[(blk + 1) & DB]);
#pragma unroll
          for (int it = 0; it < 8; ++it) {
            const int row = 4 * it + rrow;
            const float4 v = *reinterpret_cast<const float4*>(stg + row * 256 + ((rc ^ (row & 15)) << 4));
            if (tb + row < p.M && fok) {
              if (re.generic) epilogue4<EPI>(p, tb + row, fb, v.x, v.y, v.z, v.w);
              else re.apply_res(p, tb, row, fb, v, xres[blk & DB][it]);
            }
          }
        } else {
          // 3 waves per SIMD (168 VGPRs): batches of 4 rows
#pragma unroll
          for (int hb = 0; hb < 2; ++hb) {
            float4 xr[4];
#pragma unroll
            for (int it = 0; it < 4; ++it) {
              const int row = 4 * (4 * hb + it) + rrow;
              xr[it] = (tb + row < p.M && fok) ? *reinterpret_cast<const float4*>((const float*)p.out0 + (int64_t)(tb + row) * p.ldo + fb)
                                               : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int it = 0; it < 4; ++it) {
              const int row = 4 * (4 * hb + it) + rrow;
              const float4 v = *reinterpret_cast<const float4*>(stg + row * 256 + ((rc ^ (row & 15)) << 4));
              if (tb + row < p.M && fok) {
                if (re.generic) epilogue4<EPI>(p, tb + row, fb, v.x, v.y, v.z, v.w);
                else re.apply_res(p, tb, row, fb, v, xr[it]);
              }
            }
          }
        }
      } else {
#pragma unroll
        for (int it = 0; it < 8; ++it) {
          const int row = 4 * it + rrow;
          const float4 v = *reinterpret_cast<const float4*>(stg + row * 256 + ((rc ^ (row & 15)) << 4));
          if (tb + row < p.M && fok) re.apply(p, tb, row, fb, v);
        }
      }
    }
  }
  if constexpr (NI % 2 == 1) {
    // last (odd) feature block alone: 32 tokens x 32 features, 128-byte staging rows, chunk c of row r at c ^ ((r >> 1) & 7);
    // 8 lanes come back with the 32 consecutive features of one token
    constexpr int i = NI - 1;
    const int r8 = lane >> 3, c8 = lane & 7;
    const int fb = fw0 + i * 32 + 4 * c8;
    const bool fok = fb < p.N;
    RunEpi<EPI> re;
    int which = 0, h = 0, d = 0;
    if constexpr (EPI == LN3D_EPI_HEADS) { if (fok) re.init_feature(p, fb, which, h, d); }
    float4 pre_bias[4];
    if constexpr (kPreAct) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int fa = fw0 + i * 32 + 8 * g + 4 * hi;
        pre_bias[g] = (p.bias && fa < p.N) ? *reinterpret_cast<const float4*>(p.bias + fa) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int tb = __builtin_amdgcn_readfirstlane(tw0 + j * 32);
      if (fok && tb < p.M) re.init(p, fb, tb, which, h, d);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c = 2 * g + hi;
        float v0 = acc[i][j][4 * g + 0], v1 = acc[i][j][4 * g + 1], v2 = acc[i][j][4 * g + 2], v3 = acc[i][j][4 * g + 3];
        if constexpr (kPreAct) {
          const float4 b = pre_bias[g];
          v0 += b.x; v1 += b.y; v2 += b.z; v3 += b.w;
          if constexpr (EPI == LN3D_EPI_GELU_ERF) { gelu_erf2(v0, v1); gelu_erf2(v2, v3); }
          if constexpr (EPI == LN3D_EPI_GELU_TANH) { v0 = gelu_tanh(v0); v1 = gelu_tanh(v1); v2 = gelu_tanh(v2); v3 = gelu_tanh(v3); }
          if constexpr (EPI == LN3D_EPI_SILU) { v0 = silu(v0); v1 = silu(v1); v2 = silu(v2); v3 = silu(v3); }
          if constexpr (EPI == LN3D_EPI_QUICK_GELU) { v0 = quick_gelu(v0); v1 = quick_gelu(v1); v2 = quick_gelu(v2); v3 = quick_gelu(v3); }
        }
        *reinterpret_cast<float4*>(stg + l31 * 128 + ((c ^ ((l31 >> 1) & 7)) << 4)) = make_float4(v0, v1, v2, v3);
      }
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int row = 8 * it + r8;
        const float4 v = *reinterpret_cast<const float4*>(stg + row * 128 + ((c8 ^ ((row >> 1) & 7)) << 4));
        if (tb + row < p.M && fok) re.apply(p, tb, row, fb, v);
      }
    }
  }
}
