// Channel-last helpers for the conv decoder of the tri-plane VAE (ldm Decoder): GroupNorm(+swish), layout conversion, and the one
// im2col kernel for every 3x3 conv of a bf16 channel-last image: pad 1 with an optional nearest-2x upsample (this decoder), pad 1
// with a stride (the U-Net's Downsample) and pad (0,1,0,1) stride 2 (the multi-view encoder's Downsample).  For the encoder
// (include/ln3d_encoder.h) also frame pooling and the fused posterior.
// The convolutions themselves run on the MFMA GEMM (gemm_bf16.hip) with fused bias / residual epilogues.
#include "common.h"
#include "../../include/ln3d.h"
#include "../../include/ln3d_encoder.h"

// ------------------------------------------------------------------ GroupNorm (+swish) on f32 [N, HW, C] -> bf16
// Statistics from centred quantities: every chunk sums x - pivot (the group's first element in the chunk) and stores (mean, M2); the
// chunks are merged in order with Chan's formula.  E[x^2] - mean^2 in fp32 (before) lost the variance when |mean| >> std: ~3e-3 of it
// at |mean| / std = 100, 20-30 % at 1000 (gn_any_kernel had the same flaw, fixed in r6 with two passes; here x is still read once).
__global__ __launch_bounds__(256) void gn_stats_kernel(const float* x, float* stats, int HW, int C, int groups, int pix_per_block) {
  // grid (chunks, N); thread t -> channel t % C, pixel phase t / C
  const int n = blockIdx.y;
  const int c = threadIdx.x % C, ph = threadIdx.x / C, nph = 256 / C;
  const int cpg = C / groups;
  const int p0 = blockIdx.x * pix_per_block;
  const int p1 = min(p0 + pix_per_block, HW);
  const float* xc = x + ((int64_t)n * HW + p0) * C;            // pixel p0 of sample n (p0 < HW: chunks = ceil(HW / pix_per_block))
  const float pivot = xc[(c / cpg) * cpg];
  float s = 0.f, q = 0.f;
  if (ph < nph)
    for (int p = p0 + ph; p < p1; p += nph) {
      const float d = x[((int64_t)n * HW + p) * C + c] - pivot;
      s += d; q += d * d;
    }
  __shared__ float sh[2][256];
  sh[0][threadIdx.x] = s; sh[1][threadIdx.x] = q;
  __syncthreads();
  if (threadIdx.x < groups) {
    float ts = 0.f, tq = 0.f;
    for (int pp = 0; pp < nph; ++pp)
      for (int cc = 0; cc < cpg; ++cc) {
        ts += sh[0][pp * C + threadIdx.x * cpg + cc];
        tq += sh[1][pp * C + threadIdx.x * cpg + cc];
      }
    const float dm = ts / (float)((p1 - p0) * cpg);
    // per-chunk (mean, M2); gn_reduce_kernel merges them in chunk order (fp32 atomics here made the planes differ from run to run)
    float* part = stats + 2 * (int64_t)gridDim.y * groups + (((int64_t)n * gridDim.x + blockIdx.x) * groups + threadIdx.x) * 2;
    part[0] = xc[threadIdx.x * cpg] + dm;
    part[1] = fmaxf(tq - ts * dm, 0.f);
  }
}

// Chan et al.'s pairwise update, chunk by chunk; the count of chunk k is min(ppb, HW - k * ppb) * cpg.  -> stats[2 i] = mean,
// stats[2 i + 1] = biased variance of (sample, group) i
__global__ void gn_reduce_kernel(float* stats, int N, int groups, int chunks, int HW, int cpg, int ppb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;          // (n, group)
  if (i >= N * groups) return;
  const int n = i / groups, g = i % groups;
  const float* part = stats + 2 * (int64_t)N * groups + ((int64_t)n * chunks * groups + g) * 2;
  float na = 0.f, mean = 0.f, m2 = 0.f;
  for (int c = 0; c < chunks; ++c) {
    const float nb = (float)(min(ppb, HW - c * ppb) * cpg), nab = na + nb;
    const float delta = part[(int64_t)c * groups * 2] - mean;
    mean += delta * (nb / nab);
    m2 += part[(int64_t)c * groups * 2 + 1] + delta * delta * (na * (nb / nab));
    na = nab;
  }
  stats[2 * i] = mean; stats[2 * i + 1] = m2 / na;
}

__global__ void gn_apply_kernel(const float* x, const float* stats, const float* w, const float* b, bf16_t* y, int64_t total4,
                                int HW, int C, int groups, float eps, int swish) {
  const int64_t i4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i4 >= total4) return;
  const int64_t i = i4 * 4;
  const int c = (int)(i % C);
  const int64_t n = i / ((int64_t)HW * C);
  const int cpg = C / groups;
  const float4 v = *reinterpret_cast<const float4*>(x + i);
  float in[4] = {v.x, v.y, v.z, v.w}, out[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int g = (c + k) / cpg;
    const float mean = stats[(n * groups + g) * 2];
    const float var = stats[(n * groups + g) * 2 + 1];
    float t = (in[k] - mean) * rsqrtf(var + eps) * w[c + k] + b[c + k];
    if (swish) t = t / (1.0f + __expf(-t));
    out[k] = t;
  }
  uint2 o; o.x = pack2bf(out[0], out[1]); o.y = pack2bf(out[2], out[3]);
  *reinterpret_cast<uint2*>(y + i) = o;
}

extern "C" int ln3d_groupnorm_swish(const float* x, const float* w, const float* b, void* y, float* stats_scratch, int N, int HW,
                                    int C, int groups, float eps, int swish, void* stream) {
  if (!x || !w || !b || !y || !stats_scratch || N <= 0 || HW <= 0 || C <= 0 || groups <= 0) return LN3D_ERR_BAD_ARG;
  if (C % groups || 256 % C || C % 4) return LN3D_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int ppb = LN3D_GN_PIXELS_PER_CHUNK;
  const int chunks = (HW + ppb - 1) / ppb;
  hipLaunchKernelGGL(gn_stats_kernel, dim3(chunks, N), dim3(256), 0, s, x, stats_scratch, HW, C, groups, ppb);
  hipLaunchKernelGGL(gn_reduce_kernel, dim3((N * groups + 255) / 256), dim3(256), 0, s, stats_scratch, N, groups, chunks, HW, C / groups, ppb);
  const int64_t total4 = (int64_t)N * HW * C / 4;
  hipLaunchKernelGGL(gn_apply_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, s, x, stats_scratch, w, b, (bf16_t*)y, total4, HW,
                     C, groups, eps, swish);
  return ln3d_check_launch();
}

// ------------------------------------------------------------------ im2col 3x3 (channel-last bf16): one kernel, three fronts
// col[(n*Ho*Wo + oy*Wo + ox), (ky*3+kx)*C + c] = x[n, (oy*STRIDE+ky-PAD)/UP, (ox*STRIDE+kx-PAD)/UP, c] where that position lies inside the
// nearest-upsampled H*UP x W*UP image, 0 outside (PAD rows / columns in front, one behind); zero pad to Kpad.  (UP, STRIDE, PAD) are
// compile-time: the plain kernel before this one divided by a run-time `up` and the strided one multiplied by a run-time `stride`, and
// neither should pay for the other's parameter.
template <int UP, int STRIDE, int PAD>
__global__ void im2col3x3_kernel(const bf16_t* x, bf16_t* col, int H, int W, int C, int Ho, int Wo, int Kpad, int64_t total8) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // one 16-B (8 x bf16) piece
  if (i >= total8) return;
  const int k8 = Kpad / 8;
  const int64_t row = i / k8;
  const int kk = (int)(i % k8) * 8;
  const int ox = (int)(row % Wo), oy = (int)((row / Wo) % Ho);
  const int64_t n = row / ((int64_t)Wo * Ho);
  uint4 v = make_uint4(0, 0, 0, 0);
  if (kk < 9 * C) {
    const int tap = kk / C, c = kk % C, ky = tap / 3, kx = tap % 3;
    const int yy = oy * STRIDE + ky - PAD, xx = ox * STRIDE + kx - PAD;
    if (yy >= 0 && yy < H * UP && xx >= 0 && xx < W * UP)
      v = *reinterpret_cast<const uint4*>(x + (((int64_t)n * H + yy / UP) * W + xx / UP) * C + c);
  }
  *reinterpret_cast<uint4*>(col + row * Kpad + kk) = v;
}
// every front names its instantiation, so the combinations that exist are the four below and no other
template <int UP, int STRIDE, int PAD>
static int im2col3x3_launch(const void* x, void* col, int N, int H, int W, int C, int Kpad, void* stream) {
  if (!x || !col || N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 || Kpad % 8 || Kpad < 9 * C) return LN3D_ERR_BAD_ARG;
  const int64_t Ho = ((int64_t)H * UP + PAD + 1 - 3) / STRIDE + 1, Wo = ((int64_t)W * UP + PAD + 1 - 3) / STRIDE + 1;
  if (Ho > 0x7fffffff || Wo > 0x7fffffff) return LN3D_ERR_BAD_ARG;      // the kernel's H * UP, Ho and Wo are ints
  const int64_t total8 = (int64_t)N * Ho * Wo * (Kpad / 8);
  hipLaunchKernelGGL((im2col3x3_kernel<UP, STRIDE, PAD>), dim3((unsigned)((total8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)x, (bf16_t*)col, H, W, C, (int)Ho, (int)Wo, Kpad, total8);
  return ln3d_check_launch();
}
// pad 1, optional nearest-2x upsample in front (the VAE decoder's Upsample): Ho = H * up
extern "C" int ln3d_im2col3x3(const void* x, void* col, int N, int H, int W, int C, int upsample, int Kpad, void* stream) {
  if (upsample == 1) return im2col3x3_launch<1, 1, 1>(x, col, N, H, W, C, Kpad, stream);
  if (upsample == 2) return im2col3x3_launch<2, 1, 1>(x, col, N, H, W, C, Kpad, stream);
  return LN3D_ERR_BAD_ARG;
}
// pad 1 with a stride (the U-Net's Downsample.op, unet.py:150-153): Ho = (H - 1) / stride + 1
extern "C" int ln3d_im2col3x3_strided(const void* x, void* col, int N, int H, int W, int C, int stride, int Kpad, void* stream) {
  if (stride == 1) return im2col3x3_launch<1, 1, 1>(x, col, N, H, W, C, Kpad, stream);
  if (stride == 2) return im2col3x3_launch<1, 2, 1>(x, col, N, H, W, C, Kpad, stream);
  return LN3D_ERR_BAD_ARG;
}
// the encoder's Downsample: F.pad(x, (0,1,0,1)) + 3x3 conv, stride 2, padding 0: Ho = (H - 2) / 2 + 1
extern "C" int ln3d_im2col3x3_pad01(const void* x, void* col, int N, int H, int W, int C, int Kpad, void* stream) {
  if (H < 2 || W < 2) return LN3D_ERR_BAD_ARG;
  return im2col3x3_launch<1, 2, 0>(x, col, N, H, W, C, Kpad, stream);
}

// ------------------------------------------------------------------ [NP, 3, H, W, C] f32 channel-last -> [NP, 3*C, H, W] (reference layout)
__global__ void cl_to_nchw_kernel(const float* src, float* dst, int C, int HW) {
  __shared__ float tile[32][33];
  const int pn = blockIdx.y;
  const int hw0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int hw = hw0 + r;
    tile[r][tx] = (hw < HW && tx < C) ? src[((int64_t)pn * HW + hw) * C + tx] : 0.f;
  }
  __syncthreads();
  for (int c = ty; c < C; c += 8) {
    const int hw = hw0 + tx;
    if (hw < HW) dst[((int64_t)pn * C + c) * HW + hw] = tile[tx][c];
  }
}
extern "C" int ln3d_planes_to_nchw(const float* src, float* dst, int NP, int C, int H, int W, void* stream) {
  if (!src || !dst || NP <= 0 || H <= 0 || W <= 0 || C != 32) return LN3D_ERR_BAD_ARG;
  const int HW = H * W;
  hipLaunchKernelGGL(cl_to_nchw_kernel, dim3((HW + 31) / 32, NP * 3), dim3(256), 0, (hipStream_t)stream, src, dst, C, HW);
  return ln3d_check_launch();
}

// ------------------------------------------------------------------ frame pooling: [B*F, HW, C] channel-last -> mean over F, NCHW [B, C, HW]
// frames summed in order, then / F (the arithmetic of ln3d_mv_posterior's own pooling, so both routes give the same bits)
__global__ void frame_mean_kernel(const float* h, float* out, int F, int HW, int C, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;       // over B * C * HW (output order)
  if (i >= total) return;
  const int p = (int)(i % HW);
  const int64_t bc = i / HW;
  const int64_t b = bc / C; const int c = (int)(bc - b * C);
  float s = 0.f;
  for (int f = 0; f < F; ++f) s += h[((b * F + f) * HW + p) * C + c];
  out[i] = s / (float)F;
}
extern "C" int ln3d_frame_mean(const float* h, float* out, int B, int F, int HW, int C, void* stream) {
  if (!h || !out || B <= 0 || F <= 0 || HW <= 0 || C <= 0) return LN3D_ERR_BAD_ARG;
  const int64_t total = (int64_t)B * C * HW;
  hipLaunchKernelGGL(frame_mean_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h, out, F, HW, C, total);
  return ln3d_check_launch();
}

// ------------------------------------------------------------------ fused multi-view posterior (include/ln3d_encoder.h)
// One thread per (object b, pixel p): the 6C = 24 pooled channels stay in registers, the grouped 1x1 quant_conv is 24 dot products
// of 8, then the 12 (c, n) pairs of the [B, 2C, 3, HW] view are written to every output.  Memory-bound and tiny (B * 1024 threads);
// exact tanhf / expf (not the fast intrinsics): logvar reaches the latent through exp and log_q through exp twice.
#define MVP_C 4
__global__ __launch_bounds__(256) void mv_posterior_kernel(const float* h, int64_t s_frame, int64_t s_pix, int64_t s_ch, const float* qw,
                                                          const float* qb, const float* eps, float* mean_o, float* logvar_o, float* z_o,
                                                          float* tok_o, float* logq_o, float* ent_o, int B, int F, int HW) {
  constexpr int CM = 6 * MVP_C, GI = 2 * MVP_C;                  // moments, channels per quant_conv group
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * HW) return;
  const int p = (int)(i % HW);
  const int64_t b = i / HW;
  float avg[CM];
#pragma unroll
  for (int k = 0; k < CM; ++k) avg[k] = 0.f;
  for (int f = 0; f < F; ++f) {
    const float* hp = h + (b * F + f) * s_frame + (int64_t)p * s_pix;
#pragma unroll
    for (int k = 0; k < CM; ++k) avg[k] += hp[k * s_ch];
  }
#pragma unroll
  for (int k = 0; k < CM; ++k) avg[k] = avg[k] / (float)F;
  auto moment = [&](int o) {
    const int g0 = (o / GI) * GI;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < GI; ++j) acc += qw[o * GI + j] * avg[g0 + j];
    return acc + qb[o];
  };
  const float half_log_2pi = 0.91893853320467274f;
#pragma unroll
  for (int c = 0; c < MVP_C; ++c)
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      const float mean = moment(c * 3 + n);
      const float logvar = tanhf(moment((MVP_C + c) * 3 + n) / 20.0f) * 20.0f;
      const float stdv = expf(0.5f * logvar), var = expf(logvar);
      const int64_t o = ((b * MVP_C + c) * 3 + n) * HW + p;        // [B, C, 3, HW]
      const float z = eps ? mean + stdv * eps[o] : mean;
      const float ns = (z - mean) / var;
      mean_o[o] = mean;
      logvar_o[o] = logvar;
      z_o[o] = z;
      logq_o[o] = -0.5f * ns * ns - half_log_2pi - logvar;
      ent_o[o] = logvar + (half_log_2pi + 0.5f);
      tok_o[(b * 3 * HW + (int64_t)n * HW + p) * MVP_C + c] = z;     // [B, 3*HW, C]
    }
}
extern "C" int ln3d_mv_posterior(const float* h, int64_t s_frame, int64_t s_pix, int64_t s_ch, const float* qw, const float* qb, const float* eps,
                                 float* mean, float* logvar, float* z, float* latent_tok, float* log_q, float* entropy, int B, int F, int HW, int C,
                                 void* stream) {
  if (!h || !qw || !qb || !mean || !logvar || !z || !latent_tok || !log_q || !entropy) return LN3D_ERR_BAD_ARG;
  if (B <= 0 || F <= 0 || HW <= 0 || C != MVP_C || s_frame < 0 || s_pix < 0 || s_ch < 0) return LN3D_ERR_BAD_ARG;
  const int64_t n = (int64_t)B * HW;
  hipLaunchKernelGGL(mv_posterior_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h, s_frame, s_pix, s_ch, qw, qb,
                     eps, mean, logvar, z, latent_tok, log_q, entropy, B, F, HW);
  return ln3d_check_launch();
}
