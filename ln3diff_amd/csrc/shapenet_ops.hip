// Kernels of the ShapeNet VAE decoder class (include/ln3d_shapenet.h): the cross-plane attention of its paired ViT blocks and the
// layout / resize / roll-out pieces of its super-resolution convs, with the roll-out row / column means of both plane types (f32
// here, bf16 for the FFHQ class).  The convolutions themselves run on the MFMA GEMM (gemm_bf16.hip); these kernels are memory-bound
// gathers and small reductions.
#include "common.h"
#include "resize.h"
#include "../../include/ln3d.h"
#include "../../include/ln3d_shapenet.h"
#include "../../include/ln3d_ffhq.h"

// ------------------------------------------------------------------ cross-plane attention (2p keys per query, Dh 64)
// One wavefront per (query token, head): lane j < 2p scores key j, the softmax is two wave reductions, lane d sums the value column d.
__global__ __launch_bounds__(64) void axis_attention_kernel(const float* qkv, int64_t ld, bf16_t* out, int p, int H, float scale) {
  const int lane = threadIdx.x;
  const int h = blockIdx.x % H;                      // grid: row * H + h, heads fastest
  const int64_t row = blockIdx.x / H;                // (b*3 + i)*N + y*p + x
  const int N = p * p, D = H * 64;
  const int64_t bi = row / N;
  const int n = (int)(row - bi * N);
  const int64_t b = bi / 3;
  const int i = (int)(bi - b * 3);
  const int y = n / p, x = n % p;
  __shared__ float q[64];
  __shared__ float prob[64];
  q[lane] = qkv[row * ld + h * 64 + lane];
  __syncthreads();
  auto key_row = [&](int j) -> int64_t {             // token row of key j
    if (j < p) return (b * 3 + (i + 1) % 3) * N + y * p + j;
    return (b * 3 + (i + 2) % 3) * N + (j - p) * p + x;
  };
  float s = -INFINITY;
  if (lane < 2 * p) {
    const float* k = qkv + key_row(lane) * ld + D + h * 64;
    float acc = 0.f;
    for (int d = 0; d < 64; ++d) acc += q[d] * k[d];
    s = acc * scale;
  }
  const float m = wave_max(s);
  const float e = lane < 2 * p ? expf(s - m) : 0.f;
  const float sum = wave_sum(e);
  prob[lane] = e / sum;
  __syncthreads();
  float o = 0.f;
  for (int j = 0; j < 2 * p; ++j) o += prob[j] * qkv[key_row(j) * ld + 2 * D + h * 64 + lane];
  out[row * D + h * 64 + lane] = f2bf(o);
}
extern "C" int ln3d_triplane_axis_attention(const float* qkv, int64_t ld, void* out, int B, int p, int H, float scale, void* stream) {
  if (!qkv || !out || B <= 0 || p < 1 || p > 32 || H <= 0 || ld < 3 * 64 * (int64_t)H) return LN3D_ERR_BAD_ARG;
  const int64_t rows = (int64_t)B * 3 * p * p;
  // one block per (row, head) on gridDim.x (up to 2^31 - 1): with the rows on gridDim.y (limit 65536) B * 3 * p * p passed the limit
  // from B = 22 at p = 32
  if (rows * H > 0x7fffffff) return LN3D_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(axis_attention_kernel, dim3((unsigned)(rows * H)), dim3(64), 0, (hipStream_t)stream, qkv, ld, (bf16_t*)out, p, H, scale);
  return ln3d_check_launch();
}

// ------------------------------------------------------------------ decoder_pred output -> low-resolution planes + short_cut input
// one thread per 4 channels of one (b, d, Y, X) pixel, in the output order of `planes`
__global__ void sr_unpatchify_kernel(const float* pred, float* planes, bf16_t* mixed, int S, int P, int C, int64_t total4) {
  const int64_t i4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i4 >= total4) return;
  const int64_t i = i4 * 4;
  const int R = S * P;
  const int c = (int)(i % C);
  const int64_t pix = i / C;                          // ((b*3 + d)*R + Y)*R + X
  const int X = (int)(pix % R), Y = (int)((pix / R) % R);
  const int64_t bd = pix / ((int64_t)R * R);
  const int d = (int)(bd % 3);
  const int64_t b = bd / 3;
  auto src = [&](int dd, int cc) -> float {
    const int64_t tok = b * 3 * S * S + (int64_t)dd * S * S + (Y / P) * S + X / P;
    return pred[tok * (int64_t)P * P * C + ((Y % P) * P + X % P) * C + cc];
  };
  const float4 v = *reinterpret_cast<const float4*>(&pred[(b * 3 * S * S + (int64_t)d * S * S + (Y / P) * S + X / P) * (int64_t)P * P * C +
                                                          ((Y % P) * P + X % P) * C + c]);
  *reinterpret_cast<float4*>(planes + i) = v;
  // mixed[b, e = d, Y, X, k = c..c+3] = planes[b, (3k+e) / C, Y, X, (3k+e) % C]
  bf16_t m[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int f = 3 * (c + u) + d;
    m[u] = f2bf(src(f / C, f % C));
  }
  uint2 w;
  w.x = (uint32_t)m[0] | ((uint32_t)m[1] << 16);
  w.y = (uint32_t)m[2] | ((uint32_t)m[3] << 16);
  *reinterpret_cast<uint2*>(mixed + i) = w;
}
extern "C" int ln3d_sr_unpatchify(const float* pred, float* planes, void* mixed, int B, int S, int P, int C, void* stream) {
  if (!pred || !planes || !mixed || B <= 0 || S <= 0 || P <= 0 || C <= 0 || C % 4) return LN3D_ERR_BAD_ARG;
  const int64_t total4 = (int64_t)B * 3 * S * P * S * P * C / 4;
  hipLaunchKernelGGL(sr_unpatchify_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pred, planes,
                     (bf16_t*)mixed, S, P, C, total4);
  return ln3d_check_launch();
}

// ------------------------------------------------------------------ bilinear resize (align_corners False), channel-last (resize.h)
__global__ void resize_bilinear_cl_kernel(const float* x, bf16_t* y, int h, int w, int Ho, int Wo, int C, int transpose, int64_t total4) {
  const int64_t i4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i4 >= total4) return;
  const int64_t i = i4 * 4;
  const int c = (int)(i % C);
  const int64_t pix = i / C;
  const int X = (int)(pix % Wo), Y = (int)((pix / Wo) % Ho);
  const int64_t n = pix / ((int64_t)Wo * Ho);
  const float4 r = transpose ? bilin4(x, n, h, w, Ho, Wo, X, Y, C, c) : bilin4(x, n, h, w, Ho, Wo, Y, X, C, c);
  uint2 o;
  o.x = pack2bf(r.x, r.y);
  o.y = pack2bf(r.z, r.w);
  *reinterpret_cast<uint2*>(y + i) = o;
}
extern "C" int ln3d_resize_bilinear_cl(const float* x, void* y, int N, int h, int w, int Ho, int Wo, int C, int transpose, void* stream) {
  if (!x || !y || N <= 0 || h <= 0 || w <= 0 || Ho <= 0 || Wo <= 0 || C <= 0 || C % 4) return LN3D_ERR_BAD_ARG;
  if (transpose && (Ho != Wo || h != w)) return LN3D_ERR_BAD_ARG;
  const int64_t total4 = (int64_t)N * Ho * Wo * C / 4;
  hipLaunchKernelGGL(resize_bilinear_cl_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, (bf16_t*)y, h,
                     w, Ho, Wo, C, transpose, total4);
  return ln3d_check_launch();
}

__global__ void resize_add_lrelu_kernel(const float* base, const float* t, float* out, int h, int w, int Ho, int Wo, int C, float slope,
                                        int64_t total4) {
  const int64_t i4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i4 >= total4) return;
  const int64_t i = i4 * 4;
  const int c = (int)(i % C);
  const int64_t pix = i / C;
  const int X = (int)(pix % Wo), Y = (int)((pix / Wo) % Ho);
  const int64_t n = pix / ((int64_t)Wo * Ho);
  const float4 r = (h == Ho && w == Wo) ? *reinterpret_cast<const float4*>(base + i) : bilin4(base, n, h, w, Ho, Wo, Y, X, C, c);
  const float4 v = *reinterpret_cast<const float4*>(t + i);
  float4 o;
  o.x = r.x + (v.x >= 0.f ? v.x : v.x * slope);
  o.y = r.y + (v.y >= 0.f ? v.y : v.y * slope);
  o.z = r.z + (v.z >= 0.f ? v.z : v.z * slope);
  o.w = r.w + (v.w >= 0.f ? v.w : v.w * slope);
  *reinterpret_cast<float4*>(out + i) = o;
}
extern "C" int ln3d_resize_add_lrelu(const float* base, const float* t, float* out, int N, int h, int w, int Ho, int Wo, int C, float slope,
                                     void* stream) {
  if (!base || !t || !out || N <= 0 || h <= 0 || w <= 0 || Ho <= 0 || Wo <= 0 || C <= 0 || C % 4) return LN3D_ERR_BAD_ARG;
  const int64_t total4 = (int64_t)N * Ho * Wo * C / 4;
  hipLaunchKernelGGL(resize_add_lrelu_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, base, t, out, h, w,
                     Ho, Wo, C, slope, total4);
  return ln3d_check_launch();
}

// ------------------------------------------------------------------ roll-out: row / column means
// grid (H + W, N): blocks y < H reduce row y over x, blocks y >= H column y - H over the rows; thread = channel (strided by the block size)
// T = float (the ShapeNet class's f32 planes) or bf16_t (include/ln3d_ffhq.h: conv3D_0 pools the up-sampled planes, which only exist
// as the bf16 GEMM operand); BLOCK = threads per block, each entry point's own
__device__ __forceinline__ float rollout_elem(const float* p) { return *p; }
__device__ __forceinline__ float rollout_elem(const bf16_t* p) { return bf2f(*p); }
template <typename T, int BLOCK>
__global__ __launch_bounds__(BLOCK) void rollout_means_kernel(const T* x, float* rowmean, float* colmean, int H, int W, int C) {
  const int n = blockIdx.y;
  const int r = blockIdx.x;
  const T* xn = x + (int64_t)n * H * W * C;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float s = 0.f;
    if (r < H) {
      for (int xx = 0; xx < W; ++xx) s += rollout_elem(xn + ((int64_t)r * W + xx) * C + c);
      rowmean[((int64_t)n * H + r) * C + c] = s / (float)W;
    } else {
      const int xc = r - H;
      for (int yy = 0; yy < H; ++yy) s += rollout_elem(xn + ((int64_t)yy * W + xc) * C + c);
      colmean[((int64_t)n * W + xc) * C + c] = s / (float)H;
    }
  }
}
template <typename T, int BLOCK>
static int rollout_means(const void* x, float* rowmean, float* colmean, int N, int H, int W, int C, void* stream) {
  if (!x || !rowmean || !colmean || N <= 0 || N > 65535 || H <= 0 || W <= 0 || C <= 0) return LN3D_ERR_BAD_ARG;     // N: the grid's y extent
  hipLaunchKernelGGL((rollout_means_kernel<T, BLOCK>), dim3(H + W, N), dim3(BLOCK), 0, (hipStream_t)stream, static_cast<const T*>(x), rowmean,
                     colmean, H, W, C);
  return ln3d_check_launch();
}
extern "C" int ln3d_rollout_means(const float* x, float* rowmean, float* colmean, int N, int H, int W, int C, void* stream) {
  return rollout_means<float, 256>(x, rowmean, colmean, N, H, W, C, stream);
}
extern "C" int ln3d_rollout_means_bf16(const void* x, float* rowmean, float* colmean, int N, int H, int W, int C, void* stream) {
  return rollout_means<bf16_t, 128>(x, rowmean, colmean, N, H, W, C, stream);
}

// ------------------------------------------------------------------ roll-out: the gathered im2col
// one thread per 4 columns of one output row
__global__ void im2col3x3_rollout_kernel(const float* x, const float* rowmean, const float* colmean, bf16_t* col, int plane, int H, int W,
                                         int C, int Kpad, int64_t total4) {
  const int64_t i4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i4 >= total4) return;
  const int k4 = Kpad / 4;
  const int64_t row = i4 / k4;
  const int kk = (int)(i4 % k4) * 4;
  const int px = (int)(row % W), py = (int)(row / W);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  const int C3 = 3 * C;
  if (kk < 9 * C3) {
    const int tap = kk / C3, k = kk % C3, ky = tap / 3, kx = tap % 3;
    const int yy = py + ky - 1, xx = px + kx - 1;
    if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
      const float* s;
      if (k < C) s = x + (((int64_t)plane * H + yy) * W + xx) * C + k;
      else if (k < 2 * C) s = rowmean + ((int64_t)((plane + 1) % 3) * H + yy) * C + (k - C);
      else s = colmean + ((int64_t)((plane + 2) % 3) * W + xx) * C + (k - 2 * C);
      v = *reinterpret_cast<const float4*>(s);
    }
  }
  uint2 o;
  o.x = pack2bf(v.x, v.y);
  o.y = pack2bf(v.z, v.w);
  *reinterpret_cast<uint2*>(col + row * Kpad + kk) = o;
}
extern "C" int ln3d_im2col3x3_rollout(const float* x, const float* rowmean, const float* colmean, void* col, int plane, int H, int W, int C,
                                      int Kpad, void* stream) {
  if (!x || !rowmean || !colmean || !col || plane < 0 || plane > 2 || H <= 0 || W <= 0 || C <= 0 || C % 4 || Kpad % 4 || Kpad < 27 * C)
    return LN3D_ERR_BAD_ARG;
  const int64_t total4 = (int64_t)H * W * (Kpad / 4);
  hipLaunchKernelGGL(im2col3x3_rollout_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, rowmean, colmean,
                     (bf16_t*)col, plane, H, W, C, Kpad, total4);
  return ln3d_check_launch();
}
