// Kernel of the FFHQ VAE decoder class (include/ln3d_ffhq.h): the 3 x 3 roll-out group convolution of conv_sr as an implicit GEMM.
// (The class's other entry point, the roll-out means of bf16 planes, is an instantiation of shapenet_ops.hip's kernel and lives there.)
//
// The im2col + GEMM composition the ShapeNet class uses writes and re-reads a [H*W, 27*C] bf16 matrix per plane: 453 MB at C = 128,
// H = W = 256.  Here a workgroup owns TH x TW = 8 x 32 output pixels of one plane and stages what they read once in LDS, as bf16:
//   sx   [TH+2][TW+2][C]  the plane's pixels with a one-pixel halo, zero outside the image
//   srow [TH+2][C]        row means of plane (i+1) % 3 for the tile's rows (zero outside the image)
//   scol [TW+2][C]        column means of plane (i+2) % 3 for the tile's columns (zero outside the image)
// and walks the nine taps over them.  The GEMM per tap is [Cout x 3C] x [3C x pixels]: the filters are the MFMA A operand, read from
// global memory (every workgroup of a plane reads the same 27*C*Cout*2 bytes: they stay in L2), the activations the B operand, read
// from LDS.  The pooled parts are constant along a row (srow: all 32 pixels of a fragment read one LDS row, a broadcast) or along a
// column (scol); the other direction of their zero padding is a select on the fragment.
// LDS pixel stride is 2C + 16 bytes: the 32 lanes of a fragment read 16 B at consecutive pixels, and an odd number of 16-byte slots
// between them spreads a group of 8 lanes over all 32 banks.
#include "common.h"
#include "resize.h"
#include "../../include/ln3d.h"
#include "../../include/ln3d_ffhq.h"

namespace {
constexpr int TH = 8, TW = 32, HY = TH + 2, HX = TW + 2;
constexpr int ROWS_PER_WAVE = 2;                       // 4 waves x 2 rows of 32 pixels

struct ConvArgs {
  const void* x; int x_is_bf16;
  const float *rowmean, *colmean;
  const bf16_t* w;
  const float *bias, *base;
  int bh, bw;
  float* out;
  int H, W, C, Cout;
  float slope;
};

__device__ __forceinline__ uint4 pack8(const float* s) {
  const float4 a = *reinterpret_cast<const float4*>(s), b = *reinterpret_cast<const float4*>(s + 4);
  uint4 o;
  o.x = pack2bf(a.x, a.y); o.y = pack2bf(a.z, a.w); o.z = pack2bf(b.x, b.y); o.w = pack2bf(b.z, b.w);
  return o;
}

// CT: the channel count at compile time (the tap / part / K-step loops unroll completely), 0: any C % 16 == 0 at run time
template <int CT>
__global__ __launch_bounds__(256) void conv3x3_rollout_kernel(const ConvArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int C = CT ? CT : p.C;
  const int H = p.H, W = p.W, K = 27 * C;
  const int PS = 2 * C + 16;                           // bytes between pixels in LDS
  const int SROW = HY * HX * PS, SCOL = SROW + HY * PS;
  const int ncot = p.Cout / 32;
  const int plane = blockIdx.z / ncot, co0 = (blockIdx.z % ncot) * 32;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const int tid = threadIdx.x;
  const int C8 = C / 8;

  // ---- stage the tile (8 channels = 16 B of bf16 per step)
  for (int i = tid; i < HY * HX * C8; i += 256) {
    const int ch = i % C8, pix = i / C8, hx = pix % HX, hy = pix / HX;
    const int yy = y0 + hy - 1, xx = x0 + hx - 1;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
      const int64_t off = (((int64_t)plane * H + yy) * W + xx) * C + ch * 8;
      v = p.x_is_bf16 ? *reinterpret_cast<const uint4*>(static_cast<const bf16_t*>(p.x) + off) : pack8(static_cast<const float*>(p.x) + off);
    }
    *reinterpret_cast<uint4*>(lds + pix * PS + ch * 16) = v;
  }
  const int pr = (plane + 1) % 3, pc = (plane + 2) % 3;
  for (int i = tid; i < (HY + HX) * C8; i += 256) {
    const int ch = i % C8, j = i / C8;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (j < HY) {
      const int yy = y0 + j - 1;
      if (yy >= 0 && yy < H) v = pack8(p.rowmean + ((int64_t)pr * H + yy) * C + ch * 8);
      *reinterpret_cast<uint4*>(lds + SROW + j * PS + ch * 16) = v;
    } else {
      const int xx = x0 + (j - HY) - 1;
      if (xx >= 0 && xx < W) v = pack8(p.colmean + ((int64_t)pc * W + xx) * C + ch * 8);
      *reinterpret_cast<uint4*>(lds + SCOL + (j - HY) * PS + ch * 16) = v;
    }
  }
  __syncthreads();

  // ---- nine taps x three parts x C / 16 MFMA K steps
  const int lane = tid & 63, wv = tid >> 6, r = lane & 31, hf = lane >> 5;
  const bf16_t* wp = p.w + ((int64_t)plane * p.Cout + co0 + r) * K + 8 * hf;      // A: filter row r, k = 8 hf + j
  const unsigned char* lp = lds + 16 * hf;                                         // B: pixel r, k = 8 hf + j
  f32x16 acc[ROWS_PER_WAVE];
#pragma unroll
  for (int t = 0; t < ROWS_PER_WAVE; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int ky = tap / 3, kx = tap % 3;
    const uint32_t xmask = (unsigned)(x0 + r + kx - 1) < (unsigned)W ? ~0u : 0u;      // the padding a pooled vector does not carry
#pragma unroll
    for (int part = 0; part < 3; ++part) {
      const bf16_t* wk = wp + (tap * 3 + part) * C;
#pragma unroll CT ? CT / 16 : 1
      for (int kc = 0; kc < (CT ? CT / 16 : C / 16); ++kc) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(wk + kc * 16);
#pragma unroll
        for (int t = 0; t < ROWS_PER_WAVE; ++t) {
          const int ty = wv * ROWS_PER_WAVE + t;
          uint4 b;
          if (part == 0) {
            b = *reinterpret_cast<const uint4*>(lp + ((ty + ky) * HX + r + kx) * PS + kc * 32);
          } else if (part == 1) {
            b = *reinterpret_cast<const uint4*>(lp + SROW + (ty + ky) * PS + kc * 32);
            b.x &= xmask; b.y &= xmask; b.z &= xmask; b.w &= xmask;
          } else {
            b = *reinterpret_cast<const uint4*>(lp + SCOL + (r + kx) * PS + kc * 32);
            const uint32_t ymask = (unsigned)(y0 + ty + ky - 1) < (unsigned)H ? ~0u : 0u;
            b.x &= ymask; b.y &= ymask; b.z &= ymask; b.w &= ymask;
          }
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, b), acc[t], 0, 0, 0);
        }
      }
    }
  }

  // ---- epilogue: lane holds pixel r and, in registers 4g .. 4g + 3, filters 8g + 4 hf + (0 .. 3)
  const bool same = p.bh == H && p.bw == W;
  const int x = x0 + r;
#pragma unroll
  for (int t = 0; t < ROWS_PER_WAVE; ++t) {
    const int y = y0 + wv * ROWS_PER_WAVE + t;
    if (y >= H || x >= W) continue;
    const int64_t o = (((int64_t)plane * H + y) * W + x) * p.Cout;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int co = co0 + 8 * g + 4 * hf;
      const float4 bi = *reinterpret_cast<const float4*>(p.bias + plane * p.Cout + co);
      const float4 bs = same ? *reinterpret_cast<const float4*>(p.base + o + co) : bilin4(p.base, plane, p.bh, p.bw, H, W, y, x, p.Cout, co);
      float4 v = make_float4(acc[t][4 * g] + bi.x, acc[t][4 * g + 1] + bi.y, acc[t][4 * g + 2] + bi.z, acc[t][4 * g + 3] + bi.w);
      v.x = bs.x + (v.x >= 0.f ? v.x : v.x * p.slope);
      v.y = bs.y + (v.y >= 0.f ? v.y : v.y * p.slope);
      v.z = bs.z + (v.z >= 0.f ? v.z : v.z * p.slope);
      v.w = bs.w + (v.w >= 0.f ? v.w : v.w * p.slope);
      *reinterpret_cast<float4*>(p.out + o + co) = v;
    }
  }
}

template <int CT>
int launch(const ConvArgs& p, hipStream_t s) {
  const int LDS = (HY * HX + HY + HX) * (2 * p.C + 16);
  static AttrOnce attr_once;
  if (attr_once.need())
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_rollout_kernel<CT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (HY * HX + HY + HX) * (2 * 128 + 16));
  hipLaunchKernelGGL(conv3x3_rollout_kernel<CT>, dim3((p.W + TW - 1) / TW, (p.H + TH - 1) / TH, 3 * (p.Cout / 32)), dim3(256), LDS, s, p);
  return ln3d_check_launch();
}
}  // namespace

extern "C" int ln3d_conv3x3_rollout_bf16(const void* x, int x_is_bf16, const float* rowmean, const float* colmean, const void* w,
                                         const float* bias, const float* base, int bh, int bw, float* out, int H, int W, int C, int Cout,
                                         float slope, void* stream) {
  if (!x || !rowmean || !colmean || !w || !bias || !base || !out || H <= 0 || W <= 0 || bh <= 0 || bw <= 0) return LN3D_ERR_BAD_ARG;
  if (C < 16 || C > 128 || C % 16 || Cout <= 0 || Cout % 32 || (H + TH - 1) / TH > 65535 || 3 * (Cout / 32) > 65535) return LN3D_ERR_BAD_ARG;
  if (static_cast<const void*>(out) == x) return LN3D_ERR_BAD_ARG;
  const ConvArgs p{x, x_is_bf16, rowmean, colmean, static_cast<const bf16_t*>(w), bias, base, bh, bw, out, H, W, C, Cout, slope};
  hipStream_t s = (hipStream_t)stream;
  if (C == 128) return launch<128>(p, s);
  if (C == 32) return launch<32>(p, s);
  return launch<0>(p, s);
}
