// Bilinear source taps shared by the resize kernels (shapenet_ops.hip) and the fused roll-out convolution's epilogue (ffhq_ops.hip).
#pragma once
#include "common.h"

// source coordinate of output index o along an axis of `in` -> (i0, i1, l1) as ATen's upsample_bilinear2d computes it
__device__ __forceinline__ void bilin_axis(int o, int in, int out, int& i0, int& i1, float& l1) {
  const float scale = (float)in / (float)out;
  float src = scale * ((float)o + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  i0 = min((int)src, in - 1);
  i1 = min(i0 + 1, in - 1);
  l1 = src - (float)i0;
}

__device__ __forceinline__ float4 bilin4(const float* x, int64_t n, int h, int w, int Ho, int Wo, int Y, int X, int C, int c) {
  int y0, y1, x0, x1;
  float ly, lx;
  bilin_axis(Y, h, Ho, y0, y1, ly);
  bilin_axis(X, w, Wo, x0, x1, lx);
  const float* base = x + n * h * w * (int64_t)C + c;
  const float4 a = *reinterpret_cast<const float4*>(base + ((int64_t)y0 * w + x0) * C);
  const float4 bb = *reinterpret_cast<const float4*>(base + ((int64_t)y0 * w + x1) * C);
  const float4 cc = *reinterpret_cast<const float4*>(base + ((int64_t)y1 * w + x0) * C);
  const float4 dd = *reinterpret_cast<const float4*>(base + ((int64_t)y1 * w + x1) * C);
  const float wy0 = 1.f - ly, wx0 = 1.f - lx;
  float4 r;
  r.x = wy0 * (wx0 * a.x + lx * bb.x) + ly * (wx0 * cc.x + lx * dd.x);
  r.y = wy0 * (wx0 * a.y + lx * bb.y) + ly * (wx0 * cc.y + lx * dd.y);
  r.z = wy0 * (wx0 * a.z + lx * bb.z) + ly * (wx0 * cc.z + lx * dd.z);
  r.w = wy0 * (wx0 * a.w + lx * bb.w) + ly * (wx0 * cc.w + lx * dd.w);
  return r;
}
