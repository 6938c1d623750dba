// Memory-bound DiT boundary ops for gfx950: norm+modulate, embeddings, final layer, sampler steps.
// All are one-pass, vectorised (8-16 B per lane), fp32 statistics; one wavefront (64 lanes) per row
// for the row-wise ops, so reductions are pure cross-lane shuffles (no LDS, no barriers).
#include "common.h"
#include "../../include/ln3d.h"

#define MAXV 9  // D <= 1152 = 9 * 128 (float2 per lane per 128 columns)

// ------------------------------------------------------------------ norm + modulation
struct NormP {
  const float* x; bf16_t* y; int64_t rows; int D; int kind; float eps; const float* weight;
  const float* shift; const float* scale; int mod_rows; int64_t mod_ld;
  const float* shift_table; const float* scale_table; int rows_in, rows_out;
};

// One wavefront per row.  Every lane owns 8 consecutive features per 512-column chunk: two 16-byte loads and ONE 16-byte bf16 store
// (8-byte global accesses run at 0.5-0.7x the 16-byte rate on gfx950); a last partial chunk (D = 1152: 128 columns) is carried by
// its first D % 512 / 8 lanes.  r4: this is the only norm + modulate kernel (r1's float2 and r2's float4 variants served the widths
// that are not multiples of 512 - DiT-XL/2's 1152 ran 1.6x slower per byte than the 1024-wide rows).  One row per wave: r3 measured
// 14.0 / 17.2 / 20.4 us at 1 / 2 / 4 rows per wave (12288 x 1024).
// MV8 = 512-feature chunks held per lane set; FULL = D is a multiple of 512: every chunk test is wave-uniform.  (r4: with the per-lane
// test of the general form on the D = 1024 path every row load sat behind its own branch + vmcnt(0): 14.9 -> 16.9 us at 12288 x 1024.)
template <int MV8, bool FULL>
__global__ __launch_bounds__(256) void norm_modulate_kernel(NormP p) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.rows) return;
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
  // the modulation rows do not depend on the statistics - their (L2-resident) loads are issued behind the row's own loads instead
  // of after the two wave reductions, so that their latency is not a second serial segment of the wave's life
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
          if (p.scale_table) {
            const float4 t0 = *reinterpret_cast<const float4*>(p.scale_table + d);
            const float4 t1 = *reinterpret_cast<const float4*>(p.shift_table + d);
            sc[i][k].x += t0.x; sc[i][k].y += t0.y; sc[i][k].z += t0.z; sc[i][k].w += t0.w;
            sh[i][k].x += t1.x; sh[i][k].y += t1.y; sh[i][k].z += t1.z; sh[i][k].w += t1.w;
          }
        }
      }
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MV8; ++i)
#pragma unroll
    for (int k = 0; k < 2; ++k) s += (v[i][k].x + v[i][k].y) + (v[i][k].z + v[i][k].w);       // lanes beyond D hold zeros
  float mean = 0.f, rstd;
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
    rstd = rsqrtf(wave_sum_dpp(q) / p.D + p.eps);
  } else {
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MV8; ++i)
#pragma unroll
      for (int k = 0; k < 2; ++k)
        q += (v[i][k].x * v[i][k].x + v[i][k].y * v[i][k].y) + (v[i][k].z * v[i][k].z + v[i][k].w * v[i][k].w);
    rstd = rsqrtf(wave_sum_dpp(q) / p.D + p.eps);
  }
  const int64_t orow = (row / p.rows_in) * p.rows_out + (row % p.rows_in);
  bf16_t* yr = p.y + orow * p.D;
#pragma unroll
  for (int i = 0; i < MV8; ++i)
    if (ok[i]) {
      uint32_t pk[4];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int d = i * 512 + lane * 8 + 4 * k;
        float4 o = make_float4((v[i][k].x - mean) * rstd, (v[i][k].y - mean) * rstd, (v[i][k].z - mean) * rstd, (v[i][k].w - mean) * rstd);
        if (p.weight) { const float4 w = *reinterpret_cast<const float4*>(p.weight + d); o.x *= w.x; o.y *= w.y; o.z *= w.z; o.w *= w.w; }
        if (p.scale) {
          o.x = o.x * (1.f + sc[i][k].x) + sh[i][k].x; o.y = o.y * (1.f + sc[i][k].y) + sh[i][k].y;
          o.z = o.z * (1.f + sc[i][k].z) + sh[i][k].z; o.w = o.w * (1.f + sc[i][k].w) + sh[i][k].w;
        }
        pk[2 * k] = pack2bf(o.x, o.y); pk[2 * k + 1] = pack2bf(o.z, o.w);
      }
      *reinterpret_cast<uint4*>(yr + i * 512 + lane * 8) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
    }
}

extern "C" int ln3d_norm_modulate(const ln3d_norm_args* a, void* stream) {
  constexpr int MVG = (128 * MAXV + 511) / 512;                   // 512-feature chunks per lane set: widths up to 1536 (the U-Net's 1280)
  if (!a || !a->x || !a->y || a->D % 128 != 0 || a->D > 512 * MVG || a->rows <= 0) return LN3D_ERR_BAD_ARG;
  if ((a->scale == nullptr) != (a->shift == nullptr)) return LN3D_ERR_BAD_ARG;
  if (a->scale && (a->mod_ld % 4) != 0) return LN3D_ERR_BAD_ARG;                       // 16-byte modulation quads
  if ((a->scale_table == nullptr) != (a->shift_table == nullptr)) return LN3D_ERR_BAD_ARG;
  NormP p;
  p.x = a->x; p.y = (bf16_t*)a->y; p.rows = a->rows; p.D = a->D; p.kind = a->kind; p.eps = a->eps; p.weight = a->weight;
  p.shift = a->shift; p.scale = a->scale; p.mod_rows = a->mod_rows > 0 ? a->mod_rows : 1; p.mod_ld = a->mod_ld;
  p.shift_table = a->shift_table; p.scale_table = a->scale_table;
  p.rows_in = a->rows_in > 0 ? a->rows_in : (int)a->rows; p.rows_out = a->rows_out > 0 ? a->rows_out : p.rows_in;
  const dim3 grid((unsigned)((a->rows + 3) / 4));
  if (a->D % 512 == 0 && a->D <= 1024) hipLaunchKernelGGL((norm_modulate_kernel<2, true>), grid, dim3(256), 0, (hipStream_t)stream, p);
  else if (a->D % 512 == 0) hipLaunchKernelGGL((norm_modulate_kernel<MVG, true>), grid, dim3(256), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL((norm_modulate_kernel<MVG, false>), grid, dim3(256), 0, (hipStream_t)stream, p);
  return ln3d_check_launch();
}

// ------------------------------------------------------------------ text conditioner helpers
__global__ void embed_tokens_kernel(const int32_t* ids, const float4* tok, const float4* pos, float4* out, int64_t n4, int T, int D4, int vocab) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const int64_t row = i / D4; const int d = (int)(i - row * D4);
  int id = ids[row]; id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const float4 a = tok[(int64_t)id * D4 + d], b = pos[(int64_t)(row % T) * D4 + d];
  out[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
extern "C" int ln3d_embed_tokens(const int32_t* ids, const float* tok_emb, const float* pos_emb, float* out, int B, int T, int D, int vocab,
                                 void* stream) {
  if (!ids || !tok_emb || !pos_emb || !out || B <= 0 || T <= 0 || D % 4 || vocab <= 0) return LN3D_ERR_BAD_ARG;
  const int64_t n4 = (int64_t)B * T * (D / 4);
  hipLaunchKernelGGL(embed_tokens_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ids,
                     (const float4*)tok_emb, (const float4*)pos_emb, (float4*)out, n4, T, D / 4, vocab);
  return ln3d_check_launch();
}

__global__ __launch_bounds__(256) void layernorm_f32_kernel(const float* x, const float* w, const float* b, float* y, int64_t rows, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nv = D / 128;
  const float* xr = x + row * D;
  float2 v[MAXV];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i)
    if (i < nv) { v[i] = *reinterpret_cast<const float2*>(xr + i * 128 + lane * 2); s += v[i].x + v[i].y; }
  const float mean = wave_sum(s) / D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i)
    if (i < nv) { const float a = v[i].x - mean, c = v[i].y - mean; q += a * a + c * c; }
  const float rstd = rsqrtf(wave_sum(q) / D + eps);
#pragma unroll
  for (int i = 0; i < MAXV; ++i)
    if (i < nv) {
      const int d = i * 128 + lane * 2;
      const float2 ww = w ? *reinterpret_cast<const float2*>(w + d) : make_float2(1.f, 1.f);
      const float2 bb = b ? *reinterpret_cast<const float2*>(b + d) : make_float2(0.f, 0.f);
      *reinterpret_cast<float2*>(y + row * D + d) = make_float2((v[i].x - mean) * rstd * ww.x + bb.x, (v[i].y - mean) * rstd * ww.y + bb.y);
    }
}
extern "C" int ln3d_layernorm_f32(const float* x, const float* w, const float* b, float* y, int64_t rows, int D, float eps, void* stream) {
  if (!x || !y || rows <= 0 || D % 128 != 0 || D > 128 * MAXV) return LN3D_ERR_BAD_ARG;
  hipLaunchKernelGGL(layernorm_f32_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, w, b, y, rows, D, eps);
  return ln3d_check_launch();
}

// ------------------------------------------------------------------ image conditioner helpers (ViT towers)
// out[(b*G + gy)*G + gx, c*p*p + i*p + j] = bf16(img[b, c, gy*p + i, gx*p + j]), columns >= 3*p*p zero (K padded to a
// multiple of 64 for the GEMM): the patch-embedding convolution (kernel = stride = p) becomes one GEMM
__global__ void vit_patchify_kernel(const float* img, bf16_t* out, int B, int S, int p, int Kpad, int C) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int G = S / p, KK = C * p * p;
  const int64_t total = (int64_t)B * G * G * Kpad;
  if (i >= total) return;
  const int k = (int)(i % Kpad);
  const int64_t row = i / Kpad;
  float v = 0.f;
  if (k < KK) {
    const int c = k / (p * p), ij = k - c * p * p, ii = ij / p, jj = ij - ii * p;
    const int gx = (int)(row % G), gy = (int)((row / G) % G), b = (int)(row / ((int64_t)G * G));
    v = img[(((int64_t)b * C + c) * S + gy * p + ii) * S + gx * p + jj];
  }
  out[i] = f2bf(v);
}
extern "C" int ln3d_vit_patchify(const float* img, void* out, int B, int S, int p, int Kpad, int C, void* stream) {
  if (!img || !out || B <= 0 || S <= 0 || p <= 0 || S % p || C <= 0 || Kpad < C * p * p) return LN3D_ERR_BAD_ARG;
  const int64_t total = (int64_t)B * (S / p) * (S / p) * Kpad;
  hipLaunchKernelGGL(vit_patchify_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, img, (bf16_t*)out, B, S, p, Kpad, C);
  return ln3d_check_launch();
}
// Pluecker ray maps of posed views (multi-view conditioner, sgm/modules/encoders/modules.py:958-1005 gen_rays / get_plucker_ray):
// c[v] = 16 floats camera-to-world (row-major 4x4) + 9 floats normalised intrinsics (fx, 0, cx, 0, fy, cy, 0, 0, 1);
// pixel (y, x) of an S x S grid looks along normalize(((x + .5) / S - cx) / fx, ((y + .5) / S - cy) / fy, 1) rotated by c2w[:3,:3];
// out[v, 0:3] = origin x direction, out[v, 3:6] = direction   (fp32 [V, 6, S, S])
__global__ void plucker_rays_kernel(const float* c, float* out, int V, int S) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)V * S * S) return;
  const int x = (int)(i % S), y = (int)((i / S) % S), v = (int)(i / ((int64_t)S * S));
  const float* cv = c + (int64_t)v * 25;
  const float fx = cv[16], cx = cv[18], fy = cv[20], cy = cv[21];
  float dx = (((float)x + 0.5f) / (float)S - cx) / fx, dy = (((float)y + 0.5f) / (float)S - cy) / fy, dz = 1.0f;
  const float n = sqrtf(dx * dx + dy * dy + dz * dz);
  dx /= n; dy /= n; dz /= n;
  const float wx = cv[0] * dx + cv[1] * dy + cv[2] * dz, wy = cv[4] * dx + cv[5] * dy + cv[6] * dz, wz = cv[8] * dx + cv[9] * dy + cv[10] * dz;
  const float ox = cv[3], oy = cv[7], oz = cv[11];
  float* o = out + (int64_t)v * 6 * S * S + (int64_t)y * S + x;
  const int64_t pl = (int64_t)S * S;
  o[0] = oy * wz - oz * wy; o[pl] = oz * wx - ox * wz; o[2 * pl] = ox * wy - oy * wx;
  o[3 * pl] = wx; o[4 * pl] = wy; o[5 * pl] = wz;
}
extern "C" int ln3d_plucker_rays(const float* c, float* out, int V, int S, void* stream) {
  if (!c || !out || V <= 0 || S <= 0) return LN3D_ERR_BAD_ARG;
  const int64_t total = (int64_t)V * S * S;
  hipLaunchKernelGGL(plucker_rays_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, c, out, V, S);
  return ln3d_check_launch();
}
// x[b, 0] = cls + pos[0]; x[b, 1..R] = reg; x[b, 1+R+n] = patch[b, n] + pos[1+n]   (f32, T = 1 + R + L tokens)
__global__ void vit_assemble_kernel(const float* patch, const float* cls, const float* reg, const float* pos, float* x, int B, int L,
                                    int R, int D) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int T = 1 + R + L;
  if (i >= (int64_t)B * T * D) return;
  const int d = (int)(i % D);
  const int t = (int)((i / D) % T), b = (int)(i / ((int64_t)D * T));
  float v;
  if (t == 0) v = cls[d] + pos[d];
  else if (t <= R) v = reg[(int64_t)(t - 1) * D + d];
  else { const int n = t - 1 - R; v = patch[((int64_t)b * L + n) * D + d] + pos[(int64_t)(1 + n) * D + d]; }
  x[i] = v;
}
extern "C" int ln3d_vit_assemble(const float* patch, const float* cls, const float* reg, const float* pos, float* x, int B, int L, int R,
                                 int D, void* stream) {
  if (!patch || !cls || !pos || !x || (R > 0 && !reg) || B <= 0 || L <= 0 || R < 0 || D <= 0) return LN3D_ERR_BAD_ARG;
  const int64_t total = (int64_t)B * (1 + R + L) * D;
  hipLaunchKernelGGL(vit_assemble_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, patch, cls, reg, pos, x, B, L, R, D);
  return ln3d_check_launch();
}

// ------------------------------------------------------------------ small elementwise
__global__ void timestep_embedding_kernel(const float* t, bf16_t* out, int B, int dim) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int half = dim / 2;
  if (i >= B * half) return;
  const int b = i / half, k = i % half;
  const float freq = expf(-logf(10000.0f) * (float)k / (float)half);
  const float arg = t[b] * freq;
  out[(int64_t)b * dim + k] = f2bf(cosf(arg));
  out[(int64_t)b * dim + half + k] = f2bf(sinf(arg));
}
extern "C" int ln3d_timestep_embedding(const float* t, void* out, int B, int dim, void* stream) {
  if (!t || !out || B <= 0 || dim <= 0 || dim % 2) return LN3D_ERR_BAD_ARG;
  const int n = B * dim / 2;
  hipLaunchKernelGGL(timestep_embedding_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, t, (bf16_t*)out, B, dim);
  return ln3d_check_launch();
}

__global__ void add_act_cast_kernel(const float* a, const float* b, bf16_t* y, float* sum, int64_t n, int act) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v = a[i] + (b ? b[i] : 0.f);
  if (sum) sum[i] = v;
  if (act == 1) v = silu(v);
  if (y) y[i] = f2bf(v);
}
extern "C" int ln3d_add_act_cast(const float* a, const float* b, void* y, float* sum, int64_t n, int act, void* stream) {
  if (!a || n <= 0) return LN3D_ERR_BAD_ARG;
  hipLaunchKernelGGL(add_act_cast_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, (bf16_t*)y, sum, n, act);
  return ln3d_check_launch();
}

__global__ void cast_f32_bf16_kernel(const float4* x, uint2* y, int64_t n4) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n4; i += stride) {
    const float4 v = x[i];
    uint2 o; o.x = pack2bf(v.x, v.y); o.y = pack2bf(v.z, v.w);
    y[i] = o;
  }
}
extern "C" int ln3d_cast_f32_bf16(const float* x, void* y, int64_t n, void* stream) {
  if (!x || !y || n <= 0 || n % 4) return LN3D_ERR_BAD_ARG;
  const int64_t n4 = n / 4;
  int64_t blocks = (n4 + 255) / 256; if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float4*)x, (uint2*)y, n4);
  return ln3d_check_launch();
}

// ------------------------------------------------------------------ patch embed (+pos embed)
// tokens[b, n*L + (ph*G + pw), d] = bias[d] + pos[n*L + ..., d] + sum_{c,i,j} w[d, c, i, j] * s_b * x[b%Bx, c*3+n, p*ph+i, p*pw+j]
// 8 tokens per block: the [D, C*p*p] weight (196 KB at DiT-L/2) is read once per 8 tokens instead of once per token
// (one token per block re-read 2.4 GB from L2 per call); per-token arithmetic order unchanged.
#define PE_TPB 8
__global__ __launch_bounds__(256) void patch_embed_kernel(const float* x, const float* in_scale, const float* w, const float* bias,
                                                          const float* pos, float* tokens, int Bx, int Bn, int C, int S, int p, int D) {
  const int G = S / p, L = G * G;
  const int ntok = Bn * 3 * L;
  const int tok0 = blockIdx.x * PE_TPB;
  const int KK = C * p * p;              // <= 64
  __shared__ float patch[PE_TPB][64];
  for (int idx = threadIdx.x; idx < PE_TPB * KK; idx += blockDim.x) {
    const int t = idx / KK, k = idx - t * KK, tok = tok0 + t;
    float v = 0.f;
    if (tok < ntok) {
      const int b = tok / (3 * L), r = tok % (3 * L), n = r / L, l = r % L, ph = l / G, pw = l % G;
      const int c = k / (p * p), ij = k % (p * p), i = ij / p, j = ij % p;
      const float sc = in_scale ? in_scale[b] : 1.0f;
      v = sc * x[(((int64_t)(b % Bx) * C * 3 + c * 3 + n) * S + p * ph + i) * S + p * pw + j];
    }
    patch[t][k] = v;
  }
  __syncthreads();
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    float acc[PE_TPB];
    const float bd = bias[d];
#pragma unroll
    for (int t = 0; t < PE_TPB; ++t) acc[t] = bd;
    const float* wr = w + (int64_t)d * KK;
    for (int k = 0; k < KK; ++k) {
      const float wk = wr[k];
#pragma unroll
      for (int t = 0; t < PE_TPB; ++t) acc[t] += wk * patch[t][k];
    }
#pragma unroll
    for (int t = 0; t < PE_TPB; ++t) {
      const int tok = tok0 + t;
      if (tok < ntok) tokens[(int64_t)tok * D + d] = acc[t] + pos[(int64_t)(tok % (3 * L)) * D + d];
    }
  }
}
extern "C" int ln3d_patch_embed(const float* x, const float* in_scale, const float* w, const float* bias, const float* pos,
                                float* tokens, int Bx, int Bn, int C, int S, int p, int D, void* stream) {
  if (!x || !w || !bias || !pos || !tokens || Bx <= 0 || Bn <= 0 || C <= 0 || S <= 0 || p <= 0 || D <= 0) return LN3D_ERR_BAD_ARG;
  if (C * p * p > 64 || S % p) return LN3D_ERR_BAD_ARG;
  const int L = (S / p) * (S / p);
  hipLaunchKernelGGL(patch_embed_kernel, dim3((Bn * 3 * L + PE_TPB - 1) / PE_TPB), dim3(256), 0, (hipStream_t)stream, x, in_scale, w, bias, pos,
                     tokens, Bx, Bn, C, S, p, D);
  return ln3d_check_launch();
}

// ------------------------------------------------------------------ PatchEmbedTriplane (VAE decoder tokeniser)
// grouped conv (groups=3) + literal channel regroup of vit/vit_triplane.py:82-106, emitted as silu(c) in bf16
// because the decoder only ever consumes c through adaLN_modulation = Linear(SiLU(c)) (dit/dit_decoder.py:27-28):
//   oc = d*3 + j, group g = oc / D ;  c[b, j*L + l, d] = bias[oc] + sum_{cc,ky,kx} w[oc,cc,ky,kx] * latent[b, g*Cg + cc, p*ph+ky, p*pw+kx]
__global__ __launch_bounds__(256) void patch_embed_triplane_kernel(const float* latent, const float* w, const float* bias,
                                                                   bf16_t* out_silu, float* out_raw, int Cg, int S, int p, int D) {
  const int G = S / p, L = G * G;
  const int tok = blockIdx.x;            // b * 3L + j*L + l
  const int b = tok / (3 * L), r = tok % (3 * L), j = r / L, l = r % L, ph = l / G, pw = l % G;
  const int KK = Cg * p * p;             // per-group patch size (16)
  __shared__ float patch[3 * 64];
  if (threadIdx.x < 3 * KK) {
    const int g = threadIdx.x / KK, k = threadIdx.x % KK;
    const int cc = k / (p * p), ij = k % (p * p), ky = ij / p, kx = ij % p;
    patch[threadIdx.x] = latent[(((int64_t)b * 3 * Cg + g * Cg + cc) * S + p * ph + ky) * S + p * pw + kx];
  }
  __syncthreads();
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    const int oc = d * 3 + j, g = oc / D;
    float acc = bias[oc];
    const float* wr = w + (int64_t)oc * KK;
    for (int k = 0; k < KK; ++k) acc += wr[k] * patch[g * KK + k];
    if (out_raw) out_raw[(int64_t)tok * D + d] = acc;
    out_silu[(int64_t)tok * D + d] = f2bf(silu(acc));
  }
}
extern "C" int ln3d_patch_embed_triplane(const float* latent, const float* w, const float* bias, void* out_silu_bf16,
                                         float* out_raw, int B, int Cg, int S, int p, int D, void* stream) {
  if (!latent || !w || !bias || !out_silu_bf16 || B <= 0 || Cg <= 0 || S <= 0 || p <= 0 || D <= 0) return LN3D_ERR_BAD_ARG;
  if (Cg * p * p > 64 || S % p) return LN3D_ERR_BAD_ARG;
  const int L = (S / p) * (S / p);
  hipLaunchKernelGGL(patch_embed_triplane_kernel, dim3(B * 3 * L), dim3(256), 0, (hipStream_t)stream, latent, w, bias,
                     (bf16_t*)out_silu_bf16, out_raw, Cg, S, p, D);
  return ln3d_check_launch();
}

// broadcast rows: y[b, :, :] = x[:, :] (DiT2 starts from the positional embedding, dit/dit_decoder.py:104-105)
__global__ void tile_rows_kernel(const float4* x, float4* y, int64_t per4, int64_t total4) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total4) y[i] = x[i % per4];
}
extern "C" int ln3d_tile_rows(const float* x, float* y, int64_t per, int reps, void* stream) {
  if (!x || !y || per <= 0 || reps <= 0 || per % 4) return LN3D_ERR_BAD_ARG;
  const int64_t total4 = per / 4 * reps;
  hipLaunchKernelGGL(tile_rows_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float4*)x,
                     (float4*)y, per / 4, total4);
  return ln3d_check_launch();
}

// ------------------------------------------------------------------ final layer (+unpatchify)
struct FinalP {
  const float* tokens; const float* shift; const float* scale; int64_t mod_ld;
  const float* shift_table; const float* scale_table; const float* w; const float* bias; float* out;
  int Bn, C, S, p, D;
};
// One wavefront per 2 tokens (measured 1 / 2 / 4 / 8 tokens: 76 / 63 / 75 / 107 us at 12288 tokens with DPP wave sums): LN + modulate of each token in registers, then every weight row is fetched once per wave
// (one token per wave re-read the 196 KB projection from L2 for every token); per-token arithmetic order unchanged.
// r3: staging the projection in LDS once per 32-token workgroup (64 KB -> 2 workgroups = 8 waves per CU) measured SLOWER (116 vs
// 73 us at 12288 tokens: the kernel lives on wave occupancy, the L2 re-reads of the weight are cheap); not kept.
#define FL_TPW 2
__global__ __launch_bounds__(256) void final_layer_kernel(FinalP q) {
  const int lane = threadIdx.x & 63;
  const int G = q.S / q.p, L = G * G;
  const int64_t ntok = (int64_t)q.Bn * 3 * L;
  const int64_t tok0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * FL_TPW;
  if (tok0 >= ntok) return;
  const int nv = q.D / 128;
  float2 v[FL_TPW][MAXV];
#pragma unroll
  for (int t = 0; t < FL_TPW; ++t) {
    const int64_t tok = tok0 + t < ntok ? tok0 + t : ntok - 1;
    const int b = (int)(tok / (3 * L));
    const float* xr = q.tokens + tok * q.D;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
      if (i < nv) { v[t][i] = *reinterpret_cast<const float2*>(xr + i * 128 + lane * 2); s += v[t][i].x + v[t][i].y; }
    const float mean = wave_sum_dpp(s) / q.D;
    float qq = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
      if (i < nv) { const float a = v[t][i].x - mean, c = v[t][i].y - mean; qq += a * a + c * c; }
    const float rstd = rsqrtf(wave_sum_dpp(qq) / q.D + 1e-6f);
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
      if (i < nv) {
        const int d = i * 128 + lane * 2;
        float2 sc = *reinterpret_cast<const float2*>(q.scale + (int64_t)b * q.mod_ld + d);
        float2 sh = *reinterpret_cast<const float2*>(q.shift + (int64_t)b * q.mod_ld + d);
        if (q.scale_table) {
          const float2 t0 = *reinterpret_cast<const float2*>(q.scale_table + d);
          const float2 t1 = *reinterpret_cast<const float2*>(q.shift_table + d);
          sc.x += t0.x; sc.y += t0.y; sh.x += t1.x; sh.y += t1.y;
        }
        v[t][i].x = (v[t][i].x - mean) * rstd * (1.f + sc.x) + sh.x;
        v[t][i].y = (v[t][i].y - mean) * rstd * (1.f + sc.y) + sh.y;
      }
  }
  const int NO = q.p * q.p * q.C;        // outputs per token, index o = (i*p + j)*C + c
  for (int o = 0; o < NO; ++o) {
    const float* wr = q.w + (int64_t)o * q.D;
    float acc[FL_TPW];
#pragma unroll
    for (int t = 0; t < FL_TPW; ++t) acc[t] = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
      if (i < nv) {
        const float2 ww = *reinterpret_cast<const float2*>(wr + i * 128 + lane * 2);
#pragma unroll
        for (int t = 0; t < FL_TPW; ++t) acc[t] += ww.x * v[t][i].x + ww.y * v[t][i].y;
      }
    const int c = o % q.C, ij = o / q.C, i = ij / q.p, j = ij % q.p;
    const float bo = q.bias[o];
#pragma unroll
    for (int t = 0; t < FL_TPW; ++t) {
      const float a = wave_sum_dpp(acc[t]);
      const int64_t tok = tok0 + t;
      if (lane == 0 && tok < ntok) {
        const int b = (int)(tok / (3 * L)), r = (int)(tok % (3 * L)), n = r / L, l = r % L, ph = l / G, pw = l % G;
        q.out[(((int64_t)b * q.C * 3 + c * 3 + n) * q.S + q.p * ph + i) * q.S + q.p * pw + j] = a + bo;
      }
    }
  }
}
extern "C" int ln3d_final_layer(const float* tokens, const float* shift, const float* scale, int64_t mod_ld,
                                const float* shift_table, const float* scale_table, const float* w, const float* bias,
                                float* out, int Bn, int C, int S, int p, int D, void* stream) {
  if (!tokens || !shift || !scale || !w || !bias || !out || D <= 0 || D % 128 || D > 128 * MAXV) return LN3D_ERR_BAD_ARG;
  if (Bn <= 0 || C <= 0 || S <= 0 || p <= 0 || S % p) return LN3D_ERR_BAD_ARG;
  FinalP q{tokens, shift, scale, mod_ld, shift_table, scale_table, w, bias, out, Bn, C, S, p, D};
  const int64_t ntok = (int64_t)Bn * 3 * (S / p) * (S / p);
  hipLaunchKernelGGL(final_layer_kernel, dim3((unsigned)((ntok + 4 * FL_TPW - 1) / (4 * FL_TPW))), dim3(256), 0, (hipStream_t)stream, q);
  return ln3d_check_launch();
}

// ------------------------------------------------------------------ image preprocessing of the image conditioners
// kornia.geometry.transform.resize(x, (S, S), 'bicubic', align_corners=True, antialias) -> (x + 1) / 2 -> (x - mean) / std
// (sgm/modules/encoders/modules.py:633-645,802-814).  kornia as published (geometry/transform/affwarp.py): when a side shrinks,
// blur with a separable Gaussian (sigma = max((factor - 1) / 2, 0.001), kernel size max(int(4 sigma), 3) made odd, reflect border),
// then torch's bicubic interpolation (A = -0.75, align_corners, clamped taps: ATen UpSampleBicubic2d).
struct BlurP { const float* x; float* y; int64_t n; int H, W, k, axis; float w[64]; };
__global__ void image_blur_kernel(BlurP q) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= q.n) return;
  const int x = (int)(i % q.W), y = (int)((i / q.W) % q.H);
  const int64_t base = i - (int64_t)y * q.W - x;
  const int r = q.k / 2, L = q.axis ? q.H : q.W, c0 = q.axis ? y : x;
  float acc = 0.f;
  for (int t = 0; t < q.k; ++t) {
    int c = c0 + t - r;
    c = c < 0 ? -c : c;
    c = c >= L ? 2 * (L - 1) - c : c;                     // 'reflect' (the border sample is not repeated)
    acc += q.w[t] * q.x[base + (q.axis ? (int64_t)c * q.W + x : (int64_t)y * q.W + c)];
  }
  q.y[i] = acc;
}
struct ResizeP { const float* x; float* y; int NC, C, H, W, S; float sy, sx; float mean[4], rstd[4]; };
__device__ __forceinline__ void cubic_w(float t, float (&w)[4]) {
  const float A = -0.75f;
  auto c1 = [&](float x) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; };
  auto c2 = [&](float x) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; };
  w[0] = c2(t + 1.f); w[1] = c1(t); w[2] = c1(1.f - t); w[3] = c2(2.f - t);
}
__global__ void image_resize_norm_kernel(ResizeP q) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)q.NC * q.S * q.S) return;
  const int ox = (int)(i % q.S), oy = (int)((i / q.S) % q.S), nc = (int)(i / ((int64_t)q.S * q.S));
  const float fy = q.sy * oy, fx = q.sx * ox;
  const int y0 = (int)floorf(fy), x0 = (int)floorf(fx);
  float wy[4], wx[4];
  cubic_w(fy - y0, wy); cubic_w(fx - x0, wx);
  const float* img = q.x + (int64_t)nc * q.H * q.W;
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int yy = min(max(y0 - 1 + a, 0), q.H - 1);
    float row = 0.f;
#pragma unroll
    for (int b = 0; b < 4; ++b) row += wx[b] * img[(int64_t)yy * q.W + min(max(x0 - 1 + b, 0), q.W - 1)];
    acc += wy[a] * row;
  }
  const int c = nc % q.C;
  q.y[i] = ((acc + 1.0f) * 0.5f - q.mean[c]) * q.rstd[c];
}
extern "C" int ln3d_image_preprocess(const float* x, float* out, float* tmp, int N, int C, int H, int W, int S, int antialias,
                                     const float* mean_host, const float* std_host, void* stream) {
  if (!x || !out || !mean_host || !std_host || N <= 0 || C <= 0 || C > 4 || H < 2 || W < 2 || S < 2) return LN3D_ERR_BAD_ARG;
  const float f[2] = {(float)H / S, (float)W / S};
  const float* src = x;
  if (antialias && (f[0] > 1.f || f[1] > 1.f) && !(H == S && W == S)) {
    if (!tmp) return LN3D_ERR_BAD_ARG;
    const int64_t n = (int64_t)N * C * H * W;
    for (int axis = 0; axis < 2; ++axis) {              // x pass (factor of W) then y pass, like the two conv2d calls
      BlurP q;
      const float sig = fmaxf((f[1 - axis] - 1.0f) / 2.0f, 0.001f);
      int k = (int)fmaxf(2.0f * 2 * sig, 3.f);
      k += (k % 2 == 0);
      if (k > 63) return LN3D_ERR_UNSUPPORTED;
      float sum = 0.f;
      for (int t = 0; t < k; ++t) { const float d = (float)(t - k / 2); q.w[t] = expf(-d * d / (2.f * sig * sig)); sum += q.w[t]; }
      for (int t = 0; t < k; ++t) q.w[t] /= sum;
      q.x = src; q.y = tmp + (axis ? n : 0); q.n = n; q.H = H; q.W = W; q.k = k; q.axis = axis;
      hipLaunchKernelGGL(image_blur_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, q);
      src = q.y;
    }
  }
  ResizeP r;
  r.x = src; r.y = out; r.NC = N * C; r.C = C; r.H = H; r.W = W; r.S = S;
  r.sy = S > 1 ? (float)(H - 1) / (float)(S - 1) : 0.f; r.sx = S > 1 ? (float)(W - 1) / (float)(S - 1) : 0.f;
  for (int c = 0; c < 4; ++c) { r.mean[c] = c < C ? mean_host[c] : 0.f; r.rstd[c] = c < C ? 1.0f / std_host[c] : 1.f; }
  const int64_t no = (int64_t)N * C * S * S;
  hipLaunchKernelGGL(image_resize_norm_kernel, dim3((unsigned)((no + 255) / 256)), dim3(256), 0, (hipStream_t)stream, r);
  return ln3d_check_launch();
}

// ------------------------------------------------------------------ sampler steps
__global__ void edm_euler_step_kernel(float* x, const float* eps2, float sigma, float sigma_next, float scale, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float xv = x[i];
  const float den_u = eps2[i] * (-sigma) + xv;          // DiscreteDenoiser: net*c_out + x*c_skip
  const float den_c = eps2[n + i] * (-sigma) + xv;
  const float den = den_u + scale * (den_c - den_u);    // VanillaCFG
  const float d = (xv - den) / sigma;                   // to_d
  x[i] = xv + d * (sigma_next - sigma);                 // euler_step
}
extern "C" int ln3d_edm_euler_step(float* x, const float* eps2, float sigma, float sigma_next, float cfg_scale, int64_t n, void* stream) {
  if (!x || !eps2 || n <= 0) return LN3D_ERR_BAD_ARG;
  hipLaunchKernelGGL(edm_euler_step_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, eps2, sigma, sigma_next, cfg_scale, n);
  return ln3d_check_launch();
}

__global__ void ddpm_step_kernel(float* x, const float* eps, const float* noise, float a, float b, float c1, float c2,
                                 float sig, int clip, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float xv = x[i];
  float x0 = a * xv - b * eps[i];
  if (clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
  const float mean = c1 * x0 + c2 * xv;
  x[i] = mean + sig * noise[i];
}
extern "C" int ln3d_ddpm_step(float* x, const float* eps, const float* noise, float sqrt_recip, float sqrt_recipm1, float coef1,
                              float coef2, float sigma_t, int clip, int64_t n, void* stream) {
  if (!x || !eps || !noise || n <= 0) return LN3D_ERR_BAD_ARG;
  hipLaunchKernelGGL(ddpm_step_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, eps, noise, sqrt_recip,
                     sqrt_recipm1, coef1, coef2, sigma_t, clip, n);
  return ln3d_check_launch();
}

// DDIM step with optional CFG on eps (guided_diffusion/gaussian_diffusion.py:729-866, non-objv branch):
// eps = eu + s*(ec - eu); x0 = a*x - b*eps (opt. clip; eps re-derived from the clipped x0 as the reference does);
// x <- sqrt(ab_prev)*x0 + sqrt(1 - ab_prev - sigma^2)*eps + sigma*noise
__global__ void ddim_step_kernel(float* x, const float* eu, const float* ec, const float* noise, float scale, float a, float b,
                                 float sqrt_ab_prev, float coef_eps, float sigma, int clip, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float xv = x[i];
  float e_u = eu[i], e_c = ec ? ec[i] : 0.f;
  if (clip) {                     // p_mean_variance clips x0, then eps is re-derived per branch
    float x0u = fminf(fmaxf(a * xv - b * e_u, -1.f), 1.f);
    e_u = (a * xv - x0u) / b;
    if (ec) { float x0c = fminf(fmaxf(a * xv - b * e_c, -1.f), 1.f); e_c = (a * xv - x0c) / b; }
  }
  const float eps = ec ? e_u + scale * (e_c - e_u) : e_u;
  const float x0 = a * xv - b * eps;
  x[i] = x0 * sqrt_ab_prev + coef_eps * eps + (noise ? sigma * noise[i] : 0.f);
}
extern "C" int ln3d_ddim_step(float* x, const float* eps_u, const float* eps_c, const float* noise, float cfg_scale,
                              float sqrt_recip, float sqrt_recipm1, float sqrt_ab_prev, float coef_eps, float sigma, int clip,
                              int64_t n, void* stream) {
  if (!x || !eps_u || n <= 0) return LN3D_ERR_BAD_ARG;
  hipLaunchKernelGGL(ddim_step_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, eps_u, eps_c, noise,
                     cfg_scale, sqrt_recip, sqrt_recipm1, sqrt_ab_prev, coef_eps, sigma, clip, n);
  return ln3d_check_launch();
}

__global__ void flow_euler_step_kernel(float* x2, const float* v2, float dt, float scale, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float vc = v2[i], vu = v2[n + i];
  const float v = vu + scale * (vc - vu);
  x2[i] += dt * v;
  x2[n + i] += dt * v;
}
extern "C" int ln3d_flow_euler_step(float* x2, const float* v2, float dt, float cfg_scale, int64_t n_half, void* stream) {
  if (!x2 || !v2 || n_half <= 0) return LN3D_ERR_BAD_ARG;
  hipLaunchKernelGGL(flow_euler_step_kernel, dim3((unsigned)((n_half + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x2, v2, dt, cfg_scale, n_half);
  return ln3d_check_launch();
}

__global__ void axpby_kernel(const float* x, float* y, float a, float b, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = a * x[i] + b * y[i];
}
extern "C" int ln3d_axpby(const float* x, float* y, float a, float b, int64_t n, void* stream) {
  if (!x || !y || n <= 0) return LN3D_ERR_BAD_ARG;
  hipLaunchKernelGGL(axpby_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, a, b, n);
  return ln3d_check_launch();
}

// out[l, b, :] = tables[l, :] + t0[b, :]   (PixArt shared adaLN: scale_shift_table[None] + t.reshape(B,6,D),
// dit/dit_models_xformers.py:518-519) for all layers at once
__global__ void add_table_rows_kernel(const float* t0, const float* tables, float* out, int B, int64_t W, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int64_t w = i % W, lb = i / W, b = lb % B, l = lb / B;
  out[i] = tables[l * W + w] + t0[b * W + w];
}
extern "C" int ln3d_add_table_rows(const float* t0, const float* tables, float* out, int layers, int B, int64_t W, void* stream) {
  if (!t0 || !tables || !out || layers <= 0 || B <= 0 || W <= 0) return LN3D_ERR_BAD_ARG;
  const int64_t total = (int64_t)layers * B * W;
  hipLaunchKernelGGL(add_table_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, t0, tables, out, B, W, total);
  return ln3d_check_launch();
}

// forward_with_cfg (dit/dit_i23d.py:155-168): v[2B] = [cond ; uncond] -> both halves = uncond + s*(cond - uncond)
__global__ void cfg_combine_dup_kernel(float* v2, float scale, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float c = v2[i], u = v2[n + i];
  const float h = u + scale * (c - u);
  v2[i] = h; v2[n + i] = h;
}
extern "C" int ln3d_cfg_combine_dup(float* v2, float cfg_scale, int64_t n_half, void* stream) {
  if (!v2 || n_half <= 0) return LN3D_ERR_BAD_ARG;
  hipLaunchKernelGGL(cfg_combine_dup_kernel, dim3((unsigned)((n_half + 255) / 256)), dim3(256), 0, (hipStream_t)stream, v2, cfg_scale, n_half);
  return ln3d_check_launch();
}

// Runge-Kutta helpers for the adaptive ODE solver (transport 'dopri5'): out = y + sum_j c[j] * k[j] (up to 7 stages), and
// the RMS-norm error ratio accumulator sum((err / (atol + rtol * max(|y0|, |y1|)))^2).
struct LinCombP { const float* k[7]; float c[7]; int n; };
__global__ void lincomb_kernel(const float* y, LinCombP p, float* out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float acc = y ? y[i] : 0.f;
#pragma unroll
  for (int j = 0; j < 7; ++j)
    if (j < p.n) acc += p.c[j] * p.k[j][i];
  out[i] = acc;
}
extern "C" int ln3d_lincomb(const float* y, const float* const* ks, const float* cs, int nterms, float* out, int64_t n, void* stream) {
  if (!out || nterms < 0 || nterms > 7 || n <= 0) return LN3D_ERR_BAD_ARG;
  LinCombP p{};
  p.n = nterms;
  for (int j = 0; j < nterms; ++j) { p.k[j] = ks[j]; p.c[j] = cs[j]; }
  hipLaunchKernelGGL(lincomb_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, p, out, n);
  return ln3d_check_launch();
}
// sum_i (err_i / (atol + rtol max(|y0_i|, |y1_i|)))^2 -> acc[0].  ONE workgroup, fixed summation order: the accept / reject decision
// of the adaptive ODE solver reads this number, so it must not depend on the arrival order of atomics (r2 used atomicAdd).
__global__ __launch_bounds__(1024) void err_ratio_sq_kernel(const float* err, const float* y0, const float* y1, float atol, float rtol, float* acc, int64_t n) {
  __shared__ float part[16];
  float v = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    const float tol = atol + rtol * fmaxf(fabsf(y0[i]), y1 ? fabsf(y1[i]) : 0.f);
    const float r = err[i] / tol;
    v += r * r;
  }
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += part[w];
    acc[0] = t;
  }
}
extern "C" int ln3d_err_ratio_sq(const float* err, const float* y0, const float* y1, float atol, float rtol, float* acc,
                                 int64_t n, void* stream) {
  if (!err || !y0 || !acc || n <= 0) return LN3D_ERR_BAD_ARG;
  hipLaunchKernelGGL(err_ratio_sq_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, err, y0, y1, atol, rtol, acc, n);
  return ln3d_check_launch();
}

// ------------------------------------------------------------------ misc
extern "C" const char* ln3d_strerror(int code) {
  switch (code) {
    case LN3D_OK: return "ok";
    case LN3D_ERR_BAD_ARG: return "bad argument (null pointer, unsupported shape or alignment)";
    case LN3D_ERR_LAUNCH: return "HIP kernel launch failed";
    case LN3D_ERR_UNSUPPORTED: return "unsupported configuration";
    default: return "unknown error";
  }
}
extern "C" int ln3d_abi_version(void) { return 10; }
extern "C" void ln3d_gemm_reload_env(void);
extern "C" void ln3d_reload_env(void) { ln3d_gemm_reload_env(); }
