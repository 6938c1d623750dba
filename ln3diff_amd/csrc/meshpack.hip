// Binary mesh export for gfx950 (include/ln3d_meshpack.h): the records of a binary little-endian PLY and the buffer sections of a
// GLB, assembled on the device so that the host writes whole sections and touches no element.
// The PLY records are 15, 27 and 13 bytes long.  One thread per record would issue byte stores scattered over a stride that is no multiple
// of 4; instead one thread owns one aligned OUTPUT word, looks up which record and field each of its four bytes comes from, and stores
// the word once: a wavefront writes 256 contiguous bytes per store.  A word touches at most two 32-bit fields, which a one-entry cache
// keeps from being evaluated twice; the 12-byte input rows come through L1 / L2, shared by the three to seven threads whose words they feed.
// The GLB sections are arrays of whole words already: one thread per float.
#include "common.h"
#include "../../include/ln3d.h"
#include "../../include/ln3d_meshpack.h"

static inline dim3 pack_grid(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }                        // one thread per element, blocks of 256
static inline bool pack_count_ok(int64_t n) { return n >= 1 && n <= 0x7fffffffll; }
static inline bool pack_aligned(const void* p) { return ((uintptr_t)p & 3u) == 0; }

// row r of R * (x, y, z) with five roundings (a product next to a sum would otherwise be contracted into an fma, as in bake_affine)
__device__ __forceinline__ float pack_rot(const float* rot9, int r, const float* p) {
#pragma clang fp contract(off)
  const float a = rot9[3 * r] * p[0], b = rot9[3 * r + 1] * p[1], c = rot9[3 * r + 2] * p[2];
  const float ab = a + b;
  return ab + c;
}

// fmaxf(NaN, 0) = 0: a NaN colour is 0 (the rule of bake_pack_kernel)
__device__ __forceinline__ uint32_t pack_colour(float c) { return (uint32_t)(int)(fminf(fmaxf(c, 0.0f), 1.0f) * 255.0f); }

// ------------------------------------------------------------------ PLY: one thread per output word
// NF floats (3: position; 6: position, normal), then three colour bytes
template <int NF>
struct PlyVertexRecord {
  static constexpr int SIZE = 4 * NF + 3;
  const float* xyz; const float* normal; const float* rgb; const float* rot9;
  __device__ __forceinline__ uint32_t byte(int64_t r, int o, int64_t& cached, uint32_t& bits) const {
    if (o >= 4 * NF) return pack_colour(rgb[3 * r + (o - 4 * NF)]);
    const int field = o >> 2;
    const int64_t id = r * NF + field;
    if (id != cached) {
      bits = __float_as_uint(field < 3 ? pack_rot(rot9, field, xyz + 3 * r) : pack_rot(rot9, field - 3, normal + 3 * r));
      cached = id;
    }
    return (bits >> (8 * (o & 3))) & 0xffu;
  }
};

// the byte 3, then three int32
struct PlyFaceRecord {
  static constexpr int SIZE = 13;
  const int64_t* faces;
  __device__ __forceinline__ uint32_t byte(int64_t r, int o, int64_t& cached, uint32_t& bits) const {
    if (o == 0) return 3u;
    const int field = (o - 1) >> 2;
    const int64_t id = 3 * r + field;
    if (id != cached) { bits = (uint32_t)faces[id]; cached = id; }
    return (bits >> (8 * ((o - 1) & 3))) & 0xffu;
  }
};

template <typename Rec>
__global__ void pack_words_kernel(Rec rec, int64_t nbytes, int64_t nwords, uint32_t* out) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nwords) return;
  const int64_t b0 = 4 * w;
  int64_t r = b0 / Rec::SIZE, cached = -1;
  int o = (int)(b0 - r * Rec::SIZE);
  uint32_t word = 0, bits = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (b0 + k < nbytes) word |= rec.byte(r, o, cached, bits) << (8 * k);          // behind the last record: the pad bytes stay 0
    if (++o == Rec::SIZE) { o = 0; ++r; }
  }
  out[w] = word;                                                                  // little-endian: byte k of the word is byte 4 w + k
}

template <typename Rec>
static int pack_words(const Rec& rec, int64_t count, void* out, void* stream) {
  const int64_t nbytes = count * Rec::SIZE, nwords = (nbytes + 3) / 4;             // count < 2^31: nwords < 2^34, so fewer than 2^26 blocks
  hipLaunchKernelGGL(pack_words_kernel<Rec>, pack_grid(nwords), dim3(256), 0, (hipStream_t)stream, rec, nbytes, nwords, (uint32_t*)out);
  return ln3d_check_launch();
}

extern "C" int ln3d_pack_ply_vertices(const float* xyz, const float* normal, const float* rgb, const float* rot9, int64_t nv, void* out,
                                      void* stream) {
  if (!xyz || !rgb || !rot9 || !out || !pack_count_ok(nv) || !pack_aligned(out)) return LN3D_ERR_BAD_ARG;
  if (normal) return pack_words(PlyVertexRecord<6>{xyz, normal, rgb, rot9}, nv, out, stream);
  return pack_words(PlyVertexRecord<3>{xyz, nullptr, rgb, rot9}, nv, out, stream);
}

extern "C" int ln3d_pack_ply_faces(const int64_t* faces, int64_t nf, void* out, void* stream) {
  if (!faces || !out || !pack_count_ok(nf) || !pack_aligned(out)) return LN3D_ERR_BAD_ARG;
  return pack_words(PlyFaceRecord{faces}, nf, out, stream);
}

// ------------------------------------------------------------------ GLB: one thread per output float
__global__ void pack_gltf_vertices_kernel(const float* xyz, const float* normal, const float* rgb, const float* rot9, int64_t nv, float* pos,
                                          float* nrm, uint32_t* rgba) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * nv) return;
  const int64_t v = t / 3;
  const int r = (int)(t - 3 * v);
  pos[t] = pack_rot(rot9, r, xyz + 3 * v);
  if (normal) nrm[t] = pack_rot(rot9, r, normal + 3 * v);
  if (t < nv)                                                                      // the first nv threads: one colour word each
    rgba[t] = pack_colour(rgb[3 * t]) | (pack_colour(rgb[3 * t + 1]) << 8) | (pack_colour(rgb[3 * t + 2]) << 16) | 0xff000000u;
}

__global__ void pack_gltf_indices_kernel(const int64_t* faces, int64_t n, uint32_t* idx) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) idx[t] = (uint32_t)faces[t];
}

__global__ void pack_gltf_corners_kernel(const float* xyz, const float* normal, const int64_t* faces, const float* uv, const float* rot9,
                                         int64_t nv, int64_t nf, float* pos, float* nrm, float* uv_out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 9 * nf) return;
  const int64_t c = t / 3;                                                         // the corner; faces is [3 nf] flat
  const int r = (int)(t - 3 * c);
  const int64_t v = faces[c];
  const bool ok = v >= 0 && v < nv;                                                // a precondition; a bad index reads nothing
  pos[t] = ok ? pack_rot(rot9, r, xyz + 3 * v) : 0.0f;
  if (normal) nrm[t] = ok ? pack_rot(rot9, r, normal + 3 * v) : 0.0f;
  if (t < 6 * nf) uv_out[t] = (t & 1) ? 1.0f - uv[t] : uv[t];                      // the first 6 nf threads: (u, 1 - v)
}

extern "C" int ln3d_pack_gltf_vertices(const float* xyz, const float* normal, const float* rgb, const float* rot9, int64_t nv, float* pos_out,
                                       float* nrm_out, void* rgba_out, void* stream) {
  if (!xyz || !rgb || !rot9 || !pos_out || !rgba_out || (normal == nullptr) != (nrm_out == nullptr) || !pack_count_ok(nv) ||
      !pack_aligned(pos_out) || !pack_aligned(nrm_out) || !pack_aligned(rgba_out))
    return LN3D_ERR_BAD_ARG;
  hipLaunchKernelGGL(pack_gltf_vertices_kernel, pack_grid(3 * nv), dim3(256), 0, (hipStream_t)stream, xyz, normal, rgb, rot9, nv, pos_out, nrm_out,
                     (uint32_t*)rgba_out);
  return ln3d_check_launch();
}

extern "C" int ln3d_pack_gltf_indices(const int64_t* faces, int64_t nf, void* idx_out, void* stream) {
  if (!faces || !idx_out || !pack_count_ok(nf) || !pack_aligned(idx_out)) return LN3D_ERR_BAD_ARG;
  hipLaunchKernelGGL(pack_gltf_indices_kernel, pack_grid(3 * nf), dim3(256), 0, (hipStream_t)stream, faces, 3 * nf, (uint32_t*)idx_out);
  return ln3d_check_launch();
}

extern "C" int ln3d_pack_gltf_corners(const float* xyz, const float* normal, const int64_t* faces, const float* uv, const float* rot9, int64_t nv,
                                      int64_t nf, float* pos_out, float* nrm_out, float* uv_out, void* stream) {
  if (!xyz || !faces || !uv || !rot9 || !pos_out || !uv_out || (normal == nullptr) != (nrm_out == nullptr) || !pack_count_ok(nv) ||
      !pack_count_ok(nf) || !pack_aligned(pos_out) || !pack_aligned(nrm_out) || !pack_aligned(uv_out))
    return LN3D_ERR_BAD_ARG;
  hipLaunchKernelGGL(pack_gltf_corners_kernel, pack_grid(9 * nf), dim3(256), 0, (hipStream_t)stream, xyz, normal, faces, uv, rot9, nv, nf, pos_out,
                     nrm_out, uv_out);
  return ln3d_check_launch();
}

// ------------------------------------------------------------------ bounds: minimum and maximum per axis, by order-preserving integer key
// key(x) ascends with x over all floats (negative ones have every bit flipped, the others the sign bit), so min and max are integer
// operations whose result does not depend on the order they are applied in
__device__ __forceinline__ uint32_t bounds_key(float x) {
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float bounds_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

#define BOUNDS_MAX_BLOCKS 1024

__global__ void bounds_init_kernel(uint32_t* key6) {
  if (threadIdx.x < 6) key6[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;     // the identities of min and max
}

__global__ void bounds_reduce_kernel(const float* pos, int64_t n, uint32_t* key6) {
  __shared__ uint32_t part[4][6];                                                  // blocks of 256 threads: 4 wavefronts
  uint32_t k[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {     // terminates: i ascends to n
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const uint32_t q = bounds_key(pos[3 * i + a]);
      k[a] = min(k[a], q); k[3 + a] = max(k[3 + a], q);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      k[a] = min(k[a], (uint32_t)__shfl_xor((int)k[a], off, 64));
      k[3 + a] = max(k[3 + a], (uint32_t)__shfl_xor((int)k[3 + a], off, 64));
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 6; ++a) part[wave][a] = k[a];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int a = threadIdx.x;
    uint32_t q = part[0][a];
    for (int w = 1; w < 4; ++w) q = a < 3 ? min(q, part[w][a]) : max(q, part[w][a]);
    if (a < 3) atomicMin(&key6[a], q); else atomicMax(&key6[a], q);                 // one integer atomic per block and value
  }
}

__global__ void bounds_finish_kernel(uint32_t* key6) {
  if (threadIdx.x < 6) key6[threadIdx.x] = __float_as_uint(bounds_unkey(key6[threadIdx.x]));
}

extern "C" int ln3d_position_bounds(const float* pos, int64_t n, float* bounds6, void* stream) {
  if (!pos || !bounds6 || !pack_count_ok(n) || !pack_aligned(bounds6)) return LN3D_ERR_BAD_ARG;
  uint32_t* key6 = (uint32_t*)bounds6;
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(bounds_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, key6);
  hipLaunchKernelGGL(bounds_reduce_kernel, dim3((unsigned)(blocks < BOUNDS_MAX_BLOCKS ? blocks : BOUNDS_MAX_BLOCKS)), dim3(256), 0,
                     (hipStream_t)stream, pos, n, key6);
  hipLaunchKernelGGL(bounds_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, key6);
  return ln3d_check_launch();
}
