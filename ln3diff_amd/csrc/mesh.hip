// Iso-surface extraction on the sigma grid for gfx950 (the "mesh" step of the sampling drivers:
// nsr/train_util_diffusion.py:208-248 calls PyMCubes 0.1.4 `marching_cubes(sigma[G,G,G], thr)`, a third-party package
// absent from the reference tree: parity with PyMCubes itself is unpinned).  Two extractors share the count / emit passes:
//  * classic marching CUBES (Lorensen & Cline, the algorithm mcubes implements): 256-case triangle table mc_table.h, pinned
//    against scikit-image's classic implementation (tools/gen_mc_table.py, tests/golden/mcubes_classic.npz) - the default;
//  * marching TETRAHEDRA (round 1; no ambiguous cases, watertight by construction) on the Kuhn decomposition of each cell
// (6 tetrahedra around the 0-7 diagonal; face-consistent across cells, no 256-case table): every tetrahedron emits 0, 1
// or 2 triangles; vertices are identified by the grid edge they lie on (key = min_vertex_id * G^3 + max_vertex_id), so the
// host welds them with one unique() and no floating-point comparison.  Two passes (count, emit) around a prefix sum.
// The key needs G^6 < 2^63: LN3D_MESH_MAX_GRID.
#include "common.h"
#include "../../include/ln3d.h"
#include "../../include/ln3d_meshclean.h"
#include "../../include/ln3d_meshsimplify.h"
#include "../../include/ln3d_meshbake.h"
#include "../../include/ln3d_meshquadric.h"
#include "../../include/ln3d_meshsmooth.h"
#include "mc_table.h"

__constant__ int kTet[6][4] = {{0, 1, 3, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 6, 7}, {0, 4, 5, 7}, {0, 1, 5, 7}};

struct MeshP { const float* sigma; int G; float thr; };

__device__ __forceinline__ void cell_corners(const MeshP& p, int64_t cell, float v[8], int64_t gid[8], int& cx, int& cy, int& cz) {
  const int Gc = p.G - 1;
  cz = (int)(cell % Gc); cy = (int)((cell / Gc) % Gc); cx = (int)(cell / ((int64_t)Gc * Gc));   // sigma[x][y][z] (indexing='ij')
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int x = cx + (c & 1), y = cy + ((c >> 1) & 1), z = cz + (c >> 2);
    gid[c] = ((int64_t)x * p.G + y) * p.G + z;
    v[c] = p.sigma[gid[c]];
  }
}

__global__ void mesh_count_kernel(MeshP p, int64_t ncell, int32_t* counts) {
  const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= ncell) return;
  float v[8]; int64_t gid[8]; int cx, cy, cz;
  cell_corners(p, cell, v, gid, cx, cy, cz);
  int n = 0;
#pragma unroll
  for (int t = 0; t < 6; ++t) {
    int in = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) in += v[kTet[t][k]] > p.thr;
    n += (in == 1 || in == 3) ? 1 : (in == 2 ? 2 : 0);
  }
  counts[cell] = n;
}

__device__ __forceinline__ void edge_point(const MeshP& p, const float v[8], const int64_t gid[8], int cx, int cy, int cz, int a, int b,
                                           float out[3], int64_t& key) {
  if (gid[a] > gid[b]) { const int t = a; a = b; b = t; }            // canonical orientation: identical bits from every cell
  // finite inputs take the first form, bit for bit; the selects only replace what would be NaN or off the edge (include/ln3d.h):
  // v[b] - v[a] overflows between two finite values of opposite sign -> the same quotient of the halved values; a +-inf or NaN end
  // -> the vertex sits on the other, finite end; two such ends -> the midpoint
  float t = (p.thr - v[a]) / (v[b] - v[a]);
  if (isinf(v[b] - v[a])) t = (0.5f * p.thr - 0.5f * v[a]) / (0.5f * v[b] - 0.5f * v[a]);
  const bool fa = isfinite(v[a]), fb = isfinite(v[b]);
  t = fa ? (fb ? t : 0.f) : (fb ? 1.f : 0.5f);
  const float ax = cx + (a & 1), ay = cy + ((a >> 1) & 1), az = cz + (a >> 2);
  const float bx = cx + (b & 1), by = cy + ((b >> 1) & 1), bz = cz + (b >> 2);
  out[0] = ax + t * (bx - ax); out[1] = ay + t * (by - ay); out[2] = az + t * (bz - az);
  key = gid[a] * ((int64_t)p.G * p.G * p.G) + gid[b];
}

__global__ void mesh_emit_kernel(MeshP p, int64_t ncell, const int64_t* offsets, float* tri_pos, int64_t* tri_key) {
  const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= ncell) return;
  float v[8]; int64_t gid[8]; int cx, cy, cz;
  cell_corners(p, cell, v, gid, cx, cy, cz);
  int64_t o = cell == 0 ? 0 : offsets[cell - 1];                      // offsets = inclusive prefix sum of counts
  for (int t = 0; t < 6; ++t) {
    int ins[4], outs[4], ni = 0, no = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = kTet[t][k];
      if (v[c] > p.thr) ins[ni++] = c; else outs[no++] = c;
    }
    if (ni == 0 || ni == 4) continue;
    float q[4][3]; int64_t kk[4]; int nq;
    if (ni == 1) { nq = 3; for (int j = 0; j < 3; ++j) edge_point(p, v, gid, cx, cy, cz, ins[0], outs[j], q[j], kk[j]); }
    else if (ni == 3) { nq = 3; for (int j = 0; j < 3; ++j) edge_point(p, v, gid, cx, cy, cz, outs[0], ins[j], q[j], kk[j]); }
    else {
      nq = 4;
      edge_point(p, v, gid, cx, cy, cz, ins[0], outs[0], q[0], kk[0]);
      edge_point(p, v, gid, cx, cy, cz, ins[0], outs[1], q[1], kk[1]);
      edge_point(p, v, gid, cx, cy, cz, ins[1], outs[1], q[2], kk[2]);
      edge_point(p, v, gid, cx, cy, cz, ins[1], outs[0], q[3], kk[3]);
    }
    // orient: normal must point from the inside (sigma > thr) towards the outside
    float ci[3] = {0, 0, 0}, co[3] = {0, 0, 0};
    for (int j = 0; j < ni; ++j) { ci[0] += (ins[j] & 1); ci[1] += ((ins[j] >> 1) & 1); ci[2] += (ins[j] >> 2); }
    for (int j = 0; j < no; ++j) { co[0] += (outs[j] & 1); co[1] += ((outs[j] >> 1) & 1); co[2] += (outs[j] >> 2); }
    const float dir[3] = {co[0] / no - ci[0] / ni, co[1] / no - ci[1] / ni, co[2] / no - ci[2] / ni};
    const int ntri = nq == 3 ? 1 : 2;
    for (int tr = 0; tr < ntri; ++tr) {
      int i0 = 0, i1 = tr == 0 ? 1 : 2, i2 = tr == 0 ? 2 : 3;
      const float e1[3] = {q[i1][0] - q[i0][0], q[i1][1] - q[i0][1], q[i1][2] - q[i0][2]};
      const float e2[3] = {q[i2][0] - q[i0][0], q[i2][1] - q[i0][1], q[i2][2] - q[i0][2]};
      const float nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
      if (nx * dir[0] + ny * dir[1] + nz * dir[2] < 0.f) { const int s = i1; i1 = i2; i2 = s; }
      const int idx[3] = {i0, i1, i2};
      for (int j = 0; j < 3; ++j) {
        tri_pos[(o * 3 + j) * 3 + 0] = q[idx[j]][0]; tri_pos[(o * 3 + j) * 3 + 1] = q[idx[j]][1]; tri_pos[(o * 3 + j) * 3 + 2] = q[idx[j]][2];
        tri_key[o * 3 + j] = kk[idx[j]];
      }
      ++o;
    }
  }
}

// ------------------------------------------------------------------ classic marching cubes
__device__ __forceinline__ int mc_case(const MeshP& p, const float v[8]) {
  int cs = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) cs |= (v[c] > p.thr) << c;
  return cs;
}
__global__ void mcubes_count_kernel(MeshP p, int64_t ncell, int32_t* counts) {
  const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= ncell) return;
  float v[8]; int64_t gid[8]; int cx, cy, cz;
  cell_corners(p, cell, v, gid, cx, cy, cz);
  counts[cell] = kMcCount[mc_case(p, v)];
}
__global__ void mcubes_emit_kernel(MeshP p, int64_t ncell, const int64_t* offsets, float* tri_pos, int64_t* tri_key) {
  const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= ncell) return;
  float v[8]; int64_t gid[8]; int cx, cy, cz;
  cell_corners(p, cell, v, gid, cx, cy, cz);
  const int cs = mc_case(p, v);
  const int nt = kMcCount[cs];
  int64_t o = cell == 0 ? 0 : offsets[cell - 1];
  for (int t = 0; t < nt; ++t, ++o)
    for (int j = 0; j < 3; ++j) {
      const int e = kMcTri[cs][3 * t + j];
      const int ax = e >> 2, b0 = e & 1, b1 = (e >> 1) & 1;
      // edge parallel to axis ax; its other two coordinates (in axis order) are (b0, b1)
      const int a = ax == 0 ? (b0 << 1) | (b1 << 2) : (ax == 1 ? b0 | (b1 << 2) : b0 | (b1 << 1));
      const int b = a | (1 << ax);
      float q[3]; int64_t key;
      edge_point(p, v, gid, cx, cy, cz, a, b, q, key);
      tri_pos[(o * 3 + j) * 3 + 0] = q[0]; tri_pos[(o * 3 + j) * 3 + 1] = q[1]; tri_pos[(o * 3 + j) * 3 + 2] = q[2];
      tri_key[o * 3 + j] = key;
    }
}

static inline dim3 grid_1d(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }                          // one thread per element, blocks of 256
static inline bool count_ok(int64_t n) { return n >= 1 && n <= 0x7fffffffll; }                               // a vertex, face or cluster count

// The four iso-surface passes: one thread per cell of a grid with 2 <= G <= LN3D_MESH_MAX_GRID; `out` are the pass's own buffers.
template <typename... Out>
static int mesh_pass(void (*kernel)(MeshP, int64_t, Out...), const float* sigma, int G, float thr, void* stream, Out... out) {
  if (!sigma || !(out && ...) || G < 2 || G > LN3D_MESH_MAX_GRID) return LN3D_ERR_BAD_ARG;
  const int64_t ncell = (int64_t)(G - 1) * (G - 1) * (G - 1);
  hipLaunchKernelGGL(kernel, grid_1d(ncell), dim3(256), 0, (hipStream_t)stream, MeshP{sigma, G, thr}, ncell, out...);
  return ln3d_check_launch();
}

extern "C" int ln3d_mcubes_count(const float* sigma, int G, float thr, int32_t* counts, void* stream) {
  return mesh_pass(mcubes_count_kernel, sigma, G, thr, stream, counts);
}
extern "C" int ln3d_mcubes_emit(const float* sigma, int G, float thr, const int64_t* offsets, float* tri_pos, int64_t* tri_key, void* stream) {
  return mesh_pass(mcubes_emit_kernel, sigma, G, thr, stream, offsets, tri_pos, tri_key);
}
extern "C" int ln3d_mesh_count(const float* sigma, int G, float thr, int32_t* counts, void* stream) {
  return mesh_pass(mesh_count_kernel, sigma, G, thr, stream, counts);
}
extern "C" int ln3d_mesh_emit(const float* sigma, int G, float thr, const int64_t* offsets, float* tri_pos, int64_t* tri_key, void* stream) {
  return mesh_pass(mesh_emit_kernel, sigma, G, thr, stream, offsets, tri_pos, tri_key);
}

// ------------------------------------------------------------------ mesh clean-up (include/ln3d_meshclean.h)
// Connected components of the welded triangle soup by a lock-free union-find, then exact per-component counts, a keep mask and a
// compaction.  label[] is the parent array: label[x] <= x always, a root has label[x] == x, and the only writes while hooking are
// atomicMin, so every entry only ever decreases.  Every link points to a smaller index, so the root of a finished tree is the smallest
// vertex index of its component: the labels are unique by definition, whatever the schedule.
#define MC_RLX_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

__global__ void meshclean_init_kernel(int32_t* label, int64_t nv) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < nv) label[v] = (int32_t)v;
}

// Unite the sets of u and v.  Labels are read with relaxed agent-scope atomic loads (a plain load may be served from a line of this CU's
// L1 that another CU has since lowered).  A stale value is an earlier parent of the same vertex: whoever replaced it took over the duty
// of uniting it with its replacement (below), so it is still a member of the final component and following it costs steps only.
__device__ __forceinline__ void meshclean_unite(int32_t* label, int32_t u, int32_t v) {
  // terminates: every pass either returns or replaces the pair (hi, lo) by (old, lo) with old < hi and lo < hi, and the two walks only
  // lower their end, so max(u, v) strictly decreases from pass to pass and is bounded below by 0
  for (;;) {
    int32_t p;
    while ((p = MC_RLX_LOAD(&label[u])) < u) u = p;      // terminates: u strictly decreases (label[x] <= x)
    while ((p = MC_RLX_LOAD(&label[v])) < v) v = p;      // terminates: v strictly decreases
    if (u == v) return;
    const int32_t hi = u > v ? u : v, lo = u > v ? v : u;
    const int32_t old = atomicMin(&label[hi], lo);
    if (old == hi || old == lo) return;                  // hi was a root and now hangs under lo / somebody else made the same link
    // hi had been hooked under `old` between our load and the atomic: either lo < old and label[hi] = lo has just overwritten the
    // link hi -> old, or old < lo and hi keeps its parent; both ways the set of `old` still has to be united with lo
    u = old; v = lo;
  }
}

__global__ void meshclean_hook_kernel(const int64_t* faces, int64_t nf, int32_t* label) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nf) return;
  const int32_t a = (int32_t)faces[3 * f], b = (int32_t)faces[3 * f + 1], c = (int32_t)faces[3 * f + 2];
  meshclean_unite(label, a, b);                          // a - b and b - c connect all three; a - c adds nothing
  meshclean_unite(label, b, c);
}

// After the hooking launch every tree is final; the walk may meet entries that other lanes of this launch have already replaced by their
// root, which is the same root.
__global__ void meshclean_flatten_kernel(int32_t* label, int64_t nv) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv) return;
  int32_t r = (int32_t)v, p;
  while ((p = MC_RLX_LOAD(&label[r])) < r) r = p;        // terminates: r strictly decreases
  __hip_atomic_store(&label[v], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void meshclean_zero_kernel(int32_t* nvert, int32_t* nface, unsigned long long* best, int64_t nv) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < nv) { nvert[v] = 0; nface[v] = 0; }
  if (v == 0) *best = 0ull;
}

// One add per distinct destination of the wave: the lanes that share the first pending lane's destination are counted with a ballot and
// added once by that lane, then the next pending destination, and so on.  On a real mesh nearly every lane names the same component (one
// component owns almost every face), so a wave issues one or two atomics instead of 64 on one address.  Every lane of the wave must call
// this; r < 0 = nothing to add.
__device__ __forceinline__ void meshclean_wave_add(int32_t* cnt, int32_t r) {
  unsigned long long todo = __ballot(r >= 0);
  while (todo) {                                         // terminates: every pass clears at least the leading bit of todo
    const int lead = __ffsll((long long)todo) - 1;
    const int32_t r0 = __shfl(r, lead);
    const unsigned long long same = __ballot(r == r0);
    if ((int)(threadIdx.x & 63) == lead) atomicAdd(&cnt[r0], (int32_t)__popcll(same));
    todo &= ~same;
  }
}

__global__ void meshclean_count_kernel(const int64_t* faces, int64_t nf, const int32_t* label, int64_t nv, int32_t* nvert, int32_t* nface) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  meshclean_wave_add(nvert, i < nv ? label[i] : -1);
  meshclean_wave_add(nface, i < nf ? label[faces[3 * i]] : -1);
}

// best = max over the components that own a face of (nface << 32) | (0x7fffffff - root): most faces first, then the smallest root.
// One 64-bit atomic max per wave that holds a candidate.
__global__ void meshclean_best_kernel(const int32_t* label, const int32_t* nface, int64_t nv, unsigned long long* best) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long k = 0ull;
  if (v < nv && label[v] == (int32_t)v && nface[v] > 0) k = ((unsigned long long)(uint32_t)nface[v] << 32) | (unsigned long long)(0x7fffffff - (int32_t)v);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(k, o);
    k = t > k ? t : k;
  }
  if ((threadIdx.x & 63) == 0 && k) atomicMax(best, k);
}

__device__ __forceinline__ int32_t meshclean_keep(const int32_t* nface, int32_t r, int64_t min_faces, int largest_only, int32_t best_root) {
  return ((int64_t)nface[r] >= min_faces && (!largest_only || r == best_root)) ? 1 : 0;
}

__global__ void meshclean_mark_kernel(const int64_t* faces, int64_t nf, const int32_t* label, const int32_t* nface, int64_t nv, int64_t min_faces,
                                      int largest_only, const unsigned long long* best, int32_t* keep_v, int32_t* keep_f) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int32_t best_root = 0x7fffffff - (int32_t)(*best & 0xffffffffull);
  if (i < nv) keep_v[i] = meshclean_keep(nface, label[i], min_faces, largest_only, best_root);
  if (i < nf) keep_f[i] = meshclean_keep(nface, label[faces[3 * i]], min_faces, largest_only, best_root);   // = keep_v[faces[i][0]]
}

__global__ void meshclean_gather_kernel(const uint32_t* verts, const int64_t* faces, const int32_t* keep_v, const int64_t* vprefix, const int32_t* keep_f,
                                        const int64_t* fprefix, int64_t nv, int64_t nf, uint32_t* verts_out, int64_t* faces_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nv && keep_v[i]) {
    const int64_t o = vprefix[i] - 1;
    verts_out[3 * o] = verts[3 * i]; verts_out[3 * o + 1] = verts[3 * i + 1]; verts_out[3 * o + 2] = verts[3 * i + 2];
  }
  if (i < nf && keep_f[i]) {
    const int64_t o = fprefix[i] - 1;
#pragma unroll
    for (int j = 0; j < 3; ++j) faces_out[3 * o + j] = vprefix[faces[3 * i + j]] - 1;
  }
}

static inline bool meshclean_sizes_ok(int64_t nf, int64_t nv) { return count_ok(nv) && count_ok(nf); }

extern "C" int ln3d_mesh_components(const int64_t* faces, int64_t nf, int64_t nv, int32_t* label, void* stream) {
  if (!faces || !label || !meshclean_sizes_ok(nf, nv)) return LN3D_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(meshclean_init_kernel, grid_1d(nv), dim3(256), 0, s, label, nv);
  hipLaunchKernelGGL(meshclean_hook_kernel, grid_1d(nf), dim3(256), 0, s, faces, nf, label);
  hipLaunchKernelGGL(meshclean_flatten_kernel, grid_1d(nv), dim3(256), 0, s, label, nv);
  return ln3d_check_launch();
}

extern "C" int ln3d_mesh_component_counts(const int64_t* faces, int64_t nf, const int32_t* label, int64_t nv, int32_t* nvert, int32_t* nface,
                                          uint64_t* best, void* stream) {
  if (!faces || !label || !nvert || !nface || !best || !meshclean_sizes_ok(nf, nv)) return LN3D_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(meshclean_zero_kernel, grid_1d(nv), dim3(256), 0, s, nvert, nface, (unsigned long long*)best, nv);
  hipLaunchKernelGGL(meshclean_count_kernel, grid_1d(nv > nf ? nv : nf), dim3(256), 0, s, faces, nf, label, nv, nvert, nface);
  hipLaunchKernelGGL(meshclean_best_kernel, grid_1d(nv), dim3(256), 0, s, label, nface, nv, (unsigned long long*)best);
  return ln3d_check_launch();
}

extern "C" int ln3d_mesh_mark(const int64_t* faces, int64_t nf, const int32_t* label, const int32_t* nface, int64_t nv, int64_t min_faces,
                              int largest_only, const uint64_t* best, int32_t* keep_v, int32_t* keep_f, void* stream) {
  if (!faces || !label || !nface || !best || !keep_v || !keep_f || !meshclean_sizes_ok(nf, nv) || min_faces < 0) return LN3D_ERR_BAD_ARG;
  hipLaunchKernelGGL(meshclean_mark_kernel, grid_1d(nv > nf ? nv : nf), dim3(256), 0, (hipStream_t)stream, faces, nf, label, nface, nv,
                     min_faces, largest_only, (const unsigned long long*)best, keep_v, keep_f);
  return ln3d_check_launch();
}

extern "C" int ln3d_mesh_gather(const float* verts, const int64_t* faces, const int32_t* keep_v, const int64_t* vprefix, const int32_t* keep_f,
                                const int64_t* fprefix, int64_t nv, int64_t nf, float* verts_out, int64_t* faces_out, void* stream) {
  if (!verts || !faces || !keep_v || !vprefix || !keep_f || !fprefix || !verts_out || !faces_out || !meshclean_sizes_ok(nf, nv)) return LN3D_ERR_BAD_ARG;
  hipLaunchKernelGGL(meshclean_gather_kernel, grid_1d(nv > nf ? nv : nf), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)verts, faces,
                     keep_v, vprefix, keep_f, fprefix, nv, nf, (uint32_t*)verts_out, faces_out);
  return ln3d_check_launch();
}

// ------------------------------------------------------------------ mesh simplification (include/ln3d_meshsimplify.h)
// Vertex clustering.  Everything but the representatives is integer work; the representatives are sums in one stated order with correctly
// rounded operations, so every output is unique by definition.  The sorts, the unique and the prefix sums between the stages are the caller's.
#define SIMPLIFY_QMAX 2097151ll                          // 2^21 - 1: the largest lattice coordinate and cluster number a key holds

__device__ __forceinline__ int64_t simplify_cell_of(float x, float o, float cell) {
  const float q = floorf(__fdiv_rn(x - o, cell));
  return (int64_t)fminf(fmaxf(q, 0.0f), (float)SIMPLIFY_QMAX);     // fmaxf(NaN, 0) = 0: total
}

__global__ void simplify_keys_kernel(const float* verts, int64_t nv, float ox, float oy, float oz, float cell, int64_t* key) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv) return;
  key[v] = (simplify_cell_of(verts[3 * v], ox, cell) << 42) | (simplify_cell_of(verts[3 * v + 1], oy, cell) << 21) |
           simplify_cell_of(verts[3 * v + 2], oz, cell);
}

// One thread per cluster walks its row of the CSR.  The adds are sequential on purpose (the order is the definition): three independent
// chains per thread, nothing to reassociate and no product to contract.
__global__ void simplify_mean_kernel(const float* verts, const int64_t* order, const int64_t* start, int64_t nc, float* rep) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nc) return;
  const int64_t b = start[k], e = start[k + 1];
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  for (int64_t i = b; i < e; ++i) {                      // terminates: i counts up to e
    const int64_t v = order[i];
    sx += verts[3 * v]; sy += verts[3 * v + 1]; sz += verts[3 * v + 2];
  }
  const float n = (float)(e - b);
  rep[3 * k] = __fdiv_rn(sx, n); rep[3 * k + 1] = __fdiv_rn(sy, n); rep[3 * k + 2] = __fdiv_rn(sz, n);
}

__global__ void simplify_faces_kernel(const int64_t* faces, int64_t nf, const int64_t* cluster, int64_t* cfaces, int64_t* fkey) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nf) return;
  const int64_t a = cluster[faces[3 * f]], b = cluster[faces[3 * f + 1]], c = cluster[faces[3 * f + 2]];
  cfaces[3 * f] = a; cfaces[3 * f + 1] = b; cfaces[3 * f + 2] = c;
  const int64_t lo = min(a, min(b, c)), hi = max(a, max(b, c)), mid = a + b + c - lo - hi;
  fkey[f] = (a == b || b == c || a == c) ? -1ll : ((lo << 42) | (mid << 21) | hi);
}

__global__ void simplify_first_kernel(const int64_t* sorted_key, const int64_t* perm, int64_t nf, int32_t* keep_f) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nf) return;
  const int64_t k = sorted_key[i];
  keep_f[perm[i]] = (k != -1ll && (i == 0 || sorted_key[i - 1] != k)) ? 1 : 0;      // perm is a permutation: every element is written
}

__global__ void simplify_zero_kernel(int32_t* keep_v, int64_t nc) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < nc) keep_v[c] = 0;
}

__global__ void simplify_used_kernel(const int64_t* cfaces, const int32_t* keep_f, int64_t nf, int32_t* keep_v) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nf || !keep_f[f]) return;
  keep_v[cfaces[3 * f]] = 1; keep_v[cfaces[3 * f + 1]] = 1; keep_v[cfaces[3 * f + 2]] = 1;      // every writer stores the same value
}

static inline bool simplify_finite(float x) { return x - x == 0.0f; }

extern "C" int ln3d_simplify_keys(const float* verts, int64_t nv, float origin_x, float origin_y, float origin_z, float cell, int64_t* key,
                                  void* stream) {
  if (!verts || !key || !count_ok(nv) || !simplify_finite(cell) || !(cell > 0.0f) || !simplify_finite(origin_x) ||
      !simplify_finite(origin_y) || !simplify_finite(origin_z)) return LN3D_ERR_BAD_ARG;
  hipLaunchKernelGGL(simplify_keys_kernel, grid_1d(nv), dim3(256), 0, (hipStream_t)stream, verts, nv, origin_x, origin_y, origin_z, cell, key);
  return ln3d_check_launch();
}

extern "C" int ln3d_simplify_mean(const float* verts, const int64_t* order, const int64_t* start, int64_t nv, int64_t nc, float* rep, void* stream) {
  if (!verts || !order || !start || !rep || !count_ok(nv) || !count_ok(nc) || nc > nv) return LN3D_ERR_BAD_ARG;
  if (nc > SIMPLIFY_QMAX + 1) return LN3D_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(simplify_mean_kernel, grid_1d(nc), dim3(256), 0, (hipStream_t)stream, verts, order, start, nc, rep);
  return ln3d_check_launch();
}

extern "C" int ln3d_simplify_faces(const int64_t* faces, int64_t nf, const int64_t* cluster, int64_t nv, int64_t nc, int64_t* cfaces, int64_t* fkey,
                                   void* stream) {
  if (!faces || !cluster || !cfaces || !fkey || !count_ok(nf) || !count_ok(nv) || !count_ok(nc) || nc > nv)
    return LN3D_ERR_BAD_ARG;
  if (nc > SIMPLIFY_QMAX + 1) return LN3D_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(simplify_faces_kernel, grid_1d(nf), dim3(256), 0, (hipStream_t)stream, faces, nf, cluster, cfaces, fkey);
  return ln3d_check_launch();
}

extern "C" int ln3d_simplify_first(const int64_t* sorted_key, const int64_t* perm, int64_t nf, int32_t* keep_f, void* stream) {
  if (!sorted_key || !perm || !keep_f || !count_ok(nf)) return LN3D_ERR_BAD_ARG;
  hipLaunchKernelGGL(simplify_first_kernel, grid_1d(nf), dim3(256), 0, (hipStream_t)stream, sorted_key, perm, nf, keep_f);
  return ln3d_check_launch();
}

extern "C" int ln3d_simplify_used(const int64_t* cfaces, const int32_t* keep_f, int64_t nf, int64_t nc, int32_t* keep_v, void* stream) {
  if (!cfaces || !keep_f || !keep_v || !count_ok(nf) || !count_ok(nc)) return LN3D_ERR_BAD_ARG;
  if (nc > SIMPLIFY_QMAX + 1) return LN3D_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(simplify_zero_kernel, grid_1d(nc), dim3(256), 0, s, keep_v, nc);
  hipLaunchKernelGGL(simplify_used_kernel, grid_1d(nf), dim3(256), 0, s, cfaces, keep_f, nf, keep_v);
  return ln3d_check_launch();
}

// ------------------------------------------------------------------ texture baking (include/ln3d_meshbake.h)
// The per-face atlas: which face owns a texel is integer work, the point on that face is six individually rounded fp32 operations per axis,
// so both outputs are unique by definition.  (__fmul_rn and __fadd_rn are plain operators in this compiler's headers and a product next to
// a sum is contracted into an fma, which rounds once instead of twice: the expression stands under `fp contract(off)` instead.)  The field is evaluated at the points
// by the caller, through ln3d_query_points; the pack below turns its colours into the texture.
#define BAKE_MAX_T 8192

__device__ __forceinline__ float bake_affine(float v0, float v1, float v2, float s, float t) {
#pragma clang fp contract(off)
  const float e1 = v1 - v0, e2 = v2 - v0;
  const float se1 = s * e1, te2 = t * e2;
  const float a = v0 + se1;
  return a + te2;
}

__global__ void bake_points_kernel(const float* verts, const int64_t* faces, int nf, int T, int n, int c, float* points, int32_t* owner) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);                       // T * T <= 2^26
  if (i >= T * T) return;
  const int x = i % T, y = i / T;
  int f = -1, a = 0, b = 0;
  if (x < n * c && y < n * c) {
    const int kx = x / c, ky = y / c;
    a = x - kx * c; b = y - ky * c;
    f = 2 * (ky * n + kx) + (a + b <= c - 1 ? 0 : 1);                               // 2 n^2 <= 2^23
    if (f >= nf) f = -1;
  }
  owner[i] = f;
  float* p = points + 3 * (int64_t)i;
  if (f < 0) { p[0] = 0.0f; p[1] = 0.0f; p[2] = 0.0f; return; }
  const bool lower = (f & 1) == 0;
  const float d = (float)(c - 3);
  const float s = __fdiv_rn((float)(lower ? a : c - 1 - a), d), t = __fdiv_rn((float)(lower ? b : c - 1 - b), d);
  const float* v0 = verts + 3 * faces[3 * (int64_t)f];
  const float* v1 = verts + 3 * faces[3 * (int64_t)f + 1];
  const float* v2 = verts + 3 * faces[3 * (int64_t)f + 2];
#pragma unroll
  for (int k = 0; k < 3; ++k)
    p[k] = bake_affine(v0[k], v1[k], v2[k], s, t);
}

__global__ void bake_pack_kernel(const float* rgb, const int32_t* owner, int64_t P, int fill, uint8_t* tex) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  const bool own = owner[i] >= 0;
#pragma unroll
  for (int k = 0; k < 3; ++k)                                                       // fmaxf(NaN, 0) = 0: a NaN colour is 0
    tex[3 * i + k] = own ? (uint8_t)(int)(fminf(fmaxf(rgb[3 * i + k], 0.0f), 1.0f) * 255.0f) : (uint8_t)fill;
}

extern "C" int ln3d_bake_points(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, int T, int n, int c, float* points,
                                int32_t* owner, void* stream) {
  if (!verts || !faces || !points || !owner || !count_ok(nv) || !count_ok(nf) || T < 4 || T > BAKE_MAX_T || n < 1 || c < 4 ||
      (int64_t)n * c > T || nf > 2 * (int64_t)n * n) return LN3D_ERR_BAD_ARG;
  hipLaunchKernelGGL(bake_points_kernel, grid_1d((int64_t)T * T), dim3(256), 0, (hipStream_t)stream, verts, faces, (int)nf, T, n, c, points, owner);
  return ln3d_check_launch();
}

extern "C" int ln3d_bake_pack(const float* rgb, const int32_t* owner, int64_t P, int fill, uint8_t* tex, void* stream) {
  if (!rgb || !owner || !tex || !count_ok(P) || P > (int64_t)BAKE_MAX_T * BAKE_MAX_T || fill < 0 || fill > 255) return LN3D_ERR_BAD_ARG;
  hipLaunchKernelGGL(bake_pack_kernel, grid_1d(P), dim3(256), 0, (hipStream_t)stream, rgb, owner, P, fill, tex);
  return ln3d_check_launch();
}

// ------------------------------------------------------------------ mesh smoothing (include/ln3d_meshsmooth.h)
// Taubin's lambda | mu passes over the vertex adjacency.  The adjacency is integer work (edge keys, the caller's unique and sort, half-edges);
// a pass is a gather of one thread per vertex over its CSR row in ascending neighbour index, a short chain of individually rounded fp32
// operations, so every output is unique by definition.  The array a pass gathers from (12 bytes a vertex) stays in L2.
__global__ void smooth_edge_keys_kernel(const int64_t* faces, int64_t nf, int64_t* key) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nf) return;
  const int64_t v[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int64_t a = v[j], b = v[(j + 1) % 3];
    key[3 * f + j] = a == b ? -1ll : ((min(a, b) << 32) | max(a, b));
  }
}

__global__ void smooth_halfedges_kernel(const int64_t* edge, const int64_t* count, int64_t ne, int64_t nv, int64_t* dkey, int32_t* pinned) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ne) return;
  const int64_t k = edge[e], lo = k >> 32, hi = k & 0xffffffffll;
  dkey[2 * e] = k; dkey[2 * e + 1] = (hi << 32) | lo;
  if (count[e] == 1) {                                   // a boundary edge; every writer stores the same value
    if (lo >= 0 && lo < nv) pinned[lo] = 1;
    if (hi < nv) pinned[hi] = 1;
  }
}

// x + f * (s / d - x) with four roundings (as bake_affine: the product next to the sum would otherwise be contracted into an fma)
__device__ __forceinline__ float smooth_move(float x, float s, float d, float f) {
#pragma clang fp contract(off)
  const float m = __fdiv_rn(s, d);
  const float e = m - x;
  const float fe = f * e;
  return x + fe;
}

__global__ void smooth_step_kernel(const float* vin, const int64_t* start, const int32_t* nbr, const int32_t* pinned, int64_t nv, int64_t nh,
                                   float factor, float* vout) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nv) return;
  const float x = vin[3 * i], y = vin[3 * i + 1], z = vin[3 * i + 2];
  const int64_t b = max(start[i], (int64_t)0), e = min(start[i + 1], nh);
  if (pinned[i] || e <= b) { vout[3 * i] = x; vout[3 * i + 1] = y; vout[3 * i + 2] = z; return; }
  int64_t j = nbr[b];
  float sx = vin[3 * j], sy = vin[3 * j + 1], sz = vin[3 * j + 2];
  for (int64_t k = b + 1; k < e; ++k) {                  // terminates: k counts up to e; sequential on purpose (the order is the definition)
    j = nbr[k];
    sx += vin[3 * j]; sy += vin[3 * j + 1]; sz += vin[3 * j + 2];
  }
  const float d = (float)(e - b);
  vout[3 * i] = smooth_move(x, sx, d, factor); vout[3 * i + 1] = smooth_move(y, sy, d, factor); vout[3 * i + 2] = smooth_move(z, sz, d, factor);
}

extern "C" int ln3d_smooth_edge_keys(const int64_t* faces, int64_t nf, int64_t* key, void* stream) {
  if (!faces || !key || !count_ok(nf)) return LN3D_ERR_BAD_ARG;
  hipLaunchKernelGGL(smooth_edge_keys_kernel, grid_1d(nf), dim3(256), 0, (hipStream_t)stream, faces, nf, key);
  return ln3d_check_launch();
}

extern "C" int ln3d_smooth_halfedges(const int64_t* edge, const int64_t* count, int64_t ne, int64_t nv, int64_t* dkey, int32_t* pinned, void* stream) {
  if (!edge || !count || !dkey || !pinned || !count_ok(ne) || !count_ok(nv)) return LN3D_ERR_BAD_ARG;
  hipLaunchKernelGGL(smooth_halfedges_kernel, grid_1d(ne), dim3(256), 0, (hipStream_t)stream, edge, count, ne, nv, dkey, pinned);
  return ln3d_check_launch();
}

extern "C" int ln3d_smooth_step(const float* verts_in, const int64_t* start, const int32_t* nbr, const int32_t* pinned, int64_t nv, int64_t n_halfedges,
                                float factor, float* verts_out, void* stream) {
  if (!verts_in || !start || !nbr || !pinned || !verts_out || !count_ok(nv) || !count_ok(n_halfedges) || !simplify_finite(factor))
    return LN3D_ERR_BAD_ARG;
  const uintptr_t in = (uintptr_t)verts_in, out = (uintptr_t)verts_out, bytes = (uintptr_t)nv * 3 * sizeof(float);
  if ((in <= out ? out - in : in - out) < bytes) return LN3D_ERR_BAD_ARG;      // a pass reads the previous coordinates only
  hipLaunchKernelGGL(smooth_step_kernel, grid_1d(nv), dim3(256), 0, (hipStream_t)stream, verts_in, start, nbr, pinned, nv, n_halfedges, factor,
                     verts_out);
  return ln3d_check_launch();
}

// ------------------------------------------------------------------ quadric-error placement (include/ln3d_meshquadric.h)
// The opt-in second placement rule of the simplification.  The incidence is integer work (pair keys, the caller's sort and searchsorted); the
// placement is one wavefront per cluster: 64 lanes gather 64 faces' corners at a time (at 45 faces per cluster on average one round; one lane
// per cluster would walk 45 dependent gathers in a row and leave most of the device idle at 10^4 clusters), every lane sums its faces in
// ascending order and a butterfly of fixed shape adds the 64 partial sums, so the bits depend on nothing but the input.
#define QUADRIC_NONE 0x7fffffffffffffffll
#define QUADRIC_FACE_MASK 0x7fffffffll

__global__ void quadric_pairs_kernel(const int64_t* cfaces, int64_t nf, int64_t* key) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nf) return;
  const int64_t a = cfaces[3 * f], b = cfaces[3 * f + 1], c = cfaces[3 * f + 2];
  key[3 * f] = (a << 31) | f;
  key[3 * f + 1] = b != a ? ((b << 31) | f) : QUADRIC_NONE;
  key[3 * f + 2] = (c != a && c != b) ? ((c << 31) | f) : QUADRIC_NONE;
}

// p_l <- p_l + p_(l xor s) for s = 32 ... 1: every lane ends with the same bits (the addition commutes), the whole wave takes part
__device__ __forceinline__ float quadric_wave_sum(float v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

__global__ __launch_bounds__(256) void quadric_place_kernel(const float* verts, const int64_t* faces, int64_t nf, const int64_t* skey,
                                                            int64_t npairs, const int64_t* start, int64_t nc, const float* rep_mean, float ox,
                                                            float oy, float oz, float cell, const int64_t* ckey, float eps, float* rep_out,
                                                            int32_t* placed) {
  const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);      // four waves of 64 per block, one cluster each
  if (k >= nc) return;                                                 // wave-uniform: the shuffles below see whole waves
  const int lane = threadIdx.x & 63;
  const float mx = rep_mean[3 * k], my = rep_mean[3 * k + 1], mz = rep_mean[3 * k + 2];
  const int64_t b = max(start[k], (int64_t)0), e = min(start[k + 1], npairs);
  float a00 = 0.0f, a01 = 0.0f, a02 = 0.0f, a11 = 0.0f, a12 = 0.0f, a22 = 0.0f, r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
  for (int64_t i = b + lane; i < e; i += 64) {                         // terminates: i counts up to e
    const int64_t key = skey[i], f = key & QUADRIC_FACE_MASK;
    if ((key >> 31) != k || f >= nf) continue;                         // not a key of this row: skipped, never followed
    const int64_t v0 = faces[3 * f], v1 = faces[3 * f + 1], v2 = faces[3 * f + 2];
    const float ax = verts[3 * v0] - mx, ay = verts[3 * v0 + 1] - my, az = verts[3 * v0 + 2] - mz;
    const float ux = (verts[3 * v1] - mx) - ax, uy = (verts[3 * v1 + 1] - my) - ay, uz = (verts[3 * v1 + 2] - mz) - az;
    const float wx = (verts[3 * v2] - mx) - ax, wy = (verts[3 * v2 + 1] - my) - ay, wz = (verts[3 * v2 + 2] - mz) - az;
    const float nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    const float d = nx * ax + ny * ay + nz * az;
    a00 += nx * nx; a01 += nx * ny; a02 += nx * nz; a11 += ny * ny; a12 += ny * nz; a22 += nz * nz;
    r0 += d * nx; r1 += d * ny; r2 += d * nz;
  }
  a00 = quadric_wave_sum(a00); a01 = quadric_wave_sum(a01); a02 = quadric_wave_sum(a02);
  a11 = quadric_wave_sum(a11); a12 = quadric_wave_sum(a12); a22 = quadric_wave_sum(a22);
  r0 = quadric_wave_sum(r0); r1 = quadric_wave_sum(r1); r2 = quadric_wave_sum(r2);
  if (lane != 0) return;
  float x = mx, y = my, z = mz;
  int ok = 0;
  const float tr = a00 + a11 + a22;
  if (tr > 0.0f) {                                                     // false for NaN too
    const float lam = eps * tr;
    const float d0 = a00 + lam;                                        // LDL^T of A + lam I: d0, d1, d2 >= lam up to rounding
    const float l10 = a01 / d0, l20 = a02 / d0;
    const float d1 = (a11 + lam) - l10 * a01;
    const float t12 = a12 - l20 * a01;
    const float l21 = t12 / d1;
    const float d2 = (a22 + lam) - l20 * a02 - l21 * t12;
    const float y1 = r1 - l10 * r0;
    const float y2 = r2 - l20 * r0 - l21 * y1;
    const float dz = y2 / d2;
    const float dy = y1 / d1 - l21 * dz;
    const float dx = r0 / d0 - l10 * dy - l20 * dz;
    const float px = mx + dx, py = my + dy, pz = mz + dz;
    const int64_t ck = ckey[k];
    const float qx = (float)((ck >> 42) & SIMPLIFY_QMAX), qy = (float)((ck >> 21) & SIMPLIFY_QMAX), qz = (float)(ck & SIMPLIFY_QMAX);
    ok = px - px == 0.0f && py - py == 0.0f && pz - pz == 0.0f &&
         px >= fmaf(qx, cell, ox) && px <= fmaf(qx + 1.0f, cell, ox) && py >= fmaf(qy, cell, oy) && py <= fmaf(qy + 1.0f, cell, oy) &&
         pz >= fmaf(qz, cell, oz) && pz <= fmaf(qz + 1.0f, cell, oz);
    if (ok) { x = px; y = py; z = pz; }
  }
  rep_out[3 * k] = x; rep_out[3 * k + 1] = y; rep_out[3 * k + 2] = z;  // the mean's own bits when the placement is refused
  placed[k] = ok;
}

extern "C" int ln3d_quadric_pairs(const int64_t* cfaces, int64_t nf, int64_t nc, int64_t* pair_key, void* stream) {
  if (!cfaces || !pair_key || !count_ok(nf) || !count_ok(nc)) return LN3D_ERR_BAD_ARG;
  if (nc > SIMPLIFY_QMAX + 1) return LN3D_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(quadric_pairs_kernel, grid_1d(nf), dim3(256), 0, (hipStream_t)stream, cfaces, nf, pair_key);
  return ln3d_check_launch();
}

extern "C" int ln3d_quadric_place(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const int64_t* sorted_pair_key, int64_t npairs,
                                  const int64_t* start, int64_t nc, const float* rep_mean, float origin_x, float origin_y, float origin_z,
                                  float cell, const int64_t* cluster_cell_key, float eps, float* rep_out, int32_t* placed, void* stream) {
  if (!verts || !faces || !sorted_pair_key || !start || !rep_mean || !cluster_cell_key || !rep_out || !placed || !count_ok(nv) ||
      !count_ok(nf) || !count_ok(nc) || npairs < 1 || npairs > 3 * nf || nc > nv || !simplify_finite(cell) || !(cell > 0.0f) ||
      !simplify_finite(origin_x) || !simplify_finite(origin_y) || !simplify_finite(origin_z) || !simplify_finite(eps) || !(eps > 0.0f) ||
      !(eps <= 1.0f))
    return LN3D_ERR_BAD_ARG;
  if (nc > SIMPLIFY_QMAX + 1) return LN3D_ERR_UNSUPPORTED;
  const uintptr_t in = (uintptr_t)rep_mean, out = (uintptr_t)rep_out, bytes = (uintptr_t)nc * 3 * sizeof(float);
  if (in != out && (in < out ? out - in : in - out) < bytes) return LN3D_ERR_BAD_ARG;      // in place, or apart: a cluster reads its own mean only
  hipLaunchKernelGGL(quadric_place_kernel, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, (hipStream_t)stream, verts, faces, nf, sorted_pair_key,
                     npairs, start, nc, rep_mean, origin_x, origin_y, origin_z, cell, cluster_cell_key, eps, rep_out, placed);
  return ln3d_check_launch();
}
