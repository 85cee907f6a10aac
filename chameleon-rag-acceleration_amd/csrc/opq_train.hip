// gfx950 (MI355X, CDNA4) kernels of the resident OPQ trainer (faiss_amd.OPQMatrix.train_device).
//
// k_opq_assign: the Lloyd assignment (and the final encode) of all M sub-quantizers in one
// launch.  A workgroup takes one sub-quantizer m and kOpqAssignRows rows: it stages the
// [256][dsub] sub-codebook in LDS once, then walks its rows 256 * RPT at a time, lanes as rows,
// a lane's RPT rows of dsub components in registers.  Every lane of a wave reads the same
// centroid element at the same time (an LDS broadcast, no bank conflict), and one read serves
// the lane's RPT rows.  The distance is tree<K_L2> (Faiss's fvec_L2sqr order, restated below as
// in pq_flat.hip) and the comparison keeps the first minimum: launch_pq_encode_flat's codes bit
// for bit.  dsub is a template parameter so that the rows stay in registers.
//
// k_opq_labels: labels[r * M + m] = m * 256 + code, the clusters of the [n * M][dsub] view of the
// rotated rows, for launch_km_pass.
//
// k_opq_cross: C [d][d2] = sum_r xt_r (x) cb[code_r] with the decode fused in (rec is never
// written).  A workgroup takes one 64 x 64 tile (I over d, J over d2) and one row chunk and walks
// the chunk kOpqKr rows at a time.  Per step block A (32 rows x 64 columns of xt) is staged in LDS
// row-major as in k_pca_scatter, and block B is gathered on the way in: element (r, c) is
// cb[m][codes[r][m]][c - m dsub], m = c / dsub, read from the codebook in L2 (d2 KiB in all); a
// thread's 8 columns are the same in every step, so their (m, offset) are computed once.  Rows past
// the chunk and columns past d / d2 are staged as 0.  The product runs on v_mfma_f32_16x16x4_f32
// with the row index as K exactly as k_pca_scatter's: wave w owns tile rows 16 w .. 16 w + 15
// against all 64 columns, an ascending-k chain, so a chunk's partial is the sum over its rows in
// row order.  Partial tiles go to the workspace.
//
// k_opq_cross_reduce: adds the partial tiles of every chunk in chunk order (one fp32 chain per
// element).  No floating-point atomics anywhere.
// Compiled with -ffp-contract=off like the rest of the library.
#include <stdint.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "opq_train.h"
#include "pq_flat.h"

namespace chivf {

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

inline unsigned nblk(int64_t n, int t) { return (unsigned)std::max<int64_t>(1, (n + t - 1) / t); }

// |x - y|^2 over D components in the Faiss-1.7.1 AVX reduction order (tree<K_L2> of pq_flat.hip
// with d known at compile time: every index below is a constant, x stays in registers)
template <int D>
__device__ __forceinline__ float tree_l2(const float (&x)[D], const float* __restrict__ y) {
  float a8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  constexpr int D8 = D / 8 * 8;
#pragma unroll
  for (int i = 0; i < D8; i += 8) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float t = x[i + j] - y[i + j];
      a8[j] = a8[j] + t * t;
    }
  }
  float a4[4];
#pragma unroll
  for (int j = 0; j < 4; j++) a4[j] = a8[j + 4] + a8[j];
  constexpr int D4 = D8 + ((D - D8) >= 4 ? 4 : 0);
  if constexpr (D4 > D8) {  // the 4-wide remainder
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float t = x[D8 + j] - y[D8 + j];
      a4[j] = a4[j] + t * t;
    }
  }
#pragma unroll
  for (int j = 0; j < D - D4; j++) {  // the masked tail
    const float t = x[D4 + j] - y[D4 + j];
    a4[j] = a4[j] + t * t;
  }
  const float h0 = a4[0] + a4[1];
  const float h1 = a4[2] + a4[3];
  return h0 + h1;
}

// rows a lane holds at once: RPT * DSUB <= 64 registers
template <int DSUB>
constexpr int assign_rpt() {
  return DSUB <= 16 ? 4 : DSUB <= 32 ? 2 : 1;
}

// grid: (row tile, m) with m fastest (the workgroups that run together share their rows' lines)
template <int DSUB>
__global__ __launch_bounds__(256) void k_opq_assign(const float* __restrict__ xp, int64_t n, int d2,
                                                    const float* __restrict__ cb, int M,
                                                    uint8_t* __restrict__ codes) {
  constexpr int RPT = assign_rpt<DSUB>();
  __shared__ __attribute__((aligned(16))) float cbs[256 * DSUB];
  const int tid = threadIdx.x;
  const int64_t tile = blockIdx.x / M;
  const int m = (int)(blockIdx.x - tile * M);
  const float* __restrict__ src = cb + (int64_t)m * 256 * DSUB;
  for (int i = tid; i < 256 * DSUB; i += 256) cbs[i] = src[i];
  __syncthreads();
  const int64_t r0 = tile * kOpqAssignRows, r1 = min(n, r0 + kOpqAssignRows);
  for (int64_t t0 = r0; t0 < r1; t0 += 256 * RPT) {
    float xr[RPT][DSUB];
#pragma unroll
    for (int i = 0; i < RPT; i++) {
      // rows past the tile re-read its last row (their codes are not written)
      const float* __restrict__ p = xp + min(t0 + i * 256 + tid, r1 - 1) * d2 + m * DSUB;
#pragma unroll
      for (int u = 0; u < DSUB; u++) xr[i][u] = p[u];
    }
    int best[RPT];
    float bd[RPT];
#pragma unroll
    for (int i = 0; i < RPT; i++) {
      best[i] = 0;
      bd[i] = 0.f;
    }
    for (int j = 0; j < 256; j++) {
      const float* c = cbs + j * DSUB;
#pragma unroll
      for (int i = 0; i < RPT; i++) {
        const float dd = tree_l2<DSUB>(xr[i], c);
        if (j == 0 || dd < bd[i]) {
          bd[i] = dd;
          best[i] = j;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < RPT; i++) {
      const int64_t row = t0 + i * 256 + tid;
      if (row < r1) codes[row * M + m] = (uint8_t)best[i];
    }
  }
}

__global__ __launch_bounds__(256) void k_opq_labels(const uint8_t* __restrict__ codes, int64_t nm, int M,
                                                    int64_t* __restrict__ labels) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nm) return;
  labels[i] = (int64_t)(i % M) * 256 + codes[i];
}

__global__ __launch_bounds__(256) void k_opq_center(const float* __restrict__ x, int64_t nd, int d,
                                                    const float* __restrict__ mean, float* __restrict__ xt) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nd) return;
  xt[i] = x[i] - mean[i % d];
}

constexpr int T = kOpqTile, KR = kOpqKr;
constexpr int TS = T + 16;  // row stride of a staged block (floats), as in pca_moments.hip: the two rows
                            // a 32-lane group reads in an MFMA operand fall on disjoint banks
static_assert(T == 64 && KR == 32, "the staging below is written for these");

// four consecutive floats of a row at column c, zeros past d (load4 of pca_moments.hip)
template <bool VEC>
__device__ __forceinline__ f4 load4(const float* __restrict__ row, int c, int d) {
  f4 v;
  if constexpr (VEC) {
    v = *reinterpret_cast<const f4*>(row + min(c, d - 4));
    if (c >= d) v = f4{0.f, 0.f, 0.f, 0.f};
  } else {
    const float a = row[min(c, d - 1)], b = row[min(c + 1, d - 1)], e = row[min(c + 2, d - 1)],
                g = row[min(c + 3, d - 1)];
    v.x = c < d ? a : 0.f;
    v.y = c + 1 < d ? b : 0.f;
    v.z = c + 2 < d ? e : 0.f;
    v.w = c + 3 < d ? g : 0.f;
  }
  return v;
}

// grid: tiles fastest (the workgroups that run together share a row chunk), chunks slowest.
// LDS: 2 buffers x 2 blocks x 32 x 80 floats = 40 KiB.
template <bool VEC>
__global__ __launch_bounds__(256, 2) void k_opq_cross(const float* __restrict__ xt, int64_t n, int d,
                                                      const uint8_t* __restrict__ codes,
                                                      const float* __restrict__ cb, int d2, int M,
                                                      int64_t chunk_rows, int tbj, int tiles,
                                                      float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float Ls[2][2][KR * TS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, k4 = lane >> 4;
  const int chunk = blockIdx.x / tiles, tile = blockIdx.x - chunk * tiles;
  const int I = tile / tbj, J = tile - I * tbj;
  const int64_t r0 = (int64_t)chunk * chunk_rows, r1 = min(n, r0 + chunk_rows);
  const int dsub = d2 / M;

  // staging: thread t takes row t >> 3 of the step, columns 8 (t & 7) .. + 7 of block A and of block B
  const int sr = tid >> 3, sc = (tid & 7) * 8;
  const int cA = I * T + sc, cB = J * T + sc;
  int bm[8], bo[8];  // a B column's sub-quantizer, and its element of that sub-quantizer's codeword 0
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int c = min(cB + i, d2 - 1);
    bm[i] = c / dsub;
    bo[i] = bm[i] * 256 * dsub + (c - bm[i] * dsub);
  }
  f4 vA[2];
  float vB[8];
  bool live = false;  // the thread's row of the fetched step is inside the chunk
  auto fetch = [&](int64_t rr) __attribute__((always_inline)) {
    live = rr + sr < r1;
    const int64_t row = min(rr + sr, r1 - 1);
    const float* xrow = xt + row * d;
#pragma unroll
    for (int i = 0; i < 2; i++) vA[i] = load4<VEC>(xrow, cA + 4 * i, d);
    const uint8_t* crow = codes + row * M;
#pragma unroll
    for (int i = 0; i < 8; i++) vB[i] = cb[bo[i] + (int)crow[bm[i]] * dsub];
  };
  auto stage = [&](int b) __attribute__((always_inline)) {
    const f4 z = f4{0.f, 0.f, 0.f, 0.f};
    f4* pa = reinterpret_cast<f4*>(&Ls[b][0][sr * TS + sc]);
#pragma unroll
    for (int i = 0; i < 2; i++) pa[i] = live ? vA[i] : z;
    float* pb = &Ls[b][1][sr * TS + sc];
#pragma unroll
    for (int i = 0; i < 8; i++) pb[i] = (live && cB + i < d2) ? vB[i] : 0.f;
  };

  f4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; t++) acc[t] = f4{0.f, 0.f, 0.f, 0.f};

  fetch(r0);
  stage(0);
  __syncthreads();
  int b = 0;
  for (int64_t rr = r0; rr < r1; rr += KR, b ^= 1) {
    const bool more = rr + KR < r1;
    if (more) fetch(rr + KR);  // in flight during this step's MFMAs
    const float* A = &Ls[b][0][wave * 16 + i16];
    const float* B = &Ls[b][1][i16];
#pragma unroll
    for (int j = 0; j < KR / 4; j++) {
      const int kk = (4 * j + k4) * TS;
      const float av = A[kk];
#pragma unroll
      for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, B[kk + t * 16], acc[t], 0, 0, 0);
    }
    if (more) stage(b ^ 1);
    __syncthreads();
  }

  // acc[t][r] = element (16 wave + 4 k4 + r, 16 t + i16) of the tile
  float* out = part + ((int64_t)chunk * tiles + tile) * (T * T);
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int r = 0; r < 4; r++) out[(wave * 16 + k4 * 4 + r) * T + t * 16 + i16] = acc[t][r];
}

// grid: tiles x 16; a thread adds one element's partials in chunk order
__global__ __launch_bounds__(256) void k_opq_cross_reduce(const float* __restrict__ part, int chunks, int tiles,
                                                          int tbj, int d, int d2, float* __restrict__ C) {
  const int tile = blockIdx.x >> 4;
  const int e = (blockIdx.x & 15) * 256 + threadIdx.x;  // element of the tile: row e >> 6, column e & 63
  const int I = tile / tbj, J = tile - I * tbj;
  const int gi = I * T + (e >> 6), gj = J * T + (e & 63);
  if (gi >= d || gj >= d2) return;
  const float* p = part + (int64_t)tile * (T * T) + e;
  float s = 0.f;
  for (int c = 0; c < chunks; c++) s += p[(int64_t)c * tiles * (T * T)];
  C[(int64_t)gi * d2 + gj] = s;
}

template <int DSUB>
void assign_launch(const float* xp, int64_t n, int d2, const float* cb, int M, uint8_t* codes, hipStream_t s) {
  const int64_t groups = (n + kOpqAssignRows - 1) / kOpqAssignRows * M;
  hipLaunchKernelGGL(k_opq_assign<DSUB>, dim3((unsigned)groups), dim3(256), 0, s, xp, n, d2, cb, M, codes);
}

}  // namespace

bool opq_assign_in_lds(int dsub) {
  switch (dsub) {
    case 1: case 2: case 3: case 4: case 6: case 8: case 12: case 16: case 24: case 32: case 48: case 64:
      return true;
    default:
      return false;
  }
}

void launch_opq_assign(const float* xp, int64_t n, int d2, const float* cb, int M, uint8_t* codes, hipStream_t s) {
  if (n <= 0) return;
  switch (d2 / M) {
    case 1: return assign_launch<1>(xp, n, d2, cb, M, codes, s);
    case 2: return assign_launch<2>(xp, n, d2, cb, M, codes, s);
    case 3: return assign_launch<3>(xp, n, d2, cb, M, codes, s);
    case 4: return assign_launch<4>(xp, n, d2, cb, M, codes, s);
    case 6: return assign_launch<6>(xp, n, d2, cb, M, codes, s);
    case 8: return assign_launch<8>(xp, n, d2, cb, M, codes, s);
    case 12: return assign_launch<12>(xp, n, d2, cb, M, codes, s);
    case 16: return assign_launch<16>(xp, n, d2, cb, M, codes, s);
    case 24: return assign_launch<24>(xp, n, d2, cb, M, codes, s);
    case 32: return assign_launch<32>(xp, n, d2, cb, M, codes, s);
    case 48: return assign_launch<48>(xp, n, d2, cb, M, codes, s);
    case 64: return assign_launch<64>(xp, n, d2, cb, M, codes, s);
    default: return launch_pq_encode_flat(xp, n, d2, cb, M, codes, s);  // one thread per (row, m), the codebook from memory
  }
}

void launch_opq_labels(const uint8_t* codes, int64_t n, int M, int64_t* labels, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_opq_labels, dim3(nblk(n * M, 256)), dim3(256), 0, s, codes, n * M, M, labels);
}

void launch_opq_center(const float* x, int64_t n, int d, const float* mean, float* xt, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_opq_center, dim3(nblk(n * d, 256)), dim3(256), 0, s, x, n * d, d, mean, xt);
}

OpqPlan opq_plan(int64_t n, int d, int d2, int64_t set_rows) {
  OpqPlan p;
  p.tbi = (d + T - 1) / T;
  p.tbj = (d2 + T - 1) / T;
  p.tiles = p.tbi * p.tbj;
  int64_t rows;
  if (set_rows > 0) {
    rows = set_rows;
  } else {
    const int64_t want = std::max<int64_t>(1, (kOpqTargetGroups + p.tiles - 1) / p.tiles);
    rows = std::max<int64_t>((std::max<int64_t>(n, 1) + want - 1) / want, kOpqMinChunkRows);
  }
  rows = (rows + KR - 1) / KR * KR;
  p.chunk_rows = rows;
  p.chunks = (int)std::min<int64_t>((std::max<int64_t>(n, 1) + rows - 1) / rows, (int64_t)kOpqMaxChunks + 1);
  return p;
}

size_t opq_cross_workspace_bytes(const OpqPlan& p) { return (size_t)p.chunks * p.tiles * (T * T) * sizeof(float); }

void launch_opq_cross(const float* xt, int64_t n, int d, const uint8_t* codes, const float* cb, int d2, int M,
                      const OpqPlan& p, float* part, float* C, hipStream_t s) {
  const bool vec = (d & 3) == 0 && (reinterpret_cast<uintptr_t>(xt) & 15) == 0;
  const dim3 grid((unsigned)((int64_t)p.tiles * p.chunks));
  if (vec)
    hipLaunchKernelGGL(k_opq_cross<true>, grid, dim3(256), 0, s, xt, n, d, codes, cb, d2, M, p.chunk_rows, p.tbj, p.tiles,
                       part);
  else
    hipLaunchKernelGGL(k_opq_cross<false>, grid, dim3(256), 0, s, xt, n, d, codes, cb, d2, M, p.chunk_rows, p.tbj,
                       p.tiles, part);
  hipLaunchKernelGGL(k_opq_cross_reduce, dim3((unsigned)(p.tiles * 16)), dim3(256), 0, s, part, p.chunks, p.tiles, p.tbj,
                     d, d2, C);
}

}  // namespace chivf
