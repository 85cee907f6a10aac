// gfx950 (MI355X, CDNA4) kernels of the PCA training moments (faiss_amd.PCAMatrix.train):
// the column mean and the centred scatter matrix of a device-resident [n][d] fp32 matrix.
//
// k_pca_colsum / k_pca_mean: fp64 column sums over chunks of kPcaMeanRows rows (four
// interleaved row lanes per column, added in lane order), the chunk sums added in chunk
// order, divided by n in fp64 and rounded to fp32 once.
//
// k_pca_scatter: a workgroup takes one 64 x 64 tile (I, J), I <= J, of the upper triangle
// and one row chunk, and walks the chunk kPcaKr rows at a time.  Per step the 32 x 64
// column blocks I and J of x are staged in LDS row-major with the mean subtracted in fp32
// on the way in (rows past the chunk and columns past d are staged as 0, so any d works);
// a diagonal tile stages one block and reads it as both operands.  The product
// S_IJ += Xc_I^T Xc_J runs on v_mfma_f32_16x16x4_f32 with the row index as K: wave w owns
// the tile rows 16 w .. 16 w + 15 against all 64 columns (4 accumulators), a lane's A
// operand is element (row 4 j + k4, column 16 w + i16) of block I and its B operand element
// (row 4 j + k4, column 16 t + i16) of block J -- the same read for both.  The MFMA is an
// ascending-k fmaf chain, so a chunk's partial is the sum over its rows in row order.  The
// partial tile goes to the workspace; nothing is accumulated in global memory.
//
// k_pca_reduce: adds the partial tiles of every chunk in chunk order (one fp32 chain per
// element) and writes the element and its mirror; of a diagonal tile only i <= j is taken,
// so the matrix is symmetric by construction.
// Compiled with -ffp-contract=off like the rest of the library.
#include <stdint.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "pca_moments.h"

namespace chivf {

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int T = kPcaTile, KR = kPcaKr;
constexpr int TS = T + 16;  // row stride of a staged block (floats): 16 mod 32 -> the two rows a
                            // 32-lane group reads in an MFMA operand fall on disjoint banks
static_assert(T == 64 && KR == 32, "the staging below is written for these");

// four consecutive floats of a row at column c, zeros past d, without a branch (load4 of
// flat_scan.hip).  VEC: d % 4 == 0 and the rows are 16-byte aligned.
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

// grid (mean_chunks, ceil(d / 64)): psum[chunk][col] = the fp64 sum of the chunk's rows of a column
__global__ __launch_bounds__(256) void k_pca_colsum(const float* __restrict__ x, int64_t n, int d,
                                                    double* __restrict__ psum) {
  __shared__ double sh[4][64];
  const int c = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int col = blockIdx.y * 64 + c;
  const int64_t r0 = (int64_t)blockIdx.x * kPcaMeanRows, r1 = min(n, r0 + kPcaMeanRows);
  double s = 0.0;
  if (col < d)
    for (int64_t r = r0 + rl; r < r1; r += 4) s += (double)x[r * d + col];
  sh[rl][c] = s;
  __syncthreads();
  if (rl == 0 && col < d) psum[(int64_t)blockIdx.x * d + col] = ((sh[0][c] + sh[1][c]) + sh[2][c]) + sh[3][c];
}

__global__ __launch_bounds__(256) void k_pca_mean(const double* __restrict__ psum, int mean_chunks, int64_t n, int d,
                                                  float* __restrict__ mean) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= d) return;
  double s = 0.0;
  for (int c = 0; c < mean_chunks; c++) s += psum[(int64_t)c * d + col];
  mean[col] = (float)(s / (double)n);
}

// the (I, J), I <= J, of upper-triangle tile t in row-major order
__device__ __forceinline__ void tile_ij(int t, int tb, int& I, int& J) {
  I = 0;
  while (t >= tb - I) {
    t -= tb - I;
    I++;
  }
  J = I + t;
}

// grid: tiles fastest (the workgroups that run together share a row chunk), chunks slowest.
// LDS: 2 buffers x 2 blocks x 32 x 80 floats = 40 KiB.
template <bool VEC>
__global__ __launch_bounds__(256, 2) void k_pca_scatter(const float* __restrict__ x, int64_t n, int d,
                                                        const float* __restrict__ mean, int64_t chunk_rows, int tb,
                                                        int tiles, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float Ls[2][2][KR * TS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, k4 = lane >> 4;
  const int chunk = blockIdx.x / tiles, tile = blockIdx.x - chunk * tiles;
  int I, J;
  tile_ij(tile, tb, I, J);
  const bool diag = I == J;  // uniform over the workgroup
  const int64_t r0 = (int64_t)chunk * chunk_rows, r1 = min(n, r0 + chunk_rows);

  // staging: thread t loads row t >> 3 of the step, columns 8 (t & 7) .. + 7 of block I and of block J
  const int sr = tid >> 3, sc = (tid & 7) * 8;
  const int cI = I * T + sc, cJ = J * T + sc;
  f4 mI[2], mJ[2];
#pragma unroll
  for (int i = 0; i < 2; i++) {
    mI[i] = load4<VEC>(mean, cI + 4 * i, d);
    mJ[i] = load4<VEC>(mean, cJ + 4 * i, d);
  }
  f4 vI[2], vJ[2];
  bool live = false;  // the thread's row of the fetched step is inside the chunk
  auto fetch = [&](int64_t rr) __attribute__((always_inline)) {
    live = rr + sr < r1;
    const float* row = x + min(rr + sr, r1 - 1) * d;
#pragma unroll
    for (int i = 0; i < 2; i++) vI[i] = load4<VEC>(row, cI + 4 * i, d);
    if (!diag) {
#pragma unroll
      for (int i = 0; i < 2; i++) vJ[i] = load4<VEC>(row, cJ + 4 * i, d);
    }
  };
  // x - mean in fp32 (columns past d: 0 - 0), rows past the chunk as 0
  auto stage = [&](int b) __attribute__((always_inline)) {
    const f4 z = f4{0.f, 0.f, 0.f, 0.f};
    f4* pi = reinterpret_cast<f4*>(&Ls[b][0][sr * TS + sc]);
#pragma unroll
    for (int i = 0; i < 2; i++) pi[i] = live ? vI[i] - mI[i] : z;
    if (!diag) {
      f4* pj = reinterpret_cast<f4*>(&Ls[b][1][sr * TS + sc]);
#pragma unroll
      for (int i = 0; i < 2; i++) pj[i] = live ? vJ[i] - mJ[i] : z;
    }
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
    const float* B = &Ls[b][diag ? 0 : 1][i16];
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

// grid: tiles x 16; a thread adds one element's partials in chunk order and writes it and its mirror
__global__ __launch_bounds__(256) void k_pca_reduce(const float* __restrict__ part, int chunks, int tiles, int tb, int d,
                                                    float* __restrict__ S) {
  const int tile = blockIdx.x >> 4;
  const int e = (blockIdx.x & 15) * 256 + threadIdx.x;  // element of the tile: row e >> 6, column e & 63
  int I, J;
  tile_ij(tile, tb, I, J);
  const int i = e >> 6, j = e & 63;
  const int gi = I * T + i, gj = J * T + j;
  if (gi >= d || gj >= d || (I == J && i > j)) return;
  const float* p = part + (int64_t)tile * (T * T) + e;
  float s = 0.f;
  for (int c = 0; c < chunks; c++) s += p[(int64_t)c * tiles * (T * T)];
  S[(int64_t)gi * d + gj] = s;
  S[(int64_t)gj * d + gi] = s;
}

}  // namespace

PcaPlan pca_plan(int64_t n, int d, int64_t set_rows) {
  PcaPlan p;
  p.tb = (d + T - 1) / T;
  p.tiles = p.tb * (p.tb + 1) / 2;
  int64_t rows;
  if (set_rows > 0) {
    rows = set_rows;
  } else {
    const int64_t want = std::max<int64_t>(1, (kPcaTargetGroups + p.tiles - 1) / p.tiles);
    rows = std::max<int64_t>((std::max<int64_t>(n, 1) + want - 1) / want, kPcaMinChunkRows);
  }
  rows = (rows + KR - 1) / KR * KR;
  p.chunk_rows = rows;
  p.chunks = (int)std::min<int64_t>((std::max<int64_t>(n, 1) + rows - 1) / rows, (int64_t)kPcaMaxChunks + 1);
  p.mean_chunks = (int)std::min<int64_t>((std::max<int64_t>(n, 1) + kPcaMeanRows - 1) / kPcaMeanRows, INT32_MAX);
  return p;
}

size_t pca_workspace_bytes(const PcaPlan& p, int d) {
  const size_t sums = ((size_t)p.mean_chunks * d * sizeof(double) + 15) / 16 * 16;
  return sums + (size_t)p.chunks * p.tiles * (T * T) * sizeof(float);
}

void launch_pca_moments(const float* x, int64_t n, int d, const PcaPlan& p, void* ws, float* mean, float* scatter,
                        hipStream_t s) {
  double* psum = reinterpret_cast<double*>(ws);
  const size_t sums = ((size_t)p.mean_chunks * d * sizeof(double) + 15) / 16 * 16;
  float* part = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + sums);
  hipLaunchKernelGGL(k_pca_colsum, dim3((unsigned)p.mean_chunks, (unsigned)p.tb), dim3(256), 0, s, x, n, d, psum);
  hipLaunchKernelGGL(k_pca_mean, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, s, psum, p.mean_chunks, n, d, mean);
  const bool vec = (d & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(mean) & 15) == 0;
  const dim3 grid((unsigned)((int64_t)p.tiles * p.chunks));
  if (vec)
    hipLaunchKernelGGL(k_pca_scatter<true>, grid, dim3(256), 0, s, x, n, d, mean, p.chunk_rows, p.tb, p.tiles, part);
  else
    hipLaunchKernelGGL(k_pca_scatter<false>, grid, dim3(256), 0, s, x, n, d, mean, p.chunk_rows, p.tb, p.tiles, part);
  hipLaunchKernelGGL(k_pca_reduce, dim3((unsigned)(p.tiles * 16)), dim3(256), 0, s, part, p.chunks, p.tiles, p.tb, d,
                     scatter);
}

}  // namespace chivf
