// Launchers for the flat product-quantizer kernels (pq_flat.hip): the query-major
// scan behind IndexPQ.  All launchers are asynchronous on `stream` and allocate
// nothing.  Keys follow ivfpq_kernels.h: L2 ranks by the table sum itself, inner
// product by the sum of the negated entries, negated back on output; ties by label
// (= the code's position).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace chivf {

constexpr int kPqTileRows = 2048;  // granule of a code range: the rows of one pass at k <= 64 (256 threads x 8), of two above
constexpr int kPqWaves = 4;        // waves per scan workgroup = partial lists per code range

// M = 8 or a multiple of 16 up to 128 (the scan reads 8 or 16 code bytes per load)
bool pq_flat_supported_M(int M);

// T[q][m][j] = |x_q[m] - C_mj|^2 in Faiss fvec_L2sqr order (tree<K_L2>)
void launch_l2_table(const float* x, int64_t n, int d, const float* codebook, int M, float* out, hipStream_t s);

// codes[i][m] = first argmin_j |x_i[m] - C_mj|^2 (k_pq_encode without the residual)
void launch_pq_encode_flat(const float* x, int64_t n, int d, const float* codebook, int M, uint8_t* codes,
                           hipStream_t s);

// How launch_pq_scan splits a batch: G queries per workgroup, `ranges` contiguous code
// ranges of `rows` rows (a multiple of kPqTileRows), S = ranges * kPqWaves sorted
// partial lists per query.
struct PqScanPlan {
  int G = 1;
  int ranges = 1;
  int64_t rows = 0;
  int S = 0;
};
PqScanPlan pq_scan_plan(int M, int k, int64_t nq, int64_t nb);

// tab [nq][M][256] (launch_ip_table / launch_l2_table), codes [nb][M], 1 <= nb < 2^31 - 1.
// Writes partD / partI [S][nq][k]: per (range, wave) the k best of its rows as
// (distance or similarity, position), best first, padded with (FLT_MAX | -FLT_MAX, -1):
// the input of launch_merge_topk(S, nq, k, ..., ip).
void launch_pq_scan(const float* tab, int64_t nq, const uint8_t* codes, int64_t nb, int M, int k, bool ip,
                    const PqScanPlan& plan, float* partD, int64_t* partI, hipStream_t s);

}  // namespace chivf
