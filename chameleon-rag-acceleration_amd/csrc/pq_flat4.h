// Launchers for the 4-bit flat product-quantizer kernels (pq_flat4.hip): IndexPQ with
// nbits = 4.  Sixteen centroids per sub-quantizer, code rows of M / 2 bytes with
// sub-quantizer 2i in the low nibble of byte i and 2i + 1 in the high one (Faiss's
// BitstringWriter order).  Keys, ties and padding follow pq_flat.h; all launchers are
// asynchronous on `stream` and allocate nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pq_flat.h"

namespace chivf {

constexpr int kPq4Ksub = 16;

// M a multiple of 32 from 32 to 256: a code row is then one to eight whole 16-byte loads
bool pq_flat4_supported_M(int M);

// T[q][m][j] = |x_q[m] - C_mj|^2, j < 16, in Faiss fvec_L2sqr order (tree<K_L2>); d / M <= 64
void launch_l2_table4(const float* x, int64_t n, int d, const float* codebook, int M, float* out, hipStream_t s);

// codes[i][b] = argmin(2b) | argmin(2b + 1) << 4, each the first argmin_j |x_i[m] - C_mj|^2
void launch_pq_encode4(const float* x, int64_t n, int d, const float* codebook, int M, uint8_t* codes, hipStream_t s);

// pq_scan_plan_group with the 4-bit scan's four queries per workgroup
PqScanPlan pq_scan4_plan(int k, int64_t nq, int64_t nb);

// tab [nq][M][16] (launch_ip_table with ksub = 16 / launch_l2_table4), codes [nb][M / 2],
// 1 <= nb < 2^31 - 1.  Writes partD / partI [S][nq][k] as launch_pq_scan does.
void launch_pq_scan4(const float* tab, int64_t nq, const uint8_t* codes, int64_t nb, int M, int k, bool ip,
                     const PqScanPlan& plan, float* partD, int64_t* partI, hipStream_t s);

}  // namespace chivf
