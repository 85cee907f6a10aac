// Launchers for the half-precision flat-index kernels (flat_scan_f16.hip) behind
// GpuIndexFlat* with useFloat16: the exact search over a device-resident [nb][d] image of
// IEEE halves with the top-k fused in.  All launchers are asynchronous on `stream` and
// allocate nothing.  The arithmetic is Faiss-GPU's useFloat16: rows and queries rounded to
// half (nearest even; beyond the half range: +-inf, not trapped), products and sums in fp32
// on v_mfma_f32_16x16x32_f16, norms of the rounded values in fp32.  Keys, ties, padding,
// row ranges and the shared bound are flat_scan.h's; the plan is flat_scan_plan's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flat_scan.h"

namespace chivf {

constexpr int kFlatHKc = 64;  // dimensions per staged k chunk: 128 bytes of halves, two 32-wide MFMA steps

// out[n][d] = half(x[n][d]), norms[n] = sum of the squares of the rounded values (fp32);
// tau != nullptr: tau[n] set to "no bound yet" in the same pass (the queries of a search chunk)
void launch_rows_to_half(const float* x, int64_t n, int d, _Float16* out, float* norms, uint32_t* tau, hipStream_t s);
// out[count] = float(h[count])
void launch_half_to_float(const _Float16* h, int64_t count, float* out, hipStream_t s);

struct FlatScanHArgs {
  const _Float16* x;     // [nq][d] rounded queries (launch_rows_to_half, which also cleared tau)
  const float* xn;       // [nq] their norms
  int64_t nq;
  int d;
  const _Float16* base;  // [nb][d] the row image
  const float* bn;       // [nb] the rows' norms
  int64_t nb;            // 1 <= nb < 2^31 - 1
  int k;                 // 1 <= k <= 1024
  bool ip;
  // workspace, as FlatScanArgs
  uint32_t* tau;
  float* partD;
  int64_t* partI;
  float* tmpD;
  int64_t* tmpI;
  float* D;              // [nq][k] out
  int64_t* I;
};
// scan + merge of one batch; nq * plan.S * k < 2^31
void launch_flat_search_h(const FlatScanHArgs& a, const FlatScanPlan& plan, hipStream_t s);

}  // namespace chivf
