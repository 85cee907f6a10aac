// Launchers for the flat-index kernels (flat_scan.hip) behind IndexFlat / IndexFlatL2 /
// IndexFlatIP: the exact brute-force search over a device-resident [nb][d] fp32 row image
// with the top-k fused in.  All launchers are asynchronous on `stream` and allocate nothing.
// Keys follow ivfpq_kernels.h: L2 ranks by max(0, (|x|^2 + |y|^2) - 2 <x, y>), inner
// product by -<x, y>, negated back on output; ties by label = row position.  <x, y> is one
// ascending-k chain on v_mfma_f32_16x16x4_f32 (launch_l2_dist's fmaf chain, bit for bit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace chivf {

constexpr int kFlatTileQ = 64;            // queries per workgroup: 16 per wave
constexpr int kFlatTileQNarrow = 16;      // the narrow tile: batches of at most 16 queries, and k > kFlatWideMaxK
constexpr int kFlatTileRows = 128;        // base rows per pass of a workgroup (the MFMA tile is 64 x 128)
constexpr int kFlatKc = 32;               // dimensions per staged k chunk
constexpr int kFlatRangeGranule = 1024;   // a row range is a multiple of this many rows (forced ranges: of the row tile)
constexpr int kFlatTargetGroups = 1024;   // workgroups the host aims at when it picks the number of ranges
constexpr int kFlatWideMaxK = 256;        // k above this keeps sixteen-row lists: four queries per wave, the narrow tile
constexpr int kFlatMergeEntries = 2048;   // as kIvfFlatMergeEntries / kIvfFlatMergeFan: bounds of one merge call
constexpr int kFlatMergeFan = 16;

// How a batch is split: a workgroup takes tile_q queries and one range of range_rows rows;
// every (range, query) writes one sorted partial list, S lists per query go through `rounds`
// merge rounds of fan `fan`.
struct FlatScanPlan {
  int tile_q = kFlatTileQ;
  int64_t range_rows = 0;
  int ranges = 0;
  int S = 0;
  int fan = 2;
  int rounds = 0;
};
// nq: the queries of one launch (a chunk); force_rows > 0 (tests): the range size, rounded up
// to the row tile
FlatScanPlan flat_scan_plan(int64_t nq, int64_t nb, int k, int64_t force_rows);

struct FlatScanArgs {
  const float* x;     // [nq][d] queries
  const float* xn;    // [nq] |x|^2 (launch_row_norms; read for both metrics, used for L2)
  int64_t nq;
  int d;
  const float* base;  // [nb][d] the row image
  const float* bn;    // [nb] |y|^2 (launch_row_norms at add time; read for both metrics, used for L2)
  int64_t nb;         // 1 <= nb < 2^31 - 1
  int k;              // 1 <= k <= 1024
  bool ip;
  // workspace
  uint32_t* tau;      // [nq] the queries' shared bounds (set to "none" here)
  float* partD;       // [plan.S][nq][k]
  int64_t* partI;
  float* tmpD;        // [plan.S / plan.fan][nq][k]
  int64_t* tmpI;
  float* D;           // [nq][k] out
  int64_t* I;
};
// scan + merge of one batch; nq * plan.S * k < 2^31
void launch_flat_search(const FlatScanArgs& a, const FlatScanPlan& plan, hipStream_t s);

}  // namespace chivf
