// Launchers for the scalar-quantizer kernels (sq_scan.hip) behind IndexScalarQuantizer:
// encode, decode, the min/max training reduction, and the exact scan of the codes with
// the decode fused in.  All launchers are asynchronous on `stream` and allocate nothing.
//
// Codecs (Faiss's scalar-build formulas, every operation one fp32 rounding):
//   fp16:   code = (half)x, round to nearest even;  y = (float)code
//   8-bit:  xi = vdiff != 0 ? (x - vmin) / vdiff : 0, clamped to [0, 1];
//           code = (uint8)(int)(255.f * xi);  y = vmin + (((float)code + 0.5f) / 255.0f) * vdiff
//           with vmin, vdiff per dimension (QT_8bit_uniform repeats its pair d times).
// Distances are tree<> over the decoded row, keys and ties as in ivf_flat.h; the label
// of a row is its position.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ivf_flat.h"

namespace chivf {

enum SqCodec { SQ_CODEC_FP16 = 0, SQ_CODEC_8BIT = 1 };

inline int sq_code_size(int codec, int d) { return codec == SQ_CODEC_FP16 ? 2 * d : d; }

// The scan stages whole 16-byte pieces of a row's step, so it may read up to
// kSqScanSlack bytes past the last code: the code array is allocated that much longer.
constexpr int kSqScanSlack = 16;

// codes[n][code_size] <- x[n][d]; vmin / vdiff [d] are read by the 8-bit codec only
void launch_sq_encode(int codec, const float* x, int64_t n, int d, const float* vmin, const float* vdiff,
                      uint8_t* codes, hipStream_t s);
// y[n][d] <- codes[n][code_size]
void launch_sq_decode(int codec, const uint8_t* codes, int64_t n, int d, const float* vmin, const float* vdiff,
                      float* y, hipStream_t s);

// Per-dimension minimum and maximum of x[n][d] folded into lo[d] / hi[d], which hold
// order-preserving bits (sq_minmax_init sets them to "nothing seen"; sq_minmax_value
// turns them back into floats on the host).  Exact whatever the order.
void launch_sq_minmax_init(uint32_t* lo, uint32_t* hi, int d, hipStream_t s);
void launch_sq_minmax(const float* x, int64_t n, int d, uint32_t* lo, uint32_t* hi, hipStream_t s);
inline float sq_minmax_value(uint32_t u) {
  const uint32_t b = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
  float f;
  __builtin_memcpy(&f, &b, sizeof(f));
  return f;
}

struct SqScanArgs {
  int codec;
  const float* x;        // [nq][d] queries
  int64_t nq;
  int d;
  const uint8_t* codes;  // [nb][code_size], readable kSqScanSlack bytes past the end
  int64_t nb;            // 1 <= nb < 2^31 - 1
  const float* vmin;     // [d] (8-bit)
  const float* vdiff;    // [d] (8-bit)
  int k;
  bool ip;
  // workspace
  uint32_t* tau;   // [nq] the queries' shared bounds (set to "none" here)
  float* partD;    // [plan.S][nq][k]
  int64_t* partI;
  float* tmpD;     // [plan.S / plan.fan][nq][k]
  int64_t* tmpI;
  float* D;        // [nq][k] out
  int64_t* I;
};
// Row ranges of kIvfFlatRangeRows rows of one list of nb rows: the slots of every query.
inline int64_t sq_scan_ranges(int64_t nb) { return (nb + kIvfFlatRangeRows - 1) / kIvfFlatRangeRows; }
// scan + merge of one batch with plan = ivfflat_plan(k, sq_scan_ranges(nb)); 1 <= k <= 1024,
// d % 4 == 0, nq * plan.S < 2^31
void launch_sq_search(const SqScanArgs& a, const IvfFlatPlan& plan, hipStream_t s);

}  // namespace chivf
