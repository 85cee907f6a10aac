// Launchers for the IVF scalar-quantizer kernels (ivf_sq.hip) behind IndexIVFScalarQuantizer:
// the list-major scan of ivf_flat.h over lists of sq_scan.h's codes with the decode fused in,
// the per-pair residual queries, and the encode of (residual) rows into a pending set.  All
// launchers are asynchronous on `stream` and allocate nothing.  Codecs, keys and ties as in
// sq_scan.h and ivf_flat.h.
//
// Distances.  y = the decoded row, c = the centroid of the pair's list:
//   L2:  tree<> of (qr_j - y_j)^2 with qr = q - c (one fp32 subtraction per component) when
//        by_residual, else qr = q;
//   IP:  tree<> of q_j * y_j, plus the pair's coarse value as one fp32 add (coarse + ip) when
//        by_residual (Faiss's IVFSQScannerIP: accu0 = coarse_dis).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ivf_flat.h"
#include "sq_scan.h"

namespace chivf {

struct IvfSqArgs {
  IvfFlatArgs f;         // queries, probes, planning workspace and outputs; f.vecs is not read
  int codec;             // SqCodec
  const uint8_t* codes;  // [n][code_size] the image, readable kSqScanSlack bytes past the end
  const float* vmin;     // [d] (8-bit)
  const float* vdiff;    // [d] (8-bit)
  bool by_residual;
  const float* cent;     // [nlist][d] (by_residual and L2)
  const float* cdis;     // [nq][nprobe] the pairs' coarse values (by_residual and IP; null = zeros)
  // workspace of by_residual
  int32_t* probe_of;     // [nlist][nq] the probe column of every bucket entry
  float* qr;             // [nq][nprobe][d] residual queries (L2)
};
// ivfflat_plan with this scan's pairs per item: 8 at k <= 64 for fp16, otherwise 4
IvfFlatPlan ivfsq_plan(int codec, int k, int64_t slots);
// plan + (residual queries) + scan + merge of one batch with plan = ivfsq_plan(...); the limits
// of launch_ivfflat_search, and nq * nprobe < 2^31
void launch_ivfsq_search(const IvfSqArgs& a, const IvfFlatPlan& plan, hipStream_t s);

// out[i][j] = x[i / per][j] - cent[lists[i]][j] for i < n (rows whose list is outside [0, nlist)
// are left unwritten): the residual queries with per = nprobe, lists = the probes; the residuals
// of training rows with per = 1 (out may be x itself).
void launch_ivfsq_residuals(const float* x, int64_t n, int per, int d, const int64_t* lists, const float* cent,
                            int nlist, float* out, hipStream_t s);

// codes[i] = encode(by_residual ? x[i] - cent[lists[i]] : x[i]) for n rows (sq_scan.h's formulas)
void launch_ivfsq_encode(int codec, const float* x, int64_t n, int d, const int64_t* lists, const float* cent,
                         int nlist, bool by_residual, const float* vmin, const float* vdiff, uint8_t* codes,
                         hipStream_t s);

}  // namespace chivf
