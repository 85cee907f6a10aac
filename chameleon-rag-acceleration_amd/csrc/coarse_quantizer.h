// The coarse quantizer of the IVF indexes: the centroids' device copies and the launch
// that picks every query's nprobe best lists.
#pragma once
#include <vector>

#include "host_common.h"
#include "ivfpq.h"

namespace chivf {

// the per-batch scratch of CoarseQuantizer::launch
struct CoarseScratch {
  DevBuf w_dist;  // [c][nlist] key matrix
  DevBuf w_qn;    // |x|^2 of the batch's queries (tiled coarse keys)
  DevBuf w_cand;  // large-nlist coarse segment candidates
};

// What only IVF-PQ asks of the coarse launch: the batch planned by the selection
// (`plan`, over the lists [lo, hi) with offsets list_off) and T3 built alongside.
// xt / nt (nullable): T3out holds the tables of the queries xt instead of x (the
// shard step: keys of this rank's slice, tables of the global batch, one launch)
struct CoarsePqArgs {
  const ListPlan* plan = nullptr;
  const int64_t* list_off = nullptr;
  int lo = 0, hi = 0;
  float* T3out = nullptr;
  const float* cb = nullptr;
  int M = 0, ksub = 256;
  const float* xt = nullptr;
  int64_t nt = 0;
  bool hoist = false;
};

struct CoarseQuantizer {
  int d = 0, nlist = 0, metric = IVFPQ_METRIC_L2;
  DevBuf d_cent, d_centT, d_cnorm;  // [nlist][d], transposed [d][(nlist + 3) & ~3], |c|^2

  bool ip() const { return metric == IVFPQ_METRIC_INNER_PRODUCT; }

  // the device copies of centroids [nlist][d] (host); returns when they are in place
  void upload(const float* centroids, hipStream_t s) {
    d_cent.ensure(sizeof(float) * nlist * d);
    d_cnorm.ensure(sizeof(float) * nlist);
    HIPCHECK(hipMemcpyAsync(d_cent.p, centroids, sizeof(float) * nlist * d, hipMemcpyHostToDevice, s));
    launch_row_norms(d_cent.as<float>(), nlist, d, d_cnorm.as<float>(), s);
    // transposed centroids [d][nlist] for the fused coarse kernel
    const int ldc = (nlist + 3) & ~3;  // rows padded to a multiple of 4 (branch-free float4 loads)
    std::vector<float> ct((size_t)ldc * d, 0.f);
    for (int l = 0; l < nlist; l++)
      for (int t = 0; t < d; t++) ct[(size_t)t * ldc + l] = centroids[(size_t)l * d + t];
    d_centT.ensure(sizeof(float) * ct.size());
    HIPCHECK(hipMemcpyAsync(d_centT.p, ct.data(), sizeof(float) * ct.size(), hipMemcpyHostToDevice, s));
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
  }

  // Coarse quantizer for c queries at x: the np best lists and the quantizer's
  // values (L2 distances / IP similarities), from the key matrix built on the
  // matrix cores (with pq->T3out, the same launch builds T3).  With pq->plan and
  // np <= 64 the selection also plans the batch and true is returned; otherwise
  // the caller plans with launch_plan_count.
  bool launch(CoarseScratch& w, const float* x, int64_t c, int np, float* dis, int64_t* lists, hipStream_t s,
              const CoarsePqArgs* pq = nullptr) {
    CoarsePqArgs a;  // without pq: no plan, no tables, every list
    if (pq) a = *pq;
    else a.hi = nlist;
    if (!a.xt) {
      a.xt = x;
      a.nt = c;
    }
    if (nlist >= kSegmentedNlist && np <= 64) {  // large nlist: no [c][nlist] key matrix
      w.w_cand.ensure(sizeof(uint64_t) * c * coarse_segments(c, nlist, d) * np);
      if (a.T3out) launch_ip_table(a.xt, a.nt, d, a.cb, a.M, a.ksub, a.T3out, s);
      launch_coarse_segmented(x, c, d, d_centT.as<float>(), d_cnorm.as<float>(), nlist, np, w.w_cand.as<uint64_t>(),
                              dis, lists, s, ip(), a.plan, a.list_off, a.lo, a.hi, d_cent.as<float>());
      return a.plan != nullptr;
    }
    w.w_dist.ensure(sizeof(float) * c * nlist);
    w.w_qn.ensure(sizeof(float) * c);
    launch_coarse_keys(x, c, d, d_centT.as<float>(), d_cnorm.as<float>(), nlist, w.w_dist.as<float>(), s, ip(),
                       a.T3out, a.cb, a.M, w.w_qn.as<float>(), a.xt, a.nt, a.hoist);
    if (np <= 64) {
      launch_coarse_select(w.w_dist.as<float>(), c, nlist, np, dis, lists, s, ip(), a.plan, a.list_off, a.lo, a.hi, x,
                           d_cent.as<float>(), d);
      return a.plan != nullptr;
    }
    launch_select_rows(w.w_dist.as<float>(), c, nlist, np, dis, lists, s, ip());
    return false;
  }
};

}  // namespace chivf
