// gfx950 (MI355X, CDNA4) kernels for IVF over scalar-quantizer codes (IndexIVFScalarQuantizer).
//
// Faiss runs IndexIVFScalarQuantizer::search as the coarse quantizer followed by IVFSQScannerL2 /
// IVFSQScannerIP: every code of every probed list decoded and accumulated against the query (or,
// by_residual and L2, against the query minus the list's centroid), into a heap.  Here:
//  * the planning is ivf_flat.hip's (launch_ivfflat_planning): per-list buckets of (query, first
//    slot), item_off, range-major work items of one row range and up to G pairs, the pad of the
//    slots no item writes; with by_residual the plan also records every entry's probe column;
//  * k_ivfsq_residuals writes, after the planning and before the scan, the residual query
//    qr[query][probe][d] = q - centroid of every pair (by_residual, L2): the G query rows of an
//    item then differ per list, and the scan reads them like any query row, wave-uniformly
//    through the scalar cache (written by an earlier launch, so safe to read there);
//  * k_ivfsq_scan is k_ivfflat_scan's item loop around k_sq_scan's pass: a tile of 256 rows x 64
//    dimensions of CODES staged in LDS with 16-byte loads, the next one in flight, rows padded to
//    an odd number of 16-byte slots, one decode per row for all G queries, the 8-bit unit[] table
//    built with the real division.  The tile layout, the vector types and the (G, R) classes are
//    sq_pass.h's, shared with sq_scan.hip.  The item header and the pass are this file's own text,
//    copies of k_ivfflat_scan's and of sq_pass.h's scan_code_rows: on shared helpers
//    k_ivfflat_scan and this kernel each measured slower on two rows than the version before
//    allows (profiles/ivf_shared_pass_refactor.md).  A piece that straddles a row's end reads the
//    next row's (the next list's) first bytes or, at the image's last row, its slack.  For the
//    inner product with by_residual the pair's coarse value is added to the folded sum before
//    the key is formed.  The top-k holds image positions; labels are looked up at the write;
//  * wave top-k, shared bound, LDS queues above k = 64 and the merge rounds are scan_topk.h's;
//  * k_ivfsq_encode is sq_pass.h's encode of a component over x or x - centroid, one thread per
//    component.
// Compiled with -ffp-contract=off like the rest of the library.
#include <float.h>
#include <stdint.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "ivf_sq.h"
#include "scan_topk.h"
#include "sq_pass.h"

namespace chivf {

namespace {

// ------------------------------------------------------------ residuals, encode
// one thread per component (out may alias x: per = 1, every thread reads what it writes)
__global__ __launch_bounds__(256) void k_ivfsq_residuals(const float* x, int64_t total, int per, int d,
                                                         const int64_t* __restrict__ lists,
                                                         const float* __restrict__ cent, int nlist, float* out) {
  for (int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (int64_t)gridDim.x * 256) {
    const int64_t i = gid / d;
    const int j = (int)(gid - i * d);
    const int64_t l = lists[i];
    if (l < 0 || l >= nlist) continue;
    out[gid] = x[(i / per) * d + j] - cent[l * d + j];
  }
}

template <int CODEC>
__global__ __launch_bounds__(256) void k_ivfsq_encode(const float* __restrict__ x, int64_t total, int d,
                                                      const int64_t* __restrict__ lists,
                                                      const float* __restrict__ cent, int nlist, int by_residual,
                                                      const float* __restrict__ vmin, const float* __restrict__ vdiff,
                                                      uint8_t* __restrict__ codes) {
  for (int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (int64_t)gridDim.x * 256) {
    const int64_t i = gid / d;
    const int j = (int)(gid - i * d);
    float v = x[gid];
    if (by_residual) {
      const int64_t l = lists[i];
      if (l >= 0 && l < nlist) v = v - cent[l * d + j];  // (a row assigned to no list fails the merge)
    }
    encode_component<CODEC>(v, j, vmin, vdiff, codes, gid);
  }
}

// ------------------------------------------------------------------------ scan
// Persistent over work items: workgroup b takes items b, b + gridDim.x, ...
// xq: the query rows.  Pair g of an item reads row qid (probe_of null, or the inner product) or
// row qid * nprobe + probe (probe_of set, L2: the residual queries).  cdis (inner product,
// nullable): [nq][nprobe], added to the pair's sums.
// LDS: the 36 KiB (fp16) or 20 KiB (8-bit) tile, the 8-bit codec's 1 KiB of unit values,
// plus G KiB of candidate queues per wave when R > 1.
template <int KIND, int CODEC, int G, int R>
__global__ __launch_bounds__(256) void k_ivfsq_scan(const float* __restrict__ xq, int64_t nq, int d,
                                                    const uint8_t* __restrict__ codes, const int64_t* __restrict__ ids,
                                                    const int64_t* __restrict__ list_off, int nlist,
                                                    const float* __restrict__ vmin, const float* __restrict__ vdiff,
                                                    const int32_t* __restrict__ cnt, const int2* __restrict__ bucket,
                                                    const int32_t* __restrict__ item_off,
                                                    const int32_t* __restrict__ probe_of, int nprobe,
                                                    const float* __restrict__ cdis, uint32_t* tau, int k, int S,
                                                    float* __restrict__ partD, int64_t* __restrict__ partI) {
  using L = Layout<CODEC>;
  constexpr bool k8bit = CODEC == SQ_CODEC_8BIT;
  __shared__ __attribute__((aligned(16))) uint8_t tile[kTile * L::kStride];
  __shared__ float unit[k8bit ? 256 : 1];  // (code + 0.5f) / 255.0f
  constexpr bool kQueued = R > 1;
  __shared__ float qd[kQueued ? kIvfFlatWaves * G * kQ : 1];
  __shared__ int qi[kQueued ? kIvfFlatWaves * G * kQ : 1];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int64_t cs = (int64_t)d * L::kElem;
  const int nchunk = (d + kDc - 1) / kDc;
  const int total = item_off[nlist];
  const bool addc = KIND == K_IP && probe_of != nullptr && cdis != nullptr;  // uniform
  // (read after the step loop's first barriers)
  if constexpr (k8bit) unit[tid] = ((float)tid + 0.5f) / 255.0f;

  for (int item = blockIdx.x; item < total; item += gridDim.x) {
    // the item's list: the last l with item_off[l] <= item (uniform)
    int lo = 0, hi = nlist;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (item_off[mid] <= item) lo = mid;
      else hi = mid;
    }
    const int l = lo;
    const int64_t lb = list_off[l];
    const int64_t lrows = list_off[l + 1] - lb;
    // range-major within the list, as k_ivfflat_scan
    const int local = item - item_off[l];
    const int groups = (cnt[l] + G - 1) / G;
    const int rng = local / groups;
    const int grp = local - rng * groups;
    const int npair = min(G, cnt[l] - grp * G);  // >= 1
    const int64_t r0 = lb + (int64_t)rng * kIvfFlatRangeRows;
    const int64_t r1 = min(lb + lrows, r0 + kIvfFlatRangeRows);
    int qid[G], slot[G], qrow[G];  // pairs past npair repeat the first (their sums are dropped)
    float cd[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
      const int64_t at = (int64_t)l * nq + grp * G + (g < npair ? g : 0);
      const int2 e = bucket[at];
      qid[g] = __builtin_amdgcn_readfirstlane(e.x);
      slot[g] = __builtin_amdgcn_readfirstlane(e.y) + rng;
      qrow[g] = qid[g];
      cd[g] = 0.f;
      if (probe_of) {  // uniform
        const int pair = qid[g] * nprobe + __builtin_amdgcn_readfirstlane(probe_of[at]);
        if (KIND == K_L2) qrow[g] = pair;
        if (addc) cd[g] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(cdis[pair])));
      }
    }

    WaveTopK<R> tk[G];
#pragma unroll
    for (int g = 0; g < G; g++) tk[g].init(k);
    int qn[G];  // queue fills (wave-uniform, < 64 between passes)
#pragma unroll
    for (int g = 0; g < G; g++) qn[g] = 0;

    // step (t0, c): dimensions [c * kDc, +len) of rows [t0, t0 + kTile); rows past the
    // range re-read its last row (their sums are dropped at the admission)
    u4 nxt[L::kPieces];
    auto fetch = [&](int64_t t0, int c) __attribute__((always_inline)) {
      const int lenb = min(kDc, d - c * kDc) * L::kElem;
#pragma unroll
      for (int i = 0; i < L::kPieces; i++) {
        const int e = i * 256 + tid;
        const int row = e / L::kPieces, p = e % L::kPieces;
        const int64_t grow = min(t0 + row, r1 - 1);
        // (pieces past a short last step re-read its first: staged, never used; a piece that
        // straddles the row's end reads at most 12 bytes of the next row or of the slack)
        nxt[i] = *reinterpret_cast<const u4a*>(codes + grow * cs + c * L::kStepBytes + (p * 16 < lenb ? p * 16 : 0));
      }
    };
    fetch(r0, 0);

    float acc[G][8];
#pragma unroll
    for (int g = 0; g < G; g++)
#pragma unroll
      for (int j = 0; j < 8; j++) acc[g][j] = 0.f;

    // eight decoded values of the lane's row at dimensions [dim0, dim0 + 8) against every pair's query row
    auto add8 = [&](const float(&y)[8], int dim0) __attribute__((always_inline)) {
#pragma unroll
      for (int g = 0; g < G; g++) {
        const float* qp = xq + (int64_t)qrow[g] * d + dim0;  // wave-uniform
#pragma unroll
        for (int j = 0; j < 8; j++) acc[g][j] = acc[g][j] + dist_term<KIND>(qp[j], y[j]);
      }
    };
    // byte j of the pair (w0, w1) decoded at dimension dim0 + j
    auto dec8 = [&](uint32_t w0, uint32_t w1, int j, int dim0) __attribute__((always_inline)) {
      const uint32_t code = ((j < 4 ? w0 : w1) >> (8 * (j & 3))) & 0xffu;
      const float m = unit[code] * vdiff[dim0 + j];
      return vmin[dim0 + j] + m;
    };

    for (int64_t t0 = r0; t0 < r1; t0 += kTile) {
#pragma unroll
      for (int g = 0; g < G; g++) tk[g].set_cap(tau_get(tau + qid[g]));
      for (int c = 0; c < nchunk; c++) {
        const int len = min(kDc, d - c * kDc);
        __syncthreads();  // the previous step's reads are done
#pragma unroll
        for (int i = 0; i < L::kPieces; i++) {
          const int e = i * 256 + tid;
          const int row = e / L::kPieces, p = e % L::kPieces;
          *reinterpret_cast<u4*>(&tile[row * L::kStride + p * 16]) = nxt[i];
        }
        __syncthreads();
        if (c + 1 < nchunk) fetch(t0, c + 1);
        else if (t0 + kTile < r1) fetch(t0 + kTile, 0);

        const uint8_t* yrow = &tile[tid * L::kStride];
        const int n8 = len >> 3;
        const int dim_c = c * kDc;
        if constexpr (!k8bit) {
          for (int j8 = 0; j8 < n8; j8++) {
            const h8 w = *reinterpret_cast<const h8*>(yrow + j8 * 16);
            float y[8];
#pragma unroll
            for (int j = 0; j < 8; j++) y[j] = (float)w[j];
            add8(y, dim_c + j8 * 8);
          }
        } else {
          for (int j8 = 0; j8 < n8; j8 += 2) {  // sixteen codes per 16-byte read
            const u4 w = *reinterpret_cast<const u4*>(yrow + j8 * 8);
            float y[8];
#pragma unroll
            for (int j = 0; j < 8; j++) y[j] = dec8(w.x, w.y, j, dim_c + j8 * 8);
            add8(y, dim_c + j8 * 8);
            if (j8 + 1 < n8) {
#pragma unroll
              for (int j = 0; j < 8; j++) y[j] = dec8(w.z, w.w, j, dim_c + j8 * 8 + 8);
              add8(y, dim_c + j8 * 8 + 8);
            }
          }
        }
        if (c + 1 < nchunk) continue;

        // the row's last step: fold to four, the 4-wide remainder, two horizontal adds
        const int64_t rowpos = t0 + tid;
        const bool valid = rowpos < r1;
        const bool rem = (len & 4) != 0;
        const int dim_r = dim_c + n8 * 8;
        float y[4] = {0.f, 0.f, 0.f, 0.f};
        if (rem) {
          if constexpr (!k8bit) {
            const h4 w = *reinterpret_cast<const h4*>(yrow + n8 * 16);
#pragma unroll
            for (int j = 0; j < 4; j++) y[j] = (float)w[j];
          } else {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(yrow + n8 * 8);
#pragma unroll
            for (int j = 0; j < 4; j++) y[j] = dec8(w, 0u, j, dim_r);
          }
        }
#pragma unroll
        for (int g = 0; g < G; g++) {
          float a4[4];
#pragma unroll
          for (int j = 0; j < 4; j++) a4[j] = acc[g][j + 4] + acc[g][j];
          if (rem) {
            const float* qp = xq + (int64_t)qrow[g] * d + dim_r;
#pragma unroll
            for (int j = 0; j < 4; j++) a4[j] = a4[j] + dist_term<KIND>(qp[j], y[j]);
          }
          const float h0 = a4[0] + a4[1];
          const float h1 = a4[2] + a4[3];
          float dis = h0 + h1;
          if (addc) dis = cd[g] + dis;  // IVFSQScannerIP: accu0 = coarse_dis
          const float key = KIND == K_IP ? -dis : dis;
#pragma unroll
          for (int j = 0; j < 8; j++) acc[g][j] = 0.f;
          if (g >= npair) continue;  // uniform
          // admission against the pair's running k-th best
          const bool pass = valid & lexless(key, (int)rowpos, tk[g].td, tk[g].ti);
          const uint64_t mask = __ballot(pass);
          if (!mask) continue;
          if constexpr (!kQueued) {
            bulk_merge_rows<R>(tk[g], pass ? key : kInf, pass ? (int)rowpos : kNone, lane);
            tk[g].publish(tau + qid[g], lane);
          } else {
            const int before =
                __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
            if (pass) {
              const int at = (wave * G + g) * kQ + qn[g] + before;
              qd[at] = key;
              qi[at] = (int)rowpos;
            }
            qn[g] += __popcll(mask);
          }
        }
        if constexpr (kQueued)
          drain_queues<1, true>(tk, qn, t0 + kTile < r1 ? 63 : 0, qd, qi, wave, lane, tau, qid);
      }
    }

    // this wave's sorted list of every pair, labels looked up from the positions
#pragma unroll
    for (int g = 0; g < G; g++) {
      if (g >= npair || slot[g] * kIvfFlatWaves + wave >= S) continue;  // (the host's slot bound holds)
      const int64_t base = (((int64_t)slot[g] * kIvfFlatWaves + wave) * nq + qid[g]) * k;
      write_sorted<R>(tk[g], k, KIND == K_IP, partD + base, partI + base, lane, [&](int pos) { return ids[pos]; });
    }
  }
}

// one (G, R) class of sq_pass.h's launch_scan
struct ScanLaunch {
  const IvfSqArgs& a;
  const IvfFlatPlan& p;
  const float* xq;
  hipStream_t s;
  template <int KIND, int CODEC, int G, int R>
  void launch() const {
    const IvfFlatArgs& f = a.f;
    hipLaunchKernelGGL((k_ivfsq_scan<KIND, CODEC, G, R>), dim3((unsigned)p.grid), dim3(256), 0, s, xq, f.nq, f.d,
                       a.codes, f.ids, f.list_off, f.nlist, a.vmin, a.vdiff, f.cnt, f.bucket, f.item_off,
                       a.by_residual ? a.probe_of : nullptr, f.nprobe, a.cdis, f.tau, f.k, p.S, f.partD, f.partI);
  }
};

}  // namespace

IvfFlatPlan ivfsq_plan(int codec, int k, int64_t slots) {
  IvfFlatPlan p = ivfflat_plan(k, slots);
  p.G = scan_group_for(codec, k);  // the classes of launch_scan
  return p;
}

void launch_ivfsq_residuals(const float* x, int64_t n, int per, int d, const int64_t* lists, const float* cent,
                            int nlist, float* out, hipStream_t s) {
  const int64_t total = n * d;
  if (total <= 0) return;
  hipLaunchKernelGGL(k_ivfsq_residuals, dim3(elementwise_grid(total)), dim3(256), 0, s, x, total, per, d, lists, cent,
                     nlist, out);
}

void launch_ivfsq_encode(int codec, const float* x, int64_t n, int d, const int64_t* lists, const float* cent,
                         int nlist, bool by_residual, const float* vmin, const float* vdiff, uint8_t* codes,
                         hipStream_t s) {
  const int64_t total = n * d;
  if (total <= 0) return;
  if (codec == SQ_CODEC_FP16)
    hipLaunchKernelGGL(k_ivfsq_encode<SQ_CODEC_FP16>, dim3(elementwise_grid(total)), dim3(256), 0, s, x, total, d,
                       lists, cent, nlist, by_residual ? 1 : 0, vmin, vdiff, codes);
  else
    hipLaunchKernelGGL(k_ivfsq_encode<SQ_CODEC_8BIT>, dim3(elementwise_grid(total)), dim3(256), 0, s, x, total, d,
                       lists, cent, nlist, by_residual ? 1 : 0, vmin, vdiff, codes);
}

void launch_ivfsq_search(const IvfSqArgs& a, const IvfFlatPlan& p, hipStream_t s) {
  const IvfFlatArgs& f = a.f;
  if (f.nq <= 0) return;
  launch_ivfflat_planning(f, p, a.by_residual ? a.probe_of : nullptr, s);
  const float* xq = f.x;
  if (a.by_residual && !f.ip) {
    launch_ivfsq_residuals(f.x, f.nq * f.nprobe, f.nprobe, f.d, f.probes, a.cent, f.nlist, a.qr, s);
    xq = a.qr;
  }
  launch_scan(f.ip, a.codec, f.k, ScanLaunch{a, p, xq, s});
  merge_partial_lists(f.partD, f.partI, f.tmpD, f.tmpI, p.S, p.fan, f.nq, f.k, f.ip, f.D, f.I, s);
}

}  // namespace chivf
