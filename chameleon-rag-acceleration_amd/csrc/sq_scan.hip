// gfx950 (MI355X, CDNA4) kernels for the flat scalar quantizer (IndexScalarQuantizer).
//
// Faiss runs IndexScalarQuantizer::search as a distance computer that decodes every code
// and accumulates it against the query, into a heap.  Here:
//  * k_sq_encode / k_sq_decode are Faiss's scalar-build codec formulas, one thread per
//    component, every operation one fp32 rounding (the division is the IEEE one); the
//    encode of a component is sq_pass.h's, shared with k_ivfsq_encode;
//  * k_sq_minmax is the training reduction: per-dimension minimum and maximum, folded
//    with atomics on order-preserving bits, so exact whatever the order;
//  * k_sq_scan is k_ivfflat_scan (ivf_flat.hip) over one list whose rows are codes, with
//    the row codec as a template parameter.  The pass over a work item's rows -- the
//    staging of a tile of codes, the decode, the sums, the fold, the admission and the
//    drain sites -- is sq_pass.h's scan_code_rows (k_ivfsq_scan of ivf_sq.hip keeps a copy
//    of it), and so are the (G, R) classes (G = 8 at k <= 64 for halves, 4 otherwise).
//    This file keeps what is the flat scan's own: the 8-bit codec's unit[] table built
//    once per workgroup, the item numbering and the sorted write.  With one list and
//    labels equal to positions a work item is numbered arithmetically:
//    item = range * groups + group (range-major, so that the groups of a row range run
//    at about the same time and find its codes in the L2), a pair's query row is the
//    query itself and nothing is added to its sums.
//    Shared bound, register top-k, LDS queues for k > 64 and the merge rounds are those
//    of the IVF-Flat scan (scan_topk.h).
// Compiled with -ffp-contract=off like the rest of the library.
#include <float.h>
#include <stdint.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "scan_topk.h"
#include "sq_pass.h"
#include "sq_scan.h"

namespace chivf {

namespace {

// ------------------------------------------------------------- encode / decode
template <int CODEC>
__global__ __launch_bounds__(256) void k_sq_encode(const float* __restrict__ x, int64_t total, int d,
                                                   const float* __restrict__ vmin, const float* __restrict__ vdiff,
                                                   uint8_t* __restrict__ codes) {
  for (int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (int64_t)gridDim.x * 256)
    encode_component<CODEC>(x[gid], (int)(gid % d), vmin, vdiff, codes, gid);
}

template <int CODEC>
__global__ __launch_bounds__(256) void k_sq_decode(const uint8_t* __restrict__ codes, int64_t total, int d,
                                                   const float* __restrict__ vmin, const float* __restrict__ vdiff,
                                                   float* __restrict__ y) {
  for (int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (int64_t)gridDim.x * 256) {
    if constexpr (CODEC == SQ_CODEC_FP16) {
      y[gid] = (float)reinterpret_cast<const _Float16*>(codes)[gid];
    } else {
      const int j = (int)(gid % d);
      const float t = ((float)codes[gid] + 0.5f) / 255.0f;
      const float m = t * vdiff[j];
      y[gid] = vmin[j] + m;
    }
  }
}

// ------------------------------------------------------------------- training
// grid (ceil(d / 256), row blocks): a thread folds one dimension over its block's rows
__global__ __launch_bounds__(256) void k_sq_minmax(const float* __restrict__ x, int64_t n, int d,
                                                   uint32_t* __restrict__ lo, uint32_t* __restrict__ hi) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= d) return;
  const int64_t per = (n + gridDim.y - 1) / gridDim.y;
  const int64_t r0 = (int64_t)blockIdx.y * per, r1 = min(n, r0 + per);
  if (r0 >= r1) return;
  float mn = x[r0 * d + j], mx = mn;
  for (int64_t r = r0 + 1; r < r1; r++) {
    const float v = x[r * d + j];
    mn = v < mn ? v : mn;
    mx = v > mx ? v : mx;
  }
  atomicMin(&lo[j], key_bits(mn));
  atomicMax(&hi[j], key_bits(mx));
}

// ------------------------------------------------------------------------ scan
// Persistent over work items: workgroup b takes items b, b + gridDim.x, ...
// LDS: the 36 KiB (fp16) or 20 KiB (8-bit) tile, the 8-bit codec's 1 KiB of unit values,
// plus G KiB of candidate queues per wave when R > 1.
template <int KIND, int CODEC, int G, int R>
__global__ __launch_bounds__(256) void k_sq_scan(const float* __restrict__ x, int64_t nq, int d,
                                                 const uint8_t* __restrict__ codes, int64_t nb,
                                                 const float* __restrict__ vmin, const float* __restrict__ vdiff,
                                                 uint32_t* tau, int k, int S, float* __restrict__ partD,
                                                 int64_t* __restrict__ partI) {
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
  const int groups = (int)((nq + G - 1) / G);
  const int ranges = (int)((nb + kIvfFlatRangeRows - 1) / kIvfFlatRangeRows);
  const int total = ranges * groups;
  // (read after the step loop's first barriers)
  if constexpr (k8bit) unit[tid] = ((float)tid + 0.5f) / 255.0f;

  for (int item = blockIdx.x; item < total; item += gridDim.x) {
    const int rng = item / groups;
    const int grp = item - rng * groups;
    const int npair = (int)min((int64_t)G, nq - (int64_t)grp * G);  // >= 1
    const int64_t r0 = (int64_t)rng * kIvfFlatRangeRows;
    const int64_t r1 = min(nb, r0 + kIvfFlatRangeRows);
    int qid[G];  // queries past npair repeat the first (their sums are dropped)
#pragma unroll
    for (int g = 0; g < G; g++) qid[g] = grp * G + (g < npair ? g : 0);

    WaveTopK<R> tk[G];
#pragma unroll
    for (int g = 0; g < G; g++) tk[g].init(k);
    scan_code_rows<KIND, CODEC, G, R>(tk, tile, unit, qd, qi, x, d, codes, vmin, vdiff, tau, r0, r1, npair, qid);

    // this wave's sorted list of every query; the label of a row is its position
#pragma unroll
    for (int g = 0; g < G; g++) {
      if (g >= npair || rng * kIvfFlatWaves + wave >= S) continue;  // (the host's slot bound holds)
      const int64_t base = (((int64_t)rng * kIvfFlatWaves + wave) * nq + qid[g]) * k;
#pragma unroll
      for (int r = 0; r < R; r++) {
        const int idx = r * 64 + lane;
        if (idx < k) {
          const int pos = tk[g].id[r];
          const bool none = pos == kNone;
          const float key = tk[g].d[r];
          partD[base + idx] = none ? (KIND == K_IP ? -FLT_MAX : FLT_MAX) : (KIND == K_IP ? -key : key);
          partI[base + idx] = none ? -1 : (int64_t)pos;
        }
      }
    }
  }
}

// one (G, R) class of sq_pass.h's launch_scan
struct ScanLaunch {
  const SqScanArgs& a;
  const IvfFlatPlan& p;
  hipStream_t s;
  template <int KIND, int CODEC, int G, int R>
  void launch() const {
    hipLaunchKernelGGL((k_sq_scan<KIND, CODEC, G, R>), dim3((unsigned)p.grid), dim3(256), 0, s, a.x, a.nq, a.d,
                       a.codes, a.nb, a.vmin, a.vdiff, a.tau, a.k, p.S, a.partD, a.partI);
  }
};

}  // namespace

void launch_sq_encode(int codec, const float* x, int64_t n, int d, const float* vmin, const float* vdiff,
                      uint8_t* codes, hipStream_t s) {
  const int64_t total = n * d;
  if (total <= 0) return;
  if (codec == SQ_CODEC_FP16)
    hipLaunchKernelGGL(k_sq_encode<SQ_CODEC_FP16>, dim3(elementwise_grid(total)), dim3(256), 0, s, x, total, d, vmin,
                       vdiff, codes);
  else
    hipLaunchKernelGGL(k_sq_encode<SQ_CODEC_8BIT>, dim3(elementwise_grid(total)), dim3(256), 0, s, x, total, d, vmin,
                       vdiff, codes);
}

void launch_sq_decode(int codec, const uint8_t* codes, int64_t n, int d, const float* vmin, const float* vdiff,
                      float* y, hipStream_t s) {
  const int64_t total = n * d;
  if (total <= 0) return;
  if (codec == SQ_CODEC_FP16)
    hipLaunchKernelGGL(k_sq_decode<SQ_CODEC_FP16>, dim3(elementwise_grid(total)), dim3(256), 0, s, codes, total, d,
                       vmin, vdiff, y);
  else
    hipLaunchKernelGGL(k_sq_decode<SQ_CODEC_8BIT>, dim3(elementwise_grid(total)), dim3(256), 0, s, codes, total, d,
                       vmin, vdiff, y);
}

void launch_sq_minmax_init(uint32_t* lo, uint32_t* hi, int d, hipStream_t s) {
  (void)hipMemsetAsync(lo, 0xff, sizeof(uint32_t) * d, s);
  (void)hipMemsetAsync(hi, 0, sizeof(uint32_t) * d, s);
}

void launch_sq_minmax(const float* x, int64_t n, int d, uint32_t* lo, uint32_t* hi, hipStream_t s) {
  if (n <= 0) return;
  const unsigned by = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(k_sq_minmax, dim3(nblocks(d, 256), by), dim3(256), 0, s, x, n, d, lo, hi);
}

void launch_sq_search(const SqScanArgs& a, const IvfFlatPlan& p, hipStream_t s) {
  if (a.nq <= 0) return;
  (void)hipMemsetAsync(a.tau, 0xff, sizeof(uint32_t) * a.nq, s);  // no bound yet
  // the partial lists no work item writes: those past the row ranges' kIvfFlatWaves each
  const int64_t written = sq_scan_ranges(a.nb) * kIvfFlatWaves;
  if (written < p.S) {
    const int64_t at = written * a.nq * a.k;
    launch_fill_empty(a.partD + at, a.partI + at, (int64_t)p.S * a.nq * a.k - at, a.ip, s);
  }
  launch_scan(a.ip, a.codec, a.k, ScanLaunch{a, p, s});
  merge_partial_lists(a.partD, a.partI, a.tmpD, a.tmpI, p.S, p.fan, a.nq, a.k, a.ip, a.D, a.I, s);
}

}  // namespace chivf
