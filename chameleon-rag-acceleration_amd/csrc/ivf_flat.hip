// gfx950 (MI355X, CDNA4) kernels for IVF over raw vectors (IndexIVFFlat).
//
// Faiss runs IndexIVFFlat::search as the coarse quantizer followed by IVFFlatScanner:
// fvec_L2sqr / fvec_inner_product of the query against every vector of every probed
// list, into a heap.  Here:
//  * k_ivfflat_plan buckets a batch's usable (query, probe) pairs by list and
//    k_ivfflat_items numbers the work items: (list, row range of at most
//    kIvfFlatRangeRows rows, up to G pairs);
//  * k_ivfflat_scan is list-major: a workgroup passes once over an item's rows for all
//    of its G queries.  Lanes are rows: a tile of 256 rows x 32 dimensions is staged
//    in LDS with coalesced 16-byte loads (the next one already in flight) and read
//    back one row per lane; the query values are wave-uniform and come through the
//    scalar cache.  Every lane carries Faiss's eight interleaved accumulators per
//    query from one 32-dimension step to the next, so the sum is tree<>'s whatever d;
//  * each wave keeps the k best (key, image position) of its rows in registers (the
//    wave top-k of scan_topk.h, the one of all three flat scans; inside one row range
//    position order is label order) and writes them sorted with
//    their int64 labels; launch_merge_topk, composed in rounds, merges the partial
//    lists by (key, label).  No distance is written to memory.
//    Waves that hold k rows lower a per-query bound (their k-th key) that every wave
//    reads at each tile, so that later work items of a query admit almost nothing.
//    k <= 64 merges a pass's admitted rows at once; k > 64 queues them in LDS per
//    (wave, query) and merges 64 at a time, as k_pq_scan does.
//    The tail of a pass -- distance terms, the fold to a key, admission, drain sites,
//    the sorted write -- is scan_topk.h's (admission, drain sites and write shared with
//    k_pq_scan); this file keeps the planning, the fp32 staging and the item numbering.
//  * launch_fill_empty (the result of an empty index) serves every float-distance index.
// Compiled with -ffp-contract=off like the rest of the library.
#include <float.h>
#include <stdint.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "ivf_flat.h"
#include "ivfpq_kernels.h"
#include "scan_topk.h"  // the wave top-k, the shared bound, the candidate queue, the pass tail, the merge rounds

namespace chivf {

namespace {

// -------------------------------------------------------------------- planning
__device__ __forceinline__ int range_count(int64_t rows) {
  return (int)((rows + kIvfFlatRangeRows - 1) / kIvfFlatRangeRows);
}

// One thread per query: its usable probes (list in range and non-empty, not a repeat
// of an earlier probe of the row when dedup) appended to their lists' buckets with the
// query's running slot number.  The order inside a bucket is the atomics' order; no
// result depends on it.  probe_of (nullable) receives the probe column of every entry.
__global__ __launch_bounds__(256) void k_ivfflat_plan(const int64_t* __restrict__ probes, int64_t nq, int nprobe,
                                                      const int64_t* __restrict__ list_off, int nlist, int dedup,
                                                      int32_t* __restrict__ cnt, int2* __restrict__ bucket,
                                                      int32_t* __restrict__ used, int32_t* __restrict__ probe_of) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const int64_t* row = probes + q * nprobe;
  int slot = 0;
  for (int p = 0; p < nprobe; p++) {
    const int64_t l = row[p];
    if (l < 0 || l >= nlist) continue;
    const int64_t rows = list_off[l + 1] - list_off[l];
    if (rows <= 0) continue;
    if (dedup) {
      bool seen = false;
      for (int p2 = 0; p2 < p; p2++) seen |= row[p2] == l;
      if (seen) continue;
    }
    const int at = atomicAdd(&cnt[l], 1);  // < nq: a list holds at most one pair per query
    bucket[l * nq + at] = make_int2((int)q, slot);
    if (probe_of) probe_of[l * nq + at] = p;
    slot += range_count(rows);
  }
  used[q] = slot;
}

// item_off[l] = work items of the lists below l: list l has ceil(pairs / G) groups times
// its row ranges.  One workgroup; each thread sums a contiguous run of lists.
__global__ __launch_bounds__(256) void k_ivfflat_items(const int32_t* __restrict__ cnt,
                                                       const int64_t* __restrict__ list_off, int nlist, int G,
                                                       int32_t* __restrict__ item_off) {
  __shared__ int part[256];
  const int tid = threadIdx.x;
  const int per = (nlist + 255) / 256;
  const int l0 = min(tid * per, nlist), l1 = min(l0 + per, nlist);
  auto items = [&](int l) { return (cnt[l] + G - 1) / G * range_count(list_off[l + 1] - list_off[l]); };
  int sum = 0;
  for (int l = l0; l < l1; l++) sum += items(l);
  part[tid] = sum;
  __syncthreads();
  int base = 0;
  for (int t = 0; t < tid; t++) base += part[t];
  for (int l = l0; l < l1; l++) {
    item_off[l] = base;
    base += items(l);
  }
  if (tid == 255) item_off[nlist] = base;
}

// the partial lists no work item writes: slots from used[q] up
__global__ __launch_bounds__(256) void k_ivfflat_pad(const int32_t* __restrict__ used, int64_t nq, int k, int S,
                                                     float pad, float* __restrict__ partD,
                                                     int64_t* __restrict__ partI) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)S * nq * k) return;
  const int64_t sq = gid / k;
  const int s = (int)(sq / nq);
  const int64_t q = sq - (int64_t)s * nq;
  if (s < used[q] * kIvfFlatWaves) return;
  partD[gid] = pad;
  partI[gid] = -1;
}

// (pad, -1) over n entries: launch_fill_empty, for every float-distance index
__global__ __launch_bounds__(256) void k_fill_empty(float* __restrict__ D, int64_t* __restrict__ I, int64_t n,
                                                    float pad) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= n) return;
  D[gid] = pad;
  I[gid] = -1;
}

// ------------------------------------------------------------------------ scan
using f4 = float __attribute__((ext_vector_type(4)));  // a 16-byte load or LDS access, held in registers

constexpr int kDc = 32;             // dimensions per staged step (a multiple of 8)
constexpr int kRowStride = kDc + 4; // floats per LDS row: 16-byte aligned, and consecutive rows start 4 banks apart
constexpr int kTile = 256;          // rows per pass: one per thread
constexpr int kLoads = kTile * kDc / 4 / 256;  // 16-byte loads per thread and step
constexpr int kQ = kQueue<1>;       // queued candidates per (wave, query): one push per lane and pass

// Persistent over work items: workgroup b takes items b, b + gridDim.x, ...
// LDS: the 36 KiB tile, plus G KiB of candidate queues per wave when R > 1.
template <int KIND, int G, int R>
__global__ __launch_bounds__(256) void k_ivfflat_scan(const float* __restrict__ x, int64_t nq, int d,
                                                      const float* __restrict__ vecs, const int64_t* __restrict__ ids,
                                                      const int64_t* __restrict__ list_off, int nlist,
                                                      const int32_t* __restrict__ cnt, const int2* __restrict__ bucket,
                                                      const int32_t* __restrict__ item_off, uint32_t* tau,
                                                      int k, int S, float* __restrict__ partD, int64_t* __restrict__ partI) {
  __shared__ __attribute__((aligned(16))) float tile[kTile * kRowStride];
  constexpr bool kQueued = R > 1;
  __shared__ float qd[kQueued ? kIvfFlatWaves * G * kQ : 1];
  __shared__ int qi[kQueued ? kIvfFlatWaves * G * kQ : 1];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int nchunk = (d + kDc - 1) / kDc;
  const int total = item_off[nlist];

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
    // range-major within the list: the groups of one row range are neighbours in the item
    // order, run at about the same time and find the range's rows in the L2
    const int local = item - item_off[l];
    const int groups = (cnt[l] + G - 1) / G;
    const int rng = local / groups;
    const int grp = local - rng * groups;
    const int npair = min(G, cnt[l] - grp * G);  // >= 1
    const int64_t r0 = lb + (int64_t)rng * kIvfFlatRangeRows;
    const int64_t r1 = min(lb + lrows, r0 + kIvfFlatRangeRows);
    int qid[G], slot[G];  // pairs past npair repeat the first (their sums are dropped)
#pragma unroll
    for (int g = 0; g < G; g++) {
      const int2 e = bucket[(int64_t)l * nq + grp * G + (g < npair ? g : 0)];
      qid[g] = __builtin_amdgcn_readfirstlane(e.x);
      slot[g] = __builtin_amdgcn_readfirstlane(e.y) + rng;
    }

    WaveTopK<R> tk[G];
#pragma unroll
    for (int g = 0; g < G; g++) tk[g].init(k);
    int qn[G];  // queue fills (wave-uniform, < 64 between passes)
#pragma unroll
    for (int g = 0; g < G; g++) qn[g] = 0;

    // step (t0, c): dimensions [c * kDc, +len) of rows [t0, t0 + kTile); rows past the
    // range re-read its last row (their sums are dropped at the admission)
    f4 nxt[kLoads];
    auto fetch = [&](int64_t t0, int c) __attribute__((always_inline)) {
      const int len4 = min(kDc, d - c * kDc) >> 2;
#pragma unroll
      for (int i = 0; i < kLoads; i++) {
        const int e = i * 256 + tid;
        const int row = e >> 3, c4 = e & 7;
        const int64_t grow = min(t0 + row, r1 - 1);
        // (columns past a short last step re-read its first: staged, never used)
        nxt[i] = *reinterpret_cast<const f4*>(vecs + grow * d + c * kDc + (c4 < len4 ? c4 : 0) * 4);
      }
    };
    fetch(r0, 0);

    float acc[G][8];
#pragma unroll
    for (int g = 0; g < G; g++)
#pragma unroll
      for (int j = 0; j < 8; j++) acc[g][j] = 0.f;

    for (int64_t t0 = r0; t0 < r1; t0 += kTile) {
#pragma unroll
      for (int g = 0; g < G; g++) tk[g].set_cap(tau_get(tau + qid[g]));
      for (int c = 0; c < nchunk; c++) {
        const int len = min(kDc, d - c * kDc);
        __syncthreads();  // the previous step's reads are done
#pragma unroll
        for (int i = 0; i < kLoads; i++) {
          const int e = i * 256 + tid;
          const int row = e >> 3, c4 = e & 7;
          *reinterpret_cast<f4*>(&tile[row * kRowStride + c4 * 4]) = nxt[i];
        }
        __syncthreads();
        if (c + 1 < nchunk) fetch(t0, c + 1);
        else if (t0 + kTile < r1) fetch(t0 + kTile, 0);

        const float* yrow = &tile[tid * kRowStride];
        const int n8 = len >> 3;
        for (int j8 = 0; j8 < n8; j8++) {
          const f4 y0 = *reinterpret_cast<const f4*>(yrow + j8 * 8);
          const f4 y1 = *reinterpret_cast<const f4*>(yrow + j8 * 8 + 4);
          const float y[8] = {y0.x, y0.y, y0.z, y0.w, y1.x, y1.y, y1.z, y1.w};
          accumulate8<KIND>(acc, y, x, d, qid, c * kDc + j8 * 8);
        }
        if (c + 1 < nchunk) continue;

        // the row's last step: its key (with the 4-wide remainder), then the admission
        const int64_t rowpos = t0 + tid;
        const bool rem = (len & 4) != 0;
        f4 yr = {0.f, 0.f, 0.f, 0.f};
        if (rem) yr = *reinterpret_cast<const f4*>(yrow + n8 * 8);
        const float y[4] = {yr.x, yr.y, yr.z, yr.w};
#pragma unroll
        for (int g = 0; g < G; g++) {
          const float key = fold_key<KIND>(acc[g], rem, x + (int64_t)qid[g] * d + c * kDc + n8 * 8, y);
          if (g >= npair) continue;  // uniform
          if (admit<R>(tk[g], rowpos < r1, key, (int)rowpos, qn[g], qd + (wave * G + g) * kQ, qi + (wave * G + g) * kQ,
                       lane))
            tk[g].publish(tau + qid[g], lane);
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

inline int scan_group_for(int k) { return k <= 64 ? 8 : 4; }

template <int KIND, int G, int R>
void launch_scan(const IvfFlatArgs& a, const IvfFlatPlan& p, hipStream_t s) {
  hipLaunchKernelGGL((k_ivfflat_scan<KIND, G, R>), dim3((unsigned)p.grid), dim3(256), 0, s, a.x, a.nq, a.d, a.vecs,
                     a.ids, a.list_off, a.nlist, a.cnt, a.bucket, a.item_off, a.tau, a.k, p.S, a.partD, a.partI);
}
template <int KIND>
void launch_scan_kind(const IvfFlatArgs& a, const IvfFlatPlan& p, hipStream_t s) {
  switch (scan_rows_for(a.k)) {
    case 1: launch_scan<KIND, 8, 1>(a, p, s); break;
    case 4: launch_scan<KIND, 4, 4>(a, p, s); break;
    default: launch_scan<KIND, 4, 16>(a, p, s); break;
  }
}

}  // namespace

IvfFlatPlan ivfflat_plan(int k, int64_t slots) {
  IvfFlatPlan p;
  p.G = scan_group_for(k);
  int fan = 2;
  while (fan * 2 <= kIvfFlatMergeFan && fan * 2 * k <= kIvfFlatMergeEntries) fan *= 2;
  p.fan = fan;
  const int64_t need = std::max<int64_t>(1, slots) * kIvfFlatWaves;
  int64_t S = need;
  if (need > fan) {  // several rounds: every round's list count is a multiple of its fan
    S = fan;
    while (S < need) S *= 2;
  }
  p.S = (int)S;
  // eight workgroups per CU's worth of starting points on 256 CUs: items are taken
  // grid apart, so late workgroups start as early ones finish
  p.grid = 2048;
  return p;
}

void launch_fill_empty(float* D, int64_t* I, int64_t n, bool ip, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_fill_empty, dim3(nblocks(n, 256)), dim3(256), 0, s, D, I, n, ip ? -FLT_MAX : FLT_MAX);
}

void launch_ivfflat_planning(const IvfFlatArgs& a, const IvfFlatPlan& p, int32_t* probe_of, hipStream_t s) {
  (void)hipMemsetAsync(a.cnt, 0, sizeof(int32_t) * a.nlist, s);
  (void)hipMemsetAsync(a.tau, 0xff, sizeof(uint32_t) * a.nq, s);  // no bound yet
  hipLaunchKernelGGL(k_ivfflat_plan, dim3(nblocks(a.nq, 256)), dim3(256), 0, s, a.probes, a.nq, a.nprobe, a.list_off,
                     a.nlist, a.dedup ? 1 : 0, a.cnt, a.bucket, a.used, probe_of);
  hipLaunchKernelGGL(k_ivfflat_items, dim3(1), dim3(256), 0, s, a.cnt, a.list_off, a.nlist, p.G, a.item_off);
  hipLaunchKernelGGL(k_ivfflat_pad, dim3(nblocks((int64_t)p.S * a.nq * a.k, 256)), dim3(256), 0, s, a.used, a.nq, a.k,
                     p.S, a.ip ? -FLT_MAX : FLT_MAX, a.partD, a.partI);
}

void launch_ivfflat_search(const IvfFlatArgs& a, const IvfFlatPlan& p, hipStream_t s) {
  if (a.nq <= 0) return;
  launch_ivfflat_planning(a, p, nullptr, s);
  if (a.ip)
    launch_scan_kind<K_IP>(a, p, s);
  else
    launch_scan_kind<K_L2>(a, p, s);
  merge_partial_lists(a.partD, a.partI, a.tmpD, a.tmpI, p.S, p.fan, a.nq, a.k, a.ip, a.D, a.I, s);
}

}  // namespace chivf
