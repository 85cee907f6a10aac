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
//    bitonic wave top-k of ivfpq_kernels.hip, restated here for int32 positions;
//    inside one row range position order is label order) and writes them sorted with
//    their int64 labels; launch_merge_topk, composed in rounds, merges the partial
//    lists by (key, label).  No distance is written to memory.
//    Waves that hold k rows lower a per-query bound (their k-th key) that every wave
//    reads at each tile, so that later work items of a query admit almost nothing.
//    k <= 64 merges a pass's admitted rows at once; k > 64 queues them in LDS per
//    (wave, query) and merges 64 at a time, as k_pq_scan does.
// Compiled with -ffp-contract=off like the rest of the library.
#include <float.h>
#include <stdint.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "ivf_flat.h"
#include "ivfpq_kernels.h"

namespace chivf {

namespace {

constexpr float kInf = __builtin_huge_valf();
constexpr int kNone = INT32_MAX;  // "no candidate" position (real positions are < 2^31 - 1)

enum { K_IP = 0, K_L2 = 1 };

// ---- wave top-k in registers (int32 positions) ---------------------------------
__device__ __forceinline__ bool lexless(float ad, int ai, float bd, int bi) {
  return (ad < bd) | ((ad == bd) & (ai < bi));
}
__device__ __forceinline__ float readlane_f(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
template <int CTRL>
__device__ __forceinline__ int dmov(int v) {
  return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, false);
}
// lane ^ J exchange on the VALU: DPP for J <= 8, the gfx950 row / half swaps above
template <int J>
__device__ __forceinline__ int xor_i(int v) {
  if constexpr (J == 1) return dmov<0xB1>(v);
  else if constexpr (J == 2) return dmov<0x4E>(v);
  else if constexpr (J == 4) return dmov<0x1B>(dmov<0x141>(v));
  else if constexpr (J == 8) return dmov<0x128>(v);
  else if constexpr (J == 16) {
    const auto r = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
    return (int)((__lane_id() & 16) ? r[0] : r[1]);
  } else {
    const auto r = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
    return (int)((__lane_id() & 32) ? r[0] : r[1]);
  }
}
template <int J>
__device__ __forceinline__ float xor_f(float v) { return __int_as_float(xor_i<J>(__float_as_int(v))); }
__device__ __forceinline__ int rev64_i(int v) { return xor_i<16>(xor_i<32>(dmov<0x140>(v))); }
__device__ __forceinline__ float rev64_f(float v) { return __int_as_float(rev64_i(__float_as_int(v))); }

// A wave's running k best (key, position) pairs, sorted ascending across R rows x 64
// lanes (logical index r * 64 + lane); k <= 64 * R.
template <int R>
struct WaveTopK {
  float d[R];
  int id[R];
  float td;  // the admission threshold: the current k-th best, or the query's shared bound where that is lower
  int ti;
  int krow, klane;
  float cap;  // the query's shared bound as last read (every key above it is outside the final top-k)
  float pub;  // the k-th best this wave last published to the shared bound

  __device__ __forceinline__ void init(int k) {
#pragma unroll
    for (int r = 0; r < R; r++) {
      d[r] = kInf;
      id[r] = kNone;
    }
    td = kInf;
    ti = kNone;
    cap = kInf;
    pub = kInf;
    krow = (k - 1) >> 6;
    klane = (k - 1) & 63;
  }
  // a key equal to the bound may still be among the k best (ties go by label): (c, none) admits it
  __device__ __forceinline__ void set_cap(float c) {
    cap = fminf(cap, c);
    if (td > cap) {
      td = cap;
      ti = kNone;
    }
  }
  __device__ __forceinline__ void refresh_tau() {
#pragma unroll
    for (int r = 0; r < R; r++) {
      if (r == krow) {
        td = readlane_f(d[r], klane);
        ti = __builtin_amdgcn_readlane(id[r], klane);
      }
    }
    if (td > cap) {
      td = cap;
      ti = kNone;
    }
  }
  // once the wave holds k rows, its k-th key bounds the query's final k-th key: lower the shared bound to it
  __device__ __forceinline__ void publish(uint32_t* tau_q, int lane);
};

template <int KK, int J>
__device__ __forceinline__ void bitonic_step(float& cd, int& ci, int lane) {
  const float od = xor_f<J>(cd);
  const int oi = xor_i<J>(ci);
  const bool want_min = ((lane & J) == 0) == ((lane & KK) == 0);
  const bool o_lt = lexless(od, oi, cd, ci);
  const bool c_lt = lexless(cd, ci, od, oi);
  const bool take = (want_min & o_lt) | (!want_min & c_lt);
  cd = take ? od : cd;
  ci = take ? oi : ci;
}
template <int KK, int J>
__device__ __forceinline__ void bitonic_steps(float& cd, int& ci, int lane) {
  if constexpr (J >= 1) {
    bitonic_step<KK, J>(cd, ci, lane);
    bitonic_steps<KK, J / 2>(cd, ci, lane);
  }
}
template <int KK>
__device__ __forceinline__ void bitonic_sort64(float& cd, int& ci, int lane) {
  if constexpr (KK <= 64) {
    bitonic_steps<KK, KK / 2>(cd, ci, lane);
    bitonic_sort64<KK * 2>(cd, ci, lane);
  }
}

// Merge up to 64 candidates (one per lane; (inf, none) = no candidate) into the R-row
// top-k: bitonic sort of the candidates, then per row the reverse-min + bitonic merge,
// the upper half carried to the next row.
template <int R>
__device__ __forceinline__ void bulk_merge_rows(WaveTopK<R>& tk, float cd, int ci, int lane) {
  bitonic_sort64<2>(cd, ci, lane);
#pragma unroll
  for (int r = 0; r < R; r++) {
    const float rd = rev64_f(cd);
    const int ri = rev64_i(ci);
    const bool t = lexless(rd, ri, tk.d[r], tk.id[r]);
    const float lo_d = t ? rd : tk.d[r], hi_d = t ? tk.d[r] : rd;
    const int lo_i = t ? ri : tk.id[r], hi_i = t ? tk.id[r] : ri;
    tk.d[r] = lo_d;
    tk.id[r] = lo_i;
    bitonic_steps<128, 32>(tk.d[r], tk.id[r], lane);  // KK = 128: every lane ascending
    if (r + 1 < R) {
      cd = hi_d;
      ci = hi_i;
      bitonic_steps<128, 32>(cd, ci, lane);
    }
  }
  tk.refresh_tau();
}

// The shared bound of a query: the lowest k-th key any wave has reached so far in this
// batch, as order-preserving bits lowered by atomicMin (all-ones = none yet).  It only
// prunes: a row above it cannot be among the k best, whichever waves have published, so
// the merged result does not depend on the timing.  Read once per wave (readfirstlane).
__device__ __forceinline__ uint32_t key_bits(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float tau_get(const uint32_t* tau_q) {
  const uint32_t u = __builtin_amdgcn_readfirstlane(
      __hip_atomic_load(tau_q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  return u == 0xFFFFFFFFu ? kInf : __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}
template <int R>
__device__ __forceinline__ void WaveTopK<R>::publish(uint32_t* tau_q, int lane) {
  float kth = kInf;
#pragma unroll
  for (int r = 0; r < R; r++)
    if (r == krow) kth = readlane_f(d[r], klane);
  if (kth < pub) {  // uniform
    pub = kth;
    if (lane == 0) __hip_atomic_fetch_min(tau_q, key_bits(kth), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// -------------------------------------------------------------------- planning
__device__ __forceinline__ int range_count(int64_t rows) {
  return (int)((rows + kIvfFlatRangeRows - 1) / kIvfFlatRangeRows);
}

// One thread per query: its usable probes (list in range and non-empty, not a repeat
// of an earlier probe of the row when dedup) appended to their lists' buckets with the
// query's running slot number.  The order inside a bucket is the atomics' order; no
// result depends on it.
__global__ __launch_bounds__(256) void k_ivfflat_plan(const int64_t* __restrict__ probes, int64_t nq, int nprobe,
                                                      const int64_t* __restrict__ list_off, int nlist, int dedup,
                                                      int32_t* __restrict__ cnt, int2* __restrict__ bucket,
                                                      int32_t* __restrict__ used) {
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

__global__ __launch_bounds__(256) void k_ivfflat_fill_empty(float* __restrict__ D, int64_t* __restrict__ I, int64_t n,
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
constexpr int kQueue = 64 + 64;     // queued candidates per (wave, query): < 64 pending + a pass's pushes

// The first min(n, 64) candidates of a wave's queue (q_d, q_i) into its top-k, the
// rest moved to the front; n becomes the number left.
template <int R>
__device__ __forceinline__ void drain_queue(WaveTopK<R>& tk, int& n, float* q_d, int* q_i, int lane) {
  __builtin_amdgcn_wave_barrier();
  const bool have = lane < n;
  const float cd = have ? q_d[lane] : kInf;
  const int ci = have ? q_i[lane] : kNone;
  const int rem = max(n - 64, 0);
  const bool mv = lane < rem;
  const float md = mv ? q_d[64 + lane] : kInf;
  const int mi = mv ? q_i[64 + lane] : kNone;
  __builtin_amdgcn_wave_barrier();
  if (mv) {
    q_d[lane] = md;
    q_i[lane] = mi;
  }
  __builtin_amdgcn_wave_barrier();
  n = rem;
  const bool pass = lexless(cd, ci, tk.td, tk.ti);  // the bound may have moved since the push
  if (__ballot(pass)) bulk_merge_rows<R>(tk, pass ? cd : kInf, pass ? ci : kNone, lane);
}

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
  __shared__ float qd[kQueued ? kIvfFlatWaves * G * kQueue : 1];
  __shared__ int qi[kQueued ? kIvfFlatWaves * G * kQueue : 1];
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
#pragma unroll
          for (int g = 0; g < G; g++) {
            const float* qp = x + (int64_t)qid[g] * d + c * kDc + j8 * 8;  // wave-uniform
#pragma unroll
            for (int j = 0; j < 8; j++) {
              float p;
              if (KIND == K_IP) {
                p = qp[j] * y[j];
              } else {
                const float t = qp[j] - y[j];
                p = t * t;
              }
              acc[g][j] = acc[g][j] + p;
            }
          }
        }
        if (c + 1 < nchunk) continue;

        // the row's last step: fold to four, the 4-wide remainder, two horizontal adds
        const int64_t rowpos = t0 + tid;
        const bool valid = rowpos < r1;
        const bool rem = (len & 4) != 0;
        f4 yr = {0.f, 0.f, 0.f, 0.f};
        if (rem) yr = *reinterpret_cast<const f4*>(yrow + n8 * 8);
        const float y[4] = {yr.x, yr.y, yr.z, yr.w};
#pragma unroll
        for (int g = 0; g < G; g++) {
          float a4[4];
#pragma unroll
          for (int j = 0; j < 4; j++) a4[j] = acc[g][j + 4] + acc[g][j];
          if (rem) {
            const float* qp = x + (int64_t)qid[g] * d + c * kDc + n8 * 8;
#pragma unroll
            for (int j = 0; j < 4; j++) {
              float p;
              if (KIND == K_IP) {
                p = qp[j] * y[j];
              } else {
                const float t = qp[j] - y[j];
                p = t * t;
              }
              a4[j] = a4[j] + p;
            }
          }
          const float h0 = a4[0] + a4[1];
          const float h1 = a4[2] + a4[3];
          const float dis = h0 + h1;
          const float key = KIND == K_IP ? -dis : dis;
#pragma unroll
          for (int j = 0; j < 8; j++) acc[g][j] = 0.f;
          if (g >= npair) continue;  // uniform
          // admission against the query's running k-th best
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
              const int at = (wave * G + g) * kQueue + qn[g] + before;
              qd[at] = key;
              qi[at] = (int)rowpos;
            }
            qn[g] += __popcll(mask);
          }
        }
        if constexpr (kQueued) {
          // one drain site per query: full batches of 64 after every pass, the rest after the last
          const int keep = t0 + kTile < r1 ? 63 : 0;
          // (spelled out per query: a loop over g around R = 16 merges is past the
          // compiler's unroll budget, and the top-k arrays would then live in scratch)
          static_assert(G <= 4, "drain sites are spelled out for up to four queries");
#define IVFFLAT_DRAIN(g)                                                                                  \
  if constexpr (G > g) {                                                                                  \
    while (qn[g] > keep)                                                                                  \
      drain_queue<R>(tk[g], qn[g], qd + (wave * G + g) * kQueue, qi + (wave * G + g) * kQueue, lane);     \
    tk[g].publish(tau + qid[g], lane);                                                                    \
  }
          IVFFLAT_DRAIN(0);
          IVFFLAT_DRAIN(1);
          IVFFLAT_DRAIN(2);
          IVFFLAT_DRAIN(3);
#undef IVFFLAT_DRAIN
        }
      }
    }

    // this wave's sorted list of every pair, labels looked up from the positions
#pragma unroll
    for (int g = 0; g < G; g++) {
      if (g >= npair || slot[g] * kIvfFlatWaves + wave >= S) continue;  // (the host's slot bound holds)
      const int64_t base = (((int64_t)slot[g] * kIvfFlatWaves + wave) * nq + qid[g]) * k;
#pragma unroll
      for (int r = 0; r < R; r++) {
        const int idx = r * 64 + lane;
        if (idx < k) {
          const int pos = tk[g].id[r];
          const bool none = pos == kNone;
          const float key = tk[g].d[r];
          partD[base + idx] = none ? (KIND == K_IP ? -FLT_MAX : FLT_MAX) : (KIND == K_IP ? -key : key);
          partI[base + idx] = none ? -1 : ids[pos];
        }
      }
    }
  }
}

inline unsigned nblocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

inline int scan_rows_for(int k) { return k <= 64 ? 1 : k <= 256 ? 4 : 16; }
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

void launch_ivfflat_fill_empty(float* D, int64_t* I, int64_t n, bool ip, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_ivfflat_fill_empty, dim3(nblocks(n, 256)), dim3(256), 0, s, D, I, n, ip ? -FLT_MAX : FLT_MAX);
}

void launch_ivfflat_search(const IvfFlatArgs& a, const IvfFlatPlan& p, hipStream_t s) {
  if (a.nq <= 0) return;
  (void)hipMemsetAsync(a.cnt, 0, sizeof(int32_t) * a.nlist, s);
  (void)hipMemsetAsync(a.tau, 0xff, sizeof(uint32_t) * a.nq, s);  // no bound yet
  hipLaunchKernelGGL(k_ivfflat_plan, dim3(nblocks(a.nq, 256)), dim3(256), 0, s, a.probes, a.nq, a.nprobe, a.list_off,
                     a.nlist, a.dedup ? 1 : 0, a.cnt, a.bucket, a.used);
  hipLaunchKernelGGL(k_ivfflat_items, dim3(1), dim3(256), 0, s, a.cnt, a.list_off, a.nlist, p.G, a.item_off);
  hipLaunchKernelGGL(k_ivfflat_pad, dim3(nblocks((int64_t)p.S * a.nq * a.k, 256)), dim3(256), 0, s, a.used, a.nq, a.k,
                     p.S, a.ip ? -FLT_MAX : FLT_MAX, a.partD, a.partI);
  if (a.ip)
    launch_scan_kind<K_IP>(a, p, s);
  else
    launch_scan_kind<K_L2>(a, p, s);
  // Merge rounds.  A round over S lists [S][nq][k] with fan f merges, for every j below
  // S / f, the lists j, j + S / f, j + 2 S / f, ... -- read as [f][nq * S / f][k] they are
  // one launch_merge_topk call whose output is the next round's [S / f][nq][k].
  const float* inD = a.partD;
  const int64_t* inI = a.partI;
  int S = p.S;
  bool to_tmp = true;
  while (true) {
    const int f = std::min(S, p.fan);
    const int left = S / f;
    if (left == 1) {
      launch_merge_topk(f, a.nq, a.k, inD, inI, a.D, a.I, s, a.ip);
      break;
    }
    float* outD = to_tmp ? a.tmpD : a.partD;
    int64_t* outI = to_tmp ? a.tmpI : a.partI;
    launch_merge_topk(f, a.nq * left, a.k, inD, inI, outD, outI, s, a.ip);
    inD = outD;
    inI = outI;
    S = left;
    to_tmp = !to_tmp;
  }
}

}  // namespace chivf
