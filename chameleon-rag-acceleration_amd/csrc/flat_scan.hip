// gfx950 (MI355X, CDNA4) kernel of the flat index (IndexFlat / IndexFlatL2 / IndexFlatIP):
// exact brute-force search over the device-resident row image with the top-k fused in.
//
// k_flat_scan: a workgroup takes a tile of 64 queries and one row range of the base and
// walks the range 128 rows at a time.  Per pass the 64 x 128 inner products are accumulated
// on the matrix cores in the tiling of tiled_key_acc (ivfpq_kernels.hip): wave w owns the
// queries 16 w .. 16 w + 15 against all 128 rows (8 tiles of v_mfma_f32_16x16x4_f32), the A
// (queries) and B (base rows) k chunks of 32 dimensions are staged in LDS, double-buffered.
// Both operands are staged row-major -- a lane's MFMA operand is element 4 j + k4 of row
// i16, the same read for A and B -- so the base needs no transposed copy.  Every product is
// one ascending-k chain into one accumulator (no split-K; k is padded with zeros, and
// fma(0, 0, acc) == acc), which rounds like launch_l2_dist's fmaf chain bit for bit.
// The keys (coarse_key's arithmetic: max(0, (|x|^2 + |y|^2) - 2 dot), or -dot) then pass
// through LDS -- the tile aliases the B staging buffers, free between passes -- and every
// wave reads back one query's 128 keys at a time, one row per lane, into that query's wave
// top-k (scan_topk.h) under the query's shared bound tau_q; a key equal to the bound is
// admitted, so the result does not depend on which workgroup published first.  Each
// (range, query) writes one sorted partial list; merge_partial_lists reduces them.  No
// distance is written to global memory.
// Compiled with -ffp-contract=off like the rest of the library.
#include <float.h>
#include <stdint.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "flat_scan.h"
#include "ivf_flat.h"  // launch_fill_empty
#include "ivfpq_kernels.h"
#include "scan_topk.h"

namespace chivf {

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int TR = kFlatTileRows, KC = kFlatKc;
constexpr int TS = KC + 2;        // row stride of a staged tile (floats): 2 mod 32 -> conflict-free MFMA operand reads
constexpr int KS = TR + 4;        // row stride of the key tile
static_assert(kFlatTileQ * KS <= 2 * TR * TS, "the key tile aliases the B staging buffers");
static_assert(kFlatTileQ == 64 && kFlatTileQNarrow == 16 && TR == 128 && KC == 32,
              "the staging below is written for these");

// four consecutive floats of a row at dimension kk, zeros past d, without a branch: the
// addresses are clamped into the row and the values selected.  VEC: d % 4 == 0 and the rows
// are 16-byte aligned.
template <bool VEC>
__device__ __forceinline__ f4 load4(const float* __restrict__ row, int kk, int d) {
  f4 v;
  if constexpr (VEC) {
    v = *reinterpret_cast<const f4*>(row + min(kk, d - 4));
    if (kk >= d) v = f4{0.f, 0.f, 0.f, 0.f};
  } else {
    const float a = row[min(kk, d - 1)], b = row[min(kk + 1, d - 1)], c = row[min(kk + 2, d - 1)],
                e = row[min(kk + 3, d - 1)];
    v.x = kk < d ? a : 0.f;
    v.y = kk + 1 < d ? b : 0.f;
    v.z = kk + 2 < d ? c : 0.f;
    v.w = kk + 3 < d ? e : 0.f;
  }
  return v;
}

__device__ __forceinline__ float tau_decode(uint32_t u) {
  return u == 0xFFFFFFFFu ? kInf : __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

// the key from <x, y> (coarse_key of ivfpq_kernels.hip)
__device__ __forceinline__ float flat_key(float dot, float xn, float yn, int ip) {
  if (ip) return -dot;
  const float v = (xn + yn) - 2.0f * dot;
  return v < 0.f ? 0.f : v;
}

// grid: query tile fastest (the workgroups that run together share a row range, which then
// comes from HBM once), ranges slowest.  LDS: 17 KiB (4 KiB) of A staging + 34 KiB of B
// staging, and at k > 64 96 KiB (24 KiB) of candidate queues, 1.5 KiB per query.
// Waves per SIMD = workgroups per CU asked of the register allocator: three at k <= 64 with
// aligned rows (168 registers), two with unaligned rows (scalar staging loads) or with the
// narrow tile's queues at k <= 256 (62 KiB of LDS), one where a wave's lists alone are 128
// registers (16 queries of four rows, 4 queries of sixteen).
//
// TQ = 64 is the tiling above.  TQ = 16 (the narrow tile: batches of at most 16 queries, where
// three quarters of a 64-query tile would be padding, and k > 256, where only four queries'
// sixteen-row lists fit a wave's registers) splits the pass the other way: every wave takes all
// 16 queries against 32 of the 128 rows (2 MFMA tiles), and after the barrier wave w keeps
// the lists of the queries 4 w .. 4 w + 3 over all 128 rows.
template <int R, bool VEC, int TQ>
__global__ __launch_bounds__(256, (TQ / 4) * R > 16 ? 1 : R > 1 ? 2 : VEC ? 3 : 2) void k_flat_scan(
    const float* __restrict__ x, const float* __restrict__ xn, int64_t nq, int d, const float* __restrict__ base,
    const float* __restrict__ bn, int64_t nb, int64_t range_rows, int nqt, int ip, uint32_t* tau, int k,
    float* __restrict__ partD, int64_t* __restrict__ partI) {
  constexpr int QW = TQ / 4;                 // queries whose lists a wave keeps
  constexpr int NT = TQ == 64 ? TR / 16 : 2;  // 16 x 16 MFMA tiles per wave and pass
  __shared__ __attribute__((aligned(16))) float As[2][TQ * TS];
  __shared__ __attribute__((aligned(16))) float Bs[2][TR * TS];
  float* kt = &Bs[0][0];  // [TQ][KS] keys of a pass
  // k > 64: the candidate queue of every (wave, query), as in k_ivfflat_scan -- a pass pushes
  // at most two rows per lane behind fewer than 64 pending ones, and 64 candidates are merged
  // at a time
  constexpr bool kQueued = R > 1;
  constexpr int kQ = kQueue<2>;
  __shared__ float qd[kQueued ? TQ * kQ : 1];
  __shared__ int qi[kQueued ? TQ * kQ : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, k4 = lane >> 4;
  const int rng = blockIdx.x / nqt;
  // queries and row positions in 32 bits (nq of a launch and nb are below 2^31 - 1; unsigned,
  // so that a tile start past the last range's end cannot overflow): 64 bits only where a
  // row's address is formed
  const uint32_t nqu = (uint32_t)nq;
  const uint32_t q0 = (blockIdx.x - rng * nqt) * TQ;
  const int arow0 = TQ == 64 ? wave * 16 : 0;  // the wave's MFMA operand rows: queries ...
  const int brow0 = TQ == 64 ? 0 : wave * 32;  // ... and base rows of the pass
  const uint32_t r0 = (uint32_t)((int64_t)rng * range_rows);
  const uint32_t r1 = (uint32_t)min(nb, (int64_t)r0 + range_rows);

  // staging: thread t loads A row t >> 2, dimensions 8 (t & 3) .. + 7 and B row t >> 1,
  // dimensions 16 (t & 1) .. + 15 of the chunk; queries past nq and rows past the range
  // re-read the last one (their keys are dropped), dimensions past d read as 0
  const int ar = tid >> 2, ak = (tid & 3) * 8;
  const int br = tid >> 1, bk = (tid & 1) * 16;
  const bool astage = ar < TQ;  // (the narrow tile: wave 0 stages all of A)
  const float* arow = x + (int64_t)min(q0 + (astage ? ar : 0), nqu - 1) * d;
  f4 ra[2], rb[4];
  auto fetch = [&](uint32_t t0, int kc) __attribute__((always_inline)) {
    const float* brow = base + (int64_t)min(t0 + br, r1 - 1) * d;
    if (astage) {  // wave-uniform
#pragma unroll
      for (int i = 0; i < 2; i++) ra[i] = load4<VEC>(arow, kc * KC + ak + 4 * i, d);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) rb[i] = load4<VEC>(brow, kc * KC + bk + 4 * i, d);
  };
  auto stage = [&](int b) __attribute__((always_inline)) {
    if (astage) {
      float2* ap = reinterpret_cast<float2*>(&As[b][ar * TS + ak]);
#pragma unroll
      for (int i = 0; i < 2; i++) {
        ap[2 * i] = make_float2(ra[i].x, ra[i].y);
        ap[2 * i + 1] = make_float2(ra[i].z, ra[i].w);
      }
    }
    float2* bp = reinterpret_cast<float2*>(&Bs[b][br * TS + bk]);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      bp[2 * i] = make_float2(rb[i].x, rb[i].y);
      bp[2 * i + 1] = make_float2(rb[i].z, rb[i].w);
    }
  };

  // the running k best of the wave's 16 queries: only the sorted rows live across passes; the
  // wave-uniform state of a WaveTopK (threshold, bound) is rebuilt at every visit from the
  // k-th entry and the query's shared bound, so it does not occupy 64 scalar registers
  float kd[QW][R];
  int ki[QW][R];
#pragma unroll
  for (int g = 0; g < QW; g++)
#pragma unroll
    for (int r = 0; r < R; r++) {
      kd[g][r] = kInf;
      ki[g][r] = kNone;
    }
  int qn[QW];  // queue fills (wave-uniform, < 64 between passes)
#pragma unroll
  for (int g = 0; g < QW; g++) qn[g] = 0;

  // |x|^2 of the wave's queries, one per lane below QW (read back per query with readlane)
  const float xnl = xn[min(q0 + wave * QW + (lane & (QW - 1)), nqu - 1)];

  const int nk = (d + KC - 1) / KC;
  fetch(r0, 0);
  for (uint32_t t0 = r0; t0 < r1; t0 += TR) {
    // |y|^2 of the two rows this lane reads back per query (row = half * 64 + lane), in flight
    // during the products
    const float bn0 = bn[min(t0 + lane, r1 - 1)], bn1 = bn[min(t0 + 64 + lane, r1 - 1)];
    // the shared bounds of the wave's queries, one per lane below QW
    const uint32_t tau_bits =
        __hip_atomic_load(tau + min(q0 + wave * QW + (lane & (QW - 1)), nqu - 1), __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_AGENT);
    f4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) acc[t] = f4{0.f, 0.f, 0.f, 0.f};

    __syncthreads();  // the previous pass's key reads are done (the key tile aliases Bs)
    stage(0);
    __syncthreads();
    for (int kc = 0; kc < nk; kc++) {
      const int b = kc & 1;
      if (kc + 1 < nk) fetch(t0, kc + 1);  // in flight during this chunk's MFMAs
      const float* A = &As[b][(arow0 + i16) * TS];
      const float* B = &Bs[b][(brow0 + i16) * TS];
#pragma unroll
      for (int j = 0; j < KC / 4; j++) {
        const int kk = 4 * j + k4;
        const float av = A[kk];
#pragma unroll
        for (int t = 0; t < NT; t++)
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, B[t * 16 * TS + kk], acc[t], 0, 0, 0);
      }
      if (kc + 1 < nk) stage(b ^ 1);
      __syncthreads();
    }
    if (t0 + TR < r1) fetch(t0 + TR, 0);  // the next pass's first chunk, in flight during the top-k

    // the products of the wave's 16 queries x 128 rows into its rows of the key tile; the
    // norms are folded in where a query's row of it is read back
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
      for (int r = 0; r < 4; r++)
        kt[(arow0 + k4 * 4 + r) * KS + brow0 + t * 16 + i16] = acc[t][r];
    __syncthreads();

    // one query at a time: its 128 keys, one row per lane and half, against its running k-th
    // best.  (Spelled out per query, as the drain sites of scan_topk.h: the top-k arrays are
    // indexed by constants and stay in registers.)
#define FLAT_QUERY(g)                                                                              \
  if constexpr (g < QW) if (q0 + wave * QW + g < nqu) { /* uniform */                                                  \
    WaveTopK<R> tk;                                                                                \
    tk.init(k);                                                                                    \
    _Pragma("unroll") for (int r = 0; r < R; r++) {                                                \
      tk.d[r] = kd[g][r];                                                                          \
      tk.id[r] = ki[g][r];                                                                         \
    }                                                                                              \
    /* nothing at or below the bound as read now needs publishing again */                         \
    tk.cap = tk.pub = tau_decode((uint32_t)__builtin_amdgcn_readlane((int)tau_bits, g));           \
    tk.refresh_tau();                                                                              \
    const float* krow = kt + (wave * QW + g) * KS;                                                 \
    const float xng = readlane_f(xnl, g);                                                          \
    _Pragma("unroll 1") for (int h = 0; h < TR / 64; h++) {                                        \
      const uint32_t pos = t0 + h * 64 + lane;                                                     \
      const float key = flat_key(krow[h * 64 + lane], xng, h ? bn1 : bn0, ip);                     \
      const bool pass = (pos < r1) & lexless(key, (int)pos, tk.td, tk.ti);                         \
      const uint64_t mask = __ballot(pass);                                                        \
      if (!mask) continue;                                                                         \
      if constexpr (!kQueued) {                                                                    \
        /* the lane number made opaque here: the sort's lane masks are then computed at the merge, \
           not hoisted out of the pass loop into some sixty registers held across it */            \
        int ml = lane;                                                                             \
        asm volatile("" : "+v"(ml));                                                               \
        bulk_merge_rows<R>(tk, pass ? key : kInf, pass ? (int)pos : kNone, ml);                    \
        tk.publish(tau + q0 + wave * QW + g, ml);                                                  \
      } else {                                                                                     \
        const int before =                                                                         \
            __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0)); \
        if (pass) {                                                                                \
          qd[(wave * QW + g) * kQ + qn[g] + before] = key;                                         \
          qi[(wave * QW + g) * kQ + qn[g] + before] = (int)pos;                                    \
        }                                                                                          \
        qn[g] += __popcll(mask);                                                                   \
      }                                                                                            \
    }                                                                                              \
    if constexpr (kQueued) { /* full batches of 64 after every pass, the rest after the last */    \
      if (qn[g] > (t0 + TR < r1 ? 63 : 0)) {                                                       \
        int ml = lane;                                                                             \
        asm volatile("" : "+v"(ml));                                                               \
        while (qn[g] > (t0 + TR < r1 ? 63 : 0))                                                    \
          drain_queue<R, 2>(tk, qn[g], qd + (wave * QW + g) * kQ, qi + (wave * QW + g) * kQ, ml);  \
        tk.publish(tau + q0 + wave * QW + g, ml);                                                  \
      }                                                                                            \
    }                                                                                              \
    _Pragma("unroll") for (int r = 0; r < R; r++) {                                                \
      kd[g][r] = tk.d[r];                                                                          \
      ki[g][r] = tk.id[r];                                                                         \
    }                                                                                              \
  }
    FLAT_QUERY(0) FLAT_QUERY(1) FLAT_QUERY(2) FLAT_QUERY(3) FLAT_QUERY(4) FLAT_QUERY(5) FLAT_QUERY(6) FLAT_QUERY(7)
    FLAT_QUERY(8) FLAT_QUERY(9) FLAT_QUERY(10) FLAT_QUERY(11) FLAT_QUERY(12) FLAT_QUERY(13) FLAT_QUERY(14)
    FLAT_QUERY(15)
#undef FLAT_QUERY
    static_assert(QW <= 16, "the queries of a wave are spelled out");
  }

  // the sorted list of every query of the wave for this range; the label of a row is its position
#pragma unroll
  for (int g = 0; g < QW; g++) {
    const uint32_t q = q0 + wave * QW + g;
    if (q >= nqu) continue;
    const int64_t at = ((int64_t)rng * nq + (int64_t)q) * k;
    WaveTopK<R> tk;
    tk.init(k);
#pragma unroll
    for (int r = 0; r < R; r++) {
      tk.d[r] = kd[g][r];
      tk.id[r] = ki[g][r];
    }
    write_sorted<R>(tk, k, ip != 0, partD + at, partI + at, lane, [](int pos) { return (int64_t)pos; });
  }
}

}  // namespace

FlatScanPlan flat_scan_plan(int64_t nq, int64_t nb, int k, int64_t force_rows) {
  FlatScanPlan p;
  p.tile_q = (k > kFlatWideMaxK || nq <= kFlatTileQNarrow) ? kFlatTileQNarrow : kFlatTileQ;
  const int64_t nqt = std::max<int64_t>(1, (nq + p.tile_q - 1) / p.tile_q);
  int64_t rows;
  if (force_rows > 0) {
    rows = (force_rows + kFlatTileRows - 1) / kFlatTileRows * kFlatTileRows;
  } else {
    // enough ranges for kFlatTargetGroups workgroups, whatever the number of query tiles
    const int64_t want = std::max<int64_t>(1, (kFlatTargetGroups + nqt - 1) / nqt);
    rows = (std::max<int64_t>(nb, 1) + want - 1) / want;
    rows = (rows + kFlatRangeGranule - 1) / kFlatRangeGranule * kFlatRangeGranule;
  }
  p.range_rows = rows;
  p.ranges = (int)std::max<int64_t>(1, (nb + rows - 1) / rows);
  int fan = 2;
  while (fan * 2 <= kFlatMergeFan && fan * 2 * k <= kFlatMergeEntries) fan *= 2;
  p.fan = fan;
  int64_t S = p.ranges;
  if (S > fan) {  // several rounds: every round's list count is a multiple of its fan
    S = fan;
    while (S < p.ranges) S *= 2;
  }
  p.S = (int)S;
  p.rounds = 1;  // merge_partial_lists' loop
  for (int64_t left = S / std::min<int64_t>(S, fan); left > 1; left /= std::min<int64_t>(left, fan)) p.rounds++;
  return p;
}

void launch_flat_search(const FlatScanArgs& a, const FlatScanPlan& p, hipStream_t s) {
  if (a.nq <= 0) return;
  (void)hipMemsetAsync(a.tau, 0xff, sizeof(uint32_t) * a.nq, s);  // no bound yet
  if (p.ranges < p.S) {  // the partial lists no range writes
    const int64_t at = (int64_t)p.ranges * a.nq * a.k;
    launch_fill_empty(a.partD + at, a.partI + at, (int64_t)p.S * a.nq * a.k - at, a.ip, s);
  }
  const int nqt = (int)((a.nq + p.tile_q - 1) / p.tile_q);
  const dim3 grid((unsigned)((int64_t)nqt * p.ranges));
  // (the base rows are 16-byte aligned whenever d % 4 == 0; the queries are the caller's)
  const bool vec = (a.d & 3) == 0 && (reinterpret_cast<uintptr_t>(a.x) & 15) == 0;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, a.x, a.xn, a.nq, a.d, a.base, a.bn, a.nb, p.range_rows, nqt,
                       a.ip ? 1 : 0, a.tau, a.k, a.partD, a.partI);
  };
  const int rows = scan_rows_for(a.k);
  if (p.tile_q == kFlatTileQ) {  // (k <= kFlatWideMaxK)
    if (rows == 1) vec ? launch(k_flat_scan<1, true, 64>) : launch(k_flat_scan<1, false, 64>);
    else vec ? launch(k_flat_scan<4, true, 64>) : launch(k_flat_scan<4, false, 64>);
  } else {
    if (rows == 1) vec ? launch(k_flat_scan<1, true, 16>) : launch(k_flat_scan<1, false, 16>);
    else if (rows == 4) vec ? launch(k_flat_scan<4, true, 16>) : launch(k_flat_scan<4, false, 16>);
    else vec ? launch(k_flat_scan<16, true, 16>) : launch(k_flat_scan<16, false, 16>);
  }
  merge_partial_lists(a.partD, a.partI, a.tmpD, a.tmpI, p.S, p.fan, a.nq, a.k, a.ip, a.D, a.I, s);
}

}  // namespace chivf
