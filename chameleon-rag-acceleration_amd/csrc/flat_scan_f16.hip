// gfx950 (MI355X, CDNA4) kernels of the half-precision flat index (GpuIndexFlat* with
// useFloat16): the row image holds IEEE halves, the products run on v_mfma_f32_16x16x32_f16.
//
// k_rows_to_half: fp32 rows -> halves (round to nearest even; beyond the half range: +-inf)
// and, in the same pass, the fp32 squared norm of the *rounded* row; one wave per row.  It
// rounds the rows at add time and the queries of every search chunk (whose shared bounds it
// also clears).  k_half_to_float widens stored rows for get_rows.
//
// k_flat_scan_h: the tiling of k_flat_scan (flat_scan.hip) -- a workgroup takes 64 (16)
// queries and one row range and walks it 128 rows at a time, wave w owning the queries
// 16 w .. 16 w + 15 against all 128 rows (narrow tile: all 16 queries against the rows
// 32 w .. 32 w + 31) -- with a product of its own.  One MFMA covers 32 dimensions: lane l
// supplies row l & 15, elements 8 (l >> 4) .. + 7 of the step, 16 bytes, for A and for B.
//   A (queries): no LDS.  A wave's 16 queries are read by that wave alone (narrow tile: by all
//     four, the same 16), so each lane loads its own operand from global memory -- 16 bytes
//     per 32-wide step, the query chunk stays in L2 -- one k chunk ahead of its use.
//   B (base rows): staged in LDS in k chunks of 64 dimensions (128 bytes per row), double-
//     buffered, the next chunk's global loads in flight during this chunk's MFMAs.  A thread
//     stages four 16-byte pieces; eight consecutive lanes take one row's 128 bytes.  The row
//     stride is 144 bytes, 9 sixteen-byte slots: the 16 lanes of a ds_read_b128 group read
//     the same slot of 16 consecutive rows, 9 i mod 16 is a permutation, so they land on 16
//     different bank quads.
// k is padded with zeros to the 32-wide step (a chunk's second step is skipped where it is
// all padding).  The accumulator layout is that of 16x16x4_f32, so the epilogue is
// k_flat_scan's: the products pass through a key tile in LDS (it aliases the B buffers, free
// between passes), every wave reads back one query's 128 keys at a time into that query's
// wave top-k (scan_topk.h) under the shared bound tau_q, a key equal to the bound admitted.
// Each (range, query) writes one sorted partial list; merge_partial_lists reduces them.  No
// distance is written to global memory.  The MFMA's internal summation order is the
// hardware's: results are fp32 sums of exact products in an unspecified order.
// Compiled with -ffp-contract=off like the rest of the library.
#include <float.h>
#include <stdint.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "flat_scan_f16.h"
#include "ivf_flat.h"  // launch_fill_empty
#include "ivfpq_kernels.h"
#include "scan_topk.h"

namespace chivf {

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

constexpr int TR = kFlatTileRows, KC = kFlatHKc;
constexpr int TS = KC + 8;  // row stride of the staged B tile (halves): 144 bytes, 9 sixteen-byte slots
constexpr int KS = TR + 4;  // row stride of the key tile (floats)
static_assert(kFlatTileQ * KS * sizeof(float) <= 2 * TR * TS * sizeof(_Float16), "the key tile aliases the B staging buffers");
static_assert(kFlatTileQ == 64 && kFlatTileQNarrow == 16 && TR == 128 && KC == 64, "the staging below is written for these");

__global__ __launch_bounds__(256) void k_rows_to_half(const float* __restrict__ x, int64_t n, int d,
                                                      _Float16* __restrict__ out, float* __restrict__ norms,
                                                      uint32_t* __restrict__ tau) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;  // wave-uniform
  const float* xr = x + row * d;
  _Float16* o = out + row * d;
  float acc = 0.f;
  for (int j = lane; j < d; j += 64) {
    const _Float16 h = (_Float16)xr[j];
    o[j] = h;
    const float v = (float)h;
    acc = acc + v * v;
  }
  acc = acc + xor_f<1>(acc);
  acc = acc + xor_f<2>(acc);
  acc = acc + xor_f<4>(acc);
  acc = acc + xor_f<8>(acc);
  acc = acc + xor_f<16>(acc);
  acc = acc + xor_f<32>(acc);
  if (lane == 0) {
    norms[row] = acc;
    if (tau) tau[row] = 0xFFFFFFFFu;  // no bound yet
  }
}

__global__ __launch_bounds__(256) void k_half_to_float(const _Float16* __restrict__ h, int64_t count,
                                                       float* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) out[i] = (float)h[i];
}

// eight consecutive halves of a row at dimension kk (a multiple of 8), zeros past d, without
// a branch: the addresses are clamped into the row and the values selected.  VEC: d % 8 == 0,
// the rows are 16-byte aligned; otherwise a row is only 2-byte aligned and is read by halves.
template <bool VEC>
__device__ __forceinline__ h8 load8(const _Float16* __restrict__ row, int kk, int d) {
  h8 v;
  if constexpr (VEC) {
    v = *reinterpret_cast<const h8*>(row + min(kk, d - 8));
    if (kk >= d) v = h8{0, 0, 0, 0, 0, 0, 0, 0};
  } else {
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const _Float16 e = row[min(kk + j, d - 1)];
      v[j] = kk + j < d ? e : (_Float16)0;
    }
  }
  return v;
}

__device__ __forceinline__ float tau_decode(uint32_t u) {
  return u == 0xFFFFFFFFu ? kInf : __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

// the key from <x, y> (flat_scan.hip's)
__device__ __forceinline__ float flat_key(float dot, float xn, float yn, int ip) {
  if (ip) return -dot;
  const float v = (xn + yn) - 2.0f * dot;
  return v < 0.f ? 0.f : v;
}

// grid: query tile fastest, ranges slowest (the workgroups that run together share a row
// range).  LDS: 36 KiB of B staging, and at k > 64 96 KiB (24 KiB) of candidate queues.
// Waves per SIMD asked of the register allocator: as k_flat_scan (DESIGN.md 4k has what each
// form compiles to).
template <int R, bool VEC, int TQ>
__global__ __launch_bounds__(256, (TQ / 4) * R > 16 ? 1 : R > 1 ? 2 : VEC ? 3 : 2) void k_flat_scan_h(
    const _Float16* __restrict__ x, const float* __restrict__ xn, int64_t nq, int d, const _Float16* __restrict__ base,
    const float* __restrict__ bn, int64_t nb, int64_t range_rows, int nqt, int ip, uint32_t* tau, int k,
    float* __restrict__ partD, int64_t* __restrict__ partI) {
  constexpr int QW = TQ / 4;                  // queries whose lists a wave keeps
  constexpr int NT = TQ == 64 ? TR / 16 : 2;  // 16 x 16 MFMA tiles per wave and pass
  __shared__ __attribute__((aligned(16))) _Float16 Bs[2][TR * TS];
  float* kt = reinterpret_cast<float*>(&Bs[0][0]);  // [TQ][KS] keys of a pass
  constexpr bool kQueued = R > 1;
  constexpr int kQ = kQueue<2>;
  __shared__ float qd[kQueued ? TQ * kQ : 1];
  __shared__ int qi[kQueued ? TQ * kQ : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, k4 = lane >> 4;
  const int rng = blockIdx.x / nqt;
  // queries and row positions in 32 bits, unsigned (as k_flat_scan): 64 bits only where a
  // row's address is formed
  const uint32_t nqu = (uint32_t)nq;
  const uint32_t q0 = (blockIdx.x - rng * nqt) * TQ;
  const int arow0 = TQ == 64 ? wave * 16 : 0;  // the wave's MFMA operand rows: queries ...
  const int brow0 = TQ == 64 ? 0 : wave * 32;  // ... and base rows of the pass
  const uint32_t r0 = (uint32_t)((int64_t)rng * range_rows);
  const uint32_t r1 = (uint32_t)min(nb, (int64_t)r0 + range_rows);

  // B staging: piece u = 256 i + tid of a chunk is row u >> 3, dimensions 8 (u & 7) .. + 7;
  // rows past the range re-read the last one (their keys are dropped), dimensions past d
  // read as 0.  A: the lane's own operand of both steps of the chunk; queries past nq
  // re-read the last one.
  const int br = tid >> 3, bk = (tid & 7) * 8;
  const _Float16* arow = x + (int64_t)min(q0 + arow0 + i16, nqu - 1) * d;
  h8 ra[2], rb[4];
  auto fetch = [&](uint32_t t0, int kc) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < 2; s++) ra[s] = load8<VEC>(arow, kc * KC + 32 * s + 8 * k4, d);
#pragma unroll
    for (int i = 0; i < 4; i++)
      rb[i] = load8<VEC>(base + (int64_t)min(t0 + br + 32 * i, r1 - 1) * d, kc * KC + bk, d);
  };
  auto stage = [&](int b) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; i++) *reinterpret_cast<h8*>(&Bs[b][(br + 32 * i) * TS + bk]) = rb[i];
  };

  // the running k best of the wave's queries: only the sorted rows live across passes
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
    // |y|^2 of the two rows this lane reads back per query (row = half * 64 + lane)
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
      const h8 a0 = ra[0], a1 = ra[1];
      if (kc + 1 < nk) fetch(t0, kc + 1);  // in flight during this chunk's MFMAs
      const _Float16* B = &Bs[b][(brow0 + i16) * TS + 8 * k4];
#pragma unroll
      for (int t = 0; t < NT; t++)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, *reinterpret_cast<const h8*>(B + t * 16 * TS), acc[t], 0,
                                                        0, 0);
      if (kc * KC + 32 < d) {  // (uniform) the second step is not all padding
#pragma unroll
        for (int t = 0; t < NT; t++)
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, *reinterpret_cast<const h8*>(B + t * 16 * TS + 32),
                                                          acc[t], 0, 0, 0);
      }
      if (kc + 1 < nk) stage(b ^ 1);
      __syncthreads();
    }
    if (t0 + TR < r1) fetch(t0 + TR, 0);  // the next pass's first chunk, in flight during the top-k

    // the products of the wave's tiles into the key tile; the norms are folded in where a
    // query's row of it is read back
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
      for (int r = 0; r < 4; r++)
        kt[(arow0 + k4 * 4 + r) * KS + brow0 + t * 16 + i16] = acc[t][r];
    __syncthreads();

    // one query at a time: its 128 keys, one row per lane and half, against its running k-th
    // best (k_flat_scan's epilogue; spelled out per query so that the top-k arrays are
    // indexed by constants and stay in registers)
#define FLAT_QUERY(g)                                                                              \
  if constexpr (g < QW) if (q0 + wave * QW + g < nqu) { /* uniform */                              \
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
        /* the lane number made opaque: the sort's lane masks are computed at the merge */         \
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

void launch_rows_to_half(const float* x, int64_t n, int d, _Float16* out, float* norms, uint32_t* tau, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_rows_to_half, dim3(nblocks(n, 4)), dim3(256), 0, s, x, n, d, out, norms, tau);
}

void launch_half_to_float(const _Float16* h, int64_t count, float* out, hipStream_t s) {
  if (count <= 0) return;
  hipLaunchKernelGGL(k_half_to_float, dim3(elementwise_grid(count)), dim3(256), 0, s, h, count, out);
}

void launch_flat_search_h(const FlatScanHArgs& a, const FlatScanPlan& p, hipStream_t s) {
  if (a.nq <= 0) return;
  if (p.ranges < p.S) {  // the partial lists no range writes
    const int64_t at = (int64_t)p.ranges * a.nq * a.k;
    launch_fill_empty(a.partD + at, a.partI + at, (int64_t)p.S * a.nq * a.k - at, a.ip, s);
  }
  const int nqt = (int)((a.nq + p.tile_q - 1) / p.tile_q);
  const dim3 grid((unsigned)((int64_t)nqt * p.ranges));
  // (the image and the query workspace are 16-byte aligned; their rows are whenever d % 8 == 0)
  const bool vec = (a.d & 7) == 0;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, a.x, a.xn, a.nq, a.d, a.base, a.bn, a.nb, p.range_rows, nqt,
                       a.ip ? 1 : 0, a.tau, a.k, a.partD, a.partI);
  };
  const int rows = scan_rows_for(a.k);
  if (p.tile_q == kFlatTileQ) {  // (k <= kFlatWideMaxK)
    if (rows == 1) vec ? launch(k_flat_scan_h<1, true, 64>) : launch(k_flat_scan_h<1, false, 64>);
    else vec ? launch(k_flat_scan_h<4, true, 64>) : launch(k_flat_scan_h<4, false, 64>);
  } else {
    if (rows == 1) vec ? launch(k_flat_scan_h<1, true, 16>) : launch(k_flat_scan_h<1, false, 16>);
    else if (rows == 4) vec ? launch(k_flat_scan_h<4, true, 16>) : launch(k_flat_scan_h<4, false, 16>);
    else vec ? launch(k_flat_scan_h<16, true, 16>) : launch(k_flat_scan_h<16, false, 16>);
  }
  merge_partial_lists(a.partD, a.partI, a.tmpD, a.tmpI, p.S, p.fan, a.nq, a.k, a.ip, a.D, a.I, s);
}

}  // namespace chivf
