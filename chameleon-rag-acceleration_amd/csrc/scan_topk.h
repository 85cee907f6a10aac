// Device code shared by the flat scans (pq_flat.hip, ivf_flat.hip, sq_scan.hip, ivf_sq.hip):
// the wave top-k in registers over (key, int32 position) pairs, the per-query shared bound of
// the exact scans, the LDS candidate queue of k > 64, the tail of a scan pass (distance
// terms, the fold to a key, admission, drain sites, the sorted write) and the host loop
// that merges the exact scans' sorted partial lists in rounds.  k_pq_scan and
// k_ivfflat_scan take their pass tail from here, and k_ivfsq_scan its drain sites and write;
// k_sq_scan's pass (sq_pass.h) uses the top-k, the bound and the queue but spells its tail out,
// because it measured slower on the helpers (profiles/flat_scans_refactor.md).
// Everything is in an anonymous namespace: each translation unit compiles its own copy,
// inlined into its kernels.
#pragma once
#include <float.h>
#include <stdint.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "ivfpq_kernels.h"

namespace chivf {

namespace {

constexpr float kInf = __builtin_huge_valf();
constexpr int kNone = INT32_MAX;  // "no candidate" position (real positions are < 2^31 - 1)

enum { K_IP = 0, K_L2 = 1 };

inline unsigned nblocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }
// workgroups of 256 threads of a one-thread-per-component kernel that strides over `total`
inline unsigned elementwise_grid(int64_t total) { return (unsigned)std::min<int64_t>((total + 255) / 256, 1 << 20); }

// rows of 64 lanes in a wave's top-k: the three k classes of every flat scan
inline int scan_rows_for(int k) { return k <= 64 ? 1 : k <= 256 ? 4 : 16; }

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
  // the shared bound (a scan that never calls set_cap / publish keeps both at +inf, and they fold away)
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

// Queued candidates per (wave, query) when a pass pushes at most NB per lane: < 64
// pending + a pass's pushes.  NB = 1 for the exact scans (one row per lane and pass).
template <int NB>
constexpr int kQueue = 64 + NB * 64;

// The first min(n, 64) candidates of a wave's queue (q_d, q_i) into its top-k, the
// rest (up to NB blocks of 64) moved to the front; n becomes the number left.
template <int R, int NB>
__device__ __forceinline__ void drain_queue(WaveTopK<R>& tk, int& n, float* q_d, int* q_i, int lane) {
  __builtin_amdgcn_wave_barrier();
  const bool have = lane < n;
  const float cd = have ? q_d[lane] : kInf;
  const int ci = have ? q_i[lane] : kNone;
  const int rem = max(n - 64, 0);
  float md[NB];
  int mi[NB];
#pragma unroll
  for (int j = 0; j < NB; j++) {
    const bool mv = j * 64 + lane < rem;
    md[j] = mv ? q_d[64 + j * 64 + lane] : kInf;
    mi[j] = mv ? q_i[64 + j * 64 + lane] : kNone;
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int j = 0; j < NB; j++) {
    if (j * 64 + lane < rem) {
      q_d[j * 64 + lane] = md[j];
      q_i[j * 64 + lane] = mi[j];
    }
  }
  __builtin_amdgcn_wave_barrier();
  n = rem;
  const bool pass = lexless(cd, ci, tk.td, tk.ti);  // the bound may have moved since the push
  if (__ballot(pass)) bulk_merge_rows<R>(tk, pass ? cd : kInf, pass ? ci : kNone, lane);
}

// ---- the tail of a scan pass -----------------------------------------------------
// One term of a distance: (q - y)^2, or q * y for the inner product.
template <int KIND>
__device__ __forceinline__ float dist_term(float q, float y) {
  if (KIND == K_IP) return q * y;
  const float t = q - y;
  return t * t;
}

// Eight values of the lane's row at dimensions [dim0, dim0 + 8) against the G query rows
// qid of x (wave-uniform: they come through the scalar cache), into Faiss's eight
// interleaved accumulators per query.
template <int KIND, int G>
__device__ __forceinline__ void accumulate8(float (&acc)[G][8], const float (&y)[8], const float* x, int d,
                                            const int (&qid)[G], int dim0) {
#pragma unroll
  for (int g = 0; g < G; g++) {
    const float* qp = x + (int64_t)qid[g] * d + dim0;
#pragma unroll
    for (int j = 0; j < 8; j++) acc[g][j] = acc[g][j] + dist_term<KIND>(qp[j], y[j]);
  }
}

// The end of a row in tree<>'s order: the eight accumulators folded to four, the 4-wide
// remainder y against qp (when rem), two horizontal adds.  Returns the key (the negated
// similarity for the inner product) and zeroes the accumulators for the next row.
template <int KIND>
__device__ __forceinline__ float fold_key(float (&acc)[8], bool rem, const float* qp, const float (&y)[4]) {
  float a4[4];
#pragma unroll
  for (int j = 0; j < 4; j++) a4[j] = acc[j + 4] + acc[j];
  if (rem) {
#pragma unroll
    for (int j = 0; j < 4; j++) a4[j] = a4[j] + dist_term<KIND>(qp[j], y[j]);
  }
  const float h0 = a4[0] + a4[1];
  const float h1 = a4[2] + a4[3];
  const float dis = h0 + h1;
#pragma unroll
  for (int j = 0; j < 8; j++) acc[j] = 0.f;
  return KIND == K_IP ? -dis : dis;
}

// Admission of one (key, position) per lane against a query's running k-th best; a pass
// with no better row costs one compare and one ballot.  R = 1 merges the admitted rows at
// once and returns true (the top-k changed: an exact scan then publishes its k-th key);
// R > 1 pushes them behind the n candidates of the (wave, query) queue (q_d, q_i).
template <int R>
__device__ __forceinline__ bool admit(WaveTopK<R>& tk, bool valid, float key, int pos, int& n, float* q_d, int* q_i,
                                      int lane) {
  const bool pass = valid & lexless(key, pos, tk.td, tk.ti);
  const uint64_t mask = __ballot(pass);
  if (!mask) return false;
  if constexpr (R == 1) {
    bulk_merge_rows<R>(tk, pass ? key : kInf, pass ? pos : kNone, lane);
    return true;
  } else {
    const int before = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
    if (pass) {
      q_d[n + before] = key;
      q_i[n + before] = pos;
    }
    n += __popcll(mask);
    return false;
  }
}

// The drain sites of a pass, one per query: the queues (qd, qi: [waves][G][kQueue<NB>])
// drained down to `keep` candidates -- full batches of 64 after every pass (keep = 63), the
// rest after the last (keep = 0).  PUB: an exact scan then publishes the k-th key of query
// qid[g] to its shared bound in tau; a scan without one passes nullptr for both.
// (Spelled out per query: a loop over g around R = 16 merges is past the compiler's
// unroll budget, and the top-k arrays would then live in scratch.  A flag and not a
// functor: a capturing lambda here costs the exact scans their second wave per SIMD.)
template <int NB, bool PUB, int G, int R>
__device__ __forceinline__ void drain_queues(WaveTopK<R> (&tk)[G], int (&qn)[G], int keep, float* qd, int* qi, int wave,
                                             int lane, uint32_t* tau, const int* qid) {
  static_assert(G <= 4, "drain sites are spelled out for up to four queries");
#define SCAN_DRAIN(g)                                                                                             \
  if constexpr (G > g) {                                                                                          \
    while (qn[g] > keep)                                                                                          \
      drain_queue<R, NB>(tk[g], qn[g], qd + (wave * G + g) * kQueue<NB>, qi + (wave * G + g) * kQueue<NB>, lane); \
    if constexpr (PUB) tk[g].publish(tau + qid[g], lane);                                                         \
  }
  SCAN_DRAIN(0);
  SCAN_DRAIN(1);
  SCAN_DRAIN(2);
  SCAN_DRAIN(3);
#undef SCAN_DRAIN
}

// A wave's sorted list to D, I[0, k): distances or similarities (keys negated back for the
// inner product), best first, padded with (FLT_MAX | -FLT_MAX, -1); label(pos) is the
// int64 label of image position pos.
template <int R, class Label>
__device__ __forceinline__ void write_sorted(const WaveTopK<R>& tk, int k, bool ip, float* D, int64_t* I, int lane,
                                             Label label) {
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int idx = r * 64 + lane;
    if (idx < k) {
      const int pos = tk.id[r];
      const bool none = pos == kNone;
      const float key = tk.d[r];
      D[idx] = none ? (ip ? -FLT_MAX : FLT_MAX) : (ip ? -key : key);
      I[idx] = none ? -1 : label(pos);
    }
  }
}

// Merge rounds over a scan's partial lists.  A round over S lists [S][nq][k] with fan f
// merges, for every j below S / f, the lists j, j + S / f, j + 2 S / f, ... -- read as
// [f][nq * S / f][k] they are one launch_merge_topk call whose output is the next round's
// [S / f][nq][k].  The rounds alternate between part and tmp ([S / fan][nq][k]).
inline void merge_partial_lists(float* partD, int64_t* partI, float* tmpD, int64_t* tmpI, int S, int fan, int64_t nq,
                                int k, bool ip, float* D, int64_t* I, hipStream_t s) {
  const float* inD = partD;
  const int64_t* inI = partI;
  bool to_tmp = true;
  while (true) {
    const int f = std::min(S, fan);
    const int left = S / f;
    if (left == 1) {
      launch_merge_topk(f, nq, k, inD, inI, D, I, s, ip);
      break;
    }
    float* outD = to_tmp ? tmpD : partD;
    int64_t* outI = to_tmp ? tmpI : partI;
    launch_merge_topk(f, nq * left, k, inD, inI, outD, outI, s, ip);
    inD = outD;
    inI = outI;
    S = left;
    to_tmp = !to_tmp;
  }
}

}  // namespace

}  // namespace chivf
