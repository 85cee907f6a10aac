// Device code shared by the list-major exact scans (ivf_flat.hip, sq_scan.hip): the
// wave top-k in registers over (key, int32 position) pairs, the per-query shared
// bound, the LDS candidate queue of k > 64, and the host loop that merges the scans'
// sorted partial lists in rounds.  Everything is in an anonymous namespace: each
// translation unit compiles its own copy, inlined into its kernels.
#pragma once
#include <stdint.h>

#include <algorithm>

#include <hip/hip_runtime.h>

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

constexpr int kQueue = 64 + 64;  // queued candidates per (wave, query): < 64 pending + a pass's pushes

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
