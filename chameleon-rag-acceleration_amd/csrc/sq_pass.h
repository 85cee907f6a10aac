// Device code shared by the two scans of scalar-quantizer codes, k_sq_scan (sq_scan.hip) and
// k_ivfsq_scan (ivf_sq.hip): the vector types and the tile layout, the (G, R) classes both are
// launched in, and the encode of one component (k_sq_encode, k_ivfsq_encode).  It also holds
// the pass over one work item's row range, scan_code_rows, which k_sq_scan alone calls:
// k_ivfsq_scan measured slower on it and keeps its own text (profiles/ivf_shared_pass_refactor.md),
// so a change of the pass has to be made in both places.  As scan_topk.h: an anonymous namespace,
// every device function inlined into its kernels.
//
// The pass.  Lanes are rows: a tile of 256 rows x 64 dimensions of CODES (32 KiB of halves or
// 16 KiB of bytes) is staged in LDS with coalesced 16-byte loads, the next one already in
// flight, and read back one row per lane with 16-byte reads; rows are padded by 16 bytes (144 /
// 80 bytes: an odd number of 16-byte slots), which puts the 16 rows of a ds_read_b128 lane group
// on 16 distinct slots.  A lane decodes its row's eight values once and uses them for all G
// queries; the query values and the 8-bit codec's vmin / vdiff are wave-uniform and come through
// the scalar cache.  The 8-bit codec's (code + 0.5f) / 255.0f takes 256 values, which the kernel
// builds once in LDS with the real division.  The sums are tree<>'s over the decoded row.  A
// piece that straddles a row's end reads the next row's first bytes or, at the image's last
// row, its slack (kSqScanSlack).
// The tail of a pass (terms, fold, admission, drain sites) is spelled out and not taken from
// scan_topk.h's helpers as in k_ivfflat_scan: with them k_sq_scan measured slower (4.8 % at
// d = 768, fp16, k = 10; profiles/flat_scans_refactor.md).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "scan_topk.h"
#include "sq_scan.h"

namespace chivf {

namespace {

using u4 = uint32_t __attribute__((ext_vector_type(4)));  // 16 bytes of codes, held in registers
// a 16-byte global load of codes: rows are 4-byte (8-bit) or 8-byte (fp16) aligned only
typedef uint32_t u4a __attribute__((ext_vector_type(4), aligned(4)));
using h8 = _Float16 __attribute__((ext_vector_type(8)));
using h4 = _Float16 __attribute__((ext_vector_type(4)));

// The two choices DESIGN.md section 4d measures, as build switches for its A/B runs:
// dimensions per staged step, and queries per work item at k <= 64 (per codec).
#ifndef SQ_SCAN_STEP_DIMS
#define SQ_SCAN_STEP_DIMS 64
#endif
#ifndef SQ_SCAN_GROUP_SMALL_K
#define SQ_SCAN_GROUP_SMALL_K 8
#endif
#ifndef SQ_SCAN_GROUP_SMALL_K_8BIT
#define SQ_SCAN_GROUP_SMALL_K_8BIT 4
#endif
constexpr int kDc = SQ_SCAN_STEP_DIMS;  // dimensions per staged step (a multiple of 16)
static_assert(kDc % 16 == 0 && kDc >= 16 && kDc <= 128, "a step is whole 16-byte pieces of either codec");
constexpr int kTile = 256;  // rows per pass: one per thread
constexpr int kQ = kQueue<1>;  // queued candidates per (wave, query): one push per lane and pass

template <int CODEC>
struct Layout {
  static constexpr int kElem = CODEC == SQ_CODEC_FP16 ? 2 : 1;  // bytes per dimension
  static constexpr int kStepBytes = kDc * kElem;                // of a row's step: 128 / 64
  static constexpr int kPieces = kStepBytes / 16;               // 16-byte pieces per row and step = loads per thread
  static constexpr int kStride = kStepBytes + 16;               // bytes per LDS row: 144 / 80 (an odd number of 16-byte slots)
};

// ---------------------------------------------------------------------- encode
// codes[gid] = the code of v, a component at dimension j (sq_scan.h's formulas)
template <int CODEC>
__device__ __forceinline__ void encode_component(float v, int j, const float* __restrict__ vmin,
                                                 const float* __restrict__ vdiff, uint8_t* __restrict__ codes,
                                                 int64_t gid) {
  if constexpr (CODEC == SQ_CODEC_FP16) {
    reinterpret_cast<_Float16*>(codes)[gid] = (_Float16)v;  // round to nearest even, subnormals kept
  } else {
    const float vd = vdiff[j];
    float xi = 0.f;
    if (vd != 0.f) {
      xi = (v - vmin[j]) / vd;
      if (xi < 0.f) xi = 0.f;
      if (xi > 1.f) xi = 1.f;
    }
    codes[gid] = (uint8_t)(int)(255.f * xi);
  }
}

// ------------------------------------------------------------------------ pass
// One work item's rows [r0, r1) of codes against its npair (<= G) pairs, into the wave top-k
// tk[g] of every pair: initialised by the kernel (WaveTopK::init; with the init in here
// k_sq_scan<*, fp16, 4, 4> went from two waves per SIMD to one) and left to it for the sorted
// write.  Pair g reads query row qid[g] of x and shares the bound tau[qid[g]]; pairs past
// npair repeat the first (their sums are dropped).
// LDS of the kernel: tile[kTile * kStride], the 8-bit codec's unit[256] = (code + 0.5f) /
// 255.0f (written before the first call; read after the step loop's first barriers), and for
// R > 1 the queues qd, qi[kIvfFlatWaves * G * kQ].
template <int KIND, int CODEC, int G, int R>
__device__ __forceinline__ void scan_code_rows(WaveTopK<R> (&tk)[G], uint8_t* tile, const float* unit, float* qd,
                                               int* qi, const float* __restrict__ x, int d,
                                               const uint8_t* __restrict__ codes, const float* __restrict__ vmin,
                                               const float* __restrict__ vdiff, uint32_t* tau, int64_t r0, int64_t r1,
                                               int npair, const int (&qid)[G]) {
  using L = Layout<CODEC>;
  constexpr bool k8bit = CODEC == SQ_CODEC_8BIT;
  constexpr bool kQueued = R > 1;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int64_t cs = (int64_t)d * L::kElem;
  const int nchunk = (d + kDc - 1) / kDc;

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
      const float* qp = x + (int64_t)qid[g] * d + dim0;  // wave-uniform
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
          const float* qp = x + (int64_t)qid[g] * d + dim_r;
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
      if constexpr (kQueued) {
        // one drain site per query: full batches of 64 after every pass, the rest after the last
        const int keep = t0 + kTile < r1 ? 63 : 0;
        // (spelled out per query, as in k_ivfflat_scan: a loop over g around R = 16 merges is
        // past the compiler's unroll budget, and the top-k arrays would then live in scratch)
        static_assert(G <= 4, "drain sites are spelled out for up to four queries");
#define SQ_DRAIN(g)                                                                                   \
  if constexpr (G > g) {                                                                              \
    while (qn[g] > keep)                                                                              \
      drain_queue<R, 1>(tk[g], qn[g], qd + (wave * G + g) * kQ, qi + (wave * G + g) * kQ, lane); \
    tk[g].publish(tau + qid[g], lane);                                                                \
  }
        SQ_DRAIN(0);
        SQ_DRAIN(1);
        SQ_DRAIN(2);
        SQ_DRAIN(3);
#undef SQ_DRAIN
      }
    }
  }
}

// --------------------------------------------------------------------- classes
// (G, R) of a scan: the classes of ivf_flat.hip, (8, 1) for k <= 64, (4, 4) for k <= 256, (4, 16)
// above; the 8-bit codec takes G = 4 at k <= 64 too (three workgroups per CU: measured,
// DESIGN.md section 4d).
constexpr int scan_group_small_k(int codec) {
  return codec == SQ_CODEC_8BIT ? SQ_SCAN_GROUP_SMALL_K_8BIT : SQ_SCAN_GROUP_SMALL_K;
}
inline int scan_group_for(int codec, int k) { return k <= 64 ? scan_group_small_k(codec) : 4; }

// f.launch<KIND, CODEC, G, R>() for the metric, the codec and k's class
template <int KIND, int CODEC, class F>
void launch_scan_class(int k, const F& f) {
  if (k <= 64) f.template launch<KIND, CODEC, scan_group_small_k(CODEC), 1>();
  else if (k <= 256) f.template launch<KIND, CODEC, 4, 4>();
  else f.template launch<KIND, CODEC, 4, 16>();
}
template <int KIND, class F>
void launch_scan_codec(int codec, int k, const F& f) {
  if (codec == SQ_CODEC_FP16) launch_scan_class<KIND, SQ_CODEC_FP16>(k, f);
  else launch_scan_class<KIND, SQ_CODEC_8BIT>(k, f);
}
template <class F>
void launch_scan(bool ip, int codec, int k, const F& f) {
  if (ip) launch_scan_codec<K_IP>(codec, k, f);
  else launch_scan_codec<K_L2>(codec, k, f);
}

}  // namespace

}  // namespace chivf
