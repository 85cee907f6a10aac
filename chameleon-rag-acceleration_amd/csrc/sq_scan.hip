// gfx950 (MI355X, CDNA4) kernels for the flat scalar quantizer (IndexScalarQuantizer).
//
// Faiss runs IndexScalarQuantizer::search as a distance computer that decodes every code
// and accumulates it against the query, into a heap.  Here:
//  * k_sq_encode / k_sq_decode are Faiss's scalar-build codec formulas, one thread per
//    component, every operation one fp32 rounding (the division is the IEEE one);
//  * k_sq_minmax is the training reduction: per-dimension minimum and maximum, folded
//    with atomics on order-preserving bits, so exact whatever the order;
//  * k_sq_scan is k_ivfflat_scan (ivf_flat.hip) over one list whose rows are codes, with
//    the row codec as a template parameter.  Lanes are rows: a tile of 256 rows x 64
//    dimensions of CODES (32 KiB of halves or 16 KiB of bytes) is staged in LDS with
//    coalesced 16-byte loads, the next one already in flight, and read back one row per
//    lane with 16-byte reads; rows are padded by 16 bytes (144 / 80 bytes: an odd number
//    of 16-byte slots), which puts the 16 rows of a ds_read_b128 lane group on 16
//    distinct slots.  A lane decodes
//    its row's eight values once and uses them for all G queries (G = 8 at k <= 64 for
//    halves, 4 otherwise); the query values and
//    the 8-bit codec's vmin / vdiff are wave-uniform and come through the scalar cache.
//    The 8-bit codec's (code + 0.5f) / 255.0f takes 256 values: every workgroup builds
//    them once in LDS with the real division.  The sums are tree<>'s over the decoded
//    row, as k_ivfflat_scan's, so a search equals IVF1,Flat over the decoded vectors.
//    With one list and labels equal to positions a work item is numbered arithmetically:
//    item = range * groups + group (range-major, so that the groups of a row range run
//    at about the same time and find its codes in the L2).
//    Shared bound, register top-k, LDS queues for k > 64 and the merge rounds are those
//    of the IVF-Flat scan (scan_topk.h).  The tail of a pass (terms, fold, admission,
//    drain sites, sorted write) is spelled out here and not taken from scan_topk.h's
//    helpers as in k_ivfflat_scan: with them this kernel measured slower (4.8 % at
//    d = 768, fp16, k = 10; profiles/flat_scans_refactor.md).
// Compiled with -ffp-contract=off like the rest of the library.
#include <float.h>
#include <stdint.h>

#include <algorithm>

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

// ------------------------------------------------------------- encode / decode
template <int CODEC>
__global__ __launch_bounds__(256) void k_sq_encode(const float* __restrict__ x, int64_t total, int d,
                                                   const float* __restrict__ vmin, const float* __restrict__ vdiff,
                                                   uint8_t* __restrict__ codes) {
  for (int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (int64_t)gridDim.x * 256) {
    if constexpr (CODEC == SQ_CODEC_FP16) {
      reinterpret_cast<_Float16*>(codes)[gid] = (_Float16)x[gid];  // round to nearest even, subnormals kept
    } else {
      const int j = (int)(gid % d);
      const float vd = vdiff[j];
      float xi = 0.f;
      if (vd != 0.f) {
        xi = (x[gid] - vmin[j]) / vd;
        if (xi < 0.f) xi = 0.f;
        if (xi > 1.f) xi = 1.f;
      }
      codes[gid] = (uint8_t)(int)(255.f * xi);
    }
  }
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
  const int64_t cs = (int64_t)d * L::kElem;
  const int nchunk = (d + kDc - 1) / kDc;
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

    // eight decoded values of the lane's row at dimensions [dim0, dim0 + 8) against every query
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

template <int KIND, int CODEC, int G, int R>
void launch_scan(const SqScanArgs& a, const IvfFlatPlan& p, hipStream_t s) {
  hipLaunchKernelGGL((k_sq_scan<KIND, CODEC, G, R>), dim3((unsigned)p.grid), dim3(256), 0, s, a.x, a.nq, a.d, a.codes,
                     a.nb, a.vmin, a.vdiff, a.tau, a.k, p.S, a.partD, a.partI);
}
template <int KIND, int CODEC>
void launch_scan_codec(const SqScanArgs& a, const IvfFlatPlan& p, hipStream_t s) {
  // the classes of ivf_flat.hip: (G, R) = (8, 1) for k <= 64, (4, 4) for k <= 256, (4, 16) above;
  // the 8-bit codec takes G = 4 at k <= 64 too (three workgroups per CU: measured)
  constexpr int kSmallG = CODEC == SQ_CODEC_8BIT ? SQ_SCAN_GROUP_SMALL_K_8BIT : SQ_SCAN_GROUP_SMALL_K;
  if (a.k <= 64) launch_scan<KIND, CODEC, kSmallG, 1>(a, p, s);
  else if (a.k <= 256) launch_scan<KIND, CODEC, 4, 4>(a, p, s);
  else launch_scan<KIND, CODEC, 4, 16>(a, p, s);
}
template <int KIND>
void launch_scan_kind(const SqScanArgs& a, const IvfFlatPlan& p, hipStream_t s) {
  if (a.codec == SQ_CODEC_FP16) launch_scan_codec<KIND, SQ_CODEC_FP16>(a, p, s);
  else launch_scan_codec<KIND, SQ_CODEC_8BIT>(a, p, s);
}

unsigned elementwise_grid(int64_t total) { return (unsigned)std::min<int64_t>((total + 255) / 256, 1 << 20); }

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
  if (a.ip)
    launch_scan_kind<K_IP>(a, p, s);
  else
    launch_scan_kind<K_L2>(a, p, s);
  merge_partial_lists(a.partD, a.partI, a.tmpD, a.tmpI, p.S, p.fan, a.nq, a.k, a.ip, a.D, a.I, s);
}

}  // namespace chivf
