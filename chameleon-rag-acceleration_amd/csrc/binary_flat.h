// Launchers for the binary-code kernels (binary_flat.hip) behind IndexBinaryFlat: exact
// Hamming search over uint8 codes with a counting top-k.  All launchers are asynchronous
// on `stream` and allocate nothing.
//
// Contract.  search returns, per query, the k smallest (hamming, label) pairs ascending,
// ties by label (the label of a code is its position), padded with (2147483647, -1) where
// fewer than k codes exist.  Relation to Faiss's IndexBinaryFlat: the distances equal
// Faiss's for either value of use_heap; the labels equal use_heap = false
// (hammings_knn_mc, which keeps the first-seen ids per distance); Faiss's default heap
// path may keep other ties at the k-th distance and orders equal distances arbitrarily.
//
// Device image: codes [ntotal][stride] with stride = bin_stride(code_size) bytes, pad bytes
// zero; the queries are packed with the same zero pad, so padding adds 0 to every distance.
//
// The select is Faiss's counting algorithm in two streaming passes over the codes.  A work
// item is (row segment s, block of QB queries); lanes are rows, the block's query words are
// wave-uniform.
//   k_hamming_hist  per item an exact histogram of the distances in LDS, stored to
//                   hist[nq][Sg][d + 1] with plain vector stores (no global atomics)
//   k_hamming_plan  per query: T = the k-th smallest distance, need = k - #(dist < T); hist
//                   is overwritten with the output base slot of every (t <= T, s), t major
//                   and s minor; quota[q][s] = the segment's share of the `need` T-ties
//   k_hamming_emit  the same pass again: a row with dist < T takes the next slot of its
//                   (q, s, dist) group by an LDS counter; a row with dist == T is ranked in
//                   label order (the waves' tie counts exchanged through LDS once per tile,
//                   a ballot inside the wave) and written while its rank is below the quota
//   k_hamming_order per query: the k outputs sorted by (dist, label), which puts each
//                   (q, s, dist) group - already in its final range - into label order
// No buffer depends on the number of ties.  Workspace: hist is nq * Sg * (d + 1) * 4 bytes;
// the queries are chunked so that it stays within kBinHistBytes (96 MiB).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace chivf {

constexpr int kBinTileRows = 256;                     // rows of one workgroup step (one per lane)
constexpr int kBinTargetItems = 1024;                 // work items that fill 256 CUs x 2 workgroups twice
constexpr size_t kBinHistBytes = size_t(96) << 20;    // bound for a chunk's histograms
constexpr int32_t kBinPadDist = 2147483647;           // Faiss's CMax<int32_t> neutral
constexpr int kBinMaxD = 2048;

// bytes of a row in the device image: one 4- or 8-byte load, or whole 16-byte loads
inline int bin_stride(int code_size) { return code_size <= 4 ? 4 : code_size <= 8 ? 8 : (code_size + 15) & ~15; }
// queries of a work item: the block's histograms (QB * (d + 1) * 4 bytes) beside two workgroups per CU
inline int bin_query_block(int d) { return d <= 1024 ? 16 : 8; }

struct BinPlan {
  int stride = 0;        // bytes per row of the image
  int QB = 0;            // queries per work item
  int64_t qc = 0;        // queries per chunk (a multiple of QB unless it is all of them)
  int Sg = 0;            // row segments of a chunk of qc queries
  int64_t seg_rows = 0;  // rows per segment (a multiple of kBinTileRows)
};

inline void bin_segments(int64_t nb, int64_t nblocks, int* Sg, int64_t* seg_rows) {
  const int64_t tiles = std::max<int64_t>(1, (nb + kBinTileRows - 1) / kBinTileRows);
  const int64_t want = std::max<int64_t>(1, std::min<int64_t>(tiles, kBinTargetItems / std::max<int64_t>(1, nblocks)));
  const int64_t seg_tiles = (tiles + want - 1) / want;
  *seg_rows = seg_tiles * kBinTileRows;
  *Sg = (int)((tiles + seg_tiles - 1) / seg_tiles);
}

// the plan of a search of nq queries over nb codes of d bits
inline BinPlan bin_plan(int d, int64_t nb, int64_t nq) {
  BinPlan p;
  p.stride = bin_stride(d / 8);
  p.QB = bin_query_block(d);
  p.qc = std::max<int64_t>(1, nq);
  for (;;) {
    bin_segments(nb, (p.qc + p.QB - 1) / p.QB, &p.Sg, &p.seg_rows);
    if ((size_t)p.qc * p.Sg * (d + 1) * 4 <= kBinHistBytes || p.qc <= p.QB) break;
    p.qc = ((p.qc + 1) / 2 + p.QB - 1) / p.QB * p.QB;
  }
  return p;
}

// dst[n][stride] <- src[n][code_size], pad bytes zero (dst 4-byte aligned)
void launch_bin_pad_rows(const uint8_t* src, int64_t n, int code_size, int stride, uint32_t* dst, hipStream_t s);
// D[n] = kBinPadDist, I[n] = -1
void launch_bin_fill_empty(int32_t* D, int64_t* I, int64_t n, hipStream_t s);

struct BinSearchArgs {
  const uint8_t* x;       // [nq][code_size] queries, nq <= plan.qc
  int64_t nq;
  int d;                  // bits, a multiple of 8 in [8, kBinMaxD]
  const uint32_t* codes;  // [nb][plan.stride / 4]
  int64_t nb;             // 1 <= nb < 2^31 - 1
  int k;                  // 1 <= k <= 1024
  // workspace
  uint32_t* qw;     // [ceil(nq / QB) * QB * stride / 4] the packed query blocks
  uint32_t* hist;   // [nq][Sg][d + 1]
  int32_t* T;       // [nq]
  uint32_t* quota;  // [nq][Sg]
  int32_t* D;       // [nq][k] out
  int64_t* I;
};
void launch_bin_search(const BinSearchArgs& a, const BinPlan& plan, hipStream_t s);

}  // namespace chivf
