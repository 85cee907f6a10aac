// gfx950 kernels of IndexBinaryFlat: exact Hamming search with a counting top-k
// (binary_flat.h has the contract and the algorithm).
#include "binary_flat.h"

namespace chivf {

namespace {

constexpr int kT = kBinTileRows;  // threads of a scan workgroup: one row per lane
static_assert(kT == 256, "four waves per workgroup");

// ------------------------------------------------------------------ packing
// dst word (r, w) <- the little-endian bytes 4w .. 4w + 3 of src row r, zero past code_size
__global__ __launch_bounds__(256) void k_bin_pad_rows(const uint8_t* __restrict__ src, int64_t n, int code_size,
                                                      int W, uint32_t* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * W) return;
  const int64_t r = i / W;
  const int w = (int)(i - r * W);
  uint32_t v = 0;
  for (int b = 0; b < 4; b++) {
    const int c = 4 * w + b;
    if (c < code_size) v |= (uint32_t)src[r * code_size + c] << (8 * b);
  }
  dst[i] = v;
}

// qw[block][chunk j][query q][V] <- word j * V + v of query block * QB + q, zero for the pad
// bytes and for the queries past nq
__global__ __launch_bounds__(256) void k_bin_pack_queries(const uint8_t* __restrict__ x, int64_t nq, int code_size,
                                                          int W, int V, int QB, int64_t total,
                                                          uint32_t* __restrict__ qw) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int v = (int)(i % V);
  const int q = (int)((i / V) % QB);
  const int nch = W / V;
  const int j = (int)((i / ((int64_t)V * QB)) % nch);
  const int64_t blk = i / ((int64_t)V * QB * nch);
  const int64_t qg = blk * QB + q;
  const int w = j * V + v;
  uint32_t out = 0;
  if (qg < nq)
    for (int b = 0; b < 4; b++) {
      const int c = 4 * w + b;
      if (c < code_size) out |= (uint32_t)x[qg * code_size + c] << (8 * b);
    }
  qw[i] = out;
}

__global__ __launch_bounds__(256) void k_bin_fill_empty(int32_t* __restrict__ D, int64_t* __restrict__ I, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    D[i] = kBinPadDist;
    I[i] = -1;
  }
}

// ------------------------------------------------------------------ the scan's frame
// codes [nb][W] and qw [nblocks][nch][QB][V] are kernel parameters of their own (const
// __restrict__, so that the wave-uniform query words come through the scalar cache)
struct BinScanArgs {
  int nb, nq;  // rows of the image, queries of the chunk
  int d, W, k, Sg;
  int seg_rows, nblocks, nitems;
  uint32_t* hist;         // [nq][Sg][d + 1]: counts, then output base slots
  const int32_t* T;       // [nq]
  const uint32_t* quota;  // [nq][Sg]
  int32_t* D;
  int64_t* I;
};

template <int V>
struct Chunk {
  uint32_t w[V];
};

// V words of a row with one aligned load
template <int V>
__device__ __forceinline__ Chunk<V> load_chunk(const uint32_t* __restrict__ p) {
  Chunk<V> c;
  if constexpr (V == 4) {
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    c.w[0] = t.x, c.w[1] = t.y, c.w[2] = t.z, c.w[3] = t.w;
  } else if constexpr (V == 2) {
    const uint2 t = *reinterpret_cast<const uint2*>(p);
    c.w[0] = t.x, c.w[1] = t.y;
  } else {
    c.w[0] = *p;
  }
  return c;
}

// acc += popcount(x) in one instruction (the compiler splits it into a count and an add)
__device__ __forceinline__ void bcnt_acc(uint32_t& acc, uint32_t x) {
  asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc) : "v"(x));
}

// acc[q] = hamming(row, query q of the block) for the lane's row: `cur` holds the row's first
// chunk; every further chunk is loaded while the one before it is counted.  qblk is
// wave-uniform (scalar loads), so a step is v_xor_b32 with a scalar, then v_bcnt_u32_b32.
template <int V, int QB>
__device__ __forceinline__ void bin_distances(Chunk<V> cur, const uint32_t* __restrict__ rowp,
                                              const uint32_t* __restrict__ qblk, int nch, uint32_t (&acc)[QB]) {
#pragma unroll
  for (int q = 0; q < QB; q++) acc[q] = 0;
  for (int j = 0; j < nch; j++) {
    Chunk<V> nxt = cur;
    if (j + 1 < nch) nxt = load_chunk<V>(rowp + (j + 1) * V);
    const uint32_t* __restrict__ qj = qblk + j * QB * V;
#pragma unroll
    for (int q = 0; q < QB; q++)
#pragma unroll
      for (int v = 0; v < V; v++) bcnt_acc(acc[q], cur.w[v] ^ qj[q * V + v]);
    cur = nxt;
  }
}

// item -> (segment, query block): the blocks of one segment are neighbours, so the workgroups
// running together read the same rows
struct BinItem {
  int s, b, nqb, r0, r1;
};
__device__ __forceinline__ BinItem bin_item(const BinScanArgs& a, int item, int QB) {
  BinItem it;
  it.s = item / a.nblocks;
  it.b = item - it.s * a.nblocks;
  it.r0 = it.s * a.seg_rows;  // < nb
  it.r1 = a.nb - it.r0 > a.seg_rows ? it.r0 + a.seg_rows : a.nb;
  const int left = a.nq - it.b * QB;
  it.nqb = left < QB ? left : QB;
  return it;
}

// ------------------------------------------------------------------ pass 1: histograms
template <int V, int QB, int DMAX>
__global__ __launch_bounds__(kT, 2) void k_hamming_hist(BinScanArgs a, const uint32_t* __restrict__ codes,
                                                     const uint32_t* __restrict__ qw) {
  __shared__ uint32_t hist[QB * (DMAX + 1)];
  const int tid = threadIdx.x;
  const int HL = a.d + 1;
  const int nch = a.W / V;
  for (int i = tid; i < QB * HL; i += kT) hist[i] = 0;
  __syncthreads();
  for (int item = blockIdx.x; item < a.nitems; item += gridDim.x) {
    const BinItem it = bin_item(a, item, QB);
    const uint32_t* __restrict__ qblk = qw + (size_t)it.b * a.W * QB;
    int row = it.r0 + tid;
    Chunk<V> cur = load_chunk<V>(codes + (size_t)(row < it.r1 ? row : it.r1 - 1) * a.W);
    for (int t0 = it.r0; t0 < it.r1; t0 += kT) {
      row = t0 + tid;
      const bool valid = row < it.r1;
      const uint32_t* __restrict__ rowp = codes + (size_t)(valid ? row : it.r1 - 1) * a.W;
      // the next tile's first chunk is in flight while this tile is counted
      const int nrow = it.r1 - row > kT ? row + kT : it.r1 - 1;
      const Chunk<V> nxt = load_chunk<V>(codes + (size_t)nrow * a.W);
      uint32_t acc[QB];
      bin_distances<V, QB>(cur, rowp, qblk, nch, acc);
      cur = nxt;
      if (valid) {
        // (the queries past nq are zero words: their bins are counted and never stored)
#pragma unroll
        for (int q = 0; q < QB; q++) atomicAdd(&hist[q * HL + acc[q]], 1u);
      }
    }
    __syncthreads();
    for (int i = tid; i < QB * HL; i += kT) {
      const int q = i / HL;
      const int t = i - q * HL;
      if (q < it.nqb) a.hist[((size_t)(it.b * QB + q) * a.Sg + it.s) * HL + t] = hist[i];
      hist[i] = 0;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ the plan
// One workgroup per query.  kk = min(k, nb) >= 1 rows are output.
constexpr int kPlanPer = (kBinMaxD + 1 + 255) / 256;  // consecutive distances per thread of the scan

__global__ __launch_bounds__(256) void k_hamming_plan(uint32_t* __restrict__ hist, int Sg, int d, uint32_t kk,
                                                      int32_t* __restrict__ T, uint32_t* __restrict__ quota) {
  __shared__ uint32_t tot[256 * kPlanPer];
  __shared__ uint32_t part[256];
  __shared__ uint32_t sT, sNeed;
  const int tid = threadIdx.x;
  const int HL = d + 1;
  const int64_t q = blockIdx.x;
  uint32_t* __restrict__ hq = hist + (size_t)q * Sg * HL;
  for (int t = tid; t < 256 * kPlanPer; t += 256) {
    uint32_t c = 0;
    if (t < HL)
      for (int s = 0; s < Sg; s++) c += hq[(size_t)s * HL + t];
    tot[t] = c;
  }
  if (tid == 0) sT = 0, sNeed = 0;
  __syncthreads();
  uint32_t local = 0;
  for (int i = 0; i < kPlanPer; i++) local += tot[tid * kPlanPer + i];
  part[tid] = local;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const uint32_t v = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  uint32_t run = part[tid] - local;  // #(dist < the thread's first distance)
  for (int i = 0; i < kPlanPer; i++) {
    const int t = tid * kPlanPer + i;
    const uint32_t c = tot[t];
    if (run < kk && kk <= run + c) sT = (uint32_t)t, sNeed = kk - run;
    tot[t] = run;
    run += c;
  }
  __syncthreads();
  const int Tq = (int)sT;
  const uint32_t need = sNeed;
  if (tid == 0) T[q] = Tq;
  for (int t = tid; t <= Tq; t += 256) {
    const uint32_t cum = tot[t];
    uint32_t before = 0;  // rows of the earlier segments at this distance
    for (int s = 0; s < Sg; s++) {
      const uint32_t h = hq[(size_t)s * HL + t];
      if (t == Tq) {
        const uint32_t left = need > before ? need - before : 0;
        quota[q * Sg + s] = h < left ? h : left;
        hq[(size_t)s * HL + t] = cum + (before < need ? before : need);
      } else {
        hq[(size_t)s * HL + t] = cum + before;
      }
      before += h;
    }
  }
}

// ------------------------------------------------------------------ pass 2: emit
template <int V, int QB, int DMAX>
__global__ __launch_bounds__(kT, 2) void k_hamming_emit(BinScanArgs a, const uint32_t* __restrict__ codes,
                                                     const uint32_t* __restrict__ qw) {
  __shared__ uint32_t cnt[QB * (DMAX + 1)];  // rows written so far per (query, distance < T)
  __shared__ uint32_t we[2][QB][4];          // the waves' T-tie counts of a tile, per query
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int HL = a.d + 1;
  const int nch = a.W / V;
  const uint64_t below = ((uint64_t)1 << lane) - 1;
  for (int i = tid; i < QB * HL; i += kT) cnt[i] = 0;
  if (tid < 2 * QB * 4) (&we[0][0][0])[tid] = 0;
  int par = 0;  // the buffer of `we` the next tile counts into (its columns are zero)
  __syncthreads();
  for (int item = blockIdx.x; item < a.nitems; item += gridDim.x) {
    const BinItem it = bin_item(a, item, QB);
    const uint32_t* __restrict__ qblk = qw + (size_t)it.b * a.W * QB;
    // lane l < nqb keeps query l's plan; T = -1 lets no row of a missing query through
    int Tl = -1;
    uint32_t quotal = 0, baseTl = 0, seen = 0;
    if (lane < it.nqb) {
      const size_t qg = (size_t)it.b * QB + lane;
      Tl = a.T[qg];
      quotal = a.quota[qg * a.Sg + it.s];
      baseTl = a.hist[(qg * a.Sg + it.s) * HL + Tl];
    }
    // every query's T in a vector register of its own (scalar registers hold the query words)
    int Tv[QB];
#pragma unroll
    for (int q = 0; q < QB; q++) Tv[q] = __shfl(Tl, q);
    int row = it.r0 + tid;
    Chunk<V> cur = load_chunk<V>(codes + (size_t)(row < it.r1 ? row : it.r1 - 1) * a.W);
    for (int t0 = it.r0; t0 < it.r1; t0 += kT) {
      row = t0 + tid;
      const bool valid = row < it.r1;
      const uint32_t* __restrict__ rowp = codes + (size_t)(valid ? row : it.r1 - 1) * a.W;
      const int nrow = it.r1 - row > kT ? row + kT : it.r1 - 1;
      const Chunk<V> nxt = load_chunk<V>(codes + (size_t)nrow * a.W);
      uint32_t acc[QB];
      bin_distances<V, QB>(cur, rowp, qblk, nch, acc);
      cur = nxt;
      // per lane: the queries this row is a T-tie of, and those it is written for
      uint32_t eqbits = 0, lebits = 0;
#pragma unroll
      for (int q = 0; q < QB; q++) {
        eqbits |= (uint32_t)((int)acc[q] == Tv[q]) << q;
        lebits |= (uint32_t)((int)acc[q] <= Tv[q]) << q;
      }
      if (!valid) eqbits = lebits = 0;
      // the wave's T-ties per query, counted into its own column of `we`
      for (uint32_t m = eqbits; m; m &= m - 1) atomicAdd(&we[par][__builtin_ctz(m)][wave], 1u);
      __syncthreads();
      // rank of this wave's first T-tie in the segment's label order, per query in lane q;
      // the wave's column of the other buffer is cleared for the next tile
      uint32_t first = seen;
      if (lane < QB) {
        for (int w = 0; w < 4; w++) {
          const uint32_t c = we[par][lane][w];
          if (w < wave) first += c;
          seen += c;
        }
        we[par ^ 1][lane][wave] = 0;
      }
      par ^= 1;
      // one query at a time while any lane has a row to write: about k / nb of the rows do
      for (uint64_t any = __ballot(lebits != 0); any; any = __ballot(lebits != 0)) {
        const int q = __builtin_ctz(__builtin_amdgcn_readlane((int)lebits, __builtin_ctzll(any)));
        uint32_t dist = acc[0];
#pragma unroll
        for (int i = 1; i < QB; i++) dist = q == i ? acc[i] : dist;
        const bool eqb = (eqbits >> q) & 1;
        const bool lt = ((lebits >> q) & 1) && !eqb;
        lebits &= ~(1u << q);
        const uint64_t eqm = __ballot(eqb);
        const size_t qg = (size_t)it.b * QB + q;
        uint32_t slot = 0xFFFFFFFFu;
        if (lt) {
          const uint32_t r = atomicAdd(&cnt[q * HL + dist], 1u);
          slot = a.hist[(qg * a.Sg + it.s) * HL + dist] + r;
        } else if (eqb) {
          const uint32_t rank = (uint32_t)__builtin_amdgcn_readlane(first, q) + (uint32_t)__popcll(eqm & below);
          if (rank < (uint32_t)__builtin_amdgcn_readlane(quotal, q))
            slot = (uint32_t)__builtin_amdgcn_readlane(baseTl, q) + rank;
        }
        if (slot < (uint32_t)a.k) {
          a.D[qg * a.k + slot] = (int32_t)dist;
          a.I[qg * a.k + slot] = row;
        }
      }
    }
    __syncthreads();
    for (int i = tid; i < QB * HL; i += kT) cnt[i] = 0;
    __syncthreads();
  }
}

// ------------------------------------------------------------------ label order
// One workgroup per query: the k outputs as keys (dist << 32 | label) sorted ascending.
// Every (segment, distance) group already lies in its final range; this orders it by label.
__global__ __launch_bounds__(256) void k_hamming_order(int32_t* __restrict__ D, int64_t* __restrict__ I, int k) {
  __shared__ uint64_t key[1024];
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  int n2 = 2;
  while (n2 < k) n2 <<= 1;
  for (int i = tid; i < n2; i += 256)
    key[i] = i < k ? ((uint64_t)(uint32_t)D[q * k + i] << 32) | (uint32_t)I[q * k + i] : ~(uint64_t)0;
  __syncthreads();
  for (int size = 2; size <= n2; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < n2 / 2; i += 256) {
        const int lo = ((i / stride) * stride * 2) + (i % stride);
        const int hi = lo + stride;
        const bool up = (lo & size) == 0;
        const uint64_t x = key[lo], y = key[hi];
        if ((x > y) == up) key[lo] = y, key[hi] = x;
      }
      __syncthreads();
    }
  for (int i = tid; i < k; i += 256) {
    const uint32_t label = (uint32_t)key[i];
    D[q * k + i] = (int32_t)(key[i] >> 32);
    I[q * k + i] = label == 0xFFFFFFFFu ? (int64_t)-1 : (int64_t)label;
  }
}

template <int V, int QB, int DMAX>
void launch_scans(const BinScanArgs& a, const uint32_t* codes, const uint32_t* qw, uint32_t kk, int32_t* T, uint32_t* quota, hipStream_t s) {
  const unsigned grid = (unsigned)std::min(a.nitems, 2 * kBinTargetItems);
  hipLaunchKernelGGL((k_hamming_hist<V, QB, DMAX>), dim3(grid), dim3(kT), 0, s, a, codes, qw);
  hipLaunchKernelGGL(k_hamming_plan, dim3((unsigned)a.nq), dim3(256), 0, s, a.hist, a.Sg, a.d, kk, T, quota);
  hipLaunchKernelGGL((k_hamming_emit<V, QB, DMAX>), dim3(grid), dim3(kT), 0, s, a, codes, qw);
}

}  // namespace

void launch_bin_pad_rows(const uint8_t* src, int64_t n, int code_size, int stride, uint32_t* dst, hipStream_t s) {
  if (n <= 0) return;
  const int W = stride / 4;
  const int64_t total = n * W;
  hipLaunchKernelGGL(k_bin_pad_rows, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, n, code_size, W, dst);
}

void launch_bin_fill_empty(int32_t* D, int64_t* I, int64_t n, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_bin_fill_empty, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, D, I, n);
}

void launch_bin_search(const BinSearchArgs& b, const BinPlan& plan, hipStream_t s) {
  if (b.nq <= 0) return;
  const int code_size = b.d / 8;
  const int W = plan.stride / 4;
  const int V = W >= 4 ? 4 : W;
  const int QB = plan.QB;
  const int64_t nblocks = (b.nq + QB - 1) / QB;
  const int64_t total = nblocks * QB * W;
  hipLaunchKernelGGL(k_bin_pack_queries, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, b.x, b.nq, code_size,
                     W, V, QB, total, b.qw);
  if (b.nb < b.k) launch_bin_fill_empty(b.D, b.I, b.nq * b.k, s);
  BinScanArgs a;
  a.nb = (int)b.nb;
  a.nq = (int)b.nq;
  a.d = b.d;
  a.W = W;
  a.k = b.k;
  a.Sg = plan.Sg;
  a.seg_rows = (int)plan.seg_rows;
  a.nblocks = (int)nblocks;
  a.nitems = (int)(nblocks * plan.Sg);
  a.hist = b.hist;
  a.T = b.T;
  a.quota = b.quota;
  a.D = b.D;
  a.I = b.I;
  const uint32_t kk = (uint32_t)std::min<int64_t>(b.k, b.nb);
  if (QB == 8)
    launch_scans<4, 8, 2048>(a, b.codes, b.qw, kk, b.T, b.quota, s);
  else if (b.d > 256)
    launch_scans<4, 16, 1024>(a, b.codes, b.qw, kk, b.T, b.quota, s);
  else if (V == 4)
    launch_scans<4, 16, 256>(a, b.codes, b.qw, kk, b.T, b.quota, s);
  else if (V == 2)
    launch_scans<2, 16, 256>(a, b.codes, b.qw, kk, b.T, b.quota, s);
  else
    launch_scans<1, 16, 256>(a, b.codes, b.qw, kk, b.T, b.quota, s);
  if (b.k > 1) hipLaunchKernelGGL(k_hamming_order, dim3((unsigned)b.nq), dim3(256), 0, s, b.D, b.I, b.k);
}

}  // namespace chivf
