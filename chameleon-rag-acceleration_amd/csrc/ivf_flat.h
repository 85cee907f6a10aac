// Launchers for the IVF-Flat kernels (ivf_flat.hip): the list-major scan of raw fp32
// vectors behind IndexIVFFlat.  All launchers are asynchronous on `stream` and
// allocate nothing.  Keys follow ivfpq_kernels.h: L2 ranks by the distance itself,
// inner product by the negated similarity, negated back on output; ties by label.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace chivf {

constexpr int kIvfFlatRangeRows = 4096;  // granule of a row range: a longer list is cut into ranges of this many rows
constexpr int kIvfFlatWaves = 4;         // waves per scan workgroup = partial lists per (pair, row range)
// The final top-k is launch_merge_topk composed in rounds: one call never merges more
// than kIvfFlatMergeEntries entries per query (the entries that kernel stages in LDS,
// so that every binary search of a round reads LDS) nor more than kIvfFlatMergeFan lists.
constexpr int kIvfFlatMergeEntries = 2048;
constexpr int kIvfFlatMergeFan = 16;

// How a batch is split.  A (query, probe) pair whose list has n rows owns
// ceil(n / kIvfFlatRangeRows) SLOTS, one per row range; a query's slots are numbered
// in probe order.  `slots` bounds the slots of any query (the host sums the nprobe
// largest lists' range counts).  Every slot holds kIvfFlatWaves sorted partial lists.
struct IvfFlatPlan {
  int G = 1;     // pairs per work item: 8 (k <= 64) or 4
  int S = 0;     // partial lists per query in the workspace (>= slots * kIvfFlatWaves; a power of two above fan)
  int fan = 2;   // lists merged per launch_merge_topk call and query
  int grid = 1;  // scan workgroups (each takes work items grid apart)
};
IvfFlatPlan ivfflat_plan(int k, int64_t slots);

struct IvfFlatArgs {
  const float* x;           // [nq][d] queries
  int64_t nq;
  int d;
  const float* vecs;        // [n][d] the image: lists concatenated, each sorted by label
  const int64_t* ids;       // [n]
  const int64_t* list_off;  // [nlist + 1]
  int nlist;
  const int64_t* probes;    // [nq][nprobe] list ids (-1 = skipped probe)
  int nprobe;
  bool dedup;               // a list id repeated in a row is scanned once (caller-supplied probes)
  int k;
  bool ip;
  // workspace
  int32_t* cnt;       // [nlist] pairs per list (zeroed here)
  int2* bucket;       // [nlist][nq] (query, first slot) of the list's pairs
  int32_t* item_off;  // [nlist + 1] first work item of every list
  int32_t* used;      // [nq] slots the query uses
  uint32_t* tau;      // [nq] the queries' shared bounds (set to "none" here)
  float* partD;       // [plan.S][nq][k]
  int64_t* partI;
  float* tmpD;        // [plan.S / plan.fan][nq][k] (the merge rounds alternate between part and tmp)
  int64_t* tmpI;
  float* D;           // [nq][k] out
  int64_t* I;
};
// plan + scan + merge of one batch; the image holds fewer than 2^31 - 1 rows, 1 <= k <= 1024,
// d % 4 == 0, nq * plan.S < 2^31
void launch_ivfflat_search(const IvfFlatArgs& a, const IvfFlatPlan& plan, hipStream_t s);
// The planning alone, for every list-major scan (launch_ivfflat_search, ivf_sq.h): cnt zeroed,
// tau set to "none", the buckets, item_off and used filled, the partial lists of unused slots
// padded.  With plan.G pairs per item; a.x, a.vecs, a.ids and the outputs are not read.
// probe_of (nullable): [nlist][nq], the probe column of every bucket entry.
void launch_ivfflat_planning(const IvfFlatArgs& a, const IvfFlatPlan& plan, int32_t* probe_of, hipStream_t s);

// D[i] = FLT_MAX (-FLT_MAX for ip), I[i] = -1: the result of searching an empty index (every
// float-distance index), and the pad of partial lists no work item writes
void launch_fill_empty(float* D, int64_t* I, int64_t n, bool ip, hipStream_t s);

}  // namespace chivf
