// Host side of libivfpq.so: the index object behind the C-ABI of include/ivfpq.h.
//
// Owns the trained quantizers and inverted lists on the host (insertion
// order per list, as Faiss ArrayInvertedLists) and their device images in
// HBM, and drives the gfx950 kernels of ivfpq_kernels.hip.  Training and
// encoding run on the GPU; only the k-means centroid update (a per-cluster
// double-precision mean) and list bookkeeping run on the host.
//
// HBM layout (DESIGN.md §Data layout):
//   centroids f32[nlist][d], |c|^2 f32[nlist], codebook f32[M][256][d/M],
//   T1 f32[nlist][M][256] (Faiss precomputed_table), codes u8[ntotal][M]
//   with lists concatenated in list order, ids i64[ntotal] alongside,
//   list offsets i64[nlist+1].
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "ivfpq.h"
#include "ivfpq_test.h"  // the test hooks are defined here too (not part of the drop-in header)
#include "ivfpq_kernels.h"
#include "ivfpq_build.h"
#include "pq_flat.h"
#include "ivf_flat.h"
#include "sq_scan.h"
#include "binary_flat.h"
#include "flat_scan.h"
#include "pca_moments.h"

using namespace chivf;

namespace {

thread_local std::string g_err;

#define HIPCHECK(x)                                                                          \
  do {                                                                                       \
    hipError_t e_ = (x);                                                                     \
    if (e_ != hipSuccess) throw std::runtime_error(std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

void require(bool ok, const std::string& msg) {
  if (!ok) throw std::runtime_error(msg);
}

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  void ensure(size_t b) {
    if (b <= bytes && p) return;
    release();
    if (b == 0) b = 16;
    HIPCHECK(hipMalloc(&p, b));
    bytes = b;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <class T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
};

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    HIPCHECK(hipGetDevice(&prev));
    if (prev != dev) HIPCHECK(hipSetDevice(dev));
  }
  ~DeviceGuard() {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur != prev && prev >= 0) (void)hipSetDevice(prev);
  }
};

// Same generator and update rule as the oracle (oracle/ivfpq_oracle.c,
// or_rand_perm_prefix / or_kmeans_update) so GPU-trained and oracle-trained
// indexes are identical for identical input.
uint64_t splitmix(uint64_t* s) {
  uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

std::vector<int64_t> rand_perm_prefix(int64_t n, int64_t k, uint64_t seed) {
  std::vector<int64_t> p(n), out(k);
  for (int64_t i = 0; i < n; i++) p[i] = i;
  uint64_t s = seed;
  for (int64_t i = 0; i < k; i++) {
    int64_t j = i + (int64_t)(splitmix(&s) % (uint64_t)(n - i));
    std::swap(p[i], p[j]);
    out[i] = p[i];
  }
  return out;
}

// Spherical k-means step (Faiss Clustering with spherical = true, which IndexIVF
// sets for METRIC_INNER_PRODUCT; fvec_renorm_L2): every centroid scaled to unit
// L2 norm.  Same arithmetic as or_renorm_rows in oracle/ivfpq_oracle.c.
void renorm_rows(float* x, int64_t n, int d) {
  for (int64_t i = 0; i < n; i++) {
    float* xi = x + i * d;
    float nr = 0.f;
    for (int t = 0; t < d; t++) nr += xi[t] * xi[t];
    if (nr > 0.f) {
      const float inv = (float)(1.0 / (double)sqrtf(nr));
      for (int t = 0; t < d; t++) xi[t] *= inv;
    }
  }
}

void kmeans_update(const float* x, int64_t n, int d, int k, const int64_t* assign, float* cent) {
  std::vector<double> sum((size_t)k * d, 0.0);
  std::vector<int64_t> cnt(k, 0);
  for (int64_t i = 0; i < n; i++) {
    const int64_t c = assign[i];
    cnt[c]++;
    double* s = &sum[(size_t)c * d];
    const float* xi = x + i * d;
    for (int t = 0; t < d; t++) s[t] += (double)xi[t];
  }
  for (int c = 0; c < k; c++)
    if (cnt[c] > 0)
      for (int t = 0; t < d; t++) cent[(size_t)c * d + t] = (float)(sum[(size_t)c * d + t] / (double)cnt[c]);
  const float eps = 1.0f / 1024.0f;
  for (int c = 0; c < k; c++) {
    if (cnt[c] != 0) continue;
    int big = 0;
    for (int j = 1; j < k; j++)
      if (cnt[j] > cnt[big]) big = j;
    for (int t = 0; t < d; t++) {
      const float v = cent[(size_t)big * d + t];
      if (t % 2 == 0) {
        cent[(size_t)c * d + t] = v * (1.0f + eps);
        cent[(size_t)big * d + t] = v * (1.0f - eps);
      } else {
        cent[(size_t)c * d + t] = v * (1.0f - eps);
        cent[(size_t)big * d + t] = v * (1.0f + eps);
      }
    }
    cnt[c] = cnt[big] / 2;
    cnt[big] -= cnt[c];
  }
}

constexpr size_t kChunkBytes = size_t(256) << 20;    // bound for [rows][cols] fp32 scratch
constexpr size_t kPartialBytes = size_t(2048) << 20;  // bound for a chunk's per-wave partial top-k lists
// from this nlist on, the coarse quantizer never writes the key matrix (r03 A/B at
// C2, nlist 1024: segmented 22.5 + 8.5 us + a separate T3 launch 13.0 us vs key
// matrix 17.8 + 10.0 us with T3 in the same launch)
constexpr int kSegmentedNlist = 8192;
// Default of a handle's batches-in-flight switch (ivfpq_set_inflight): with it
// on, device searches on different streams overlap, each on its own per-stream
// workspace; off, a search is ordered after every search still in flight on
// another stream.  IVFPQ_INFLIGHT=1 in the environment turns it on for new handles.
bool inflight_default() {
  const char* e = std::getenv("IVFPQ_INFLIGHT");
  return e && e[0] == '1';
}

}  // namespace

struct ivfpq_index {
  int d = 0, nlist = 0, M = 0, nbits = 8, ksub = 256, metric = IVFPQ_METRIC_L2, device = 0;
  int nprobe = 1;
  int list_lo = 0, list_hi = 0;
  bool trained = false;
  std::vector<float> centroids, codebook;
  std::vector<std::vector<uint8_t>> lcodes;
  std::vector<std::vector<int64_t>> lids;
  int64_t ntotal = 0;
  int64_t next_id = 0;

  DevBuf d_cent, d_centT, d_cnorm, d_cb, d_T1, d_codes, d_ids, d_off, d_order;
  bool dirty = true;
  hipStream_t stream = nullptr;
  // scratch
  DevBuf w_x, w_xn, w_D, w_I, w_lno, w_codes, w_cent, w_cn;
  DevBuf h_D, h_I, h_Iq, h_Dq;  // device staging of the host-buffer entry points
  // device-side adds not yet merged into the image (add_dev / flush_pending): list
  // numbers (any list; entries outside [list_lo, list_hi) are dropped at the merge),
  // labels and codes, q_n of them (q_kept inside the range); a_off: small scratch
  DevBuf q_lists, q_ids, q_codes, a_off;
  int64_t q_n = 0, q_kept = 0, q_cap = 0;
  int64_t img_n = 0;  // entries in the device image (ntotal = img_n + q_kept)
  bool host_stale = false;  // the device image holds entries the host lists lack (device-side adds)
  // T3 of a batch computed ahead (ivfpq_precompute_tables_device), handed to a
  // preassigned search by the token that call returned (seq)
  struct PreT3 {
    DevBuf buf;
    int64_t n = 0;
    uint64_t seq = 0;  // the token; 0 = free
    uint64_t freed_seq = 0;  // order in which free entries were consumed (reuse the longest-free one)
    hipEvent_t ready = nullptr;  // recorded after the table launch
    hipStream_t ready_stream = nullptr;
    hipEvent_t freed = nullptr;  // recorded after the consuming search's scans
    hipStream_t freed_stream = nullptr;
    bool ready_pending = false, freed_pending = false;
  };
  static constexpr int kPreT3 = 3;  // tables of up to three batches ahead (batches in flight)
  PreT3 pre[kPreT3];
  uint64_t pre_seq = 0;
  // The per-batch workspaces of a device search (coarse keys, probes, T3, the
  // list-major plan of ivfpq_kernels.h ListPlan and the partial lists).  A handle
  // holds kSlots of them, one per stream in use (begin_slot), so that up to
  // kSlots batches can be in flight on different streams at once: the next
  // batch's coarse step and list scan start while this batch's scan drains
  // (DESIGN.md §4).
  struct Work {
    DevBuf w_dist, w_lists, w_dis0, w_T3, w_cand;  // w_cand: large-nlist coarse segment candidates
    DevBuf w_qn;  // |x|^2 of the batch's queries (tiled coarse keys)
    DevBuf p_cnt, p_bucket, p_recs, p_hdr, p_part, p_N, p_pd0, p_done, p_tau, p_qmask, p_evlog;
    uint32_t epoch = 0;  // tag of the last batch planned in this workspace (ListPlan::tauq)
    // every use records `done` on its stream; the slot's next user (on another
    // stream) waits for it, and whatever frees or rewrites shared device buffers
    // synchronizes on every slot's first
    hipEvent_t done = nullptr;
    hipStream_t done_stream = nullptr;
    bool done_pending = false;
    uint64_t last_use = 0;
  };
  static constexpr int kSlots = 3;
  Work work[kSlots];
  int slot = 0;  // the workspace of the current (last begun) device call
  uint64_t uses = 0;
  bool inflight = inflight_default();
  int fault_inj = 0;  // test hook (ivfpq_set_fault_injection): ListPlan::fault
  std::vector<uint64_t> tau_seed;  // test hook (ivfpq_debug_seed_tau): the next batch's starting bounds
  std::mutex mu;

  Work& W() { return work[slot]; }
  // The workspace of a device call on stream s: the one last used on s (stream
  // order already protects it, and a one-stream caller keeps a single
  // workspace), else the least recently used one, ordered after its last user.
  // With inflight on, this call may run concurrently with calls on other streams;
  // otherwise it is ordered after every call in flight.
  void begin_slot(hipStream_t s) {
    int pick = -1;
    for (int i = 0; i < kSlots && pick < 0; i++)
      if (work[i].done_pending && work[i].done_stream == s) pick = i;
    if (pick < 0) {
      pick = 0;
      for (int i = 1; i < kSlots; i++)
        if (work[i].last_use < work[pick].last_use) pick = i;
    }
    slot = pick;
    Work& w = work[slot];
    w.last_use = ++uses;
    // Taking over another stream's workspace (more streams than kSlots) waits on
    // the host: a device-side wait here let a k = 100 batch on a fourth stream see
    // its predecessor's partial lists (1 batch in 480, tests/test_gpu_parity.py
    // test_batches_in_flight_on_round_robin_streams), which two or three streams
    // never do.
    if (w.done_pending && w.done_stream != s) {
      HIPCHECK(hipEventSynchronize(w.done));
      w.done_pending = false;
    }
    if (!inflight) order_after_all(s);
  }
  // ordered after every device call still in flight (for paths that touch the
  // shared staging buffers or T3-ahead state)
  void order_after_all(hipStream_t s) {
    for (auto& w : work)
      if (w.done_pending && w.done_stream != s) HIPCHECK(hipStreamWaitEvent(s, w.done, 0));
  }
  void mark_done(hipStream_t s) {
    Work& w = W();
    HIPCHECK(hipEventRecord(w.done, s));
    w.done_stream = s;
    w.done_pending = true;
  }
  void quiesce() {
    for (auto& w : work) {
      if (w.done_pending) HIPCHECK(hipEventSynchronize(w.done));
      w.done_pending = false;
    }
  }

  ListPlan make_plan(int64_t nq, int np, int k, hipStream_t s, bool leave_free = false) {
    const int nloc = std::max(list_hi - list_lo, 1);
    Work& w = W();
    const int G = list_scan_group(M, k);
    ListPlan pl;
    pl.cap = (int)nq;
    pl.max_items = list_scan_max_items(nq * np, nloc, G);
    if (!w.p_cnt.p || w.p_cnt.bytes < sizeof(int32_t) * 2 * nloc) {
      // kept zero between batches by k_scan_lists; zeroed once here
      w.p_cnt.ensure(sizeof(int32_t) * 2 * nloc);
      HIPCHECK(hipMemsetAsync(w.p_cnt.p, 0, w.p_cnt.bytes, s));
    }
    w.p_bucket.ensure(sizeof(int2) * 2 * (size_t)nloc * nq);
    w.p_recs.ensure(sizeof(int32_t) * 16 * (size_t)pl.max_items);
    if (!w.p_hdr.p) {  // hdr[2] (the scan's work counter) is kept zero between batches by k_merge_probes
      w.p_hdr.ensure(sizeof(int32_t) * 16);
      HIPCHECK(hipMemsetAsync(w.p_hdr.p, 0, w.p_hdr.bytes, s));
    }
    pl.ks = part_stride(k);
    w.p_part.ensure(sizeof(uint4) * nq * np * 4 * pl.ks);
    w.p_N.ensure(sizeof(uint2) * nq * np * 4);
    w.p_pd0.ensure(sizeof(float) * nq * np);
    if (!w.p_evlog.p) {
      w.p_evlog.ensure(sizeof(uint32_t) * 8 * kEvLog);
      HIPCHECK(hipMemsetAsync(w.p_evlog.p, 0, w.p_evlog.bytes, s));
    }
    if (!w.p_done.p || w.p_done.bytes < sizeof(int32_t) * nq) {  // kept zero between batches by k_merge_probes
      w.p_done.ensure(sizeof(int32_t) * nq);
      HIPCHECK(hipMemsetAsync(w.p_done.p, 0, w.p_done.bytes, s));
    }
    if (!w.p_tau.p || w.p_tau.bytes < sizeof(uint64_t) * nq) {  // all-ones: no batch's bound (ListPlan::tauq)
      w.p_tau.ensure(sizeof(uint64_t) * nq);
      HIPCHECK(hipMemsetAsync(w.p_tau.p, 0xff, w.p_tau.bytes, s));
    }
    if (++w.epoch >= 0xFFFFFFF0u) {  // tag space used up (after ~4e9 batches): start over on a clean buffer
      if (w.done_pending) HIPCHECK(hipEventSynchronize(w.done));
      HIPCHECK(hipMemsetAsync(w.p_tau.p, 0xff, w.p_tau.bytes, s));
      w.epoch = 1;
    }
    if (!tau_seed.empty()) {  // one-shot: this batch starts with the seeded bounds (its own tag)
      // disarmed before the check: a mismatched seed fails this search only, not every later one
      // (the hook applies to single-chunk searches of exactly the seeded size)
      std::vector<uint64_t> seed;
      seed.swap(tau_seed);
      require((int64_t)seed.size() == nq, "seeded bounds: one per query of the next batch (single-chunk searches)");
      for (auto& v : seed) v = ((uint64_t)(~w.epoch) << 32) | (uint32_t)v;
      HIPCHECK(hipMemcpyAsync(w.p_tau.p, seed.data(), sizeof(uint64_t) * nq, hipMemcpyHostToDevice, s));
      HIPCHECK(hipStreamSynchronize(s));
    }
    pl.qmw = (np + 63) / 64;
    w.p_qmask.ensure(sizeof(uint64_t) * nq * pl.qmw);
    pl.cnt = w.p_cnt.as<int32_t>();
    pl.bucket = w.p_bucket.as<int2>();
    pl.recs = w.p_recs.as<int32_t>();
    pl.hdr = w.p_hdr.as<int32_t>();
    pl.part = w.p_part.as<uint4>();
    pl.partN = w.p_N.as<uint2>();
    pl.pd0 = w.p_pd0.as<float>();
    pl.evlog = w.p_evlog.as<uint32_t>();
    pl.fault = fault_inj;
    pl.qdone = w.p_done.as<int32_t>();
    pl.tauq = w.p_tau.as<uint64_t>();
    pl.epoch = w.epoch;
    pl.err = w.p_hdr.as<int32_t>() + 15;
    pl.qmask = w.p_qmask.as<uint64_t>();
    pl.order = d_order.p ? d_order.as<int32_t>() : nullptr;
    pl.fused = scan_fused_plan(nloc, pl.max_items, M) ? 1 : 0;
    // leave_free (a full search with batches in flight): the scan leaves
    // scan_inflight_free_cus() CUs, chosen per scan kernel, to the other streams' coarse
    // and merge kernels (r06x sweep of the one-pass scans: C2 step -2.5 %;
    // DESIGN.md section 4); one batch at a time, and in the shard flow's preassigned
    // searches, where the sweep was inconclusive, it takes them all
    // (and the four-pass scan is capped at scan_inflight_wgs_per_cu() workgroups per CU)
    pl.grid = scan_lists_grid(M, k, pl.fused != 0, leave_free ? scan_inflight_free_cus(M, k, pl.fused != 0) : 0,
                              leave_free ? scan_inflight_wgs_per_cu(M, k, pl.fused != 0) : 0, &pl.lds_pad);
    return pl;
  }

  // stage timing (HIP events recorded on the launch stream around each stage)
  enum Stage { ST_COARSE = 0, ST_TABLES = 1, ST_SCAN = 2, ST_LISTS = 3, ST_N = 4 };
  int timing = 0;  // 0 off, 1 every stage, 2 the list-scan kernel only
  struct Mark {
    int stage;
    hipEvent_t a, b;  // adjacent: &a is passed as an event pair
  };
  std::vector<Mark> marks;
  std::vector<hipEvent_t> ev_pool;

  hipEvent_t take_event() {
    if (!ev_pool.empty()) {
      hipEvent_t e = ev_pool.back();
      ev_pool.pop_back();
      return e;
    }
    hipEvent_t e;
    HIPCHECK(hipEventCreate(&e));
    return e;
  }
  // returns an index into marks (or -1 when timing is off)
  // record = false: the caller records the pair itself (ST_LISTS, around one kernel)
  int mark_begin(int stage, hipStream_t s, bool record = true) {
    if (!timing || (timing == 2 && stage != ST_LISTS)) return -1;
    Mark m{stage, take_event(), take_event()};
    if (record) HIPCHECK(hipEventRecord(m.a, s));
    marks.push_back(m);
    return (int)marks.size() - 1;
  }
  void mark_end(int idx, hipStream_t s) {
    if (idx >= 0) HIPCHECK(hipEventRecord(marks[idx].b, s));
  }
  void collect_timing(double* ms, int64_t* cnt) {
    for (int i = 0; i < ST_N; i++) {
      ms[i] = 0.0;
      cnt[i] = 0;
    }
    for (auto& m : marks) {
      HIPCHECK(hipEventSynchronize(m.b));
      float t = 0.f;
      HIPCHECK(hipEventElapsedTime(&t, m.a, m.b));
      ms[m.stage] += t;
      cnt[m.stage] += 1;
      ev_pool.push_back(m.a);
      ev_pool.push_back(m.b);
    }
    marks.clear();
  }

  ~ivfpq_index() {
    for (auto& m : marks) {
      (void)hipEventDestroy(m.a);
      (void)hipEventDestroy(m.b);
    }
    for (auto e : ev_pool) (void)hipEventDestroy(e);
    for (auto& w : work)
      if (w.done) (void)hipEventDestroy(w.done);
    for (auto& p : pre) {
      if (p.ready) (void)hipEventDestroy(p.ready);
      if (p.freed) (void)hipEventDestroy(p.freed);
    }
    if (stream) (void)hipStreamDestroy(stream);
  }

  void init_stream() {
    if (!stream) HIPCHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (auto& w : work)
      if (!w.done) HIPCHECK(hipEventCreateWithFlags(&w.done, hipEventDisableTiming));
    for (auto& p : pre) {
      if (!p.ready) HIPCHECK(hipEventCreateWithFlags(&p.ready, hipEventDisableTiming));
      if (!p.freed) HIPCHECK(hipEventCreateWithFlags(&p.freed, hipEventDisableTiming));
    }
  }

  // ---------------------------------------------------------------- helpers
  // Row-wise top-1 of x [n][dd] against c (already on device with norms):
  // writes assignments (host) for all rows. Uses w_x / w_xn / w_dist / w_D / w_I.
  // ip: assign to the largest inner product (the IndexFlatIP quantizer of an IP index)
  void assign_top1(const float* x_host, int64_t n, int dd, const float* dc, const float* dcn, int nc,
                   int64_t* assign_host, const float* x_dev = nullptr, bool ip_assign = false) {
    const int64_t rows = std::max<int64_t>(1, std::min<int64_t>(n, kChunkBytes / ((size_t)nc * 4)));
    w_xn.ensure(sizeof(float) * rows);
    W().w_dist.ensure(sizeof(float) * rows * nc);
    w_D.ensure(sizeof(float) * rows);
    w_I.ensure(sizeof(int64_t) * rows);
    if (!x_dev) w_x.ensure(sizeof(float) * rows * dd);
    for (int64_t r0 = 0; r0 < n; r0 += rows) {
      const int64_t c = std::min(rows, n - r0);
      const float* xd;
      if (x_dev) {
        xd = x_dev + r0 * dd;
      } else {
        HIPCHECK(hipMemcpyAsync(w_x.p, x_host + r0 * dd, sizeof(float) * c * dd, hipMemcpyHostToDevice, stream));
        xd = w_x.as<float>();
      }
      if (!ip_assign) launch_row_norms(xd, c, dd, w_xn.as<float>(), stream);
      launch_l2_dist(xd, w_xn.as<float>(), c, dc, dcn, nc, dd, W().w_dist.as<float>(), stream, ip_assign);
      launch_select_rows(W().w_dist.as<float>(), c, nc, 1, w_D.as<float>(), w_I.as<int64_t>(), stream);
      HIPCHECK(hipGetLastError());
      HIPCHECK(hipMemcpyAsync(assign_host + r0, w_I.p, sizeof(int64_t) * c, hipMemcpyDeviceToHost, stream));
      HIPCHECK(hipStreamSynchronize(stream));
    }
  }

  void kmeans(const float* x, int64_t n, int dd, int k, int niter, uint64_t seed, float* cent,
              bool ip_assign = false) {
    require(n >= k, "k-means: need at least as many training points as centroids (" + std::to_string(n) + " < " +
                        std::to_string(k) + ")");
    const auto init = rand_perm_prefix(n, k, seed);
    for (int c = 0; c < k; c++) std::memcpy(cent + (size_t)c * dd, x + init[c] * dd, sizeof(float) * dd);
    if (ip_assign) renorm_rows(cent, k, dd);  // spherical: unit-norm centroids (Faiss post_process_centroids)
    // keep the whole training set resident when it fits the scratch bound
    DevBuf xall;
    const bool resident = (size_t)n * dd * 4 <= (size_t(2) << 30);
    if (resident) {
      xall.ensure(sizeof(float) * n * dd);
      HIPCHECK(hipMemcpyAsync(xall.p, x, sizeof(float) * n * dd, hipMemcpyHostToDevice, stream));
    }
    std::vector<int64_t> assign(n);
    w_cent.ensure(sizeof(float) * k * dd);
    w_cn.ensure(sizeof(float) * k);
    for (int it = 0; it < niter; it++) {
      HIPCHECK(hipMemcpyAsync(w_cent.p, cent, sizeof(float) * k * dd, hipMemcpyHostToDevice, stream));
      launch_row_norms(w_cent.as<float>(), k, dd, w_cn.as<float>(), stream);
      assign_top1(x, n, dd, w_cent.as<float>(), w_cn.as<float>(), k, assign.data(),
                  resident ? xall.as<float>() : nullptr, ip_assign);
      kmeans_update(x, n, dd, k, assign.data(), cent);
      if (ip_assign) renorm_rows(cent, k, dd);
    }
  }

  void upload_trained() {
    quiesce();
    drop_tables();
    d_cent.ensure(sizeof(float) * nlist * d);
    d_cnorm.ensure(sizeof(float) * nlist);
    d_cb.ensure(sizeof(float) * M * ksub * (d / M));
    d_T1.ensure(sizeof(float) * (size_t)nlist * M * ksub);
    HIPCHECK(hipMemcpyAsync(d_cent.p, centroids.data(), sizeof(float) * nlist * d, hipMemcpyHostToDevice, stream));
    HIPCHECK(hipMemcpyAsync(d_cb.p, codebook.data(), sizeof(float) * codebook.size(), hipMemcpyHostToDevice,
                            stream));
    launch_row_norms(d_cent.as<float>(), nlist, d, d_cnorm.as<float>(), stream);
    {  // transposed centroids [d][nlist] for the fused coarse kernel
      const int ldc = (nlist + 3) & ~3;  // rows padded to a multiple of 4 (branch-free float4 loads)
      std::vector<float> ct((size_t)ldc * d, 0.f);
      for (int l = 0; l < nlist; l++)
        for (int t = 0; t < d; t++) ct[(size_t)t * ldc + l] = centroids[(size_t)l * d + t];
      d_centT.ensure(sizeof(float) * ct.size());
      HIPCHECK(hipMemcpyAsync(d_centT.p, ct.data(), sizeof(float) * ct.size(), hipMemcpyHostToDevice, stream));
      HIPCHECK(hipStreamSynchronize(stream));
    }
    launch_precompute_T1(d_cent.as<float>(), nlist, d, d_cb.as<float>(), M, ksub, d_T1.as<float>(), stream);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(stream));
    trained = true;
  }

  void upload_lists() {
    flush_pending(stream);
    if (!dirty) return;
    quiesce();  // in-flight searches may still read the old device lists
    std::vector<int64_t> off(nlist + 1, 0);
    for (int l = 0; l < nlist; l++) off[l + 1] = off[l] + (int64_t)lids[l].size();
    const int64_t tot = off[nlist];
    std::vector<uint8_t> codes((size_t)tot * M);
    std::vector<int64_t> ids((size_t)tot);
    // Device image: each list sorted by label (stable).  Results do not depend
    // on the order inside a list, and label-sorted lists let the scan kernels
    // rank candidates by code position instead of loading labels.
    std::vector<int64_t> perm;
    for (int l = 0; l < nlist; l++) {
      const int64_t n = (int64_t)lids[l].size();
      if (!n) continue;
      perm.resize(n);
      for (int64_t i = 0; i < n; i++) perm[i] = i;
      const int64_t* lid = lids[l].data();
      std::stable_sort(perm.begin(), perm.end(), [lid](int64_t a, int64_t b) { return lid[a] < lid[b]; });
      for (int64_t i = 0; i < n; i++) {
        uint8_t* dst = codes.data() + (off[l] + i) * M;
        const uint8_t* src = lcodes[l].data() + perm[i] * M;
        std::memcpy(dst, src, M);
        ids[off[l] + i] = lid[perm[i]];
      }
    }
    set_list_order(off);
    d_codes.ensure(std::max<size_t>(16, codes.size()));
    d_ids.ensure(std::max<size_t>(16, sizeof(int64_t) * ids.size()));
    d_off.ensure(sizeof(int64_t) * off.size());
    if (tot) {
      HIPCHECK(hipMemcpyAsync(d_codes.p, codes.data(), codes.size(), hipMemcpyHostToDevice, stream));
      HIPCHECK(hipMemcpyAsync(d_ids.p, ids.data(), sizeof(int64_t) * ids.size(), hipMemcpyHostToDevice, stream));
    }
    HIPCHECK(hipMemcpyAsync(d_off.p, off.data(), sizeof(int64_t) * off.size(), hipMemcpyHostToDevice, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    img_n = tot;
    dirty = false;
  }

  // The host lists from the device image (after device-side adds), in image
  // order: each list label-sorted.
  void sync_host() {
    if (!host_stale) return;
    flush_pending(stream);
    quiesce();
    std::vector<int64_t> off(nlist + 1);
    HIPCHECK(hipMemcpy(off.data(), d_off.p, sizeof(int64_t) * (nlist + 1), hipMemcpyDeviceToHost));
    const int64_t tot = off[nlist];
    std::vector<uint8_t> codes((size_t)tot * M);
    std::vector<int64_t> ids((size_t)tot);
    if (tot) {
      HIPCHECK(hipMemcpy(codes.data(), d_codes.p, codes.size(), hipMemcpyDeviceToHost));
      HIPCHECK(hipMemcpy(ids.data(), d_ids.p, sizeof(int64_t) * ids.size(), hipMemcpyDeviceToHost));
    }
    for (int l = 0; l < nlist; l++) {
      lids[l].assign(ids.begin() + off[l], ids.begin() + off[l + 1]);
      lcodes[l].assign(codes.begin() + off[l] * M, codes.begin() + off[l + 1] * M);
    }
    host_stale = false;
  }

  // Device-side add of n vectors (x on the host or the device; ids nullable =
  // sequential): coarse assignment on the matrix cores (the search's coarse
  // kernels, top-1) and PQ encode into the pending set (q_*), no per-chunk host
  // synchronization.  The pending set is merged into the image (flush_pending)
  // before the lists are next read, or once it holds as many entries as the
  // image: every entry is then moved O(1) times over any sequence of adds
  // (Chameleon adds a 1e9 base in 1e6 slices, bench_gpu_1bn.py:598-658; beir in
  // 50k chunks, faiss_index.py:40-42), instead of the whole image being
  // re-sorted at every add.
  void add_dev(int64_t n, const float* x, bool x_on_device, const int64_t* ids, bool ids_on_device, hipStream_t s) {
    require(trained, "index is not trained");
    if (n <= 0) return;
    upload_lists();  // host-side adds not yet in the image
    order_after_all(s);
    quiesce();
    // the pending sort permutes entries with 32-bit indices
    require(q_n + n < (int64_t(1) << 32) - 1, "more than 2^32 - 2 vectors pending in one merge");
    const int64_t rows = nlist >= kSegmentedNlist ? std::min<int64_t>(n, 1 << 18)
                                                  : std::max<int64_t>(1, std::min<int64_t>(n, kChunkBytes / ((size_t)nlist * 4)));
    pend_reserve(q_n + n, s);
    int64_t* lists = q_lists.as<int64_t>() + q_n;
    w_D.ensure(sizeof(float) * rows);
    if (!x_on_device) w_x.ensure(sizeof(float) * rows * d);
    for (int64_t r0 = 0; r0 < n; r0 += rows) {
      const int64_t c = std::min(rows, n - r0);
      const float* xd = x + r0 * d;
      if (!x_on_device) {
        HIPCHECK(hipMemcpyAsync(w_x.p, xd, sizeof(float) * c * d, hipMemcpyHostToDevice, s));
        xd = w_x.as<float>();
      }
      coarse_launch(xd, c, 1, w_D.as<float>(), lists + r0, s);
      launch_pq_encode(xd, c, d, d_cent.as<float>(), lists + r0, d_cb.as<float>(), M, ksub,
                       q_codes.as<uint8_t>() + (q_n + r0) * M, s);
      HIPCHECK(hipGetLastError());
      if (!x_on_device) HIPCHECK(hipStreamSynchronize(s));  // w_x is reused by the next chunk's copy
    }
    if (!ids) {
      launch_iota_i64(q_ids.as<int64_t>() + q_n, n, next_id, s);
      next_id += n;
    } else {
      HIPCHECK(hipMemcpyAsync(q_ids.as<int64_t>() + q_n, ids, sizeof(int64_t) * n,
                              ids_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    }
    int64_t kept = n;
    if (list_lo > 0 || list_hi < nlist) {  // a list-range shard keeps its own lists only
      a_off.ensure(sizeof(unsigned long long));
      HIPCHECK(hipMemsetAsync(a_off.p, 0, sizeof(unsigned long long), s));
      HIPCHECK(count_kept(lists, n, list_lo, list_hi, a_off.as<unsigned long long>(), s));
      unsigned long long k = 0;
      HIPCHECK(hipMemcpyAsync(&k, a_off.p, sizeof(k), hipMemcpyDeviceToHost, s));
      HIPCHECK(hipStreamSynchronize(s));
      kept = (int64_t)k;
    } else {
      HIPCHECK(hipStreamSynchronize(s));
    }
    q_n += n;
    q_kept += kept;
    ntotal += kept;
    host_stale = true;
    dirty = false;
    if (q_n >= std::max<int64_t>(img_n, int64_t(1) << 24)) flush_pending(s);
  }

  void pend_reserve(int64_t need, hipStream_t s) {
    if (need <= q_cap) return;
    const int64_t cap = std::max<int64_t>(need, q_cap * 2);
    DevBuf l2, i2, c2;
    l2.ensure(sizeof(int64_t) * cap);
    i2.ensure(sizeof(int64_t) * cap);
    c2.ensure((size_t)cap * M);
    if (q_n > 0) {
      HIPCHECK(hipMemcpyAsync(l2.p, q_lists.p, sizeof(int64_t) * q_n, hipMemcpyDeviceToDevice, s));
      HIPCHECK(hipMemcpyAsync(i2.p, q_ids.p, sizeof(int64_t) * q_n, hipMemcpyDeviceToDevice, s));
      HIPCHECK(hipMemcpyAsync(c2.p, q_codes.p, (size_t)q_n * M, hipMemcpyDeviceToDevice, s));
      HIPCHECK(hipStreamSynchronize(s));
    }
    std::swap(q_lists.p, l2.p);
    std::swap(q_lists.bytes, l2.bytes);
    std::swap(q_ids.p, i2.p);
    std::swap(q_ids.bytes, i2.bytes);
    std::swap(q_codes.p, c2.p);
    std::swap(q_codes.bytes, c2.bytes);
    q_cap = cap;
  }

  void drop_pending() {
    q_lists.release();
    q_ids.release();
    q_codes.release();
    q_n = q_kept = q_cap = 0;
  }

  // The pending entries merged into the device image: sorted by (list, label)
  // alone (rocprim radix sorts of the pending set, out-of-range lists dropped),
  // then interleaved list by list into the label-sorted image (ivfpq_build.h
  // image_merge_lists).  The result equals a stable (list, label) sort of old +
  // new, the image order of DESIGN.md §3.
  void flush_pending(hipStream_t s) {
    if (q_n == 0) return;
    quiesce();  // in-flight searches read the current image
    ImageMergeArgs g;
    g.nlist = nlist;
    g.lo = list_lo;
    g.hi = list_hi;
    g.M = M;
    g.n_old = 0;
    g.n_new = q_n;
    g.new_lists = q_lists.as<int64_t>();
    g.new_ids = q_ids.as<int64_t>();
    g.new_codes = q_codes.as<uint8_t>();
    DevBuf new_off, out_off;
    new_off.ensure(sizeof(int64_t) * (nlist + 1));
    g.off_out = new_off.as<int64_t>();
    {
      const size_t sb = image_merge_scratch_bytes(q_n, nlist);
      DevBuf scratch, codes_n, ids_n;
      scratch.ensure(sb);
      HIPCHECK(image_merge_sort(g, scratch.p, sb, s));
      std::vector<int64_t> noff(nlist + 1), ooff(nlist + 1);
      HIPCHECK(hipMemcpyAsync(noff.data(), new_off.p, sizeof(int64_t) * (nlist + 1), hipMemcpyDeviceToHost, s));
      HIPCHECK(hipMemcpyAsync(ooff.data(), d_off.p, sizeof(int64_t) * (nlist + 1), hipMemcpyDeviceToHost, s));
      HIPCHECK(hipStreamSynchronize(s));
      const int64_t kept = noff[nlist];
      require(kept == q_kept, "pending merge: kept entries disagree with the add-time count");
      codes_n.ensure(std::max<size_t>(16, (size_t)kept * M));
      ids_n.ensure(std::max<size_t>(16, sizeof(int64_t) * kept));
      g.codes_out = codes_n.as<uint8_t>();
      g.ids_out = ids_n.as<int64_t>();
      HIPCHECK(image_merge_gather(g, kept, scratch.p, s));
      scratch.release();
      std::vector<int64_t> off(nlist + 1);
      int64_t mx = 0;
      for (int l = 0; l <= nlist; l++) {
        off[l] = ooff[l] + noff[l];
        if (l < nlist) mx = std::max(mx, (ooff[l + 1] - ooff[l]) + (noff[l + 1] - noff[l]));
      }
      const int64_t n_out = off[nlist];
      DevBuf codes2, ids2;
      codes2.ensure(std::max<size_t>(16, (size_t)n_out * M));
      ids2.ensure(std::max<size_t>(16, sizeof(int64_t) * n_out));
      out_off.ensure(sizeof(int64_t) * (nlist + 1));
      ListMergeArgs m;
      m.nlist = nlist;
      m.lo = list_lo;
      m.hi = list_hi;
      m.M = M;
      m.max_list = mx;
      m.old_off = d_off.as<int64_t>();
      m.old_codes = d_codes.as<uint8_t>();
      m.old_ids = d_ids.as<int64_t>();
      m.new_off = new_off.as<int64_t>();
      m.new_codes = codes_n.as<uint8_t>();
      m.new_ids = ids_n.as<int64_t>();
      m.out_off = out_off.as<int64_t>();
      m.out_codes = codes2.as<uint8_t>();
      m.out_ids = ids2.as<int64_t>();
      HIPCHECK(image_merge_lists(m, s));
      HIPCHECK(hipStreamSynchronize(s));
      std::swap(d_codes.p, codes2.p);
      std::swap(d_codes.bytes, codes2.bytes);
      std::swap(d_ids.p, ids2.p);
      std::swap(d_ids.bytes, ids2.bytes);
      std::swap(d_off.p, out_off.p);
      std::swap(d_off.bytes, out_off.bytes);
      img_n = n_out;
      set_list_order(off);
    }
    drop_pending();
    require(img_n == ntotal, "pending merge: image size disagrees with ntotal");
  }

  // Scheduling order of the shard's lists: largest first (the list scan takes
  // items in this order within each kind, so the items that finish last are the
  // short ones: longest-processing-time-first bounds the persistent grid's tail).
  void set_list_order(const std::vector<int64_t>& off) {
    const int nloc = std::max(list_hi - list_lo, 1);
    std::vector<int32_t> order(nloc);
    for (int j = 0; j < nloc; j++) order[j] = j;
    if (list_hi > list_lo)
      std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        return off[list_lo + a + 1] - off[list_lo + a] > off[list_lo + b + 1] - off[list_lo + b];
      });
    d_order.ensure(sizeof(int32_t) * nloc);
    HIPCHECK(hipMemcpyAsync(d_order.p, order.data(), sizeof(int32_t) * nloc, hipMemcpyHostToDevice, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }

  void append(int64_t n, const int64_t* lno, const uint8_t* codes, const int64_t* ids) {
    sync_host();
    for (int64_t i = 0; i < n; i++) {
      const int64_t l = lno[i];
      require(l >= 0 && l < nlist, "list number out of range");
      if (l < list_lo || l >= list_hi) continue;  // another shard's list
      lcodes[l].insert(lcodes[l].end(), codes + i * M, codes + (i + 1) * M);
      lids[l].push_back(ids[i]);
      ntotal++;
    }
    dirty = true;
  }

  int eff_nprobe() const { return std::min(nprobe, nlist); }

  void check_search(int64_t n, int k) {
    require(trained, "index is not trained");
    require(n >= 0, "n must be >= 0");
    require(k >= 1 && k <= kMaxK, "k must be in [1, " + std::to_string(kMaxK) + "]");
  }

  bool ip() const { return metric == IVFPQ_METRIC_INNER_PRODUCT; }

  // Coarse quantizer for c queries at x: the nprobe best lists and the
  // quantizer's values (L2 distances / IP similarities), from the key matrix
  // built on the matrix cores (with T3out, the same launch builds T3).  With
  // `plan` and nprobe <= 64 the selection also plans the batch and true is
  // returned; otherwise the caller plans with launch_plan_count.
  // xt / nt (nullable): T3out holds the tables of the queries xt instead of x (the
  // shard step: keys of this rank's slice, tables of the global batch, one launch)
  bool coarse_launch(const float* x, int64_t c, int np, float* dis, int64_t* lists, hipStream_t s,
                     const ListPlan* plan = nullptr, float* T3out = nullptr, const float* xt = nullptr,
                     int64_t nt = 0, bool hoist = false) {
    if (!xt) {
      xt = x;
      nt = c;
    }
    if (nlist >= kSegmentedNlist && np <= 64) {  // large nlist: no [c][nlist] key matrix
      W().w_cand.ensure(sizeof(uint64_t) * c * coarse_segments(c, nlist, d) * np);
      if (T3out) launch_ip_table(xt, nt, d, d_cb.as<float>(), M, ksub, T3out, s);
      launch_coarse_segmented(x, c, d, d_centT.as<float>(), d_cnorm.as<float>(), nlist, np, W().w_cand.as<uint64_t>(),
                              dis, lists, s, ip(), plan, d_off.as<int64_t>(), list_lo, list_hi, d_cent.as<float>());
      return plan != nullptr;
    }
    W().w_dist.ensure(sizeof(float) * c * nlist);
    W().w_qn.ensure(sizeof(float) * c);
    launch_coarse_keys(x, c, d, d_centT.as<float>(), d_cnorm.as<float>(), nlist, W().w_dist.as<float>(), s, ip(), T3out,
                       d_cb.as<float>(), M, W().w_qn.as<float>(), xt, nt, hoist);
    if (np <= 64) {
      launch_coarse_select(W().w_dist.as<float>(), c, nlist, np, dis, lists, s, ip(), plan, d_off.as<int64_t>(), list_lo,
                           list_hi, x, d_cent.as<float>(), d);
      return plan != nullptr;
    }
    launch_select_rows(W().w_dist.as<float>(), c, nlist, np, dis, lists, s, ip());
    return false;
  }

  // The full search on device pointers, on stream s.  Iq/Dq non-null = preassigned.
  // tables: a token of tables_dev (preassigned searches only; 0 = build T3 here)
  void search_dev(int64_t n, const float* x, int k, float* D, int64_t* I, const int64_t* Iq, const float* Dq,
                  bool preassigned, hipStream_t s, uint64_t tables = 0) {
    check_search(n, k);
    upload_lists();
    if (n == 0) return;
    begin_slot(s);
    const int np = preassigned ? nprobe : eff_nprobe();
    const int64_t qc = query_chunk(n, np, k);
    W().w_T3.ensure(sizeof(float) * qc * M * ksub);
    if (!preassigned) {
      W().w_lists.ensure(sizeof(int64_t) * qc * np);
      W().w_dis0.ensure(sizeof(float) * qc * np);
    }
    const int G = list_scan_group(M, k);
    // tables computed ahead (tables_dev): exactly the entry of the token, which
    // this search consumes
    int pi = -1;
    if (tables) {
      require(preassigned, "precomputed tables are for preassigned searches");
      for (int i = 0; i < kPreT3; i++)
        if (pre[i].seq == tables) pi = i;
      require(pi >= 0, "tables token " + std::to_string(tables) +
                           " is not pending (already consumed, or overwritten by later precomputes)");
      require(pre[pi].n == n, "tables token was computed for " + std::to_string(pre[pi].n) + " queries, not " +
                                  std::to_string(n));
      pre[pi].seq = 0;
      pre[pi].freed_seq = ++pre_seq;
    }
    const bool use_pre = pi >= 0;
    for (int64_t q0 = 0; q0 < n; q0 += qc) {
      const int64_t c = std::min(qc, n - q0);
      const float* xq = x + q0 * d;
      const ListPlan plan = make_plan(c, np, k, s, inflight && !preassigned);
      const int64_t* lists;
      bool planned = false;
      const int tm = mark_begin(ST_COARSE, s);
      if (preassigned) {
        lists = Iq + q0 * np;
        launch_plan_count(lists, (Dq && !ip()) ? Dq + q0 * np : nullptr, xq, d_cent.as<float>(), c, d, np,
                          d_off.as<int64_t>(), list_lo, list_hi, ip(), true, k, plan, s);
      } else {
        planned =
            coarse_launch(xq, c, np, W().w_dis0.as<float>(), W().w_lists.as<int64_t>(), s, &plan, W().w_T3.as<float>(),
                          nullptr, 0, /*hoist: the scan is not k_scan_lean*/ !(k <= 16 && M <= 16));
        lists = W().w_lists.as<int64_t>();
        if (!planned)
          launch_plan_count(lists, ip() ? nullptr : W().w_dis0.as<float>(), xq, d_cent.as<float>(), c, d, np,
                            d_off.as<int64_t>(), list_lo, list_hi, ip(), false, k, plan, s);
      }
      mark_end(tm, s);
      const float* T3 = W().w_T3.as<float>();
      if (preassigned && use_pre) {  // T3 computed ahead on another stream
        if (pre[pi].ready_stream != s) HIPCHECK(hipStreamWaitEvent(s, pre[pi].ready, 0));
        T3 = pre[pi].buf.as<float>() + q0 * M * ksub;
      } else if (preassigned) {  // T3 (the coarse launch builds it otherwise)
        const int tt = mark_begin(ST_TABLES, s);
        launch_ip_table(xq, c, d, d_cb.as<float>(), M, ksub, W().w_T3.as<float>(), s);
        mark_end(tt, s);
      }
      ScanArgs a;
      a.T1 = d_T1.as<float>();
      a.T3 = T3;
      a.codes = d_codes.as<uint8_t>();
      a.ids = d_ids.as<int64_t>();
      a.list_off = d_off.as<int64_t>();
      a.n_codes = img_n;
      a.probe_list = lists;
      a.nq = c;
      a.nprobe = np;
      a.k = k;
      a.M = M;
      a.ip = ip() ? 1 : 0;
      a.list_lo = list_lo;
      a.list_hi = list_hi;
      a.outD = D + q0 * k;
      a.outI = I + q0 * k;
      const int ts = mark_begin(ST_SCAN, s);
      launch_plan_items(plan, d_off.as<int64_t>(), list_lo, list_hi, G, s);
      // ST_LISTS: its two events are recorded around the list-scan kernel alone
      const int tl = mark_begin(ST_LISTS, s, false);
      launch_scan_lists(a, plan, s, tl >= 0 ? &marks[tl].a : nullptr);
      mark_end(ts, s);
      HIPCHECK(hipGetLastError());
    }
    if (use_pre) {  // the entry's buffer may be rewritten once these scans are done
      HIPCHECK(hipEventRecord(pre[pi].freed, s));
      pre[pi].freed_stream = s;
      pre[pi].freed_pending = true;
    }
    mark_done(s);
  }

  // The query chunk of a search: [c][nlist] keys, T3 and buckets within
  // kChunkBytes; the per-wave partial lists ([c][np][4][k] 16-B records, 64 B per
  // entry and query) within kPartialBytes, so large k still runs whole
  // 1024-query batches (C3, k = 1000, nprobe 32: 2 MB per query).
  int64_t query_chunk(int64_t n, int np, int k) const {
    const int nloc = std::max(list_hi - list_lo, 1);
    const size_t per_q = std::max({(size_t)nlist * 4, (size_t)M * ksub * 4, (size_t)nloc * 16});
    return std::max<int64_t>(
        1, std::min<int64_t>({n, (int64_t)(kChunkBytes / per_q), (int64_t)(kPartialBytes / ((size_t)np * part_stride(k) * 64))}));
  }

  // T3 [n][M][ksub] of the queries x, on stream s, ahead of a preassigned search
  // of exactly those queries (the shard flow computes it while the probes are
  // all-gathered), into one of kPreT3 buffers so that batches in flight each have
  // their own.  Returns the token the search takes (ivfpq.h).
  uint64_t tables_dev(int64_t n, const float* x, hipStream_t s) {
    PreT3& p = take_pre(n, s);
    launch_ip_table(x, n, d, d_cb.as<float>(), M, ksub, p.buf.as<float>(), s);
    HIPCHECK(hipGetLastError());
    return publish_pre(p, n, s);
  }
  // A table entry for n queries, ordered on s after its last consumer and producer.
  PreT3& take_pre(int64_t n, hipStream_t s) {
    require(trained, "index is not trained");
    require(n >= 1, "precompute_tables needs at least one query");
    const int64_t cap = (int64_t)(kChunkBytes / ((size_t)M * ksub * 4));
    require(n <= cap, "precompute_tables: n = " + std::to_string(n) + " exceeds the " + std::to_string(cap) +
                          " queries one table buffer holds (split the batch)");
    // the free entry computed longest ago, else the oldest pending one (dropped);
    // ordered after its last consumer's scans and its last table launch
    int r = 0;
    for (int i = 1; i < kPreT3; i++) {
      const bool fi = pre[i].seq == 0, fr = pre[r].seq == 0;
      // a free entry first, the one consumed longest ago (its consumer's scans are the
      // likeliest to be done, so the wait below rarely stalls the side stream); else
      // the oldest pending entry
      if ((fi && !fr) || (fi && fr && pre[i].freed_seq < pre[r].freed_seq) ||
          (!fi && !fr && pre[i].seq < pre[r].seq))
        r = i;
    }
    PreT3& p = pre[r];
    if (p.freed_pending && p.freed_stream != s) HIPCHECK(hipStreamWaitEvent(s, p.freed, 0));
    if (p.ready_pending && p.ready_stream != s) HIPCHECK(hipStreamWaitEvent(s, p.ready, 0));
    p.buf.ensure(sizeof(float) * (size_t)n * M * ksub);
    p.seq = 0;  // (being rewritten: not consumable until published)
    return p;
  }
  uint64_t publish_pre(PreT3& p, int64_t n, hipStream_t s) {
    HIPCHECK(hipEventRecord(p.ready, s));
    p.ready_stream = s;
    p.ready_pending = true;
    p.n = n;
    p.seq = ++pre_seq;
    return p.seq;
  }
  // tables computed ahead are meaningless once the codebook changes or the index is reset
  void drop_tables() {
    for (auto& p : pre) p.seq = 0;
  }

  // The list-range shard step's front half on one stream: the coarse quantizer of
  // this rank's n queries x and T3 of the nt queries xt of the global batch (the
  // key workgroups and the table workgroups of one launch at nlist < 8192), the
  // tables handed to the preassigned search of xt by the returned token.  No side
  // stream (side streams past the box's four hardware queues cost a
  // third of the throughput).
  uint64_t coarse_tables_dev(int64_t n, const float* x, int64_t* Iq, float* Dq, int64_t nt, const float* xt,
                             hipStream_t s) {
    require(trained, "index is not trained");
    require(n >= 1 && nt >= 1, "coarse_tables needs queries");
    PreT3& p = take_pre(nt, s);
    begin_slot(s);
    const int np = eff_nprobe();
    const int64_t qc = std::max<int64_t>(1, std::min<int64_t>(n, kChunkBytes / ((size_t)nlist * 4)));
    for (int64_t q0 = 0; q0 < n; q0 += qc) {
      const int64_t c = std::min(qc, n - q0);
      const bool with_t3 = q0 == 0;  // the first chunk's launch also builds every table
      coarse_launch(x + q0 * d, c, np, Dq + q0 * np, Iq + q0 * np, s, nullptr,
                    with_t3 ? p.buf.as<float>() : nullptr, with_t3 ? xt : nullptr, with_t3 ? nt : 0);
      HIPCHECK(hipGetLastError());
    }
    mark_done(s);
    return publish_pre(p, nt, s);
  }

  void coarse_dev(int64_t n, const float* x, int64_t* Iq, float* Dq, hipStream_t s) {
    require(trained, "index is not trained");
    if (n <= 0) return;
    begin_slot(s);
    const int np = eff_nprobe();
    const int64_t qc = std::max<int64_t>(1, std::min<int64_t>(n, kChunkBytes / ((size_t)nlist * 4)));
    for (int64_t q0 = 0; q0 < n; q0 += qc) {
      const int64_t c = std::min(qc, n - q0);
      coarse_launch(x + q0 * d, c, np, Dq + q0 * np, Iq + q0 * np, s);
      HIPCHECK(hipGetLastError());
    }
    mark_done(s);
  }

  // host-buffer search (copies in/out on the handle's stream; device staging
  // buffers persist across calls)
  void search_host(int64_t n, const float* x, int k, float* D, int64_t* I, const int64_t* Iq, const float* Dq,
                   bool preassigned) {
    check_search(n, k);
    if (n == 0) return;
    order_after_all(stream);
    const int np = nprobe;
    w_x.ensure(sizeof(float) * n * d);
    h_D.ensure(sizeof(float) * n * k);
    h_I.ensure(sizeof(int64_t) * n * k);
    HIPCHECK(hipMemcpyAsync(w_x.p, x, sizeof(float) * n * d, hipMemcpyHostToDevice, stream));
    if (preassigned) {
      h_Iq.ensure(sizeof(int64_t) * n * np);
      HIPCHECK(hipMemcpyAsync(h_Iq.p, Iq, sizeof(int64_t) * n * np, hipMemcpyHostToDevice, stream));
      if (Dq) {
        h_Dq.ensure(sizeof(float) * n * np);
        HIPCHECK(hipMemcpyAsync(h_Dq.p, Dq, sizeof(float) * n * np, hipMemcpyHostToDevice, stream));
      }
    }
    search_dev(n, w_x.as<float>(), k, h_D.as<float>(), h_I.as<int64_t>(), h_Iq.as<int64_t>(),
               Dq ? h_Dq.as<float>() : nullptr, preassigned, stream);
    HIPCHECK(hipMemcpyAsync(D, h_D.p, sizeof(float) * n * k, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipMemcpyAsync(I, h_I.p, sizeof(int64_t) * n * k, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }

  // One FaissServer request in the ralm wire format
  // (ralm/retriever/serialization_utils.py): header integers big-endian
  // (BYTE_ORDER_PY = 'big', :5), arrays in native order (tobytes, :59, :86-87).
  //   with_lists 0: k | queries f32[B][dim]                      (encode_request :38-67)
  //   with_lists 1: B, dim, nprobe, k | queries | lists i64[B][np] (encode_request_with_lists :69-94)
  // The answer is I i64[B][k] | D f32[B][k] (encode_answer :223-258), copied from
  // HBM straight into the answer buffer.  Shape checks follow decode_request*
  // (asserts at :211-213) and FaissServer.start (faiss_server.py:241-277).
  void serve(const uint8_t* msg, int64_t len, int with_lists, int B, int dim, int np, uint8_t* ans, int64_t cap,
             int64_t* ans_len) {
    auto be32 = [](const uint8_t* p) {
      return (int64_t)(int32_t)(((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]);
    };
    require(B > 0 && dim == d, "server shape: batch_size must be > 0 and dim must equal the index's d");
    const int64_t qbytes = (int64_t)B * dim * 4;
    int64_t k;
    const uint8_t* qp;
    const uint8_t* lp = nullptr;
    if (with_lists) {
      require(np >= 1, "nprobe must be >= 1");
      require(len == 16 + qbytes + (int64_t)B * np * 8,
              "request length " + std::to_string(len) + " != request_message_length_with_lists(" +
                  std::to_string(B) + ", " + std::to_string(dim) + ", " + std::to_string(np) + ")");
      require(be32(msg) == B && be32(msg + 4) == dim && be32(msg + 8) == np,
              "request header (batch_size, dim, nprobe) does not match the server's shape");
      k = be32(msg + 12);
      qp = msg + 16;
      lp = msg + 16 + qbytes;
    } else {
      require(len == 4 + qbytes, "request length " + std::to_string(len) + " != request_message_length(" +
                                     std::to_string(B) + ", " + std::to_string(dim) + ")");
      k = be32(msg);
      qp = msg + 4;
    }
    require(k >= 1 && k <= kMaxK, "k in the request must be in [1, " + std::to_string(kMaxK) + "]");
    const int64_t need = (int64_t)B * k * 12;
    require(ans != nullptr && cap >= need, "answer buffer holds " + std::to_string(cap) + " bytes, the answer needs " +
                                               std::to_string(need));
    check_search(B, (int)k);
    order_after_all(stream);
    w_x.ensure(qbytes);
    h_D.ensure(sizeof(float) * B * k);
    h_I.ensure(sizeof(int64_t) * B * k);
    HIPCHECK(hipMemcpyAsync(w_x.p, qp, qbytes, hipMemcpyHostToDevice, stream));
    if (with_lists) {
      // the list ids sit at an arbitrary byte offset of the message: validate on the host, copy as bytes
      for (int64_t i = 0; i < (int64_t)B * np; i++) {
        int64_t l;
        std::memcpy(&l, lp + 8 * i, 8);
        require(l < nlist, "list id out of range in the request");
      }
      const int saved = nprobe;
      nprobe = np;  // search_preassigned scans list_nos.shape[1] probes
      h_Iq.ensure(sizeof(int64_t) * B * np);
      HIPCHECK(hipMemcpyAsync(h_Iq.p, lp, sizeof(int64_t) * B * np, hipMemcpyHostToDevice, stream));
      try {
        search_dev(B, w_x.as<float>(), (int)k, h_D.as<float>(), h_I.as<int64_t>(), h_Iq.as<int64_t>(), nullptr, true,
                   stream);
      } catch (...) {
        nprobe = saved;
        throw;
      }
      nprobe = saved;
    } else {
      search_dev(B, w_x.as<float>(), (int)k, h_D.as<float>(), h_I.as<int64_t>(), nullptr, nullptr, false, stream);
    }
    HIPCHECK(hipMemcpyAsync(ans, h_I.p, sizeof(int64_t) * B * k, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipMemcpyAsync(ans + (int64_t)B * k * 8, h_D.p, sizeof(float) * B * k, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    if (ans_len) *ans_len = need;
  }
};

// ====================================================================== C-ABI
namespace {

template <class F>
int guarded(F&& f) {
  try {
    g_err.clear();
    f();
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
  } catch (...) {
    g_err = "unknown error";
  }
  return -1;
}

void check_handle(const ivfpq_index* h) { require(h != nullptr, "null index handle"); }

std::atomic<int64_t> g_pca_chunk_rows{0};  // > 0: the scatter's row chunk (ivfpq_pca_set_chunk_rows)

// the plan of ivfpq_pca_moments_device, or the reason the shape cannot run
PcaPlan checked_pca_plan(int64_t n, int d) {
  require(n >= 1, "PCA moments need at least one row (n = " + std::to_string(n) + ")");
  require(d >= 1 && d <= (1 << 16), "d must be in [1, 65536]");
  const PcaPlan p = pca_plan(n, d, g_pca_chunk_rows.load());
  require(p.chunks <= kPcaMaxChunks && (int64_t)p.chunks * p.tiles < (int64_t)INT32_MAX / 16,
          "too many row chunks for one launch: raise the chunk length");
  return p;
}

}  // namespace

extern "C" {

const char* ivfpq_last_error(void) { return g_err.c_str(); }

int ivfpq_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int ivfpq_create(int d, int nlist, int M, int nbits, int metric, int device, ivfpq_index** out) {
  return guarded([&] {
    require(out != nullptr, "null output pointer");
    require(d > 0 && nlist > 0 && M > 0, "d, nlist and M must be positive");
    require(d % M == 0, "d must be a multiple of M");
    require(nbits == 8, "only nbits=8 is supported");
    require(scan_supported_M(M), "M=" + std::to_string(M) + " not supported on the GPU (8, 16, 32, 48, 64)");
    require(d <= 2048, "d > 2048 not supported");
    require(metric == IVFPQ_METRIC_L2 || metric == IVFPQ_METRIC_INNER_PRODUCT, "unknown metric");
    int ndev = 0;
    HIPCHECK(hipGetDeviceCount(&ndev));
    require(device >= 0 && device < ndev, "device ordinal out of range");
    DeviceGuard g(device);
    auto h = std::make_unique<ivfpq_index>();
    h->d = d;
    h->nlist = nlist;
    h->M = M;
    h->nbits = nbits;
    h->ksub = 1 << nbits;
    h->metric = metric;
    h->device = device;
    h->list_lo = 0;
    h->list_hi = nlist;
    h->lcodes.resize(nlist);
    h->lids.resize(nlist);
    h->init_stream();
    *out = h.release();
  });
}

int ivfpq_free(ivfpq_index* h) {
  return guarded([&] {
    if (!h) return;
    DeviceGuard g(h->device);
    (void)hipStreamSynchronize(h->stream);
    h->quiesce();
    delete h;
  });
}

int ivfpq_train(ivfpq_index* h, int64_t n, const float* x, int niter_coarse, int niter_pq, uint64_t seed) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(x != nullptr && n > 0, "empty training set");
    h->quiesce();  // the k-means scratch buffers are shared with the search path
    const int d = h->d, M = h->M, dsub = d / M, ksub = h->ksub, nlist = h->nlist;
    std::vector<float> cent((size_t)nlist * d);
    h->kmeans(x, n, d, nlist, niter_coarse, seed, cent.data(), h->ip());
    // residuals to the final coarse centroids
    h->w_cent.ensure(sizeof(float) * nlist * d);
    h->w_cn.ensure(sizeof(float) * nlist);
    HIPCHECK(hipMemcpyAsync(h->w_cent.p, cent.data(), sizeof(float) * nlist * d, hipMemcpyHostToDevice, h->stream));
    launch_row_norms(h->w_cent.as<float>(), nlist, d, h->w_cn.as<float>(), h->stream);
    std::vector<int64_t> assign(n);
    h->assign_top1(x, n, d, h->w_cent.as<float>(), h->w_cn.as<float>(), nlist, assign.data(), nullptr, h->ip());
    std::vector<float> sub((size_t)n * dsub);
    std::vector<float> cb((size_t)M * ksub * dsub);
    for (int m = 0; m < M; m++) {
      for (int64_t i = 0; i < n; i++) {
        const float* xi = x + i * d + m * dsub;
        const float* ci = cent.data() + assign[i] * d + m * dsub;
        for (int t = 0; t < dsub; t++) sub[(size_t)i * dsub + t] = xi[t] - ci[t];
      }
      h->kmeans(sub.data(), n, dsub, ksub, niter_pq, seed + 1 + (uint64_t)m, cb.data() + (size_t)m * ksub * dsub);
    }
    h->centroids = std::move(cent);
    h->codebook = std::move(cb);
    h->upload_trained();
  });
}

int ivfpq_set_trained(ivfpq_index* h, const float* centroids, const float* codebook) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(centroids && codebook, "null centroids/codebook");
    h->centroids.assign(centroids, centroids + (size_t)h->nlist * h->d);
    h->codebook.assign(codebook, codebook + (size_t)h->M * h->ksub * (h->d / h->M));
    h->upload_trained();
  });
}

int ivfpq_add(ivfpq_index* h, int64_t n, const float* x, const int64_t* ids) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(h->trained, "index is not trained");
    if (n <= 0) return;
    require(x != nullptr, "null x");
    h->add_dev(n, x, false, ids, false, h->stream);
  });
}

int ivfpq_add_device(ivfpq_index* h, int64_t n, const float* x, const int64_t* ids, void* stream) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(h->trained, "index is not trained");
    if (n <= 0) return;
    require(x != nullptr, "null x");
    h->add_dev(n, x, true, ids, true, stream ? (hipStream_t)stream : h->stream);
  });
}

int ivfpq_add_preencoded(ivfpq_index* h, int64_t n, const int64_t* list_no, const uint8_t* codes,
                         const int64_t* ids) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    if (n <= 0) return;
    require(list_no && codes, "null list_no/codes");
    std::vector<int64_t> seq;
    if (!ids) {
      seq.resize(n);
      for (int64_t i = 0; i < n; i++) seq[i] = h->next_id + i;
      ids = seq.data();
      h->next_id += n;
    }
    h->append(n, list_no, codes, ids);
  });
}

int ivfpq_reset(ivfpq_index* h) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    for (auto& v : h->lcodes) v.clear();
    for (auto& v : h->lids) v.clear();
    DeviceGuard g(h->device);
    h->quiesce();
    h->drop_tables();
    h->drop_pending();
    h->host_stale = false;
    h->ntotal = 0;
    h->next_id = 0;
    h->dirty = true;
  });
}

int ivfpq_set_nprobe(ivfpq_index* h, int nprobe) {
  return guarded([&] {
    check_handle(h);
    require(nprobe >= 1 && nprobe <= kMaxK, "nprobe must be in [1, " + std::to_string(kMaxK) + "]");
    h->nprobe = nprobe;
  });
}

int ivfpq_get_nprobe(const ivfpq_index* h) { return h ? h->nprobe : -1; }

int ivfpq_set_list_range(ivfpq_index* h, int lo, int hi) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    require(0 <= lo && lo <= hi && hi <= h->nlist, "invalid list range");
    require(h->ntotal == 0 && h->q_n == 0, "set the list range before adding vectors");
    h->list_lo = lo;
    h->list_hi = hi;
    h->dirty = true;  // the device image (list order) follows the range
  });
}

int ivfpq_search(ivfpq_index* h, int64_t n, const float* x, int k, float* D, int64_t* I) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(n == 0 || (x && D && I), "null buffer");
    h->search_host(n, x, k, D, I, nullptr, nullptr, false);
  });
}

int ivfpq_search_preassigned(ivfpq_index* h, int64_t n, const float* x, int k, const int64_t* Iq, const float* Dq,
                             float* D, int64_t* I) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(n == 0 || (x && Iq && D && I), "null buffer");
    for (int64_t i = 0; i < n * h->nprobe; i++)
      require(Iq[i] < h->nlist, "list id out of range in Iq");
    h->search_host(n, x, k, D, I, Iq, Dq, true);
  });
}

int ivfpq_search_device(ivfpq_index* h, int64_t n, const float* x, int k, float* D, int64_t* I, void* stream) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->search_dev(n, x, k, D, I, nullptr, nullptr, false, (hipStream_t)stream);
  });
}

int ivfpq_search_preassigned_device(ivfpq_index* h, int64_t n, const float* x, int k, const int64_t* Iq,
                                    const float* Dq, float* D, int64_t* I, void* stream) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->search_dev(n, x, k, D, I, Iq, Dq, true, (hipStream_t)stream);
  });
}

int ivfpq_serve_request(ivfpq_index* h, const uint8_t* msg, int64_t msg_len, int with_lists, int batch_size, int dim,
                        int nprobe, uint8_t* answer, int64_t answer_cap, int64_t* answer_len) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(msg != nullptr, "null request message");
    h->serve(msg, msg_len, with_lists, batch_size, dim, nprobe, answer, answer_cap, answer_len);
  });
}

int ivfpq_precompute_tables_device(ivfpq_index* h, int64_t n, const float* x, void* stream, uint64_t* token) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(x != nullptr && token != nullptr, "null x or token");
    *token = h->tables_dev(n, x, stream ? (hipStream_t)stream : h->stream);
  });
}

int ivfpq_search_preassigned_tables_device(ivfpq_index* h, int64_t n, const float* x, int k, const int64_t* Iq,
                                           const float* Dq, float* D, int64_t* I, uint64_t token, void* stream) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(token != 0, "tables token 0 (use ivfpq_search_preassigned_device without tables)");
    h->search_dev(n, x, k, D, I, Iq, Dq, true, (hipStream_t)stream, token);
  });
}

int ivfpq_set_inflight(ivfpq_index* h, int on) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(on == 0 || on == 1, "inflight must be 0 or 1");
    h->quiesce();  // searches issued under the previous setting complete first
    h->inflight = on == 1;
  });
}

int ivfpq_get_inflight(const ivfpq_index* h) { return h ? (h->inflight ? 1 : 0) : -1; }

int ivfpq_overlap_built(void) { return 1; }

int ivfpq_get_error_count(ivfpq_index* h, int64_t* out) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(out != nullptr, "null output");
    h->quiesce();
    int64_t tot = 0;
    for (auto& w : h->work) {
      if (!w.p_hdr.p) continue;
      int32_t hdr[16];
      HIPCHECK(hipMemcpy(hdr, w.p_hdr.p, sizeof(hdr), hipMemcpyDeviceToHost));
      tot += hdr[15];
    }
    *out = tot;
  });
}

int ivfpq_get_repair_stats(ivfpq_index* h, int64_t* stale_reads, int64_t* repairs) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(stale_reads != nullptr && repairs != nullptr, "null output");
    h->quiesce();
    int64_t st = 0, rp = 0;
    for (auto& w : h->work) {
      if (!w.p_hdr.p) continue;
      int32_t hdr[16];
      HIPCHECK(hipMemcpy(hdr, w.p_hdr.p, sizeof(hdr), hipMemcpyDeviceToHost));
      st += hdr[kHdrStale];
      rp += hdr[kHdrRepair];
    }
    *stale_reads = st;
    *repairs = rp;
  });
}

int ivfpq_get_repair_log(ivfpq_index* h, uint32_t* out, int max_events, int* n_events) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(n_events != nullptr && (out != nullptr || max_events == 0) && max_events >= 0, "bad output arguments");
    h->quiesce();
    int got = 0;
    for (auto& w : h->work) {
      if (!w.p_hdr.p || !w.p_evlog.p) continue;
      int32_t hdr[16];
      HIPCHECK(hipMemcpy(hdr, w.p_hdr.p, sizeof(hdr), hipMemcpyDeviceToHost));
      const int kept = std::min(hdr[kHdrLog], kEvLog);
      std::vector<uint32_t> ev((size_t)8 * kEvLog);
      HIPCHECK(hipMemcpy(ev.data(), w.p_evlog.p, ev.size() * 4, hipMemcpyDeviceToHost));
      for (int e = 0; e < kept && got < max_events; e++, got++) std::memcpy(out + 8 * got, &ev[8 * e], 32);
    }
    *n_events = got;
  });
}

int ivfpq_debug_workspace(ivfpq_index* h, int ws, int what, void* dst, int64_t cap, int64_t* bytes) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(ws >= 0 && ws < ivfpq_index::kSlots && bytes != nullptr, "bad workspace index");
    h->quiesce();
    auto& w = h->work[ws];
    if (what >= 7) {  // host words: 7 the epoch of the last batch planned there, 8 the stream it ran on
      const uint64_t v = what == 7 ? (uint64_t)w.epoch : (uint64_t)(uintptr_t)w.done_stream;
      *bytes = 8;
      if (dst && cap >= 8) std::memcpy(dst, &v, 8);
      return;
    }
    const DevBuf* b = what == 0 ? &w.p_part : what == 1 ? &w.p_N : what == 2 ? &w.p_qmask : what == 3 ? &w.p_tau
                    : what == 4 ? &w.p_hdr : what == 5 ? &w.w_lists : &w.w_dis0;
    *bytes = (int64_t)b->bytes;
    if (dst && b->p) HIPCHECK(hipMemcpy(dst, b->p, std::min<size_t>(b->bytes, (size_t)cap), hipMemcpyDeviceToHost));
  });
}

int ivfpq_set_fault_injection(ivfpq_index* h, int every) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    require(every >= 0, "fault injection period must be >= 0");
    h->fault_inj = every;
  });
}

int ivfpq_debug_seed_tau(ivfpq_index* h, int64_t n, const float* keys) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    require(n >= 0 && (n == 0 || keys), "null buffer");
    h->tau_seed.resize(n);
    for (int64_t i = 0; i < n; i++) {  // the ordered-int word of the key (ivfpq_kernels.hip tau_lower)
      int32_t b;
      std::memcpy(&b, keys + i, 4);
      const int32_t o = b >= 0 ? b : b ^ 0x7FFFFFFF;
      h->tau_seed[i] = (uint32_t)o ^ 0x80000000u;
    }
  });
}

int ivfpq_coarse_tables_device(ivfpq_index* h, int64_t n, const float* x, int64_t* Iq, float* Dq, int64_t n_tables,
                               const float* x_tables, void* stream, uint64_t* token) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(x != nullptr && Iq != nullptr && Dq != nullptr && x_tables != nullptr && token != nullptr,
            "null pointer argument");
    *token = h->coarse_tables_dev(n, x, Iq, Dq, n_tables, x_tables, stream ? (hipStream_t)stream : h->stream);
  });
}

int ivfpq_coarse_device(ivfpq_index* h, int64_t n, const float* x, int64_t* Iq, float* Dq, void* stream) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->coarse_dev(n, x, Iq, Dq, (hipStream_t)stream);
  });
}

int ivfpq_merge_topk_device(int S, int64_t n, int k, int metric, const float* Din, const int64_t* Iin, float* Dout,
                            int64_t* Iout, void* stream) {
  return guarded([&] {
    require(S >= 1 && k >= 1 && n >= 0, "invalid merge shape");
    require(metric == IVFPQ_METRIC_L2 || metric == IVFPQ_METRIC_INNER_PRODUCT, "unknown metric");
    launch_merge_topk(S, n, k, Din, Iin, Dout, Iout, (hipStream_t)stream, metric == IVFPQ_METRIC_INNER_PRODUCT);
    HIPCHECK(hipGetLastError());
  });
}

int ivfpq_linear_transform_device(int64_t n, int d_in, int d_out, const float* AT, const float* b, const float* x,
                                  float* y, void* stream) {
  return guarded([&] {
    require(n >= 0 && d_in >= 1 && d_out >= 1, "invalid transform shape");
    require(n == 0 || (AT && x && y), "null buffer");
    launch_linear_transform(x, n, d_in, AT, b, d_out, y, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

int ivfpq_set_timing(ivfpq_index* h, int on) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    require(on >= 0 && on <= 2, "timing mode must be 0, 1 or 2");
    h->timing = on;
  });
}

int ivfpq_get_timing(ivfpq_index* h, double* ms, int64_t* count) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(ms && count, "null output");
    h->collect_timing(ms, count);
  });
}

int64_t ivfpq_ntotal(const ivfpq_index* h) { return h ? h->ntotal : -1; }

int ivfpq_is_trained(const ivfpq_index* h) { return h && h->trained ? 1 : 0; }

int ivfpq_get_dims(const ivfpq_index* h, int* d, int* nlist, int* M, int* nbits, int* metric) {
  return guarded([&] {
    check_handle(h);
    if (d) *d = h->d;
    if (nlist) *nlist = h->nlist;
    if (M) *M = h->M;
    if (nbits) *nbits = h->nbits;
    if (metric) *metric = h->metric;
  });
}

int ivfpq_get_centroids(const ivfpq_index* h, float* out) {
  return guarded([&] {
    check_handle(h);
    require(h->trained, "index is not trained");
    std::memcpy(out, h->centroids.data(), sizeof(float) * h->centroids.size());
  });
}

int ivfpq_get_codebook(const ivfpq_index* h, float* out) {
  return guarded([&] {
    check_handle(h);
    require(h->trained, "index is not trained");
    std::memcpy(out, h->codebook.data(), sizeof(float) * h->codebook.size());
  });
}

int ivfpq_get_list_sizes(const ivfpq_index* ch, int64_t* out) {
  return guarded([&] {
    check_handle(ch);
    auto* h = const_cast<ivfpq_index*>(ch);  // the host lists are a cache of the device image
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    if (h->host_stale) {  // from the device image's offsets (no download of the lists)
      h->flush_pending(h->stream);
      h->quiesce();
      std::vector<int64_t> off(h->nlist + 1);
      HIPCHECK(hipMemcpy(off.data(), h->d_off.p, sizeof(int64_t) * (h->nlist + 1), hipMemcpyDeviceToHost));
      for (int l = 0; l < h->nlist; l++) out[l] = off[l + 1] - off[l];
      return;
    }
    for (int l = 0; l < h->nlist; l++) out[l] = (int64_t)h->lids[l].size();
  });
}

int ivfpq_get_list(const ivfpq_index* ch, int list, uint8_t* codes, int64_t* ids) {
  return guarded([&] {
    check_handle(ch);
    auto* h = const_cast<ivfpq_index*>(ch);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->sync_host();
    require(list >= 0 && list < h->nlist, "list id out of range");
    if (codes) std::memcpy(codes, h->lcodes[list].data(), h->lcodes[list].size());
    if (ids) std::memcpy(ids, h->lids[list].data(), sizeof(int64_t) * h->lids[list].size());
  });
}

int ivfpq_get_precomputed_table(ivfpq_index* h, float* out) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(h->trained, "index is not trained");
    HIPCHECK(hipMemcpy(out, h->d_T1.p, sizeof(float) * (size_t)h->nlist * h->M * h->ksub, hipMemcpyDeviceToHost));
  });
}

// ----------------------------------------------------------------- save/load
namespace {
constexpr char kMagic[8] = {'C', 'H', 'I', 'V', 'F', 'P', 'Q', '1'};

struct File {
  FILE* f;
  File(const char* p, const char* m) : f(std::fopen(p, m)) {
    require(f != nullptr, std::string("cannot open ") + p);
  }
  ~File() {
    if (f) std::fclose(f);
  }
  void w(const void* p, size_t n) { require(std::fwrite(p, 1, n, f) == n, "write failed"); }
  void r(void* p, size_t n) { require(std::fread(p, 1, n, f) == n, "truncated index file"); }
};
}  // namespace

int ivfpq_save(ivfpq_index* h, const char* path) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->sync_host();
    File f(path, "wb");
    f.w(kMagic, 8);
    int32_t hdr[8] = {h->d, h->nlist, h->M, h->nbits, h->metric, h->nprobe, h->trained ? 1 : 0, 0};
    f.w(hdr, sizeof(hdr));
    int64_t cnt[2] = {h->ntotal, h->next_id};
    f.w(cnt, sizeof(cnt));
    if (h->trained) {
      f.w(h->centroids.data(), sizeof(float) * h->centroids.size());
      f.w(h->codebook.data(), sizeof(float) * h->codebook.size());
    }
    for (int l = 0; l < h->nlist; l++) {
      int64_t sz = (int64_t)h->lids[l].size();
      f.w(&sz, 8);
      if (sz) {
        f.w(h->lcodes[l].data(), h->lcodes[l].size());
        f.w(h->lids[l].data(), sizeof(int64_t) * sz);
      }
    }
  });
}

int ivfpq_load(const char* path, int device, ivfpq_index** out) {
  ivfpq_index* h = nullptr;
  int rc = guarded([&] {
    File f(path, "rb");
    char magic[8];
    f.r(magic, 8);
    require(std::memcmp(magic, kMagic, 8) == 0, "not a CHIVFPQ1 index file");
    int32_t hdr[8];
    f.r(hdr, sizeof(hdr));
    int64_t cnt[2];
    f.r(cnt, sizeof(cnt));
    if (ivfpq_create(hdr[0], hdr[1], hdr[2], hdr[3], hdr[4], device, &h) != 0) throw std::runtime_error(g_err);
    h->nprobe = hdr[5];
    DeviceGuard g(device);
    if (hdr[6]) {
      h->centroids.resize((size_t)h->nlist * h->d);
      h->codebook.resize((size_t)h->M * h->ksub * (h->d / h->M));
      f.r(h->centroids.data(), sizeof(float) * h->centroids.size());
      f.r(h->codebook.data(), sizeof(float) * h->codebook.size());
      h->upload_trained();
    }
    for (int l = 0; l < h->nlist; l++) {
      int64_t sz;
      f.r(&sz, 8);
      require(sz >= 0, "corrupt list size");
      h->lcodes[l].resize((size_t)sz * h->M);
      h->lids[l].resize((size_t)sz);
      if (sz) {
        f.r(h->lcodes[l].data(), h->lcodes[l].size());
        f.r(h->lids[l].data(), sizeof(int64_t) * sz);
      }
    }
    h->ntotal = cnt[0];
    h->next_id = cnt[1];
    h->dirty = true;
    *out = h;
  });
  if (rc != 0 && h) {
    std::string e = g_err;
    ivfpq_free(h);
    g_err = e;
  }
  return rc;
}

int ivfpq_flat_search(int device, int d, int64_t nb, const float* xb, int64_t n, const float* x, int k, int metric,
                      float* D, int64_t* I) {
  return guarded([&] {
    require(d > 0 && nb >= 0 && n >= 0, "invalid shape");
    require(metric == IVFPQ_METRIC_L2 || metric == IVFPQ_METRIC_INNER_PRODUCT, "unknown metric");
    const bool ip = metric == IVFPQ_METRIC_INNER_PRODUCT;
    require(k >= 1 && k <= kMaxK, "k must be in [1, " + std::to_string(kMaxK) + "]");
    if (n == 0) return;
    DeviceGuard g(device);
    hipStream_t s;
    HIPCHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    std::unique_ptr<void, void (*)(void*)> sguard((void*)s, [](void* p) { (void)hipStreamDestroy((hipStream_t)p); });
    DevBuf dxb, dbn, dx, dxn, ddist, dD, dI;
    const int64_t nbb = std::max<int64_t>(nb, 1);
    dxb.ensure(sizeof(float) * nbb * d);
    dbn.ensure(sizeof(float) * nbb);
    if (nb) HIPCHECK(hipMemcpyAsync(dxb.p, xb, sizeof(float) * nb * d, hipMemcpyHostToDevice, s));
    launch_row_norms(dxb.as<float>(), nb, d, dbn.as<float>(), s);
    const int64_t qc = std::max<int64_t>(1, std::min<int64_t>(n, kChunkBytes / ((size_t)nbb * 4)));
    dx.ensure(sizeof(float) * qc * d);
    dxn.ensure(sizeof(float) * qc);
    ddist.ensure(sizeof(float) * qc * nbb);
    dD.ensure(sizeof(float) * qc * k);
    dI.ensure(sizeof(int64_t) * qc * k);
    for (int64_t q0 = 0; q0 < n; q0 += qc) {
      const int64_t c = std::min(qc, n - q0);
      HIPCHECK(hipMemcpyAsync(dx.p, x + q0 * d, sizeof(float) * c * d, hipMemcpyHostToDevice, s));
      launch_row_norms(dx.as<float>(), c, d, dxn.as<float>(), s);
      launch_l2_dist(dx.as<float>(), dxn.as<float>(), c, dxb.as<float>(), dbn.as<float>(), (int)nb, d,
                     ddist.as<float>(), s, ip);
      launch_select_rows(ddist.as<float>(), c, (int)nb, k, dD.as<float>(), dI.as<int64_t>(), s, ip);
      HIPCHECK(hipGetLastError());
      HIPCHECK(hipMemcpyAsync(D + q0 * k, dD.p, sizeof(float) * c * k, hipMemcpyDeviceToHost, s));
      HIPCHECK(hipMemcpyAsync(I + q0 * k, dI.p, sizeof(int64_t) * c * k, hipMemcpyDeviceToHost, s));
      HIPCHECK(hipStreamSynchronize(s));
    }
  });
}

}  // extern "C"

// ================================================================ the flat indexes' code store
// What IndexPQ, IndexScalarQuantizer and IndexBinaryFlat share: one device image of
// fixed-size code rows [ntotal][row_bytes] that grows geometrically (with `slack` bytes
// behind it where the scan reads past a row), the label of a code being its position;
// the handle's own stream; and the ordering of device calls on different streams one
// after the other (one workspace per handle).
namespace {

struct CodeStore {
  const char* const name;  // the Faiss index, for messages
  int device = 0;
  int64_t ntotal = 0, cap = 0;      // codes in the image, rows allocated
  size_t row_bytes = 0, slack = 0;  // bytes per image row, bytes allocated behind the last row
  DevBuf d_codes;
  DevBuf w_x;  // staging of host rows
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;  // recorded after every device call, on done_stream
  hipStream_t done_stream = nullptr;
  bool done_pending = false;
  std::mutex mu;

  explicit CodeStore(const char* index_name) : name(index_name) {}
  ~CodeStore() {
    if (done) (void)hipEventDestroy(done);
    if (stream) (void)hipStreamDestroy(stream);
  }

  void order_after(hipStream_t s) {
    if (done_pending && done_stream != s) HIPCHECK(hipStreamWaitEvent(s, done, 0));
  }
  void mark_done(hipStream_t s) {
    HIPCHECK(hipEventRecord(done, s));
    done_stream = s;
    done_pending = true;
  }
  void quiesce() {
    if (done_pending) HIPCHECK(hipEventSynchronize(done));
    done_pending = false;
  }

  uint8_t* row(int64_t i) const { return d_codes.as<uint8_t>() + (size_t)i * row_bytes; }

  // room for n more codes: the image doubles (at least) when it is full
  void reserve(int64_t n, hipStream_t s) {
    require(ntotal + n < (int64_t)INT32_MAX, std::string(name) + " holds at most 2^31 - 2 codes");
    if (ntotal + n <= cap) return;
    quiesce();
    const int64_t ncap = std::max<int64_t>({ntotal + n, 2 * cap, 1024});
    const size_t nbytes = (size_t)ncap * row_bytes + slack;
    void* np = nullptr;
    HIPCHECK(hipMalloc(&np, nbytes));
    if (ntotal) {
      hipError_t e = hipMemcpyAsync(np, d_codes.p, (size_t)ntotal * row_bytes, hipMemcpyDeviceToDevice, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess) {
        (void)hipFree(np);
        HIPCHECK(e);
      }
    }
    d_codes.release();
    d_codes.p = np;
    d_codes.bytes = nbytes;
    cap = ncap;
  }

  // n host rows [n][row_bytes] behind the image; returns when they are in place
  void append_rows(int64_t n, const uint8_t* codes) {
    reserve(n, stream);
    quiesce();
    HIPCHECK(hipMemcpyAsync(row(ntotal), codes, (size_t)n * row_bytes, hipMemcpyHostToDevice, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    ntotal += n;
  }

  // the first out_bytes (<= row_bytes) of the rows [i0, i0 + n) to the host
  void read_rows(int64_t i0, int64_t n, uint8_t* out, size_t out_bytes) {
    quiesce();
    if (out_bytes == row_bytes)
      HIPCHECK(hipMemcpyAsync(out, row(i0), (size_t)n * row_bytes, hipMemcpyDeviceToHost, stream));
    else
      HIPCHECK(hipMemcpy2DAsync(out, out_bytes, row(i0), row_bytes, out_bytes, n, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }

  void reset() {
    quiesce();
    d_codes.release();
    ntotal = cap = 0;
  }

  // rows per chunk of n host rows of in_bytes each that pass through a staging buffer
  static int64_t host_rows(int64_t n, size_t in_bytes) {
    return std::max<int64_t>(1, std::min<int64_t>(n, kChunkBytes / in_bytes));
  }

  // n host rows of in_bytes each, staged chunk by chunk in w_x; add(c) puts the c staged
  // rows behind the image on the handle's stream and returns when they are in place
  template <class F>
  void add_host(int64_t n, const void* x, size_t in_bytes, F add) {
    const int64_t rows = host_rows(n, in_bytes);
    quiesce();
    w_x.ensure((size_t)rows * in_bytes);
    for (int64_t r0 = 0; r0 < n; r0 += rows) {
      const int64_t c = std::min(rows, n - r0);
      HIPCHECK(hipMemcpyAsync(w_x.p, (const uint8_t*)x + (size_t)r0 * in_bytes, (size_t)c * in_bytes,
                              hipMemcpyHostToDevice, stream));
      add(c);
    }
  }
};

// the end of every *_create: the device checked, the handle's stream and event made on it
template <class H>
void open_store(std::unique_ptr<H> h, int device, H** out) {
  int ndev = 0;
  HIPCHECK(hipGetDeviceCount(&ndev));
  require(device >= 0 && device < ndev, "device ordinal out of range");
  DeviceGuard g(device);
  h->device = device;
  HIPCHECK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  HIPCHECK(hipEventCreateWithFlags(&h->done, hipEventDisableTiming));
  *out = h.release();
}

// every *_free
template <class H>
int free_store(H* h) {
  return guarded([&] {
    if (!h) return;
    DeviceGuard g(h->device);
    (void)hipStreamSynchronize(h->stream);
    h->quiesce();
    delete h;
  });
}

// the search arguments of the three indexes (one that needs no training passes true)
void check_search_args(bool trained, int64_t n, const void* x, int k, const void* D, const void* I) {
  require(k >= 1 && k <= kMaxK, "k must be in [1, " + std::to_string(kMaxK) + "]");
  require(trained, "index is not trained");
  require(n >= 0, "negative query count");
  require(n == 0 || (x && D && I), "null x / D / I");
}

}  // namespace

// ================================================================ flat PQ (IndexPQ)
// faiss.IndexPQ: no coarse quantizer and no inverted lists -- one product quantizer
// over the raw vectors, every code scanned for every query (pq_flat.hip).  The codes
// live in a CodeStore of M bytes per row.
namespace {

// queries per chunk of a flat-PQ search: the tables (M KiB per query) within kChunkBytes,
// the grid's y extent (shared by the handle and ivfpq_pq_debug_plan)
int64_t pq_query_chunk(int M, int64_t n) {
  return std::max<int64_t>(1, std::min<int64_t>({n, (int64_t)(kChunkBytes / ((size_t)M * 1024)), 4096}));
}

const char* pq_supported_M_text() { return " not supported on the GPU (8, 16, 32, 48, 64, 80, 96, 112, 128)"; }

}  // namespace

struct ivfpq_pq_index : CodeStore {
  int d = 0, M = 0, nbits = 8, ksub = 256, metric = IVFPQ_METRIC_L2;
  bool trained = false;
  std::vector<float> codebook;  // [M][256][d / M]
  DevBuf d_cb;
  DevBuf w_tab, w_pD, w_pI, w_D, w_I;  // tables, partial lists, results of the host entry points

  ivfpq_pq_index() : CodeStore("IndexPQ") {}
  bool ip() const { return metric == IVFPQ_METRIC_INNER_PRODUCT; }

  void upload_codebook() {
    quiesce();
    d_cb.ensure(sizeof(float) * codebook.size());
    HIPCHECK(hipMemcpyAsync(d_cb.p, codebook.data(), sizeof(float) * codebook.size(), hipMemcpyHostToDevice, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    trained = true;
  }

  // encode n device-resident vectors behind the image; returns when they are in place
  void add_dev(int64_t n, const float* xd, hipStream_t s) {
    reserve(n, s);
    order_after(s);
    launch_pq_encode_flat(xd, n, d, d_cb.as<float>(), M, row(ntotal), s);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    ntotal += n;
  }

  int64_t query_chunk(int64_t n) const { return pq_query_chunk(M, n); }

  // c device-resident queries -> D, I (device), all on s
  void search_chunk(const float* xd, int64_t c, int k, float* D, int64_t* I, hipStream_t s) {
    if (ntotal == 0) {
      launch_fill_empty(D, I, c * k, ip(), s);
      return;
    }
    w_tab.ensure(sizeof(float) * c * M * 256);
    if (ip())
      launch_ip_table(xd, c, d, d_cb.as<float>(), M, ksub, w_tab.as<float>(), s);
    else
      launch_l2_table(xd, c, d, d_cb.as<float>(), M, w_tab.as<float>(), s);
    const PqScanPlan pl = pq_scan_plan(M, k, c, ntotal);
    w_pD.ensure(sizeof(float) * pl.S * c * k);
    w_pI.ensure(sizeof(int64_t) * pl.S * c * k);
    launch_pq_scan(w_tab.as<float>(), c, d_codes.as<uint8_t>(), ntotal, M, k, ip(), pl, w_pD.as<float>(),
                   w_pI.as<int64_t>(), s);
    launch_merge_topk(pl.S, c, k, w_pD.as<float>(), w_pI.as<int64_t>(), D, I, s, ip());
    HIPCHECK(hipGetLastError());
  }

  void search_dev(int64_t n, const float* xd, int k, float* D, int64_t* I, hipStream_t s) {
    const int64_t qc = query_chunk(n);
    order_after(s);
    for (int64_t q0 = 0; q0 < n; q0 += qc) {
      const int64_t c = std::min(qc, n - q0);
      search_chunk(xd + q0 * d, c, k, D + q0 * k, I + q0 * k, s);
    }
    mark_done(s);
  }

  void search_host(int64_t n, const float* x, int k, float* D, int64_t* I) {
    const int64_t qc = query_chunk(n);
    quiesce();
    w_x.ensure(sizeof(float) * qc * d);
    w_D.ensure(sizeof(float) * qc * k);
    w_I.ensure(sizeof(int64_t) * qc * k);
    for (int64_t q0 = 0; q0 < n; q0 += qc) {
      const int64_t c = std::min(qc, n - q0);
      HIPCHECK(hipMemcpyAsync(w_x.p, x + q0 * d, sizeof(float) * c * d, hipMemcpyHostToDevice, stream));
      search_chunk(w_x.as<float>(), c, k, w_D.as<float>(), w_I.as<int64_t>(), stream);
      HIPCHECK(hipMemcpyAsync(D + q0 * k, w_D.p, sizeof(float) * c * k, hipMemcpyDeviceToHost, stream));
      HIPCHECK(hipMemcpyAsync(I + q0 * k, w_I.p, sizeof(int64_t) * c * k, hipMemcpyDeviceToHost, stream));
      HIPCHECK(hipStreamSynchronize(stream));
    }
  }
};

namespace {

void check_pq(const ivfpq_pq_index* h) { require(h != nullptr, "null index handle"); }

}  // namespace

extern "C" {

int ivfpq_pq_create(int d, int M, int nbits, int metric, int device, ivfpq_pq_index** out) {
  return guarded([&] {
    require(out != nullptr, "null output pointer");
    require(d > 0 && M > 0, "d and M must be positive");
    require(d % M == 0, "d must be a multiple of M");
    require(nbits == 8, "only nbits=8 is supported");
    require(pq_flat_supported_M(M), "M=" + std::to_string(M) + pq_supported_M_text());
    require(d <= 2048, "d > 2048 not supported");
    require(metric == IVFPQ_METRIC_L2 || metric == IVFPQ_METRIC_INNER_PRODUCT, "unknown metric");
    auto h = std::make_unique<ivfpq_pq_index>();
    h->d = d;
    h->M = M;
    h->nbits = nbits;
    h->metric = metric;
    h->row_bytes = (size_t)M;
    open_store(std::move(h), device, out);
  });
}

int ivfpq_pq_free(ivfpq_pq_index* h) { return free_store(h); }

int ivfpq_pq_train(ivfpq_pq_index* h, int64_t n, const float* x, int niter, uint64_t seed) {
  return guarded([&] {
    check_pq(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(x != nullptr && n > 0, "empty training set");
    const int d = h->d, M = h->M, dsub = d / M;
    // the IVF-PQ handle's GPU k-means (assignment on the GPU, double-precision mean on
    // the host), run from a scratch handle that holds only its stream and workspaces
    ivfpq_index km;
    km.device = h->device;
    km.init_stream();
    std::vector<float> sub((size_t)n * dsub);
    std::vector<float> cb((size_t)M * 256 * dsub);
    for (int m = 0; m < M; m++) {
      for (int64_t i = 0; i < n; i++) std::memcpy(&sub[(size_t)i * dsub], x + i * d + m * dsub, sizeof(float) * dsub);
      km.kmeans(sub.data(), n, dsub, 256, niter, seed + 1 + (uint64_t)m, cb.data() + (size_t)m * 256 * dsub);
    }
    HIPCHECK(hipStreamSynchronize(km.stream));
    h->codebook = std::move(cb);
    h->upload_codebook();
  });
}

int ivfpq_pq_set_trained(ivfpq_pq_index* h, const float* codebook) {
  return guarded([&] {
    check_pq(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(codebook != nullptr, "null codebook");
    h->codebook.assign(codebook, codebook + (size_t)h->M * 256 * (h->d / h->M));
    h->upload_codebook();
  });
}

int ivfpq_pq_add(ivfpq_pq_index* h, int64_t n, const float* x) {
  return guarded([&] {
    check_pq(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(h->trained, "index is not trained");
    if (n <= 0) return;
    require(x != nullptr, "null x");
    h->add_host(n, x, sizeof(float) * h->d, [&](int64_t c) { h->add_dev(c, h->w_x.as<float>(), h->stream); });
  });
}

int ivfpq_pq_add_device(ivfpq_pq_index* h, int64_t n, const float* x, void* stream) {
  return guarded([&] {
    check_pq(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(h->trained, "index is not trained");
    if (n <= 0) return;
    require(x != nullptr, "null x");
    h->add_dev(n, x, (hipStream_t)stream);
  });
}

int ivfpq_pq_add_codes(ivfpq_pq_index* h, int64_t n, const uint8_t* codes) {
  return guarded([&] {
    check_pq(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(h->trained, "index is not trained");
    if (n <= 0) return;
    require(codes != nullptr, "null codes");
    h->append_rows(n, codes);
  });
}

int ivfpq_pq_reset(ivfpq_pq_index* h) {
  return guarded([&] {
    check_pq(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->reset();
  });
}

int ivfpq_pq_search(ivfpq_pq_index* h, int64_t n, const float* x, int k, float* D, int64_t* I) {
  return guarded([&] {
    check_pq(h);
    check_search_args(h->trained, n, x, k, D, I);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    if (n == 0) return;
    h->search_host(n, x, k, D, I);
  });
}

int ivfpq_pq_search_device(ivfpq_pq_index* h, int64_t n, const float* x, int k, float* D, int64_t* I, void* stream) {
  return guarded([&] {
    check_pq(h);
    check_search_args(h->trained, n, x, k, D, I);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    if (n == 0) return;
    h->search_dev(n, x, k, D, I, (hipStream_t)stream);
  });
}

int64_t ivfpq_pq_ntotal(const ivfpq_pq_index* h) { return h ? h->ntotal : -1; }

int ivfpq_pq_is_trained(const ivfpq_pq_index* h) { return h && h->trained ? 1 : 0; }

int ivfpq_pq_get_dims(const ivfpq_pq_index* h, int* d, int* M, int* nbits, int* metric) {
  return guarded([&] {
    check_pq(h);
    if (d) *d = h->d;
    if (M) *M = h->M;
    if (nbits) *nbits = h->nbits;
    if (metric) *metric = h->metric;
  });
}

int ivfpq_pq_get_codebook(const ivfpq_pq_index* h, float* out) {
  return guarded([&] {
    check_pq(h);
    require(h->trained, "index is not trained");
    require(out != nullptr, "null output pointer");
    std::memcpy(out, h->codebook.data(), sizeof(float) * h->codebook.size());
  });
}

int ivfpq_pq_get_codes(ivfpq_pq_index* h, int64_t i0, int64_t n, uint8_t* out) {
  return guarded([&] {
    check_pq(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(i0 >= 0 && n >= 0 && i0 + n <= h->ntotal, "code range outside [0, ntotal)");
    if (n == 0) return;
    require(out != nullptr, "null output pointer");
    h->read_rows(i0, n, out, h->row_bytes);
  });
}

// Test hook (ivfpq_test.h): host arithmetic only, no handle and no device call.
int ivfpq_pq_debug_plan(int M, int k, int64_t nq, int64_t nb, int* G, int* ranges, int64_t* rows, int* S,
                        int64_t* query_chunk) {
  return guarded([&] {
    require(pq_flat_supported_M(M), "M=" + std::to_string(M) + pq_supported_M_text());
    require(k >= 1 && k <= kMaxK, "k must be in [1, " + std::to_string(kMaxK) + "]");
    require(nq >= 1, "query count must be positive");
    require(nb >= 1 && nb < (int64_t)INT32_MAX, "IndexPQ holds at most 2^31 - 2 codes");
    const int64_t qc = pq_query_chunk(M, nq);
    const PqScanPlan pl = pq_scan_plan(M, k, std::min(nq, qc), nb);
    if (G) *G = pl.G;
    if (ranges) *ranges = pl.ranges;
    if (rows) *rows = pl.rows;
    if (S) *S = pl.S;
    if (query_chunk) *query_chunk = qc;
  });
}

}  // extern "C"

// ============================================================ IVF-Flat (IndexIVFFlat)
// faiss.IndexIVFFlat: the IVF-PQ handle's coarse quantizer (k-means, matrix-core keys,
// top-nprobe selection) over inverted lists of the raw fp32 vectors, scanned by
// ivf_flat.hip.  The vectors live only in the device image {list_off, vectors, ids},
// every list sorted by label; adds wait in a pending set on the device and are merged
// with the image kernels of ivfpq_build.h at code size 4 d.  Device calls on different
// streams are ordered one after the other (one workspace per handle).
struct ivfpq_ivfflat_index {
  int d = 0, nlist = 0, metric = IVFPQ_METRIC_L2, device = 0;
  int nprobe = 1;
  bool trained = false;
  std::vector<float> centroids;  // [nlist][d]
  // the coarse quantizer: an IVF-PQ handle that holds only the centroids' device copies,
  // its stream and the k-means / coarse workspaces
  ivfpq_index base;
  int64_t ntotal = 0, next_id = 0;
  int64_t img_n = 0;  // vectors in the image (ntotal = img_n + q_n)
  DevBuf d_vecs, d_ids, d_off;
  std::vector<int64_t> h_off;      // the image's list offsets
  std::vector<int64_t> range_top;  // range_top[p] = row ranges of the p longest lists (the slot bound)
  DevBuf q_lists, q_ids, q_x;      // pending adds: list numbers, labels, vectors
  int64_t q_n = 0, q_cap = 0;
  DevBuf w_D, w_x, h_D, h_I, h_Iq;  // add scratch; staging of the host entry points
  DevBuf w_lists, w_dis, p_cnt, p_bucket, p_items, p_used, p_tau, p_partD, p_partI, p_tmpD, p_tmpI;
  hipStream_t stream = nullptr;  // = base.stream
  hipEvent_t done = nullptr;     // recorded after every device call, on done_stream
  hipStream_t done_stream = nullptr;
  bool done_pending = false;
  std::mutex mu;

  ~ivfpq_ivfflat_index() {
    if (done) (void)hipEventDestroy(done);
  }
  bool ip() const { return metric == IVFPQ_METRIC_INNER_PRODUCT; }
  size_t row_bytes() const { return sizeof(float) * (size_t)d; }

  void order_after(hipStream_t s) {
    if (done_pending && done_stream != s) HIPCHECK(hipStreamWaitEvent(s, done, 0));
  }
  void mark_done(hipStream_t s) {
    HIPCHECK(hipEventRecord(done, s));
    done_stream = s;
    done_pending = true;
  }
  void quiesce() {
    if (done_pending) HIPCHECK(hipEventSynchronize(done));
    done_pending = false;
  }

  // the centroids' device copies of ivfpq_index::upload_trained (no codebook, no T1)
  void upload_centroids() {
    quiesce();
    base.d_cent.ensure(sizeof(float) * nlist * d);
    base.d_cnorm.ensure(sizeof(float) * nlist);
    HIPCHECK(hipMemcpyAsync(base.d_cent.p, centroids.data(), sizeof(float) * nlist * d, hipMemcpyHostToDevice, stream));
    launch_row_norms(base.d_cent.as<float>(), nlist, d, base.d_cnorm.as<float>(), stream);
    const int ldc = (nlist + 3) & ~3;
    std::vector<float> ct((size_t)ldc * d, 0.f);
    for (int l = 0; l < nlist; l++)
      for (int t = 0; t < d; t++) ct[(size_t)t * ldc + l] = centroids[(size_t)l * d + t];
    base.d_centT.ensure(sizeof(float) * ct.size());
    HIPCHECK(hipMemcpyAsync(base.d_centT.p, ct.data(), sizeof(float) * ct.size(), hipMemcpyHostToDevice, stream));
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(stream));
    trained = true;
  }

  void set_offsets(std::vector<int64_t> off) {
    h_off = std::move(off);
    std::vector<int64_t> r(nlist);
    for (int l = 0; l < nlist; l++) r[l] = (h_off[l + 1] - h_off[l] + kIvfFlatRangeRows - 1) / kIvfFlatRangeRows;
    std::sort(r.begin(), r.end(), std::greater<int64_t>());
    range_top.assign(nlist + 1, 0);
    for (int l = 0; l < nlist; l++) range_top[l + 1] = range_top[l] + r[l];
  }

  // an empty image (create, reset)
  void clear_image() {
    quiesce();
    q_lists.release();
    q_ids.release();
    q_x.release();
    q_n = q_cap = 0;
    d_vecs.release();
    d_ids.release();
    d_off.ensure(sizeof(int64_t) * (nlist + 1));
    HIPCHECK(hipMemsetAsync(d_off.p, 0, sizeof(int64_t) * (nlist + 1), stream));
    HIPCHECK(hipStreamSynchronize(stream));
    set_offsets(std::vector<int64_t>(nlist + 1, 0));
    img_n = ntotal = next_id = 0;
  }

  void pend_reserve(int64_t need, hipStream_t s) {
    if (need <= q_cap) return;
    const int64_t cap = std::max<int64_t>(need, q_cap * 2);
    DevBuf l2, i2, x2;
    l2.ensure(sizeof(int64_t) * cap);
    i2.ensure(sizeof(int64_t) * cap);
    x2.ensure(row_bytes() * cap);
    if (q_n > 0) {
      HIPCHECK(hipMemcpyAsync(l2.p, q_lists.p, sizeof(int64_t) * q_n, hipMemcpyDeviceToDevice, s));
      HIPCHECK(hipMemcpyAsync(i2.p, q_ids.p, sizeof(int64_t) * q_n, hipMemcpyDeviceToDevice, s));
      HIPCHECK(hipMemcpyAsync(x2.p, q_x.p, row_bytes() * q_n, hipMemcpyDeviceToDevice, s));
      HIPCHECK(hipStreamSynchronize(s));
    }
    std::swap(q_lists.p, l2.p);
    std::swap(q_lists.bytes, l2.bytes);
    std::swap(q_ids.p, i2.p);
    std::swap(q_ids.bytes, i2.bytes);
    std::swap(q_x.p, x2.p);
    std::swap(q_x.bytes, x2.bytes);
    q_cap = cap;
  }

  // n vectors (host or device) into the pending set: copied behind it, then assigned
  // there by the search's coarse kernels (top-1), as ivfpq_index::add_dev assigns.
  // Merged into the image before the lists are next read, or once the pending set is
  // as large as the image (and at least kChunkBytes), so that a sequence of adds
  // moves every vector O(1) times.
  void add_dev(int64_t n, const float* x, bool x_on_device, const int64_t* ids, bool ids_on_device, hipStream_t s) {
    require(trained, "index is not trained");
    if (n <= 0) return;
    require(ntotal + n < (int64_t)INT32_MAX, "IndexIVFFlat holds fewer than 2^31 - 1 vectors");
    order_after(s);
    quiesce();
    const int64_t rows = nlist >= kSegmentedNlist ? std::min<int64_t>(n, 1 << 18)
                                                  : std::max<int64_t>(1, std::min<int64_t>(n, kChunkBytes / ((size_t)nlist * 4)));
    pend_reserve(q_n + n, s);
    float* xd = q_x.as<float>() + q_n * d;
    int64_t* lists = q_lists.as<int64_t>() + q_n;
    HIPCHECK(hipMemcpyAsync(xd, x, row_bytes() * n, x_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    w_D.ensure(sizeof(float) * rows);
    for (int64_t r0 = 0; r0 < n; r0 += rows) {
      const int64_t c = std::min(rows, n - r0);
      base.coarse_launch(xd + r0 * d, c, 1, w_D.as<float>(), lists + r0, s);
      HIPCHECK(hipGetLastError());
    }
    if (!ids) {
      launch_iota_i64(q_ids.as<int64_t>() + q_n, n, next_id, s);
      next_id += n;
    } else {
      HIPCHECK(hipMemcpyAsync(q_ids.as<int64_t>() + q_n, ids, sizeof(int64_t) * n,
                              ids_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    }
    HIPCHECK(hipStreamSynchronize(s));
    q_n += n;
    ntotal += n;
    if (q_n >= std::max<int64_t>(img_n, (int64_t)(kChunkBytes / row_bytes()))) flush_pending(s);
  }

  // The pending vectors merged into the image: sorted by (list, label) alone, then
  // interleaved list by list into the label-sorted image (ivfpq_index::flush_pending
  // with the vector's 4 d bytes as the code).
  void flush_pending(hipStream_t s) {
    if (q_n == 0) return;
    quiesce();
    ImageMergeArgs g;
    g.nlist = nlist;
    g.lo = 0;
    g.hi = nlist;
    g.M = (int)row_bytes();
    g.n_old = 0;
    g.n_new = q_n;
    g.new_lists = q_lists.as<int64_t>();
    g.new_ids = q_ids.as<int64_t>();
    g.new_codes = q_x.as<uint8_t>();
    DevBuf new_off, out_off, scratch, vecs_n, ids_n;
    new_off.ensure(sizeof(int64_t) * (nlist + 1));
    g.off_out = new_off.as<int64_t>();
    const size_t sb = image_merge_scratch_bytes(q_n, nlist);
    scratch.ensure(sb);
    HIPCHECK(image_merge_sort(g, scratch.p, sb, s));
    std::vector<int64_t> noff(nlist + 1);
    HIPCHECK(hipMemcpyAsync(noff.data(), new_off.p, sizeof(int64_t) * (nlist + 1), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    require(noff[nlist] == q_n, "pending merge: a vector was assigned to no list");
    vecs_n.ensure(std::max<size_t>(16, row_bytes() * q_n));
    ids_n.ensure(std::max<size_t>(16, sizeof(int64_t) * q_n));
    g.codes_out = vecs_n.as<uint8_t>();
    g.ids_out = ids_n.as<int64_t>();
    HIPCHECK(image_merge_gather(g, q_n, scratch.p, s));
    HIPCHECK(hipStreamSynchronize(s));
    scratch.release();
    q_x.release();  // (gathered: the pending vectors now live in vecs_n)
    std::vector<int64_t> off(nlist + 1);
    int64_t mx = 0;
    for (int l = 0; l <= nlist; l++) {
      off[l] = h_off[l] + noff[l];
      if (l < nlist) mx = std::max(mx, (h_off[l + 1] - h_off[l]) + (noff[l + 1] - noff[l]));
    }
    const int64_t n_out = off[nlist];
    DevBuf vecs2, ids2;
    vecs2.ensure(std::max<size_t>(16, row_bytes() * n_out));
    ids2.ensure(std::max<size_t>(16, sizeof(int64_t) * n_out));
    out_off.ensure(sizeof(int64_t) * (nlist + 1));
    ListMergeArgs m;
    m.nlist = nlist;
    m.lo = 0;
    m.hi = nlist;
    m.M = (int)row_bytes();
    m.max_list = mx;
    m.old_off = d_off.as<int64_t>();
    m.old_codes = d_vecs.as<uint8_t>();
    m.old_ids = d_ids.as<int64_t>();
    m.new_off = new_off.as<int64_t>();
    m.new_codes = vecs_n.as<uint8_t>();
    m.new_ids = ids_n.as<int64_t>();
    m.out_off = out_off.as<int64_t>();
    m.out_codes = vecs2.as<uint8_t>();
    m.out_ids = ids2.as<int64_t>();
    HIPCHECK(image_merge_lists(m, s));
    HIPCHECK(hipStreamSynchronize(s));
    std::swap(d_vecs.p, vecs2.p);
    std::swap(d_vecs.bytes, vecs2.bytes);
    std::swap(d_ids.p, ids2.p);
    std::swap(d_ids.bytes, ids2.bytes);
    std::swap(d_off.p, out_off.p);
    std::swap(d_off.bytes, out_off.bytes);
    img_n = n_out;
    set_offsets(std::move(off));
    q_lists.release();
    q_ids.release();
    q_n = q_cap = 0;
    require(img_n == ntotal, "pending merge: image size disagrees with ntotal");
  }

  void check_search(int64_t n, const void* x, int k, const void* D, const void* I) const {
    require(trained, "index is not trained");
    require(n >= 0, "n must be >= 0");
    require(k >= 1 && k <= kMaxK, "k must be in [1, " + std::to_string(kMaxK) + "]");
    require(n == 0 || (x && D && I), "null buffer");
  }

  // The search on device pointers, on stream s.  Iq non-null = preassigned probes
  // [n][nprobe] (the handle's nprobe, as ivfpq_search_preassigned).
  void search_dev(int64_t n, const float* x, int k, float* D, int64_t* I, const int64_t* Iq, hipStream_t s) {
    flush_pending(s);
    if (n == 0) return;
    order_after(s);
    if (img_n == 0) {
      launch_fill_empty(D, I, n * k, ip(), s);
      HIPCHECK(hipGetLastError());
      mark_done(s);
      return;
    }
    const int np = Iq ? nprobe : std::min(nprobe, nlist);
    const IvfFlatPlan pl = ivfflat_plan(k, range_top[std::min(np, nlist)]);
    // queries per chunk: the [c][nlist] coarse keys and buckets within kChunkBytes, the
    // partial lists (12 bytes per entry, and the first merge round's output) within kPartialBytes
    const size_t part_q = (size_t)pl.S * k * 12 * 2;
    const int64_t qc = std::max<int64_t>(
        1, std::min<int64_t>({n, (int64_t)(kChunkBytes / ((size_t)nlist * 8)), (int64_t)(kPartialBytes / part_q),
                              (int64_t)(INT32_MAX / 2) / ((int64_t)pl.S * k)}));
    if (!Iq) {
      w_lists.ensure(sizeof(int64_t) * qc * np);
      w_dis.ensure(sizeof(float) * qc * np);
    }
    p_cnt.ensure(sizeof(int32_t) * nlist);
    p_bucket.ensure(sizeof(int2) * (size_t)nlist * qc);
    p_items.ensure(sizeof(int32_t) * (nlist + 1));
    p_used.ensure(sizeof(int32_t) * qc);
    p_tau.ensure(sizeof(uint32_t) * qc);
    p_partD.ensure(sizeof(float) * (size_t)pl.S * qc * k);
    p_partI.ensure(sizeof(int64_t) * (size_t)pl.S * qc * k);
    const size_t tmp_lists = (size_t)std::max(1, pl.S / pl.fan);
    p_tmpD.ensure(sizeof(float) * tmp_lists * qc * k);
    p_tmpI.ensure(sizeof(int64_t) * tmp_lists * qc * k);
    for (int64_t q0 = 0; q0 < n; q0 += qc) {
      const int64_t c = std::min(qc, n - q0);
      const float* xq = x + q0 * d;
      IvfFlatArgs a;
      a.x = xq;
      a.nq = c;
      a.d = d;
      a.vecs = d_vecs.as<float>();
      a.ids = d_ids.as<int64_t>();
      a.list_off = d_off.as<int64_t>();
      a.nlist = nlist;
      if (Iq) {
        a.probes = Iq + q0 * np;
      } else {
        base.coarse_launch(xq, c, np, w_dis.as<float>(), w_lists.as<int64_t>(), s);
        a.probes = w_lists.as<int64_t>();
      }
      a.nprobe = np;
      a.dedup = Iq != nullptr;
      a.k = k;
      a.ip = ip();
      a.cnt = p_cnt.as<int32_t>();
      a.bucket = p_bucket.as<int2>();
      a.item_off = p_items.as<int32_t>();
      a.used = p_used.as<int32_t>();
      a.tau = p_tau.as<uint32_t>();
      a.partD = p_partD.as<float>();
      a.partI = p_partI.as<int64_t>();
      a.tmpD = p_tmpD.as<float>();
      a.tmpI = p_tmpI.as<int64_t>();
      a.D = D + q0 * k;
      a.I = I + q0 * k;
      launch_ivfflat_search(a, pl, s);
      HIPCHECK(hipGetLastError());
    }
    mark_done(s);
  }

  // host-buffer search (copies in and out on the handle's stream)
  void search_host(int64_t n, const float* x, int k, float* D, int64_t* I, const int64_t* Iq) {
    if (n == 0) return;
    quiesce();
    w_x.ensure(sizeof(float) * n * d);
    h_D.ensure(sizeof(float) * n * k);
    h_I.ensure(sizeof(int64_t) * n * k);
    HIPCHECK(hipMemcpyAsync(w_x.p, x, sizeof(float) * n * d, hipMemcpyHostToDevice, stream));
    if (Iq) {
      h_Iq.ensure(sizeof(int64_t) * n * nprobe);
      HIPCHECK(hipMemcpyAsync(h_Iq.p, Iq, sizeof(int64_t) * n * nprobe, hipMemcpyHostToDevice, stream));
    }
    search_dev(n, w_x.as<float>(), k, h_D.as<float>(), h_I.as<int64_t>(), Iq ? h_Iq.as<int64_t>() : nullptr, stream);
    HIPCHECK(hipMemcpyAsync(D, h_D.p, sizeof(float) * n * k, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipMemcpyAsync(I, h_I.p, sizeof(int64_t) * n * k, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }
};

namespace {
void check_ivfflat(const ivfpq_ivfflat_index* h) { require(h != nullptr, "null index handle"); }
}  // namespace

extern "C" {

int ivfpq_ivfflat_create(int d, int nlist, int metric, int device, ivfpq_ivfflat_index** out) {
  return guarded([&] {
    require(out != nullptr, "null output pointer");
    require(d >= 4 && d <= 2048 && d % 4 == 0,
            "IndexIVFFlat: d must be a multiple of 4 in [4, 2048] (d = " + std::to_string(d) + ")");
    require(nlist >= 1, "nlist must be >= 1");
    require(metric == IVFPQ_METRIC_L2 || metric == IVFPQ_METRIC_INNER_PRODUCT, "unknown metric");
    int ndev = 0;
    HIPCHECK(hipGetDeviceCount(&ndev));
    require(device >= 0 && device < ndev, "device ordinal out of range");
    DeviceGuard g(device);
    auto h = std::make_unique<ivfpq_ivfflat_index>();
    h->d = d;
    h->nlist = nlist;
    h->metric = metric;
    h->device = device;
    h->base.d = d;
    h->base.nlist = nlist;
    h->base.metric = metric;
    h->base.device = device;
    h->base.list_hi = nlist;
    h->base.init_stream();
    h->stream = h->base.stream;
    HIPCHECK(hipEventCreateWithFlags(&h->done, hipEventDisableTiming));
    h->clear_image();
    *out = h.release();
  });
}

int ivfpq_ivfflat_free(ivfpq_ivfflat_index* h) {
  return guarded([&] {
    if (!h) return;
    DeviceGuard g(h->device);
    (void)hipStreamSynchronize(h->stream);
    h->quiesce();
    delete h;
  });
}

int ivfpq_ivfflat_train(ivfpq_ivfflat_index* h, int64_t n, const float* x, int niter, uint64_t seed) {
  return guarded([&] {
    check_ivfflat(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(x != nullptr && n > 0, "empty training set");
    h->quiesce();
    std::vector<float> cent((size_t)h->nlist * h->d);
    h->base.kmeans(x, n, h->d, h->nlist, niter, seed, cent.data(), h->ip());  // ivfpq_train's coarse stage
    HIPCHECK(hipStreamSynchronize(h->stream));
    h->centroids = std::move(cent);
    h->upload_centroids();
  });
}

int ivfpq_ivfflat_set_trained(ivfpq_ivfflat_index* h, const float* centroids) {
  return guarded([&] {
    check_ivfflat(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(centroids != nullptr, "null centroids");
    h->centroids.assign(centroids, centroids + (size_t)h->nlist * h->d);
    h->upload_centroids();
  });
}

int ivfpq_ivfflat_add(ivfpq_ivfflat_index* h, int64_t n, const float* x, const int64_t* ids) {
  return guarded([&] {
    check_ivfflat(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(h->trained, "index is not trained");
    if (n <= 0) return;
    require(x != nullptr, "null x");
    h->add_dev(n, x, false, ids, false, h->stream);
  });
}

int ivfpq_ivfflat_add_device(ivfpq_ivfflat_index* h, int64_t n, const float* x, const int64_t* ids, void* stream) {
  return guarded([&] {
    check_ivfflat(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(h->trained, "index is not trained");
    if (n <= 0) return;
    require(x != nullptr, "null x");
    h->add_dev(n, x, true, ids, true, stream ? (hipStream_t)stream : h->stream);
  });
}

int ivfpq_ivfflat_reset(ivfpq_ivfflat_index* h) {
  return guarded([&] {
    check_ivfflat(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->clear_image();
  });
}

int ivfpq_ivfflat_set_nprobe(ivfpq_ivfflat_index* h, int nprobe) {
  return guarded([&] {
    check_ivfflat(h);
    require(nprobe >= 1 && nprobe <= kMaxK, "nprobe must be in [1, " + std::to_string(kMaxK) + "]");
    h->nprobe = nprobe;
  });
}

int ivfpq_ivfflat_get_nprobe(const ivfpq_ivfflat_index* h) { return h ? h->nprobe : -1; }

int ivfpq_ivfflat_search(ivfpq_ivfflat_index* h, int64_t n, const float* x, int k, float* D, int64_t* I) {
  return guarded([&] {
    check_ivfflat(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->check_search(n, x, k, D, I);
    h->search_host(n, x, k, D, I, nullptr);
  });
}

int ivfpq_ivfflat_search_preassigned(ivfpq_ivfflat_index* h, int64_t n, const float* x, int k, const int64_t* Iq,
                                     const float* Dq, float* D, int64_t* I) {
  return guarded([&] {
    check_ivfflat(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    (void)Dq;  // the scan computes whole distances (IVFFlatScanner ignores the coarse distance)
    h->check_search(n, x, k, D, I);
    require(n == 0 || Iq, "null Iq");
    for (int64_t i = 0; i < n * h->nprobe; i++) require(Iq[i] < h->nlist, "list id out of range in Iq");
    h->search_host(n, x, k, D, I, Iq);
  });
}

int ivfpq_ivfflat_search_device(ivfpq_ivfflat_index* h, int64_t n, const float* x, int k, float* D, int64_t* I,
                                void* stream) {
  return guarded([&] {
    check_ivfflat(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->check_search(n, x, k, D, I);
    h->search_dev(n, x, k, D, I, nullptr, (hipStream_t)stream);
  });
}

int ivfpq_ivfflat_search_preassigned_device(ivfpq_ivfflat_index* h, int64_t n, const float* x, int k,
                                            const int64_t* Iq, const float* Dq, float* D, int64_t* I, void* stream) {
  return guarded([&] {
    check_ivfflat(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    (void)Dq;
    h->check_search(n, x, k, D, I);
    require(n == 0 || Iq, "null Iq");
    h->search_dev(n, x, k, D, I, n ? Iq : nullptr, (hipStream_t)stream);
  });
}

int64_t ivfpq_ivfflat_ntotal(const ivfpq_ivfflat_index* h) { return h ? h->ntotal : -1; }

int ivfpq_ivfflat_is_trained(const ivfpq_ivfflat_index* h) { return h && h->trained ? 1 : 0; }

int ivfpq_ivfflat_get_dims(const ivfpq_ivfflat_index* h, int* d, int* nlist, int* metric) {
  return guarded([&] {
    check_ivfflat(h);
    if (d) *d = h->d;
    if (nlist) *nlist = h->nlist;
    if (metric) *metric = h->metric;
  });
}

int ivfpq_ivfflat_get_centroids(const ivfpq_ivfflat_index* h, float* out) {
  return guarded([&] {
    check_ivfflat(h);
    require(h->trained, "index is not trained");
    require(out != nullptr, "null output pointer");
    std::memcpy(out, h->centroids.data(), sizeof(float) * h->centroids.size());
  });
}

int ivfpq_ivfflat_get_list_sizes(ivfpq_ivfflat_index* h, int64_t* out) {
  return guarded([&] {
    check_ivfflat(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(out != nullptr, "null output pointer");
    h->flush_pending(h->stream);
    for (int l = 0; l < h->nlist; l++) out[l] = h->h_off[l + 1] - h->h_off[l];
  });
}

int ivfpq_ivfflat_get_list(ivfpq_ivfflat_index* h, int list, float* vectors, int64_t* ids) {
  return guarded([&] {
    check_ivfflat(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    require(list >= 0 && list < h->nlist, "list id out of range");
    h->flush_pending(h->stream);
    h->quiesce();
    const int64_t b = h->h_off[list], n = h->h_off[list + 1] - b;
    if (n == 0) return;
    if (vectors)
      HIPCHECK(hipMemcpyAsync(vectors, h->d_vecs.as<float>() + b * h->d, h->row_bytes() * n, hipMemcpyDeviceToHost,
                              h->stream));
    if (ids)
      HIPCHECK(hipMemcpyAsync(ids, h->d_ids.as<int64_t>() + b, sizeof(int64_t) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
  });
}

}  // extern "C"

// ============================================================ flat scalar quantizer (IndexScalarQuantizer)
// faiss.IndexScalarQuantizer: every component stored as a half or as an 8-bit code
// between the trained per-dimension (or global) minimum and maximum, every code scanned
// for every query with the decode fused in (sq_scan.hip).  The codes live in a CodeStore
// of code_size bytes per row, with the scan's read slack behind the image.
namespace {

const char* sq_qtype_name(int qtype) {
  switch (qtype) {
    case IVFPQ_SQ_8BIT: return "QT_8bit";
    case IVFPQ_SQ_4BIT: return "QT_4bit";
    case IVFPQ_SQ_8BIT_UNIFORM: return "QT_8bit_uniform";
    case IVFPQ_SQ_4BIT_UNIFORM: return "QT_4bit_uniform";
    case IVFPQ_SQ_FP16: return "QT_fp16";
    case IVFPQ_SQ_8BIT_DIRECT: return "QT_8bit_direct";
    case IVFPQ_SQ_6BIT: return "QT_6bit";
    default: return nullptr;
  }
}

}  // namespace

struct ivfpq_sq_index : CodeStore {
  int d = 0, qtype = IVFPQ_SQ_FP16, metric = IVFPQ_METRIC_L2;
  int codec = SQ_CODEC_FP16, code_size = 0;
  bool trained = false;
  std::vector<float> params;  // Faiss's sq.trained: [vmin (d), vdiff (d)], [vmin, vdiff] (uniform) or empty (fp16)
  DevBuf d_vmin, d_vdiff;
  DevBuf w_codes, w_mm, w_D, w_I, p_tau, p_partD, p_partI, p_tmpD, p_tmpI;

  ivfpq_sq_index() : CodeStore("IndexScalarQuantizer") {}
  bool ip() const { return metric == IVFPQ_METRIC_INNER_PRODUCT; }
  bool uniform() const { return qtype == IVFPQ_SQ_8BIT_UNIFORM; }
  size_t nparams() const { return codec == SQ_CODEC_FP16 ? 0 : uniform() ? 2 : 2 * (size_t)d; }
  int64_t host_rows(int64_t n) const { return CodeStore::host_rows(n, sizeof(float) * d); }

  // the 8-bit codec's device parameters: per dimension, a uniform pair repeated d times
  void upload_params() {
    quiesce();
    if (codec == SQ_CODEC_8BIT) {
      std::vector<float> mn(d), df(d);
      for (int j = 0; j < d; j++) {
        mn[j] = uniform() ? params[0] : params[j];
        df[j] = uniform() ? params[1] : params[(size_t)d + j];
      }
      d_vmin.ensure(sizeof(float) * d);
      d_vdiff.ensure(sizeof(float) * d);
      HIPCHECK(hipMemcpyAsync(d_vmin.p, mn.data(), sizeof(float) * d, hipMemcpyHostToDevice, stream));
      HIPCHECK(hipMemcpyAsync(d_vdiff.p, df.data(), sizeof(float) * d, hipMemcpyHostToDevice, stream));
      HIPCHECK(hipStreamSynchronize(stream));
    }
    trained = true;
  }

  // RS_minmax with rangestat_arg = 0 over n host vectors
  void train_host(int64_t n, const float* x) {
    if (codec == SQ_CODEC_FP16) return;
    quiesce();
    const int64_t rows = host_rows(n);
    w_x.ensure(sizeof(float) * rows * d);
    w_mm.ensure(sizeof(uint32_t) * 2 * d);
    uint32_t* lo = w_mm.as<uint32_t>();
    uint32_t* hi = lo + d;
    launch_sq_minmax_init(lo, hi, d, stream);
    for (int64_t r0 = 0; r0 < n; r0 += rows) {
      const int64_t c = std::min(rows, n - r0);
      HIPCHECK(hipMemcpyAsync(w_x.p, x + r0 * d, sizeof(float) * c * d, hipMemcpyHostToDevice, stream));
      launch_sq_minmax(w_x.as<float>(), c, d, lo, hi, stream);
      HIPCHECK(hipGetLastError());
      HIPCHECK(hipStreamSynchronize(stream));  // w_x is reused
    }
    std::vector<uint32_t> bits(2 * (size_t)d);
    HIPCHECK(hipMemcpyAsync(bits.data(), w_mm.p, sizeof(uint32_t) * 2 * d, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    std::vector<float> mn(d), mx(d);
    for (int j = 0; j < d; j++) {
      mn[j] = sq_minmax_value(bits[j]);
      mx[j] = sq_minmax_value(bits[(size_t)d + j]);
    }
    if (uniform()) {
      const float lo_all = *std::min_element(mn.begin(), mn.end());
      const float hi_all = *std::max_element(mx.begin(), mx.end());
      params = {lo_all, hi_all - lo_all};
    } else {
      params.resize(2 * (size_t)d);
      for (int j = 0; j < d; j++) {
        params[j] = mn[j];
        params[(size_t)d + j] = mx[j] - mn[j];
      }
    }
    upload_params();
  }

  // encode n device-resident vectors behind the image; returns when they are in place
  void add_dev(int64_t n, const float* xd, hipStream_t s) {
    reserve(n, s);
    order_after(s);
    launch_sq_encode(codec, xd, n, d, d_vmin.as<float>(), d_vdiff.as<float>(), row(ntotal), s);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    ntotal += n;
  }

  // sa_encode / sa_decode of host buffers, in chunks through the staging buffers
  void encode_host(int64_t n, const float* x, uint8_t* out) {
    const int64_t rows = host_rows(n);
    quiesce();
    w_x.ensure(sizeof(float) * rows * d);
    w_codes.ensure((size_t)rows * code_size);
    for (int64_t r0 = 0; r0 < n; r0 += rows) {
      const int64_t c = std::min(rows, n - r0);
      HIPCHECK(hipMemcpyAsync(w_x.p, x + r0 * d, sizeof(float) * c * d, hipMemcpyHostToDevice, stream));
      launch_sq_encode(codec, w_x.as<float>(), c, d, d_vmin.as<float>(), d_vdiff.as<float>(), w_codes.as<uint8_t>(),
                       stream);
      HIPCHECK(hipGetLastError());
      HIPCHECK(hipMemcpyAsync(out + r0 * code_size, w_codes.p, (size_t)c * code_size, hipMemcpyDeviceToHost, stream));
      HIPCHECK(hipStreamSynchronize(stream));
    }
  }
  void decode_host(int64_t n, const uint8_t* codes, float* out) {
    const int64_t rows = host_rows(n);
    quiesce();
    w_x.ensure(sizeof(float) * rows * d);
    w_codes.ensure((size_t)rows * code_size);
    for (int64_t r0 = 0; r0 < n; r0 += rows) {
      const int64_t c = std::min(rows, n - r0);
      HIPCHECK(hipMemcpyAsync(w_codes.p, codes + r0 * code_size, (size_t)c * code_size, hipMemcpyHostToDevice, stream));
      launch_sq_decode(codec, w_codes.as<uint8_t>(), c, d, d_vmin.as<float>(), d_vdiff.as<float>(), w_x.as<float>(),
                       stream);
      HIPCHECK(hipGetLastError());
      HIPCHECK(hipMemcpyAsync(out + r0 * d, w_x.p, sizeof(float) * c * d, hipMemcpyDeviceToHost, stream));
      HIPCHECK(hipStreamSynchronize(stream));
    }
  }

  // n device-resident queries -> D, I (device), all on s
  void search_dev(int64_t n, const float* xd, int k, float* D, int64_t* I, hipStream_t s) {
    if (n == 0) return;
    order_after(s);
    if (ntotal == 0) {
      launch_fill_empty(D, I, n * k, ip(), s);
      HIPCHECK(hipGetLastError());
      mark_done(s);
      return;
    }
    const IvfFlatPlan pl = ivfflat_plan(k, sq_scan_ranges(ntotal));
    // queries per chunk: the partial lists (12 bytes per entry, and the first merge round's
    // output) within kPartialBytes, their count within the merge's 32-bit indexing
    const size_t part_q = (size_t)pl.S * k * 12 * 2;
    const int64_t qc = std::max<int64_t>(
        1, std::min<int64_t>({n, (int64_t)(kPartialBytes / part_q), (int64_t)(INT32_MAX / 2) / ((int64_t)pl.S * k)}));
    p_tau.ensure(sizeof(uint32_t) * qc);
    p_partD.ensure(sizeof(float) * (size_t)pl.S * qc * k);
    p_partI.ensure(sizeof(int64_t) * (size_t)pl.S * qc * k);
    const size_t tmp_lists = (size_t)std::max(1, pl.S / pl.fan);
    p_tmpD.ensure(sizeof(float) * tmp_lists * qc * k);
    p_tmpI.ensure(sizeof(int64_t) * tmp_lists * qc * k);
    for (int64_t q0 = 0; q0 < n; q0 += qc) {
      SqScanArgs a;
      a.codec = codec;
      a.x = xd + q0 * d;
      a.nq = std::min(qc, n - q0);
      a.d = d;
      a.codes = d_codes.as<uint8_t>();
      a.nb = ntotal;
      a.vmin = d_vmin.as<float>();
      a.vdiff = d_vdiff.as<float>();
      a.k = k;
      a.ip = ip();
      a.tau = p_tau.as<uint32_t>();
      a.partD = p_partD.as<float>();
      a.partI = p_partI.as<int64_t>();
      a.tmpD = p_tmpD.as<float>();
      a.tmpI = p_tmpI.as<int64_t>();
      a.D = D + q0 * k;
      a.I = I + q0 * k;
      launch_sq_search(a, pl, s);
      HIPCHECK(hipGetLastError());
    }
    mark_done(s);
  }

  void search_host(int64_t n, const float* x, int k, float* D, int64_t* I) {
    if (n == 0) return;
    quiesce();
    w_x.ensure(sizeof(float) * n * d);
    w_D.ensure(sizeof(float) * n * k);
    w_I.ensure(sizeof(int64_t) * n * k);
    HIPCHECK(hipMemcpyAsync(w_x.p, x, sizeof(float) * n * d, hipMemcpyHostToDevice, stream));
    search_dev(n, w_x.as<float>(), k, w_D.as<float>(), w_I.as<int64_t>(), stream);
    HIPCHECK(hipMemcpyAsync(D, w_D.p, sizeof(float) * n * k, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipMemcpyAsync(I, w_I.p, sizeof(int64_t) * n * k, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }
};

namespace {
void check_sq(const ivfpq_sq_index* h) { require(h != nullptr, "null index handle"); }
}  // namespace

extern "C" {

int ivfpq_sq_create(int d, int qtype, int metric, int device, ivfpq_sq_index** out) {
  return guarded([&] {
    require(out != nullptr, "null output pointer");
    require(d >= 4 && d <= 2048 && d % 4 == 0,
            "IndexScalarQuantizer: d must be a multiple of 4 in [4, 2048] (d = " + std::to_string(d) + ")");
    const char* qn = sq_qtype_name(qtype);
    require(qn != nullptr, "unknown scalar quantizer type " + std::to_string(qtype));
    require(qtype == IVFPQ_SQ_8BIT || qtype == IVFPQ_SQ_8BIT_UNIFORM || qtype == IVFPQ_SQ_FP16,
            std::string("scalar quantizer type ") + qn + " is not supported (QT_fp16, QT_8bit, QT_8bit_uniform)");
    require(metric == IVFPQ_METRIC_L2 || metric == IVFPQ_METRIC_INNER_PRODUCT, "unknown metric");
    auto h = std::make_unique<ivfpq_sq_index>();
    h->d = d;
    h->qtype = qtype;
    h->codec = qtype == IVFPQ_SQ_FP16 ? SQ_CODEC_FP16 : SQ_CODEC_8BIT;
    h->code_size = sq_code_size(h->codec, d);
    h->row_bytes = (size_t)h->code_size;
    h->slack = kSqScanSlack;  // the scan's 16-byte loads may straddle the last row's end
    h->metric = metric;
    h->trained = qtype == IVFPQ_SQ_FP16;  // nothing to train
    open_store(std::move(h), device, out);
  });
}

int ivfpq_sq_free(ivfpq_sq_index* h) { return free_store(h); }

int ivfpq_sq_train(ivfpq_sq_index* h, int64_t n, const float* x) {
  return guarded([&] {
    check_sq(h);
    require(x != nullptr && n > 0, "empty training set");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->train_host(n, x);
  });
}

int ivfpq_sq_set_trained(ivfpq_sq_index* h, const float* trained, int64_t count) {
  return guarded([&] {
    check_sq(h);
    require(count == (int64_t)h->nparams(),
            "trained has " + std::to_string(count) + " values, this quantizer " + std::to_string(h->nparams()));
    require(count == 0 || trained != nullptr, "null trained");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->params.assign(trained, trained + count);
    h->upload_params();
  });
}

int ivfpq_sq_add(ivfpq_sq_index* h, int64_t n, const float* x) {
  return guarded([&] {
    check_sq(h);
    require(h->trained, "index is not trained");
    if (n <= 0) return;
    require(x != nullptr, "null x");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->add_host(n, x, sizeof(float) * h->d, [&](int64_t c) { h->add_dev(c, h->w_x.as<float>(), h->stream); });
  });
}

int ivfpq_sq_add_device(ivfpq_sq_index* h, int64_t n, const float* x, void* stream) {
  return guarded([&] {
    check_sq(h);
    require(h->trained, "index is not trained");
    if (n <= 0) return;
    require(x != nullptr, "null x");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->add_dev(n, x, (hipStream_t)stream);
  });
}

int ivfpq_sq_add_codes(ivfpq_sq_index* h, int64_t n, const uint8_t* codes) {
  return guarded([&] {
    check_sq(h);
    require(h->trained, "index is not trained");
    if (n <= 0) return;
    require(codes != nullptr, "null codes");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->append_rows(n, codes);
  });
}

int ivfpq_sq_reset(ivfpq_sq_index* h) {
  return guarded([&] {
    check_sq(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->reset();
  });
}

int ivfpq_sq_search(ivfpq_sq_index* h, int64_t n, const float* x, int k, float* D, int64_t* I) {
  return guarded([&] {
    check_sq(h);
    check_search_args(h->trained, n, x, k, D, I);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->search_host(n, x, k, D, I);
  });
}

int ivfpq_sq_search_device(ivfpq_sq_index* h, int64_t n, const float* x, int k, float* D, int64_t* I, void* stream) {
  return guarded([&] {
    check_sq(h);
    check_search_args(h->trained, n, x, k, D, I);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->search_dev(n, x, k, D, I, (hipStream_t)stream);
  });
}

int64_t ivfpq_sq_ntotal(const ivfpq_sq_index* h) { return h ? h->ntotal : -1; }

int ivfpq_sq_is_trained(const ivfpq_sq_index* h) { return h && h->trained ? 1 : 0; }

int ivfpq_sq_get_dims(const ivfpq_sq_index* h, int* d, int* qtype, int* metric, int* code_size) {
  return guarded([&] {
    check_sq(h);
    if (d) *d = h->d;
    if (qtype) *qtype = h->qtype;
    if (metric) *metric = h->metric;
    if (code_size) *code_size = h->code_size;
  });
}

int ivfpq_sq_get_trained(const ivfpq_sq_index* h, float* out, int64_t* count) {
  return guarded([&] {
    check_sq(h);
    require(h->trained, "index is not trained");
    if (count) *count = (int64_t)h->params.size();
    if (out && !h->params.empty()) std::memcpy(out, h->params.data(), sizeof(float) * h->params.size());
  });
}

int ivfpq_sq_get_codes(ivfpq_sq_index* h, int64_t i0, int64_t n, uint8_t* out) {
  return guarded([&] {
    check_sq(h);
    std::lock_guard<std::mutex> lk(h->mu);
    require(i0 >= 0 && n >= 0 && i0 + n <= h->ntotal, "code range outside [0, ntotal)");
    if (n == 0) return;
    require(out != nullptr, "null output pointer");
    DeviceGuard g(h->device);
    h->read_rows(i0, n, out, h->row_bytes);
  });
}

int ivfpq_sq_encode(ivfpq_sq_index* h, int64_t n, const float* x, uint8_t* codes) {
  return guarded([&] {
    check_sq(h);
    require(h->trained, "index is not trained");
    if (n <= 0) return;
    require(x != nullptr && codes != nullptr, "null x / codes");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->encode_host(n, x, codes);
  });
}

int ivfpq_sq_decode(ivfpq_sq_index* h, int64_t n, const uint8_t* codes, float* x) {
  return guarded([&] {
    check_sq(h);
    require(h->trained, "index is not trained");
    if (n <= 0) return;
    require(x != nullptr && codes != nullptr, "null x / codes");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->decode_host(n, codes, x);
  });
}

}  // extern "C"

// ============================================================ flat binary codes (IndexBinaryFlat)
// faiss.IndexBinaryFlat: uint8 codes of d bits, every code compared with every query by
// Hamming distance and the k smallest (distance, label) selected by counting
// (binary_flat.hip).  The codes live in a CodeStore of stride bytes per row (rows padded
// with zero bytes to whole loads).
struct ivfpq_bin_index : CodeStore {
  int d = 0, code_size = 0, stride = 0;  // stride = row_bytes: a row padded to whole loads
  DevBuf w_D, w_I, p_qw, p_hist, p_T, p_quota;

  ivfpq_bin_index() : CodeStore("IndexBinaryFlat") {}

  // pad n device-resident codes [n][code_size] behind the image; returns when they are in place
  void add_dev(int64_t n, const uint8_t* xd, hipStream_t s) {
    reserve(n, s);
    order_after(s);
    launch_bin_pad_rows(xd, n, code_size, stride, d_codes.as<uint32_t>() + (size_t)ntotal * (stride / 4), s);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    ntotal += n;
  }

  // n device-resident queries -> D, I (device), all on s
  void search_dev(int64_t n, const uint8_t* xd, int k, int32_t* D, int64_t* I, hipStream_t s) {
    if (n == 0) return;
    order_after(s);
    if (ntotal == 0) {
      launch_bin_fill_empty(D, I, n * k, s);
      HIPCHECK(hipGetLastError());
      mark_done(s);
      return;
    }
    const BinPlan pl = bin_plan(d, ntotal, n);
    const int64_t qc = std::min(pl.qc, n);
    const int64_t nblocks = (qc + pl.QB - 1) / pl.QB;
    p_qw.ensure((size_t)nblocks * pl.QB * pl.stride);
    p_hist.ensure(sizeof(uint32_t) * (size_t)qc * pl.Sg * (d + 1));
    p_T.ensure(sizeof(int32_t) * qc);
    p_quota.ensure(sizeof(uint32_t) * (size_t)qc * pl.Sg);
    for (int64_t q0 = 0; q0 < n; q0 += qc) {
      BinSearchArgs a;
      a.x = xd + q0 * code_size;
      a.nq = std::min(qc, n - q0);
      a.d = d;
      a.codes = d_codes.as<uint32_t>();
      a.nb = ntotal;
      a.k = k;
      a.qw = p_qw.as<uint32_t>();
      a.hist = p_hist.as<uint32_t>();
      a.T = p_T.as<int32_t>();
      a.quota = p_quota.as<uint32_t>();
      a.D = D + q0 * k;
      a.I = I + q0 * k;
      launch_bin_search(a, pl, s);
      HIPCHECK(hipGetLastError());
    }
    mark_done(s);
  }

  void search_host(int64_t n, const uint8_t* x, int k, int32_t* D, int64_t* I) {
    if (n == 0) return;
    quiesce();
    w_x.ensure((size_t)n * code_size);
    w_D.ensure(sizeof(int32_t) * n * k);
    w_I.ensure(sizeof(int64_t) * n * k);
    HIPCHECK(hipMemcpyAsync(w_x.p, x, (size_t)n * code_size, hipMemcpyHostToDevice, stream));
    search_dev(n, w_x.as<uint8_t>(), k, w_D.as<int32_t>(), w_I.as<int64_t>(), stream);
    HIPCHECK(hipMemcpyAsync(D, w_D.p, sizeof(int32_t) * n * k, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipMemcpyAsync(I, w_I.p, sizeof(int64_t) * n * k, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }
};

namespace {
void check_bin(const ivfpq_bin_index* h) { require(h != nullptr, "null index handle"); }
void check_bin_d(int d) {
  require(d >= 8 && d <= kBinMaxD && d % 8 == 0,
          "IndexBinaryFlat: d must be a multiple of 8 in [8, 2048] (d = " + std::to_string(d) + ")");
}
}  // namespace

extern "C" {

int ivfpq_bin_create(int d, int device, ivfpq_bin_index** out) {
  return guarded([&] {
    require(out != nullptr, "null output pointer");
    check_bin_d(d);
    auto h = std::make_unique<ivfpq_bin_index>();
    h->d = d;
    h->code_size = d / 8;
    h->stride = bin_stride(h->code_size);
    h->row_bytes = (size_t)h->stride;
    open_store(std::move(h), device, out);
  });
}

int ivfpq_bin_free(ivfpq_bin_index* h) { return free_store(h); }

int ivfpq_bin_reset(ivfpq_bin_index* h) {
  return guarded([&] {
    check_bin(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->reset();
  });
}

int ivfpq_bin_add(ivfpq_bin_index* h, int64_t n, const uint8_t* x) {
  return guarded([&] {
    check_bin(h);
    if (n <= 0) return;
    require(x != nullptr, "null x");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->add_host(n, x, (size_t)h->code_size, [&](int64_t c) { h->add_dev(c, h->w_x.as<uint8_t>(), h->stream); });
  });
}

int ivfpq_bin_add_device(ivfpq_bin_index* h, int64_t n, const uint8_t* x, void* stream) {
  return guarded([&] {
    check_bin(h);
    if (n <= 0) return;
    require(x != nullptr, "null x");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->add_dev(n, x, (hipStream_t)stream);
  });
}

int ivfpq_bin_search(ivfpq_bin_index* h, int64_t n, const uint8_t* x, int k, int32_t* D, int64_t* I) {
  return guarded([&] {
    check_search_args(true, n, x, k, D, I);  // nothing to train
    check_bin(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->search_host(n, x, k, D, I);
  });
}

int ivfpq_bin_search_device(ivfpq_bin_index* h, int64_t n, const uint8_t* x, int k, int32_t* D, int64_t* I,
                            void* stream) {
  return guarded([&] {
    check_search_args(true, n, x, k, D, I);  // nothing to train
    check_bin(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->search_dev(n, x, k, D, I, (hipStream_t)stream);
  });
}

int64_t ivfpq_bin_ntotal(const ivfpq_bin_index* h) { return h ? h->ntotal : -1; }

int ivfpq_bin_get_dims(const ivfpq_bin_index* h, int* d, int* code_size) {
  return guarded([&] {
    check_bin(h);
    if (d) *d = h->d;
    if (code_size) *code_size = h->code_size;
  });
}

int ivfpq_bin_get_codes(ivfpq_bin_index* h, int64_t i0, int64_t n, uint8_t* out) {
  return guarded([&] {
    check_bin(h);
    std::lock_guard<std::mutex> lk(h->mu);
    require(i0 >= 0 && n >= 0 && i0 + n <= h->ntotal, "code range outside [0, ntotal)");
    if (n == 0) return;
    require(out != nullptr, "null output pointer");
    DeviceGuard g(h->device);
    h->read_rows(i0, n, out, (size_t)h->code_size);  // the rows without their pad bytes
  });
}

int ivfpq_bin_get_plan(int d, int64_t ntotal, int64_t nq, int k, int* stride, int* query_block, int* segments,
                       int64_t* segment_rows, int64_t* query_chunk) {
  return guarded([&] {
    check_bin_d(d);
    require(k >= 1 && k <= kMaxK, "k must be in [1, " + std::to_string(kMaxK) + "]");
    require(ntotal >= 0 && ntotal < (int64_t)INT32_MAX && nq >= 0, "ntotal / nq out of range");
    const BinPlan pl = bin_plan(d, ntotal, nq);
    if (stride) *stride = pl.stride;
    if (query_block) *query_block = pl.QB;
    if (segments) *segments = pl.Sg;
    if (segment_rows) *segment_rows = pl.seg_rows;
    if (query_chunk) *query_chunk = pl.qc;
  });
}

}  // extern "C"

// ============================================================ flat fp32 rows (IndexFlat)
// faiss.IndexFlat / IndexFlatL2 / IndexFlatIP: the raw vectors, every row compared with
// every query (flat_scan.hip).  The rows live in a CodeStore of 4 d bytes per row; their
// |y|^2 (launch_row_norms' tree order) are computed once, when the rows are added, and kept
// beside the image.  Every k runs the fused scan: no distance is written to memory.
namespace {

// the queries of one launch and its plan: the partial lists (12 bytes per entry, and the first
// merge round's output) within kPartialBytes, their count within the merge's 32-bit indexing
int64_t flat_query_chunk(int64_t n, int64_t nb, int k, int64_t force, FlatScanPlan* out) {
  int64_t qc = std::max<int64_t>(1, std::min<int64_t>(n, 1 << 16));
  FlatScanPlan pl = flat_scan_plan(qc, nb, k, force);
  while (true) {
    const size_t per_q = (size_t)pl.S * k * 12 * 2;
    const int64_t lim =
        std::max<int64_t>(1, std::min<int64_t>((int64_t)(kPartialBytes / per_q), (int64_t)(INT32_MAX / 2) / ((int64_t)pl.S * k)));
    if (qc <= lim) break;
    qc = std::max<int64_t>(1, std::min(lim, qc / 2));
    pl = flat_scan_plan(qc, nb, k, force);  // fewer query tiles: more ranges
  }
  if (out) *out = pl;
  return qc;
}

}  // namespace

struct ivfpq_flat_index : CodeStore {
  int d = 0, metric = IVFPQ_METRIC_L2;
  DevBuf d_norms;              // [cap] |y|^2 of the image's rows
  int64_t norms_cap = 0;
  int64_t rows_from_host = 0;  // rows copied from the host since create (ivfpq_flat_index_get_stats)
  int64_t reallocs = 0;        // times the image was reallocated
  int64_t range_rows = 0;      // > 0: the row range of a scan workgroup (ivfpq_flat_index_set_range_rows)
  DevBuf w_xn, w_D, w_I, p_tau, p_partD, p_partI, p_tmpD, p_tmpI;

  ivfpq_flat_index() : CodeStore("IndexFlat") {}
  bool ip() const { return metric == IVFPQ_METRIC_INNER_PRODUCT; }
  float* base() const { return d_codes.as<float>(); }

  // room for n more rows in the image and the norms beside it
  void reserve_rows(int64_t n, hipStream_t s) {
    const int64_t before = cap;
    reserve(n, s);
    if (cap != before) reallocs++;
    if (cap <= norms_cap) return;
    void* np = nullptr;
    HIPCHECK(hipMalloc(&np, sizeof(float) * (size_t)cap));
    if (ntotal) {
      hipError_t e = hipMemcpyAsync(np, d_norms.p, sizeof(float) * (size_t)ntotal, hipMemcpyDeviceToDevice, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess) {
        (void)hipFree(np);
        HIPCHECK(e);
      }
    }
    d_norms.release();
    d_norms.p = np;
    d_norms.bytes = sizeof(float) * (size_t)cap;
    norms_cap = cap;
  }

  // n rows (device-resident, or host rows when from_host) behind the image with their norms;
  // returns when they are in place
  void add_rows(int64_t n, const float* x, bool from_host, hipStream_t s) {
    reserve_rows(n, s);
    if (from_host) quiesce();
    else order_after(s);
    float* dst = base() + (size_t)ntotal * d;
    HIPCHECK(hipMemcpyAsync(dst, x, sizeof(float) * (size_t)n * d, from_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
    launch_row_norms(dst, n, d, d_norms.as<float>() + ntotal, s);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    ntotal += n;
    if (from_host) rows_from_host += n;
  }

  void reset_rows() {
    reset();
    d_norms.release();
    norms_cap = 0;
  }

  // n device-resident queries -> D, I (device), all on s
  void search_dev(int64_t n, const float* xd, int k, float* D, int64_t* I, hipStream_t s) {
    if (n == 0) return;
    order_after(s);
    if (ntotal == 0) {
      launch_fill_empty(D, I, n * k, ip(), s);
      HIPCHECK(hipGetLastError());
      mark_done(s);
      return;
    }
    FlatScanPlan pl;
    const int64_t qc = flat_query_chunk(n, ntotal, k, range_rows, &pl);
    w_xn.ensure(sizeof(float) * qc);
    p_tau.ensure(sizeof(uint32_t) * qc);
    p_partD.ensure(sizeof(float) * (size_t)pl.S * qc * k);
    p_partI.ensure(sizeof(int64_t) * (size_t)pl.S * qc * k);
    const size_t tmp_lists = (size_t)std::max(1, pl.S / pl.fan);
    p_tmpD.ensure(sizeof(float) * tmp_lists * qc * k);
    p_tmpI.ensure(sizeof(int64_t) * tmp_lists * qc * k);
    for (int64_t q0 = 0; q0 < n; q0 += qc) {
      const int64_t c = std::min(qc, n - q0);
      const float* xq = xd + q0 * d;
      launch_row_norms(xq, c, d, w_xn.as<float>(), s);
      FlatScanArgs a;
      a.x = xq;
      a.xn = w_xn.as<float>();
      a.nq = c;
      a.d = d;
      a.base = base();
      a.bn = d_norms.as<float>();
      a.nb = ntotal;
      a.k = k;
      a.ip = ip();
      a.tau = p_tau.as<uint32_t>();
      a.partD = p_partD.as<float>();
      a.partI = p_partI.as<int64_t>();
      a.tmpD = p_tmpD.as<float>();
      a.tmpI = p_tmpI.as<int64_t>();
      a.D = D + q0 * k;
      a.I = I + q0 * k;
      // (a shorter last chunk keeps the plan: its tile and ranges are valid for any nq)
      launch_flat_search(a, pl, s);
      HIPCHECK(hipGetLastError());
    }
    mark_done(s);
  }

  void search_host(int64_t n, const float* x, int k, float* D, int64_t* I) {
    if (n == 0) return;
    quiesce();
    w_x.ensure(sizeof(float) * n * d);
    w_D.ensure(sizeof(float) * n * k);
    w_I.ensure(sizeof(int64_t) * n * k);
    HIPCHECK(hipMemcpyAsync(w_x.p, x, sizeof(float) * n * d, hipMemcpyHostToDevice, stream));
    search_dev(n, w_x.as<float>(), k, w_D.as<float>(), w_I.as<int64_t>(), stream);
    HIPCHECK(hipMemcpyAsync(D, w_D.p, sizeof(float) * n * k, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipMemcpyAsync(I, w_I.p, sizeof(int64_t) * n * k, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }
};

namespace {
void check_flat(const ivfpq_flat_index* h) { require(h != nullptr, "null index handle"); }
}  // namespace

extern "C" {

int ivfpq_flat_index_create(int device, int d, int metric, ivfpq_flat_index** out) {
  return guarded([&] {
    require(out != nullptr, "null output pointer");
    require(d >= 1, "IndexFlat: d must be at least 1 (d = " + std::to_string(d) + ")");
    require(metric == IVFPQ_METRIC_L2 || metric == IVFPQ_METRIC_INNER_PRODUCT, "unknown metric");
    auto h = std::make_unique<ivfpq_flat_index>();
    h->d = d;
    h->metric = metric;
    h->row_bytes = sizeof(float) * (size_t)d;
    open_store(std::move(h), device, out);
  });
}

int ivfpq_flat_index_free(ivfpq_flat_index* h) { return free_store(h); }

int ivfpq_flat_index_reset(ivfpq_flat_index* h) {
  return guarded([&] {
    check_flat(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->reset_rows();
  });
}

int ivfpq_flat_index_add(ivfpq_flat_index* h, int64_t n, const float* x) {
  return guarded([&] {
    check_flat(h);
    if (n <= 0) return;
    require(x != nullptr, "null x");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->add_rows(n, x, true, h->stream);
  });
}

int ivfpq_flat_index_add_device(ivfpq_flat_index* h, int64_t n, const float* x, void* stream) {
  return guarded([&] {
    check_flat(h);
    if (n <= 0) return;
    require(x != nullptr, "null x");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->add_rows(n, x, false, (hipStream_t)stream);
  });
}

int ivfpq_flat_index_search(ivfpq_flat_index* h, int64_t n, const float* x, int k, float* D, int64_t* I) {
  return guarded([&] {
    check_search_args(true, n, x, k, D, I);  // nothing to train
    check_flat(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->search_host(n, x, k, D, I);
  });
}

int ivfpq_flat_index_search_device(ivfpq_flat_index* h, int64_t n, const float* x, int k, float* D, int64_t* I,
                                   void* stream) {
  return guarded([&] {
    check_search_args(true, n, x, k, D, I);  // nothing to train
    check_flat(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->search_dev(n, x, k, D, I, (hipStream_t)stream);
  });
}

int64_t ivfpq_flat_index_ntotal(const ivfpq_flat_index* h) { return h ? h->ntotal : -1; }

int ivfpq_flat_index_get_dims(const ivfpq_flat_index* h, int* d, int* metric) {
  return guarded([&] {
    check_flat(h);
    if (d) *d = h->d;
    if (metric) *metric = h->metric;
  });
}

int ivfpq_flat_index_get_rows(ivfpq_flat_index* h, int64_t i0, int64_t n, float* out) {
  return guarded([&] {
    check_flat(h);
    std::lock_guard<std::mutex> lk(h->mu);
    require(i0 >= 0 && n >= 0 && i0 + n <= h->ntotal, "row range outside [0, ntotal)");
    if (n == 0) return;
    require(out != nullptr, "null output pointer");
    DeviceGuard g(h->device);
    h->read_rows(i0, n, reinterpret_cast<uint8_t*>(out), h->row_bytes);
  });
}

int ivfpq_flat_index_get_stats(ivfpq_flat_index* h, int64_t* rows_from_host, int64_t* capacity, int64_t* reallocs) {
  return guarded([&] {
    check_flat(h);
    std::lock_guard<std::mutex> lk(h->mu);
    if (rows_from_host) *rows_from_host = h->rows_from_host;
    if (capacity) *capacity = h->cap;
    if (reallocs) *reallocs = h->reallocs;
  });
}

int ivfpq_flat_index_set_range_rows(ivfpq_flat_index* h, int64_t rows) {
  return guarded([&] {
    check_flat(h);
    require(rows >= 0, "negative range size");
    std::lock_guard<std::mutex> lk(h->mu);
    h->range_rows = rows;
  });
}

int ivfpq_flat_index_get_plan(int64_t nq, int64_t nb, int k, int64_t set_rows, int* tile_q, int64_t* range_rows,
                              int* ranges, int* S, int* fan, int* rounds, int64_t* query_chunk) {
  return guarded([&] {
    require(k >= 1 && k <= kMaxK, "k must be in [1, " + std::to_string(kMaxK) + "]");
    require(nb >= 0 && nb < (int64_t)INT32_MAX && nq >= 0 && set_rows >= 0, "nb / nq / range size out of range");
    FlatScanPlan pl;
    const int64_t qc = flat_query_chunk(nq, nb, k, set_rows, &pl);
    if (tile_q) *tile_q = pl.tile_q;
    if (range_rows) *range_rows = pl.range_rows;
    if (ranges) *ranges = pl.ranges;
    if (S) *S = pl.S;
    if (fan) *fan = pl.fan;
    if (rounds) *rounds = pl.rounds;
    if (query_chunk) *query_chunk = qc;
  });
}

// ---- PCA training moments (faiss_amd.PCAMatrix.train) ----

int ivfpq_pca_moments_device(int64_t n, int d, const float* x, float* mean_out, float* scatter_out, void* stream) {
  return guarded([&] {
    const PcaPlan p = checked_pca_plan(n, d);
    require(x != nullptr && mean_out != nullptr && scatter_out != nullptr, "null buffer");
    DevBuf ws;
    ws.ensure(pca_workspace_bytes(p, d));
    launch_pca_moments(x, n, d, p, ws.p, mean_out, scatter_out, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize((hipStream_t)stream));  // the workspace is released on return
  });
}

int ivfpq_pca_set_chunk_rows(int64_t rows) {
  return guarded([&] {
    require(rows >= 0, "negative chunk length");
    g_pca_chunk_rows.store(rows);
  });
}

int ivfpq_pca_get_plan(int64_t n, int d, int* chunks, int64_t* chunk_rows, int* tiles) {
  return guarded([&] {
    const PcaPlan p = checked_pca_plan(n, d);
    if (chunks) *chunks = p.chunks;
    if (chunk_rows) *chunk_rows = p.chunk_rows;
    if (tiles) *tiles = p.tiles;
  });
}

}  // extern "C"
