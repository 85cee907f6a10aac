// The device image of inverted lists and the device-side adds waiting to be merged into
// it, as IVF-PQ (rows = PQ codes) and IVF-Flat (rows = the fp32 vectors) keep them.
#pragma once
#include <vector>

#include "host_common.h"
#include "ivfpq_build.h"

namespace chivf {

// lists concatenated in list order, every list sorted by label: offsets i64[nlist + 1],
// rows u8[n][row_bytes], labels i64[n]
struct ListImage {
  DevBuf off, rows, ids;
};

// Device-side adds not yet merged into the image: list numbers (any list), labels and
// rows, n of them.
struct PendingSet {
  size_t row_bytes = 0;
  size_t image_slack = 0;  // bytes the merged image's rows are allocated past their end (a scan's read slack)
  DevBuf lists, ids, rows;
  int64_t n = 0, cap = 0;

  // room for `need` entries: the set doubles (at least) when it is full
  void reserve(int64_t need, hipStream_t s) {
    if (need <= cap) return;
    const int64_t ncap = std::max<int64_t>(need, cap * 2);
    DevBuf l2, i2, r2;
    l2.ensure(sizeof(int64_t) * ncap);
    i2.ensure(sizeof(int64_t) * ncap);
    r2.ensure(row_bytes * ncap);
    if (n > 0) {
      HIPCHECK(hipMemcpyAsync(l2.p, lists.p, sizeof(int64_t) * n, hipMemcpyDeviceToDevice, s));
      HIPCHECK(hipMemcpyAsync(i2.p, ids.p, sizeof(int64_t) * n, hipMemcpyDeviceToDevice, s));
      HIPCHECK(hipMemcpyAsync(r2.p, rows.p, row_bytes * n, hipMemcpyDeviceToDevice, s));
      HIPCHECK(hipStreamSynchronize(s));
    }
    lists.swap(l2);
    ids.swap(i2);
    rows.swap(r2);
    cap = ncap;
  }
  void drop() {
    lists.release();
    ids.release();
    rows.release();
    n = cap = 0;
  }
};

// The pending entries merged into the image: sorted by (list, label) alone (rocprim
// radix sorts of the pending set, lists outside [lo, hi) dropped), then interleaved
// list by list into the label-sorted image (ivfpq_build.h image_merge_lists).  The
// result equals a stable (list, label) sort of old + new, the image order of
// DESIGN.md §3.  old_off: the image's offsets on the host (null: read from the
// device).  `kept` entries must survive the range, else kept_msg.  The pending rows are
// released once gathered, so the merge peaks at row_bytes per pending entry less.
// Returns the new image's offsets; the pending set is left empty.
inline std::vector<int64_t> merge_pending(PendingSet& q, ListImage& img, int nlist, int lo, int hi,
                                          const int64_t* old_off, int64_t kept, const char* kept_msg, hipStream_t s) {
  ImageMergeArgs g;
  g.nlist = nlist;
  g.lo = lo;
  g.hi = hi;
  g.M = (int)q.row_bytes;
  g.n_old = 0;
  g.n_new = q.n;
  g.new_lists = q.lists.as<int64_t>();
  g.new_ids = q.ids.as<int64_t>();
  g.new_codes = q.rows.as<uint8_t>();
  DevBuf new_off, scratch, rows_n, ids_n;
  new_off.ensure(sizeof(int64_t) * (nlist + 1));
  g.off_out = new_off.as<int64_t>();
  const size_t sb = image_merge_scratch_bytes(q.n, nlist);
  scratch.ensure(sb);
  HIPCHECK(image_merge_sort(g, scratch.p, sb, s));
  std::vector<int64_t> noff(nlist + 1), ooff(nlist + 1);
  HIPCHECK(hipMemcpyAsync(noff.data(), new_off.p, sizeof(int64_t) * (nlist + 1), hipMemcpyDeviceToHost, s));
  if (old_off)
    ooff.assign(old_off, old_off + nlist + 1);
  else
    HIPCHECK(hipMemcpyAsync(ooff.data(), img.off.p, sizeof(int64_t) * (nlist + 1), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  require(noff[nlist] == kept, kept_msg);
  rows_n.ensure(std::max<size_t>(16, q.row_bytes * kept));
  ids_n.ensure(std::max<size_t>(16, sizeof(int64_t) * kept));
  g.codes_out = rows_n.as<uint8_t>();
  g.ids_out = ids_n.as<int64_t>();
  HIPCHECK(image_merge_gather(g, kept, scratch.p, s));
  HIPCHECK(hipStreamSynchronize(s));
  scratch.release();
  q.rows.release();  // (gathered: the pending rows now live in rows_n)
  std::vector<int64_t> off(nlist + 1);
  int64_t mx = 0;
  for (int l = 0; l <= nlist; l++) {
    off[l] = ooff[l] + noff[l];
    if (l < nlist) mx = std::max(mx, (ooff[l + 1] - ooff[l]) + (noff[l + 1] - noff[l]));
  }
  const int64_t n_out = off[nlist];
  ListImage out;
  out.rows.ensure(std::max<size_t>(16, q.row_bytes * n_out + q.image_slack));
  out.ids.ensure(std::max<size_t>(16, sizeof(int64_t) * n_out));
  out.off.ensure(sizeof(int64_t) * (nlist + 1));
  ListMergeArgs m;
  m.nlist = nlist;
  m.lo = lo;
  m.hi = hi;
  m.M = (int)q.row_bytes;
  m.max_list = mx;
  m.old_off = img.off.as<int64_t>();
  m.old_codes = img.rows.as<uint8_t>();
  m.old_ids = img.ids.as<int64_t>();
  m.new_off = new_off.as<int64_t>();
  m.new_codes = rows_n.as<uint8_t>();
  m.new_ids = ids_n.as<int64_t>();
  m.out_off = out.off.as<int64_t>();
  m.out_codes = out.rows.as<uint8_t>();
  m.out_ids = out.ids.as<int64_t>();
  HIPCHECK(image_merge_lists(m, s));
  HIPCHECK(hipStreamSynchronize(s));
  img.rows.swap(out.rows);
  img.ids.swap(out.ids);
  img.off.swap(out.off);
  q.drop();
  return off;
}

}  // namespace chivf
