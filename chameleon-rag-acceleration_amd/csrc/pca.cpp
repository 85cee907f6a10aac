// PCA training moments (faiss_amd.PCAMatrix.train) behind the C-ABI of include/ivfpq.h.
#include <atomic>

#include "host_common.h"
#include "ivfpq.h"
#include "ivfpq_test.h"
#include "pca_moments.h"

using namespace chivf;

namespace {

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
