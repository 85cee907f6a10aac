// Launchers for the PCA training moments (pca_moments.hip) behind faiss_amd.PCAMatrix.train:
// the column mean and the centred scatter matrix S = sum_r (x_r - mean)(x_r - mean)^T of a
// device-resident [n][d] fp32 matrix.  The mean is an fp64 column sum over fixed row chunks,
// rounded to fp32 once; the scatter is accumulated on v_mfma_f32_16x16x4_f32 with the row
// index as the K dimension, one partial tile per (upper-triangle tile, row chunk), and the
// partials are added in chunk order.  No floating-point atomics: the result depends on
// (n, d, chunk_rows) and the input alone.  All launchers are asynchronous on `stream` and
// allocate nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace chivf {

constexpr int kPcaTile = 64;            // an output tile is 64 x 64 dimensions: 16 rows of it per wave
constexpr int kPcaKr = 32;              // rows of x per staged step (the K chunk of the product)
constexpr int kPcaMinChunkRows = 256;   // the default plan takes no shorter chunks
constexpr int kPcaTargetGroups = 1024;  // workgroups the default plan aims at (a constant: the plan never asks the device)
constexpr int kPcaMeanRows = 1024;      // rows per fp64 column-sum chunk (fixed: the mean does not depend on the scatter plan)
constexpr int kPcaMaxChunks = 65535;

// How the rows are split: `chunks` chunks of chunk_rows rows (a multiple of kPcaKr; the last
// one shorter), `tiles` = tb (tb + 1) / 2 upper-triangle output tiles, tb = ceil(d / 64).
struct PcaPlan {
  int tb = 0;
  int tiles = 0;
  int64_t chunk_rows = 0;
  int chunks = 0;
  int mean_chunks = 0;
};
// set_rows > 0: the chunk length (rounded up to kPcaKr); 0: chosen from (n, d) alone so that
// tiles * chunks is about kPcaTargetGroups.  n >= 1, d >= 1.
PcaPlan pca_plan(int64_t n, int d, int64_t set_rows);
// [mean_chunks][d] fp64 column sums, then [chunks][tiles][64 * 64] fp32 partial tiles
size_t pca_workspace_bytes(const PcaPlan& p, int d);
// x [n][d]; mean [d]; scatter [d][d] (full, exactly symmetric, not divided by n); ws: pca_workspace_bytes
void launch_pca_moments(const float* x, int64_t n, int d, const PcaPlan& p, void* ws, float* mean, float* scatter,
                        hipStream_t s);

}  // namespace chivf
