// Launchers of the resident OPQ trainer (opq_train.hip) behind faiss_amd.OPQMatrix.train_device
// (opq.cpp): the Lloyd assignment of all M sub-quantizers of the rotated rows in one launch, the
// labels that hand its update to km_update.h, and the Procrustes cross matrix
// C [d][d2] = sum_r xt_r (x) cb[code_r] on v_mfma_f32_16x16x4_f32 with the decode fused in, one
// partial tile per (64 x 64 tile, row chunk), the partials added in chunk order.  No
// floating-point atomics: the result depends on (n, d, d2, chunk_rows) and the input alone.
// All launchers are asynchronous on `stream` and allocate nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace chivf {

constexpr int kOpqTile = 64;            // an output tile of the cross is 64 dimensions of xt x 64 of rec
constexpr int kOpqKr = 32;              // rows per staged step (the K chunk of the product)
constexpr int kOpqMinChunkRows = 256;   // the default plan takes no shorter chunks
constexpr int kOpqTargetGroups = 1024;  // workgroups the default plan aims at (a constant: the plan never asks the device)
constexpr int kOpqMaxChunks = 65535;
constexpr int kOpqAssignRows = 1024;    // rows of one assignment workgroup (its codebook stage is paid once for them)
constexpr int kOpqMaxDsub = 64;         // a [256][dsub] sub-codebook of at most 64 KiB is staged in LDS

// How the cross splits its rows: `chunks` chunks of chunk_rows rows (a multiple of kOpqKr; the last
// one shorter), tiles = tbi * tbj output tiles, tbi = ceil(d / 64), tbj = ceil(d2 / 64).
struct OpqPlan {
  int tbi = 0, tbj = 0;
  int tiles = 0;
  int64_t chunk_rows = 0;
  int chunks = 0;
};
// set_rows > 0: the chunk length (rounded up to kOpqKr); 0: chosen from (n, d, d2) alone so that
// tiles * chunks is about kOpqTargetGroups.  n >= 1, d >= d2 >= 1.
OpqPlan opq_plan(int64_t n, int d, int d2, int64_t set_rows);
// [chunks][tiles][64 * 64] fp32 partial tiles
size_t opq_cross_workspace_bytes(const OpqPlan& p);

// xt[r][c] = x[r][c] - mean[c] in fp32 (x and xt may be the same buffer)
void launch_opq_center(const float* x, int64_t n, int d, const float* mean, float* xt, hipStream_t s);

// codes[r][m] = first argmin_j |xp_r[m] - cb[m][j]|^2 in tree<K_L2> order: the codes of
// launch_pq_encode_flat bit for bit.  xp [n][d2], cb [M][256][d2 / M].  A workgroup takes one
// sub-quantizer and kOpqAssignRows rows with the sub-codebook in LDS; a dsub without such a
// kernel (opq_assign_in_lds false: dsub > kOpqMaxDsub among them) goes to launch_pq_encode_flat.
bool opq_assign_in_lds(int dsub);
void launch_opq_assign(const float* xp, int64_t n, int d2, const float* cb, int M, uint8_t* codes, hipStream_t s);

// labels[r * M + m] = m * 256 + codes[r][m]: the clusters of the [n * M][dsub] view of xp, for launch_km_pass
void launch_opq_labels(const uint8_t* codes, int64_t n, int M, int64_t* labels, hipStream_t s);

// C [d][d2] = sum_r xt_r (x) rec_r, rec_r[c] = cb[c / dsub][codes[r][c / dsub]][c % dsub];
// xt [n][d] (centred), part: opq_cross_workspace_bytes
void launch_opq_cross(const float* xt, int64_t n, int d, const uint8_t* codes, const float* cb, int d2, int M,
                      const OpqPlan& p, float* part, float* C, hipStream_t s);

}  // namespace chivf
