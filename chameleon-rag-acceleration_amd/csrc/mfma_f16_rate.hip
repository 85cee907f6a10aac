// mfma_f16_rate.hip — the box's measured rate of v_mfma_f32_16x16x32_f16, the instruction of
// flat_scan_f16.hip, for the MFMA floor of profiles/indexflat_f16_bench.py.  Not part of the
// library or its C-ABI: a separate libmfmarate.so, like libhbmstream.so.
//
// Every wave issues `iters` rounds of eight independent accumulator chains (no memory in the
// loop, the operands stay in registers); the grid is eight workgroups of four waves per CU,
// eight waves per SIMD, more than the matrix pipe needs to stay full.  Timed with HIP events on
// the caller's stream, best of `reps` launches; flop = waves x iters x 8 x 2 x 16 x 16 x 32.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
constexpr int kThreads = 256;
constexpr int kChains = 8;

__global__ __launch_bounds__(kThreads) void k_mfma_f16_rate(int iters, float* __restrict__ sink) {
  const int lane = threadIdx.x & 63;
  h8 a, b;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    a[j] = (_Float16)(0.001f * (float)(lane + j));
    b[j] = (_Float16)(0.002f * (float)(lane - j));
  }
  f4 acc[kChains];
#pragma unroll
  for (int c = 0; c < kChains; c++) acc[c] = f4{0.f, 0.f, 0.f, 0.f};
  for (int it = 0; it < iters; it++) {
#pragma unroll
    for (int c = 0; c < kChains; c++) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc[c], 0, 0, 0);
  }
  float v = 0.f;
#pragma unroll
  for (int c = 0; c < kChains; c++) v += acc[c][0] + acc[c][1] + acc[c][2] + acc[c][3];
  sink[(int64_t)blockIdx.x * kThreads + threadIdx.x] = v;  // (keeps the chains)
}

}  // namespace

extern "C" {

// Best time (ms) of `reps` launches of `iters` rounds per wave on `stream`; *flop is what one
// launch computes.  `sink`: device scratch of at least *grid x 256 floats -- call first with
// sink == NULL to learn the grid.  Returns 0, or a hipError_t.
int mfma_f16_rate_measure(int iters, int reps, void* sink, int64_t sink_bytes, void* stream, int* grid_out,
                          float* best_ms, double* flop) {
  int dev = 0, cus = 256;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  const int grid = cus * 8;
  if (grid_out) *grid_out = grid;
  if (!sink) return 0;
  if (sink_bytes < (int64_t)grid * kThreads * 4 || iters < 1 || reps < 1) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  hipEvent_t a, b;
  if ((e = hipEventCreate(&a)) != hipSuccess) return (int)e;
  if ((e = hipEventCreate(&b)) != hipSuccess) return (int)e;
  float best = 1e30f;
  for (int r = 0; r <= reps; r++) {  // (launch 0: warm-up)
    (void)hipEventRecord(a, s);
    hipLaunchKernelGGL(k_mfma_f16_rate, dim3(grid), dim3(kThreads), 0, s, iters, (float*)sink);
    (void)hipEventRecord(b, s);
    (void)hipEventSynchronize(b);
    float t = 0.f;
    (void)hipEventElapsedTime(&t, a, b);
    if (r > 0 && t < best) best = t;
  }
  e = hipGetLastError();
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  *best_ms = best;
  *flop = (double)grid * (kThreads / 64) * (double)iters * kChains * 2.0 * 16 * 16 * 32;
  return (int)e;
}

}  // extern "C"
