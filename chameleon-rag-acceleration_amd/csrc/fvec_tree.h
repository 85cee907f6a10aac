// Faiss-1.7.1 AVX reduction order (or_tree in oracle/ivfpq_oracle.c; the same function as
// tree<> in ivfpq_kernels.hip), shared by the flat product-quantizer kernels (pq_flat.hip,
// pq_flat4.hip).  In an anonymous namespace like scan_topk.h: each translation unit compiles
// its own copy, inlined into its kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "scan_topk.h"  // K_IP, K_L2

namespace chivf {

namespace {

template <int KIND, class FX, class FY>
__device__ __forceinline__ float tree(FX fx, FY fy, int d) {
  float a8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int i = 0;
  for (; i + 8 <= d; i += 8) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
      float p;
      if (KIND == K_IP) {
        p = fx(i + j) * fy(i + j);
      } else {
        float t = fx(i + j) - fy(i + j);
        p = t * t;
      }
      a8[j] = a8[j] + p;
    }
  }
  float a4[4];
#pragma unroll
  for (int j = 0; j < 4; j++) a4[j] = a8[j + 4] + a8[j];
#pragma unroll
  for (int pass = 0; pass < 2; pass++) {
    // pass 0: the 4-wide remainder (d - i >= 4); pass 1: the masked tail
    if (pass == 0 && i + 4 > d) continue;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (i + j < d) {
        float p;
        if (KIND == K_IP) {
          p = fx(i + j) * fy(i + j);
        } else {
          float t = fx(i + j) - fy(i + j);
          p = t * t;
        }
        a4[j] = a4[j] + p;
      }
    }
    if (pass == 0) i += 4;
  }
  float h0 = a4[0] + a4[1];
  float h1 = a4[2] + a4[3];
  return h0 + h1;
}

}  // namespace

}  // namespace chivf
