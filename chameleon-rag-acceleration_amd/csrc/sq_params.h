// What the scalar-quantizer indexes (sq_index.cpp, ivfsq_index.cpp) share on the host: the
// quantizer types and their rejection by name, and Faiss's sq.trained -- from the min/max
// reduction's bits, and expanded to the per-dimension arrays the kernels read.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "host_common.h"
#include "ivfpq.h"
#include "sq_scan.h"

namespace chivf {

inline const char* sq_qtype_name(int qtype) {
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

// the supported types pass; the others are rejected by name, unknown values by number
inline void check_sq_qtype(int qtype) {
  const char* qn = sq_qtype_name(qtype);
  require(qn != nullptr, "unknown scalar quantizer type " + std::to_string(qtype));
  require(qtype == IVFPQ_SQ_8BIT || qtype == IVFPQ_SQ_8BIT_UNIFORM || qtype == IVFPQ_SQ_FP16,
          std::string("scalar quantizer type ") + qn + " is not supported (QT_fp16, QT_8bit, QT_8bit_uniform)");
}

inline int sq_codec_of(int qtype) { return qtype == IVFPQ_SQ_FP16 ? SQ_CODEC_FP16 : SQ_CODEC_8BIT; }

// length of sq.trained: [vmin (d), vdiff (d)], [vmin, vdiff] (uniform) or empty (fp16)
inline size_t sq_nparams(int qtype, int d) {
  return qtype == IVFPQ_SQ_FP16 ? 0 : qtype == IVFPQ_SQ_8BIT_UNIFORM ? 2 : 2 * (size_t)d;
}

// sq.trained of an 8-bit type from launch_sq_minmax's bits [lo (d), hi (d)] (RS_minmax, rangestat_arg 0)
inline std::vector<float> sq_trained_from_minmax(const std::vector<uint32_t>& bits, int qtype, int d) {
  std::vector<float> mn(d), mx(d);
  for (int j = 0; j < d; j++) {
    mn[j] = sq_minmax_value(bits[j]);
    mx[j] = sq_minmax_value(bits[(size_t)d + j]);
  }
  if (qtype == IVFPQ_SQ_8BIT_UNIFORM) {
    const float lo_all = *std::min_element(mn.begin(), mn.end());
    const float hi_all = *std::max_element(mx.begin(), mx.end());
    return {lo_all, hi_all - lo_all};
  }
  std::vector<float> params(2 * (size_t)d);
  for (int j = 0; j < d; j++) {
    params[j] = mn[j];
    params[(size_t)d + j] = mx[j] - mn[j];
  }
  return params;
}

// the 8-bit codec's device parameters: per dimension, a uniform pair repeated d times
inline void sq_upload_params(const std::vector<float>& params, int qtype, int d, DevBuf& d_vmin, DevBuf& d_vdiff,
                             hipStream_t stream) {
  const bool uniform = qtype == IVFPQ_SQ_8BIT_UNIFORM;
  std::vector<float> mn(d), df(d);
  for (int j = 0; j < d; j++) {
    mn[j] = uniform ? params[0] : params[j];
    df[j] = uniform ? params[1] : params[(size_t)d + j];
  }
  d_vmin.ensure(sizeof(float) * d);
  d_vdiff.ensure(sizeof(float) * d);
  HIPCHECK(hipMemcpyAsync(d_vmin.p, mn.data(), sizeof(float) * d, hipMemcpyHostToDevice, stream));
  HIPCHECK(hipMemcpyAsync(d_vdiff.p, df.data(), sizeof(float) * d, hipMemcpyHostToDevice, stream));
  HIPCHECK(hipStreamSynchronize(stream));
}

}  // namespace chivf
