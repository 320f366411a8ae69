// Epilogue activations of the FP8 GEMMs (gemm_fp8.hip, gemm_mxfp8.hip).
#pragma once

#include "common.h"

// ACT_GEGLU is not an activation of gemm_fp8: it selects the paired-column
// epilogue of gemm_fp8_geglu_kernel
enum { ACT_NONE = 0, ACT_SILU = 1, ACT_GELU = 2, ACT_GEGLU = 3 };

#if defined(__HIP_DEVICE_COMPILE__)
#define FP8_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define FP8_NO_PK_F32
#endif

__device__ __forceinline__ float gelu_tanh_f(float x) {
  // 0.5 x (1 + tanh(u)) = x * sigmoid(2u), u = sqrt(2/pi) (x + 0.044715 x^3);
  // the sigmoid form has no 1 + tanh cancellation for negative x
  const float u2 = 1.5957691216057308f * (x + 0.044715f * x * x * x);
  return x / (1.0f + __expf(-u2));
}

template <int ACT>
__device__ __forceinline__ float act_q(float v) {
  if (ACT == ACT_SILU) return silu_f(v);
  if (ACT == ACT_GELU) return gelu_tanh_f(v);
  return v;
}
