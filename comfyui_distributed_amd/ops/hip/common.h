// Common device helpers for the CDNA4 (gfx950) kernels.
// All kernels in this extension are written directly for MI355X: wave64,
// LDS-staged tiles, MFMA for matmul-shaped work, bf16 activations with fp32
// accumulation. No CUDA-compat paths.
#pragma once

#include <torch/extension.h>  // the host helpers below: TORCH_CHECK, Tensor
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>

#define WAVE_SIZE 64

using bf16_t = __hip_bfloat16;

// Raw-bits bf16 <-> f32 (load path: shift; store path: RNE via builtin).
__device__ __forceinline__ float bf16_bits_to_f32(uint16_t u) {
  union { uint32_t u32; float f; } cvt;
  cvt.u32 = (uint32_t)u << 16;
  return cvt.f;
}

__device__ __forceinline__ uint16_t f32_to_bf16_bits(float f) {
  union { __hip_bfloat16 b; uint16_t u; } cvt;
  cvt.b = __float2bfloat16(f);  // round-to-nearest-even
  return cvt.u;
}

// Vector types for wide loads (G13: always vectorize bf16).
typedef uint16_t ushort8_t __attribute__((ext_vector_type(8)));
typedef float float4_t __attribute__((ext_vector_type(4)));

// Wave-wide reductions (64 lanes).
__device__ __forceinline__ float wave_reduce_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ float wave_reduce_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// Block reduction over up to 1024 threads via LDS (caller provides scratch
// of >= blockDim.x / 64 floats).
template <typename Op>
__device__ __forceinline__ float block_reduce(float v, float* scratch, Op op,
                                              float identity) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nwaves = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
  if (lane == 0) scratch[wave] = v;
  __syncthreads();
  float r = identity;
  if (wave == 0) {
    r = (lane < nwaves) ? scratch[lane] : identity;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) r = op(r, __shfl_xor(r, off, 64));
    if (lane == 0) scratch[0] = r;
  }
  __syncthreads();
  r = scratch[0];
  __syncthreads();
  return r;
}

struct SumOp {
  __device__ float operator()(float a, float b) const { return a + b; }
};
struct MaxOp {
  __device__ float operator()(float a, float b) const { return fmaxf(a, b); }
};

__device__ __forceinline__ float silu_f(float x) {
  return x / (1.0f + __expf(-x));
}

// Per-row FP8 (OCP e4m3fn) quantisation of bf16 rows, shared by
// quant_rows_fp8_kernel (gemm_fp8.hip) and the FP8 tail of
// norm_modulate_kernel (dit_ops.hip), so the two give the same bytes:
//   scale = max(amax, 2^-126 * 448) * (1/448)     one fp32 multiply
//   q     = rne_e4m3(clamp(x * (1/scale), +-448))
#define E4M3_MAX 448.0f
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));

// absmax of 8 packed bf16 values, folded into `amax`
__device__ __forceinline__ float fp8_absmax8(const ushort8_t v, float amax) {
#pragma unroll
  for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(bf16_bits_to_f32(v[j])));
  return amax;
}

// 2^-126 * 448: an all-zero row gets the smallest scale, not a division by
// zero
__device__ __forceinline__ float fp8_row_scale(float amax) {
  return fmaxf(amax, 0x1p-126f * E4M3_MAX) * (1.0f / E4M3_MAX);
}

// the scale can come out just under 2^-126; keep the reciprocal's operand
// normal
__device__ __forceinline__ float fp8_row_inv_scale(float s) {
  return 1.0f / fmaxf(s, 0x1p-126f);
}

// 8 packed bf16 values times inv -> 8 e4m3 bytes, channel j in byte j
__device__ __forceinline__ u32x2_t fp8_quant8(const ushort8_t v, float inv) {
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
    f[j] = fminf(fmaxf(bf16_bits_to_f32(v[j]) * inv, -E4M3_MAX), E4M3_MAX);
  // v_cvt_pk_fp8_f32: two fp32 -> two OCP e4m3 bytes, round to nearest
  // even, into the low or high half of a dword
  int w0 = 0, w1 = 0;
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], w0, false);
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w0, true);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], w1, false);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], w1, true);
  return u32x2_t{(unsigned)w0, (unsigned)w1};
}

// fp32 device pointer of an optional per-channel bias for a launcher:
// nullptr when the tensor is undefined or empty. The fp32 copy (the bias
// itself when it already is contiguous fp32) is left in `keep`, which the
// caller holds until the kernel is enqueued.
static inline const float* bias_f32_ptr(const torch::Tensor& bias,
                                        torch::Tensor& keep) {
  if (!bias.defined() || bias.numel() == 0) return nullptr;
  keep = bias.contiguous().to(at::kFloat);
  return keep.data_ptr<float>();
}

// At least 128 zero bytes on `like`'s device: where a kernel redirects the
// loads of out-of-range rows. Intentionally leaked: a static torch::Tensor's
// destructor would run at process exit AFTER the HIP context is torn down.
inline const void* device_zero_page(const torch::Tensor& like) {
  static torch::Tensor* page = nullptr;
  if (!page || page->device() != like.device())
    page = new torch::Tensor(
        torch::zeros({128}, like.options().dtype(at::kByte)));
  return page->data_ptr();
}

#define HIP_CHECK_LAUNCH()                                                  \
  do {                                                                       \
    hipError_t err = hipGetLastError();                                      \
    if (err != hipSuccess) {                                                 \
      TORCH_CHECK(false, "HIP kernel launch failed: ",                       \
                  hipGetErrorString(err));                                   \
    }                                                                        \
  } while (0)
