// Fused normalization kernels for the diffusion hot path (MI355X/gfx950).
//
// The reference delegates these ops to ComfyUI's eager torch stack
// (GroupNorm+SiLU inside UNet/VAE blocks); here they
// are single-pass fused HIP kernels: one workgroup per (batch, group) row,
// fp32 Welford-free two-phase reduction, bf16 I/O vectorized 8-wide (G13),
// normalize+affine+SiLU fused into the same kernel that computed the stats
// (HBM-bound op: one read + one write total).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

// ---------------------------------------------------------------------------
// GroupNorm (+ optional SiLU). Input NCHW bf16, weight/bias fp32 per channel.
// One block per (n, g); elements of a group are Cg contiguous channel planes.
// ---------------------------------------------------------------------------

template <bool FUSE_SILU>
__global__ void groupnorm_kernel(const uint16_t* __restrict__ x,
                                 uint16_t* __restrict__ y,
                                 const float* __restrict__ weight,
                                 const float* __restrict__ bias,
                                 int C, int G, int HW, float eps) {
  const int n = blockIdx.x / G;
  const int g = blockIdx.x % G;
  const int Cg = C / G;
  const long long base = ((long long)n * C + (long long)g * Cg) * HW;
  const long long count = (long long)Cg * HW;

  __shared__ float scratch[16];
  __shared__ float s_mean, s_rstd;

  // Phase 1: sum / sumsq over the group, 8-wide bf16 loads.
  float sum = 0.f, sumsq = 0.f;
  long long i = (long long)threadIdx.x * 8;
  const long long stride = (long long)blockDim.x * 8;
  for (; i + 7 < count; i += stride) {
    ushort8_t v = *reinterpret_cast<const ushort8_t*>(x + base + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = bf16_bits_to_f32(v[j]);
      sum += f;
      sumsq += f * f;
    }
  }
  {  // tail: < 8 elements, one per low thread
    const long long tail_start = (count / 8) * 8;
    const long long k = tail_start + threadIdx.x;
    if (k < count) {
      float f = bf16_bits_to_f32(x[base + k]);
      sum += f;
      sumsq += f * f;
    }
  }
  sum = block_reduce(sum, scratch, SumOp{}, 0.f);
  sumsq = block_reduce(sumsq, scratch, SumOp{}, 0.f);
  if (threadIdx.x == 0) {
    float mean = sum / (float)count;
    float var = sumsq / (float)count - mean * mean;
    s_mean = mean;
    s_rstd = rsqrtf(fmaxf(var, 0.f) + eps);
  }
  __syncthreads();
  const float mean = s_mean, rstd = s_rstd;

  // Phase 2: normalize + affine (+ SiLU), same traversal.
  i = (long long)threadIdx.x * 8;
  for (; i + 7 < count; i += stride) {
    ushort8_t v = *reinterpret_cast<const ushort8_t*>(x + base + i);
    ushort8_t o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      long long idx = i + j;
      int c = (int)(idx / HW) + g * Cg;
      float f = (bf16_bits_to_f32(v[j]) - mean) * rstd;
      f = f * weight[c] + bias[c];
      if (FUSE_SILU) f = silu_f(f);
      o[j] = f32_to_bf16_bits(f);
    }
    *reinterpret_cast<ushort8_t*>(y + base + i) = o;
  }
  {
    const long long tail_start = (count / 8) * 8;
    const long long k = tail_start + threadIdx.x;
    if (k < count) {
      int c = (int)(k / HW) + g * Cg;
      float f = (bf16_bits_to_f32(x[base + k]) - mean) * rstd;
      f = f * weight[c] + bias[c];
      if (FUSE_SILU) f = silu_f(f);
      y[base + k] = f32_to_bf16_bits(f);
    }
  }
}

torch::Tensor group_norm_fused(torch::Tensor x, int64_t groups,
                               torch::Tensor weight, torch::Tensor bias,
                               double eps, bool fuse_silu) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4, "x must be NCHW on device");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "x must be bf16");
  auto xc = x.contiguous();
  auto w = weight.contiguous().to(at::kFloat);
  auto b = bias.contiguous().to(at::kFloat);
  const int N = xc.size(0), C = xc.size(1);
  const int HW = xc.size(2) * xc.size(3);
  TORCH_CHECK(C % groups == 0, "C must divide groups");
  auto y = torch::empty_like(xc);
  dim3 grid(N * groups);
  // few groups + huge spatial (VAE decode output) starves the chip at 256
  // threads x few blocks; scale the block up instead
  const long long per_group = (long long)(C / groups) * HW;
  dim3 block(N * groups >= 128 ? 256 : (per_group > (1 << 20) ? 1024 : 256));
  auto stream = at::hip::getCurrentHIPStream();
  if (fuse_silu)
    hipLaunchKernelGGL((groupnorm_kernel<true>), grid, block, 0, stream,
                       (const uint16_t*)xc.data_ptr(), (uint16_t*)y.data_ptr(),
                       w.data_ptr<float>(), b.data_ptr<float>(), C, (int)groups,
                       HW, (float)eps);
  else
    hipLaunchKernelGGL((groupnorm_kernel<false>), grid, block, 0, stream,
                       (const uint16_t*)xc.data_ptr(), (uint16_t*)y.data_ptr(),
                       w.data_ptr<float>(), b.data_ptr<float>(), C, (int)groups,
                       HW, (float)eps);
  HIP_CHECK_LAUNCH();
  return y;
}

// ---------------------------------------------------------------------------
// LayerNorm over the last dim. x: [T, C] bf16 (rows = flattened tokens),
// gamma/beta fp32. One wave per row for C <= 2048, one block per row above.
// ---------------------------------------------------------------------------

__global__ void layernorm_wave_kernel(const uint16_t* __restrict__ x,
                                      uint16_t* __restrict__ y,
                                      const float* __restrict__ gamma,
                                      const float* __restrict__ beta,
                                      int C, long long nrows, float eps) {
  const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= nrows) return;
  const int lane = threadIdx.x & 63;
  const long long base = row * C;

  float sum = 0.f, sumsq = 0.f;
  for (int i = lane * 8; i + 7 < C; i += 64 * 8) {
    ushort8_t v = *reinterpret_cast<const ushort8_t*>(x + base + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = bf16_bits_to_f32(v[j]);
      sum += f;
      sumsq += f * f;
    }
  }
  // tail (C not multiple of 512): scalar, owned by lane (c/8)%64
  const int tail_start = (C / 8) * 8;
  for (int c = tail_start + lane; c < C; c += 64) {
    float f = bf16_bits_to_f32(x[base + c]);
    sum += f;
    sumsq += f * f;
  }
  sum = wave_reduce_sum(sum);
  sumsq = wave_reduce_sum(sumsq);
  const float mean = sum / C;
  const float rstd = rsqrtf(fmaxf(sumsq / C - mean * mean, 0.f) + eps);

  for (int i = lane * 8; i + 7 < C; i += 64 * 8) {
    ushort8_t v = *reinterpret_cast<const ushort8_t*>(x + base + i);
    ushort8_t o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = (bf16_bits_to_f32(v[j]) - mean) * rstd;
      o[j] = f32_to_bf16_bits(f * gamma[i + j] + beta[i + j]);
    }
    *reinterpret_cast<ushort8_t*>(y + base + i) = o;
  }
  for (int c = tail_start + lane; c < C; c += 64) {
    float f = (bf16_bits_to_f32(x[base + c]) - mean) * rstd;
    y[base + c] = f32_to_bf16_bits(f * gamma[c] + beta[c]);
  }
}

torch::Tensor layer_norm_bf16(torch::Tensor x, torch::Tensor gamma,
                              torch::Tensor beta, double eps) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16);
  auto xc = x.contiguous();
  const int C = xc.size(-1);
  const long long T = xc.numel() / C;
  auto g = gamma.contiguous().to(at::kFloat);
  auto b = beta.contiguous().to(at::kFloat);
  auto y = torch::empty_like(xc);
  // 4 waves per block, one wave per row.
  const int waves_per_block = 4;
  dim3 block(64 * waves_per_block);
  dim3 grid((unsigned)((T + waves_per_block - 1) / waves_per_block));
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(layernorm_wave_kernel, grid, block, 0, stream,
                     (const uint16_t*)xc.data_ptr(), (uint16_t*)y.data_ptr(),
                     g.data_ptr<float>(), b.data_ptr<float>(), C, T, (float)eps);
  HIP_CHECK_LAUNCH();
  return y;
}

// ---------------------------------------------------------------------------
// GEGLU / SiLU-mul: out = a * act(b), bf16, elementwise 8-wide.
// ---------------------------------------------------------------------------

template <bool GELU>
__global__ void act_mul_kernel(const uint16_t* __restrict__ a,
                               const uint16_t* __restrict__ b,
                               uint16_t* __restrict__ y, long long n) {
  long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  const long long stride = (long long)gridDim.x * blockDim.x * 8;
  for (; i + 7 < n; i += stride) {
    ushort8_t va = *reinterpret_cast<const ushort8_t*>(a + i);
    ushort8_t vb = *reinterpret_cast<const ushort8_t*>(b + i);
    ushort8_t o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float fb = bf16_bits_to_f32(vb[j]);
      float act = GELU ? 0.5f * fb * (1.f + tanhf(0.7978845608f * (fb + 0.044715f * fb * fb * fb)))
                       : silu_f(fb);
      o[j] = f32_to_bf16_bits(bf16_bits_to_f32(va[j]) * act);
    }
    *reinterpret_cast<ushort8_t*>(y + i) = o;
  }
  if (blockIdx.x == 0 && threadIdx.x < 8) {
    for (long long k = (n / 8) * 8 + threadIdx.x; k < n; k += 8) {
      float fb = bf16_bits_to_f32(b[k]);
      float act = GELU ? 0.5f * fb * (1.f + tanhf(0.7978845608f * (fb + 0.044715f * fb * fb * fb)))
                       : silu_f(fb);
      y[k] = f32_to_bf16_bits(bf16_bits_to_f32(a[k]) * act);
    }
  }
}

// Row-strided operands read in place: a and b are [rows, cols] views with a
// contiguous last dim and their own row pitch (the two chunk(2, -1) halves
// of a GEGLU projection: pitch 2*cols, b starting cols elements in); y is
// contiguous. cols8 = cols / 8; rows * cols8 < 2^32.
template <bool GELU>
__global__ void act_mul_rows_kernel(const uint16_t* __restrict__ a,
                                    const uint16_t* __restrict__ b,
                                    uint16_t* __restrict__ y,
                                    unsigned nvec, unsigned cols8,
                                    long long pitch_a, long long pitch_b) {
  const unsigned stride = gridDim.x * blockDim.x;
  // nvec + stride may pass 2^32: count the trips in 64 bits
  for (unsigned long long i = blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += stride) {
    const unsigned v = (unsigned)i;
    const unsigned row = v / cols8;
    const unsigned col = (v - row * cols8) << 3;
    ushort8_t va = *reinterpret_cast<const ushort8_t*>(a + row * pitch_a + col);
    ushort8_t vb = *reinterpret_cast<const ushort8_t*>(b + row * pitch_b + col);
    ushort8_t o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float fb = bf16_bits_to_f32(vb[j]);
      float act = GELU ? 0.5f * fb * (1.f + tanhf(0.7978845608f * (fb + 0.044715f * fb * fb * fb)))
                       : silu_f(fb);
      o[j] = f32_to_bf16_bits(bf16_bits_to_f32(va[j]) * act);
    }
    *reinterpret_cast<ushort8_t*>(y + ((unsigned long long)v << 3)) = o;
  }
}

// True when t's outer dims collapse to one row index with one pitch and 16-byte
// loads can read its rows in place: last dim contiguous and a multiple of 8
// long, every outer stride and the start a multiple of 8 elements.
static bool act_mul_row_view(const torch::Tensor& t, long long* pitch) {
  const int64_t d = t.dim();
  if (d < 1 || t.numel() == 0) return false;
  const int64_t cols = t.size(d - 1);
  if (cols % 8 != 0 || (cols > 1 && t.stride(d - 1) != 1)) return false;
  if (t.storage_offset() % 8 != 0
      || reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 != 0)
    return false;
  // innermost outer dim of size > 1 sets the pitch; every dim above it must
  // continue it (stride[i] == stride[i+1] * size[i+1])
  long long p = cols, span = 0;
  bool have = false;
  for (int64_t i = d - 2; i >= 0; --i) {
    if (t.size(i) == 1) continue;
    if (!have) {
      p = t.stride(i);
      span = p * t.size(i);
      have = true;
    } else {
      if (t.stride(i) != span) return false;
      span *= t.size(i);
    }
    if (t.stride(i) % 8 != 0 || t.stride(i) < cols) return false;
  }
  *pitch = p;
  return true;
}

torch::Tensor act_mul_bf16(torch::Tensor a, torch::Tensor b, bool gelu) {
  TORCH_CHECK(a.is_cuda() && a.scalar_type() == at::kBFloat16);
  TORCH_CHECK(b.is_cuda() && b.scalar_type() == at::kBFloat16);
  TORCH_CHECK(a.sizes() == b.sizes());
  long long pitch_a = 0, pitch_b = 0;
  if (!(a.is_contiguous() && b.is_contiguous())
      && act_mul_row_view(a, &pitch_a) && act_mul_row_view(b, &pitch_b)
      && a.numel() / 8 < (1LL << 32)) {
    const long long cols = a.size(-1);
    const long long nvec = a.numel() / 8;
    auto y = torch::empty(a.sizes(), a.options());
    int blocks = (int)std::min<long long>((nvec + 255) / 256, 2048);
    auto stream = at::hip::getCurrentHIPStream();
    if (gelu)
      hipLaunchKernelGGL((act_mul_rows_kernel<true>), dim3(blocks), dim3(256),
                         0, stream, (const uint16_t*)a.data_ptr(),
                         (const uint16_t*)b.data_ptr(), (uint16_t*)y.data_ptr(),
                         (unsigned)nvec, (unsigned)(cols / 8), pitch_a, pitch_b);
    else
      hipLaunchKernelGGL((act_mul_rows_kernel<false>), dim3(blocks), dim3(256),
                         0, stream, (const uint16_t*)a.data_ptr(),
                         (const uint16_t*)b.data_ptr(), (uint16_t*)y.data_ptr(),
                         (unsigned)nvec, (unsigned)(cols / 8), pitch_a, pitch_b);
    HIP_CHECK_LAUNCH();
    return y;
  }
  auto ac = a.contiguous(), bc = b.contiguous();
  auto y = torch::empty_like(ac);
  long long n = ac.numel();
  int blocks = (int)std::min<long long>((n / 8 + 255) / 256 + 1, 2048);
  auto stream = at::hip::getCurrentHIPStream();
  if (gelu)
    hipLaunchKernelGGL((act_mul_kernel<true>), dim3(blocks), dim3(256), 0,
                       stream, (const uint16_t*)ac.data_ptr(),
                       (const uint16_t*)bc.data_ptr(), (uint16_t*)y.data_ptr(), n);
  else
    hipLaunchKernelGGL((act_mul_kernel<false>), dim3(blocks), dim3(256), 0,
                       stream, (const uint16_t*)ac.data_ptr(),
                       (const uint16_t*)bc.data_ptr(), (uint16_t*)y.data_ptr(), n);
  HIP_CHECK_LAUNCH();
  return y;
}
