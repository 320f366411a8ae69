// Fused glue kernels for the DiT families (WAN / Flux) on MI355X/gfx950:
// everything that sits between the attention kernel and the hipBLASLt
// Linears in a transformer block.
//
//   qk_norm_rope    per-head RMSNorm + rotary embedding of q and k, one launch
//   norm_modulate   row RMSNorm / LayerNorm + adaLN (1 + scale) / shift
//   norm_modulate_fp8   the same, stored as e4m3 rows + fp32 row scales for
//                   the FP8 Linears (gemm_fp8.hip) the norm feeds
//   gated_residual  x + gate[b] * y
//
// Same conventions as norms.hip: bf16 I/O through 16-byte ushort8_t
// accesses, fp32 math with one rounding on store, long long row offsets,
// launched on the current stream with no host sync (graph-capture safe).
// All three are HBM-bound: one read of every input, one write of the output.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

// ---------------------------------------------------------------------------
// qk_norm_rope. q/k: [B, N, H*D] bf16 views (last dim contiguous, batch/row
// strides in elements), read in place out of a fused projection output.
// One lane owns 8 consecutive channels (4 rotary pairs); a head is a group
// of G lanes, G = D/8 rounded up to a power of two, and the sum of squares
// is reduced with width-G shuffles. blockIdx.y selects q (0) or k (1).
// Input row n goes to output row token_offset + n and is rotated with table
// row token_offset + n; other output rows are not touched.
// ---------------------------------------------------------------------------

struct QkSide {
  const uint16_t* x;
  const float* w;
  uint16_t* out;
  long long stride_b, stride_n;  // input strides, elements
};

template <int G>
__global__ void qk_norm_rope_kernel(QkSide q, QkSide k,
                                    const float* __restrict__ cos,
                                    const float* __restrict__ sin,
                                    int N, int H, int D, int Ntot,
                                    int token_offset, long long ngroups,
                                    float eps) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long group = t / G;
  // G divides the wave, so this exits whole groups only: every lane that
  // reaches the shuffles below has its G-1 partners with it
  if (group >= ngroups) return;
  const int c0 = (int)(t % G) * 8;
  const bool active = c0 < D;  // padded lanes of a non-power-of-two group
  const QkSide s = blockIdx.y == 0 ? q : k;

  const int h = (int)(group % H);
  const long long row = group / H;
  const int n = (int)(row % N);
  const long long b = row / N;

  float f[8];
  float sumsq = 0.f;
  if (active) {
    const ushort8_t v = *reinterpret_cast<const ushort8_t*>(
        s.x + b * s.stride_b + (long long)n * s.stride_n + (long long)h * D + c0);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f[j] = bf16_bits_to_f32(v[j]);
      sumsq += f[j] * f[j];
    }
  }
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) sumsq += __shfl_xor(sumsq, off, G);
  if (!active) return;
  const float rstd = rsqrtf(sumsq / (float)D + eps);

  const float4_t w0 = *reinterpret_cast<const float4_t*>(s.w + c0);
  const float4_t w1 = *reinterpret_cast<const float4_t*>(s.w + c0 + 4);
  const long long pos = (long long)token_offset + n;
  const long long tab = pos * (D / 2) + c0 / 2;
  const float4_t c = *reinterpret_cast<const float4_t*>(cos + tab);
  const float4_t sn = *reinterpret_cast<const float4_t*>(sin + tab);

  ushort8_t o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float y0 = f[2 * i] * rstd * (i < 2 ? w0[2 * i] : w1[2 * i - 4]);
    const float y1 = f[2 * i + 1] * rstd * (i < 2 ? w0[2 * i + 1] : w1[2 * i - 3]);
    o[2 * i] = f32_to_bf16_bits(y0 * c[i] - y1 * sn[i]);
    o[2 * i + 1] = f32_to_bf16_bits(y0 * sn[i] + y1 * c[i]);
  }
  *reinterpret_cast<ushort8_t*>(
      s.out + ((b * Ntot + pos) * H + h) * (long long)D + c0) = o;
}

// every tensor here is touched with 16-byte accesses
static void check_aligned16(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
              " must start on a 16-byte boundary");
}

static void check_qk_view(const torch::Tensor& x, const char* name) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3, name, " must be [B, N, H*D] on device");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, name, " must be bf16");
  TORCH_CHECK(x.stride(2) == 1, name, ": last dim must be contiguous");
  TORCH_CHECK(x.stride(0) % 8 == 0 && x.stride(1) % 8 == 0 &&
                  x.storage_offset() % 8 == 0,
              name, ": strides and start offset must be multiples of 8 elements");
  check_aligned16(x, name);
}

void qk_norm_rope(torch::Tensor q, torch::Tensor k, torch::Tensor q_weight,
                  torch::Tensor k_weight, torch::Tensor cos, torch::Tensor sin,
                  torch::Tensor out_q, torch::Tensor out_k, int64_t heads,
                  double eps, int64_t token_offset) {
  check_qk_view(q, "q");
  check_qk_view(k, "k");
  TORCH_CHECK(q.sizes() == k.sizes(), "q and k must have the same shape");
  const long long B = q.size(0), N = q.size(1), HD = q.size(2);
  TORCH_CHECK(heads > 0 && HD % heads == 0, "H*D must divide heads");
  const int H = (int)heads, D = (int)(HD / heads);
  TORCH_CHECK(D % 8 == 0 && D >= 16 && D <= 256,
              "head dim must be a multiple of 8 in [16, 256], got ", D);
  for (const torch::Tensor* w : {&q_weight, &k_weight})
    TORCH_CHECK(w->is_cuda() && w->scalar_type() == at::kFloat &&
                    w->is_contiguous() && w->numel() == D,
                "q_weight/k_weight must be contiguous fp32 [D]");
  for (const torch::Tensor* o : {&out_q, &out_k})
    TORCH_CHECK(o->is_cuda() && o->scalar_type() == at::kBFloat16 &&
                    o->is_contiguous() && o->dim() == 3 && o->size(0) == B &&
                    o->size(2) == HD && o->size(1) == out_q.size(1),
                "out_q/out_k must be contiguous bf16 [B, Ntot, H*D]");
  const long long Ntot = out_q.size(1);
  TORCH_CHECK(token_offset >= 0 && token_offset + N <= Ntot,
              "token window [", token_offset, ", ", token_offset + N,
              ") exceeds the output's ", Ntot, " rows");
  for (const torch::Tensor* t : {&cos, &sin})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat &&
                    t->is_contiguous() && t->dim() == 2 &&
                    t->size(1) == D / 2 && t->size(0) >= token_offset + N,
                "cos/sin must be contiguous fp32 [Npos >= token_offset + N, D/2]");
  TORCH_CHECK(Ntot < (1LL << 31) && N < (1LL << 31));
  for (const torch::Tensor* t :
       {&q_weight, &k_weight, &cos, &sin, &out_q, &out_k})
    check_aligned16(*t, "qk_norm_rope operand");
  const long long ngroups = B * N * H;
  if (ngroups == 0) return;

  QkSide sq{(const uint16_t*)q.data_ptr(), q_weight.data_ptr<float>(),
            (uint16_t*)out_q.data_ptr(), q.stride(0), q.stride(1)};
  QkSide sk{(const uint16_t*)k.data_ptr(), k_weight.data_ptr<float>(),
            (uint16_t*)out_k.data_ptr(), k.stride(0), k.stride(1)};
  int G = 2;
  while (G * 8 < D) G <<= 1;
  const int threads = 256;
  const long long nblocks = (ngroups * G + threads - 1) / threads;
  TORCH_CHECK(nblocks < (1LL << 31), "qk_norm_rope: too many tokens");
  dim3 grid((unsigned)nblocks, 2), block(threads);
  auto stream = at::hip::getCurrentHIPStream();
#define LAUNCH_QK(GV)                                                          \
  hipLaunchKernelGGL((qk_norm_rope_kernel<GV>), grid, block, 0, stream, sq,   \
                     sk, cos.data_ptr<float>(), sin.data_ptr<float>(), (int)N, \
                     H, D, (int)Ntot, (int)token_offset, ngroups, (float)eps)
  switch (G) {
    case 2: LAUNCH_QK(2); break;
    case 4: LAUNCH_QK(4); break;
    case 8: LAUNCH_QK(8); break;
    case 16: LAUNCH_QK(16); break;
    default: LAUNCH_QK(32); break;
  }
#undef LAUNCH_QK
  HIP_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------
// norm_modulate. x: [T, C] bf16 rows (T = B*N), one wave per row. The row
// is loaded from HBM once into registers (ITERS statically unrolled 16-byte
// chunks per lane, so the array never becomes runtime-indexed scratch); both
// the statistics and the normalise pass read those registers. LAYER mode
// takes the variance around the mean from the registers (no sumsq - mean^2
// cancellation). scale/shift: [B, C] bf16 rows with a row stride, b = row / N.
//
// FP8 = false stores the bf16 row to y. FP8 = true is norm_modulate_fp8,
// defined as quant_rows_fp8 of that bf16 row: each chunk's bf16-rounded
// result goes back into the packed registers it came from, the row absmax is
// a second wave reduction over them, and the e4m3 bytes go to q (8 bytes per
// lane per chunk) with the row's fp32 scale in fp8.scale[row]; y is not read.
// The scale and the conversion are common.h's, shared with
// quant_rows_fp8_kernel, so the two paths give the same bytes.
// ---------------------------------------------------------------------------

// Where the FP8 tail writes. The last kernel argument; empty without FP8,
// which leaves the arguments of the bf16 instantiations laid out as they
// are without it.
template <bool FP8> struct NormFp8Out {};
template <> struct NormFp8Out<true> {
  uint8_t* q;     // [T, C] e4m3
  float* scale;   // [T]
};

template <int ITERS, bool LAYER, bool FP8>
__global__ void __launch_bounds__(256)
norm_modulate_kernel(const uint16_t* __restrict__ x, uint16_t* __restrict__ y,
                     const float* __restrict__ weight,
                     const uint16_t* __restrict__ scale,
                     const uint16_t* __restrict__ shift,
                     long long scale_stride, long long shift_stride, int C,
                     int N, long long nrows, float eps,
                     const NormFp8Out<FP8> fp8) {
  const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= nrows) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const long long base = row * C;

  // the row stays packed (4 VGPRs per chunk); widening is one shift per use
  ushort8_t v[ITERS];
  float sum = 0.f;
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int i = (it * 64 + lane) * 8;
    if (i < C) {
      v[it] = *reinterpret_cast<const ushort8_t*>(x + base + i);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = bf16_bits_to_f32(v[it][j]);
        sum += LAYER ? f : f * f;
      }
    }
  }
  sum = wave_reduce_sum(sum);
  float mean = 0.f, rstd;
  if (LAYER) {
    mean = sum / C;
    float var = 0.f;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      if ((it * 64 + lane) * 8 < C) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float d = bf16_bits_to_f32(v[it][j]) - mean;
          var += d * d;
        }
      }
    }
    var = wave_reduce_sum(var);
    rstd = rsqrtf(var / C + eps);
  } else {
    rstd = rsqrtf(sum / C + eps);
  }

  const long long b = row / N;
  const uint16_t* sc = scale ? scale + b * scale_stride : nullptr;
  const uint16_t* sh = shift ? shift + b * shift_stride : nullptr;
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int i = (it * 64 + lane) * 8;
    if (i < C) {
      float g[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        g[j] = (bf16_bits_to_f32(v[it][j]) - mean) * rstd;
      if (!LAYER) {
        const float4_t w0 = *reinterpret_cast<const float4_t*>(weight + i);
        const float4_t w1 = *reinterpret_cast<const float4_t*>(weight + i + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          g[j] *= w0[j];
          g[j + 4] *= w1[j];
        }
      }
      if (sc) {
        const ushort8_t vs = *reinterpret_cast<const ushort8_t*>(sc + i);
        const ushort8_t vh = *reinterpret_cast<const ushort8_t*>(sh + i);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          g[j] = g[j] * (1.f + bf16_bits_to_f32(vs[j])) + bf16_bits_to_f32(vh[j]);
      }
      ushort8_t o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = f32_to_bf16_bits(g[j]);
      if constexpr (FP8)
        v[it] = o;  // the bf16 row replaces the input row it was made from
      else
        *reinterpret_cast<ushort8_t*>(y + base + i) = o;
    }
  }

  if constexpr (FP8) {
    // idle lanes and chunks hold nothing and contribute 0
    float amax = 0.f;
#pragma unroll
    for (int it = 0; it < ITERS; ++it)
      if ((it * 64 + lane) * 8 < C) amax = fp8_absmax8(v[it], amax);
    amax = wave_reduce_max(amax);
    const float s = fp8_row_scale(amax);
    const float inv = fp8_row_inv_scale(s);
    if (lane == 0) fp8.scale[row] = s;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int i = (it * 64 + lane) * 8;
      if (i < C)
        *reinterpret_cast<u32x2_t*>(fp8.q + base + i) = fp8_quant8(v[it], inv);
    }
  }
}

static void check_mod_view(const torch::Tensor& m, long long B, long long C,
                           const char* name) {
  TORCH_CHECK(m.is_cuda() && m.scalar_type() == at::kBFloat16 && m.dim() == 2 &&
                  m.size(0) == B && m.size(1) == C,
              name, " must be a bf16 [B, C] view on device");
  TORCH_CHECK(m.stride(1) == 1 && m.stride(0) % 8 == 0 &&
                  m.storage_offset() % 8 == 0,
              name, ": last dim contiguous, row stride and start offset "
                    "multiples of 8 elements");
  check_aligned16(m, name);
}

// The argument contract both entry points share. weight: fp32 [C] selects
// RMSNorm, an empty tensor the affine-free LayerNorm. scale/shift: both
// [B, C] or both empty (no modulation).
static void check_norm_modulate(const torch::Tensor& x,
                                const torch::Tensor& weight,
                                const torch::Tensor& scale,
                                const torch::Tensor& shift) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3 && x.is_contiguous(),
              "x must be contiguous [B, N, C] on device");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "x must be bf16");
  const long long B = x.size(0), N = x.size(1), C = x.size(2);
  TORCH_CHECK(C % 8 == 0 && C >= 8 && C <= 8192,
              "C must be a multiple of 8 in [8, 8192], got ", C);
  TORCH_CHECK(N < (1LL << 31));
  const bool layer = weight.numel() == 0;
  if (!layer)
    TORCH_CHECK(weight.is_cuda() && weight.scalar_type() == at::kFloat &&
                    weight.is_contiguous() && weight.numel() == C,
                "weight must be contiguous fp32 [C]");
  check_aligned16(x, "x");
  if (!layer) check_aligned16(weight, "weight");
  const bool has_mod = scale.numel() != 0;
  TORCH_CHECK(has_mod == (shift.numel() != 0),
              "scale and shift come together");
  if (has_mod) {
    check_mod_view(scale, B, C, "scale");
    check_mod_view(shift, B, C, "shift");
  }
}

// One wave per row, 4 rows per block. The arguments are checked; y is the
// bf16 output, or null with FP8.
template <bool FP8>
static void launch_norm_modulate(const torch::Tensor& x,
                                 const torch::Tensor& weight,
                                 const torch::Tensor& scale,
                                 const torch::Tensor& shift, double eps,
                                 uint16_t* y, const NormFp8Out<FP8> fp8) {
  const long long B = x.size(0), N = x.size(1), C = x.size(2);
  const bool layer = weight.numel() == 0;
  const bool has_mod = scale.numel() != 0;
  const long long T = B * N;
  if (T == 0) return;

  const int waves_per_block = 4;
  dim3 block(64 * waves_per_block);
  const long long nblocks = (T + waves_per_block - 1) / waves_per_block;
  TORCH_CHECK(nblocks < (1LL << 31), "norm_modulate: too many rows");
  dim3 grid((unsigned)nblocks);
  auto stream = at::hip::getCurrentHIPStream();
  const uint16_t* sc = has_mod ? (const uint16_t*)scale.data_ptr() : nullptr;
  const uint16_t* sh = has_mod ? (const uint16_t*)shift.data_ptr() : nullptr;
  const long long sc_stride = has_mod ? scale.stride(0) : 0;
  const long long sh_stride = has_mod ? shift.stride(0) : 0;
  const float* w = layer ? nullptr : weight.data_ptr<float>();
#define LAUNCH_NM(IT)                                                          \
  do {                                                                         \
    if (layer)                                                                 \
      hipLaunchKernelGGL((norm_modulate_kernel<IT, true, FP8>), grid, block,   \
                         0, stream, (const uint16_t*)x.data_ptr(), y, w, sc,   \
                         sh, sc_stride, sh_stride, (int)C, (int)N, T,          \
                         (float)eps, fp8);                                     \
    else                                                                       \
      hipLaunchKernelGGL((norm_modulate_kernel<IT, false, FP8>), grid, block,  \
                         0, stream, (const uint16_t*)x.data_ptr(), y, w, sc,   \
                         sh, sc_stride, sh_stride, (int)C, (int)N, T,          \
                         (float)eps, fp8);                                     \
  } while (0)
  // 512 channels per unrolled chunk; pick the smallest instantiation
  const int iters = (int)((C + 511) / 512);
  if (iters <= 1) LAUNCH_NM(1);
  else if (iters <= 2) LAUNCH_NM(2);
  else if (iters <= 4) LAUNCH_NM(4);
  else if (iters <= 6) LAUNCH_NM(6);
  else if (iters <= 8) LAUNCH_NM(8);
  else if (iters <= 10) LAUNCH_NM(10);
  else if (iters <= 12) LAUNCH_NM(12);
  else LAUNCH_NM(16);
#undef LAUNCH_NM
  HIP_CHECK_LAUNCH();
}

torch::Tensor norm_modulate(torch::Tensor x, torch::Tensor weight,
                            torch::Tensor scale, torch::Tensor shift,
                            double eps) {
  check_norm_modulate(x, weight, scale, shift);
  auto y = torch::empty_like(x);
  launch_norm_modulate<false>(x, weight, scale, shift, eps,
                              (uint16_t*)y.data_ptr(), NormFp8Out<false>{});
  return y;
}

// quant_rows_fp8(norm_modulate(x, ...)) in one launch: (q [B, N, C]
// float8_e4m3fn, scale [B, N] fp32). C % 128 == 0 and 128 <= C <= 8192: the
// FP8 GEMM's K contract within the row the kernel holds in registers.
std::tuple<torch::Tensor, torch::Tensor> norm_modulate_fp8(
    torch::Tensor x, torch::Tensor weight, torch::Tensor scale,
    torch::Tensor shift, double eps) {
  check_norm_modulate(x, weight, scale, shift);
  const long long C = x.size(2);
  TORCH_CHECK(C % 128 == 0 && C >= 128,
              "C must be a multiple of 128 in [128, 8192], got ", C);
  auto q = torch::empty(x.sizes(), x.options().dtype(at::kFloat8_e4m3fn));
  auto qscale =
      torch::empty({x.size(0), x.size(1)}, x.options().dtype(at::kFloat));
  launch_norm_modulate<true>(
      x, weight, scale, shift, eps, nullptr,
      NormFp8Out<true>{(uint8_t*)q.data_ptr(), qscale.data_ptr<float>()});
  return {q, qscale};
}

// ---------------------------------------------------------------------------
// gated_residual: out = x + gate[b] * y. x, y: [B, N, C] bf16 contiguous,
// gate: [B, C] bf16 rows with a row stride. C % 8 == 0 keeps every 8-wide
// chunk inside one row, so the flat length has no sub-8 tail.
// ---------------------------------------------------------------------------

__global__ void gated_residual_kernel(const uint16_t* __restrict__ x,
                                      const uint16_t* __restrict__ y,
                                      const uint16_t* __restrict__ gate,
                                      uint16_t* __restrict__ out,
                                      long long gate_stride, int C,
                                      long long per_batch, long long n) {
  long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  const long long stride = (long long)gridDim.x * blockDim.x * 8;
  for (; i + 7 < n; i += stride) {
    const long long b = i / per_batch;
    const int c = (int)(i % C);
    const ushort8_t vx = *reinterpret_cast<const ushort8_t*>(x + i);
    const ushort8_t vy = *reinterpret_cast<const ushort8_t*>(y + i);
    const ushort8_t vg =
        *reinterpret_cast<const ushort8_t*>(gate + b * gate_stride + c);
    ushort8_t o;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      o[j] = f32_to_bf16_bits(bf16_bits_to_f32(vx[j]) +
                              bf16_bits_to_f32(vg[j]) * bf16_bits_to_f32(vy[j]));
    *reinterpret_cast<ushort8_t*>(out + i) = o;
  }
}

torch::Tensor gated_residual(torch::Tensor x, torch::Tensor gate,
                             torch::Tensor y) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3 && x.is_contiguous() &&
                  x.scalar_type() == at::kBFloat16,
              "x must be contiguous bf16 [B, N, C] on device");
  TORCH_CHECK(y.is_cuda() && y.is_contiguous() &&
                  y.scalar_type() == at::kBFloat16 && y.sizes() == x.sizes(),
              "y must match x");
  const long long B = x.size(0), N = x.size(1), C = x.size(2);
  TORCH_CHECK(C % 8 == 0 && C < (1LL << 31), "C must be a multiple of 8, got ", C);
  check_mod_view(gate, B, C, "gate");
  check_aligned16(x, "x");
  check_aligned16(y, "y");
  auto out = torch::empty_like(x);
  const long long n = x.numel();
  if (n == 0) return out;
  const int blocks = (int)std::min<long long>((n / 8 + 255) / 256, 4096);
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(gated_residual_kernel, dim3(blocks), dim3(256), 0, stream,
                     (const uint16_t*)x.data_ptr(), (const uint16_t*)y.data_ptr(),
                     (const uint16_t*)gate.data_ptr(), (uint16_t*)out.data_ptr(),
                     (long long)gate.stride(0), (int)C, N * C, n);
  HIP_CHECK_LAUNCH();
  return out;
}
