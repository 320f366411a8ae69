// Fused normalization kernels for the diffusion hot path (MI355X/gfx950).
//
// The reference delegates these ops to ComfyUI's eager torch stack
// (GroupNorm+SiLU inside UNet/VAE blocks); here they
// are fused HIP kernels with bf16 I/O vectorized 8-wide (G13) and fp32
// statistics (sum and sum of squares, var = E[x^2] - mean^2):
//  - GroupNorm, one workgroup per (batch, group): groupnorm_kernel (NCHW)
//    and groupnorm_nhwc_kernel (NHWC shapes the two-pass kernels do not
//    take). Statistics and normalize+affine+SiLU in the same kernel; the two
//    differ only in how they walk a group (gn_block_stats, gn_finish);
//  - GroupNorm NHWC, the UNet/VAE hot path (gn_stats_kernel,
//    gn_finalize_kernel, gn_apply_kernel): two coalesced passes over the
//    tensor, many workgroups per image, optional per-sample addend;
//  - LayerNorm: one wave per row;
//  - act_mul (SiLU-mul / GEGLU): elementwise.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <type_traits>
#include "common.h"

// ---------------------------------------------------------------------------
// Host helpers shared by the launchers below.
// ---------------------------------------------------------------------------

// A launcher's runtime bool as the compile-time constant a kernel template
// wants: f(std::true_type{}) or f(std::false_type{}). Every kernel launch
// below is written once, inside such an f.
template <typename F>
static void with_bool(bool v, F&& f) {
  if (v) f(std::true_type{});
  else f(std::false_type{});
}

// Contiguous fp32 copy of a per-channel parameter (the tensor itself when it
// already is one). The kernels index it with every channel of x and check
// nothing, so a short or host-side tensor is refused here.
static torch::Tensor param_f32(const torch::Tensor& t, const torch::Tensor& x,
                               int64_t C, const char* name) {
  TORCH_CHECK(t.defined() && t.device() == x.device() && t.numel() == C, name,
              " must have ", C, " elements on x's device");
  return t.contiguous().to(at::kFloat);
}

// ---------------------------------------------------------------------------
// GroupNorm (+ optional SiLU), one block per (n, g). Input bf16, weight/bias
// fp32 per channel. NCHW: a group is Cg contiguous channel planes, walked as
// one flat range. NHWC: a group is Cg contiguous channels of every pixel
// (Cg*2 bytes at a pitch of C*2), walked pixel by pixel.
// ---------------------------------------------------------------------------

// Block size: few groups + huge spatial (VAE decode output) starves the chip
// at 256 threads x few blocks; scale the block up instead.
static int gn_row_block_threads(long long rows, long long per_group) {
  return rows >= 128 ? 256 : (per_group > (1 << 20) ? 1024 : 256);
}

// Every thread's partial (sum, sumsq) over `count` elements -> the group's
// (mean, rstd) in every thread.
__device__ __forceinline__ void gn_block_stats(float sum, float sumsq,
                                               float count, float eps,
                                               float& mean, float& rstd) {
  __shared__ float scratch[16];
  __shared__ float s_mean, s_rstd;
  sum = block_reduce(sum, scratch, SumOp{}, 0.f);
  sumsq = block_reduce(sumsq, scratch, SumOp{}, 0.f);
  if (threadIdx.x == 0) {
    float m = sum / count;
    float var = sumsq / count - m * m;
    s_mean = m;
    s_rstd = rsqrtf(fmaxf(var, 0.f) + eps);
  }
  __syncthreads();
  mean = s_mean;
  rstd = s_rstd;
}

// One element of channel c: normalize, affine, optional SiLU, round to bf16.
// weight[c] and bias[c] are loaded here, after the subtraction, not handed in
// as values or references: either moves the loads and the NCHW kernel's tail
// comes out in another instruction order (profiles/r13_norms.md).
template <bool FUSE_SILU>
__device__ __forceinline__ uint16_t gn_finish(uint16_t x, float mean,
                                              float rstd, const float* weight,
                                              const float* bias, int c) {
  float f = (bf16_bits_to_f32(x) - mean) * rstd;
  f = f * weight[c] + bias[c];
  if (FUSE_SILU) f = silu_f(f);
  return f32_to_bf16_bits(f);
}

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
  float mean, rstd;
  gn_block_stats(sum, sumsq, (float)count, eps, mean, rstd);

  // Phase 2: normalize + affine (+ SiLU), same traversal.
  i = (long long)threadIdx.x * 8;
  for (; i + 7 < count; i += stride) {
    ushort8_t v = *reinterpret_cast<const ushort8_t*>(x + base + i);
    ushort8_t o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      long long idx = i + j;
      int c = (int)(idx / HW) + g * Cg;
      o[j] = gn_finish<FUSE_SILU>(v[j], mean, rstd, weight, bias, c);
    }
    *reinterpret_cast<ushort8_t*>(y + base + i) = o;
  }
  {
    const long long tail_start = (count / 8) * 8;
    const long long k = tail_start + threadIdx.x;
    if (k < count) {
      int c = (int)(k / HW) + g * Cg;
      y[base + k] =
          gn_finish<FUSE_SILU>(x[base + k], mean, rstd, weight, bias, c);
    }
  }
}

template <bool FUSE_SILU>
__global__ void groupnorm_nhwc_kernel(const uint16_t* __restrict__ x,
                                      uint16_t* __restrict__ y,
                                      const float* __restrict__ weight,
                                      const float* __restrict__ bias,
                                      int C, int G, long long HW, float eps) {
  const int n = blockIdx.x / G;
  const int g = blockIdx.x % G;
  const int Cg = C / G;
  const long long base = (long long)n * HW * C + (long long)g * Cg;

  float sum = 0.f, sumsq = 0.f;
  // per-pixel traversal: each thread reads its pixel's Cg contiguous
  // channels (vector-8 where possible) — measured faster than a
  // flat-index scheme whose per-element divisions dominate
  for (long long pp = threadIdx.x; pp < HW; pp += blockDim.x) {
    const uint16_t* px = x + base + pp * C;
    int c = 0;
    for (; c + 7 < Cg; c += 8) {
      ushort8_t v = *reinterpret_cast<const ushort8_t*>(px + c);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = bf16_bits_to_f32(v[j]);
        sum += f;
        sumsq += f * f;
      }
    }
    for (; c < Cg; ++c) {
      float f = bf16_bits_to_f32(px[c]);
      sum += f;
      sumsq += f * f;
    }
  }
  float mean, rstd;
  gn_block_stats(sum, sumsq, (float)HW * Cg, eps, mean, rstd);

  for (long long pp = threadIdx.x; pp < HW; pp += blockDim.x) {
    const uint16_t* px = x + base + pp * C;
    uint16_t* py = y + base + pp * C;
    int c = 0;
    for (; c + 7 < Cg; c += 8) {
      ushort8_t v = *reinterpret_cast<const ushort8_t*>(px + c);
      ushort8_t o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int ch = g * Cg + c + j;
        o[j] = gn_finish<FUSE_SILU>(v[j], mean, rstd, weight, bias, ch);
      }
      *reinterpret_cast<ushort8_t*>(py + c) = o;
    }
    for (; c < Cg; ++c) {
      const int ch = g * Cg + c;
      py[c] = gn_finish<FUSE_SILU>(px[c], mean, rstd, weight, bias, ch);
    }
  }
}

// The launch of either kernel above: grid N*G, block from
// gn_row_block_threads. kernel_of(std::bool_constant<SILU>) names the
// instantiation; the NCHW kernel takes HW as an int.
template <typename KernelOf>
static void gn_per_group_launch(KernelOf kernel_of, const torch::Tensor& x,
                                torch::Tensor& y, const torch::Tensor& w,
                                const torch::Tensor& b, int N, int C, int G,
                                long long HW, double eps, bool fuse_silu) {
  dim3 grid(N * G);
  dim3 block(gn_row_block_threads((long long)N * G, (long long)(C / G) * HW));
  auto stream = at::hip::getCurrentHIPStream();
  with_bool(fuse_silu, [&](auto SILU) {
    hipLaunchKernelGGL(kernel_of(SILU), grid, block, 0, stream,
                       (const uint16_t*)x.data_ptr(), (uint16_t*)y.data_ptr(),
                       w.data_ptr<float>(), b.data_ptr<float>(), C, G, HW,
                       (float)eps);
  });
  HIP_CHECK_LAUNCH();
}

torch::Tensor group_norm_fused(torch::Tensor x, int64_t groups,
                               torch::Tensor weight, torch::Tensor bias,
                               double eps, bool fuse_silu) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4, "x must be NCHW on device");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "x must be bf16");
  const int N = x.size(0), C = x.size(1);
  const int HW = x.size(2) * x.size(3);
  TORCH_CHECK(groups > 0 && C % groups == 0, "C must divide groups");
  auto w = param_f32(weight, x, C, "weight");
  auto b = param_f32(bias, x, C, "bias");
  auto xc = x.contiguous();
  auto y = torch::empty_like(xc);
  gn_per_group_launch(
      [](auto SILU) { return groupnorm_kernel<decltype(SILU)::value>; }, xc,
      y, w, b, N, C, (int)groups, HW, eps, fuse_silu);
  return y;
}

// ---------------------------------------------------------------------------
// NHWC GroupNorm in two fully-coalesced passes. A block per (n, g) reads each
// pixel's Cg*2 bytes at C*2-byte stride: ~6% of a 128-byte line is useful at
// Cg = 4..10. These kernels stream the tensor linearly twice (stats, then
// fused normalize+affine+SiLU): 3 x bytes of traffic total, which is the
// memory-bound floor for an unfused GN.
//
// Lane mapping, both passes. A pixel is V = C/8 16-byte vectors ("slots").
// A lane owns the same slot for its whole loop, so everything that depends
// on the channel alone (the group split of the vector, weight, bias, the
// two groups' mean/rstd, the per-sample addend) is computed once and stays
// in registers; the loop body is load, arithmetic, store. With NS =
// ceil(V/256) slots per lane and TH = ceil(V/NS) lanes per pixel, a block
// step covers P = 256/TH whole pixels; lane t works on pixel row t / TH at
// slots t % TH + k*TH. Each block sweeps a stripe of `ppb` pixels of ONE
// image, `ppb` a multiple of P, with four loads in flight per lane.
//
// Pass 1 keeps a lane's two (sum, sumsq) pairs in registers (a vector spans
// at most two groups when Cg >= 8 or Cg == 4), reduces them through LDS in
// a fixed order (pixel rows of a slot, then the slots of a group) and
// writes all G pairs of the block, zeros included, with plain stores into
// partial[B][bpi][G][2]: no atomics, no memset, and the same bits on every
// call. A block whose stripe is empty writes zeros. gn_finalize_kernel sums
// the partials in block order and leaves (mean, rstd) per (b, g).
// With ADD, both passes work on bf16_rne(x + addend[b, c]), the tensor the
// eager broadcast add would have produced.
//
// The two passes' pixel sweeps ("four loads in flight, then up to three left
// over") are written out in each kernel. With a shared sweep that takes the
// per-vector work as a callable, gn_stats_kernel runs out of SGPRs (55-70 ->
// 106), spills 20-36 bytes per lane to scratch and doubles in length
// (profiles/r13_norms.md).
// ---------------------------------------------------------------------------

#define GN_MAXG 64
#define GN_THREADS 256
#define GN_MAX_SLOTS 2

struct GnPlan {
  int ns;         // slots per lane
  int th;         // lanes per pixel
  int p;          // pixels per block step
  int threads;    // block size: p * th rounded up to whole waves
  int bpi;        // blocks per image (grid.x); grid.y = B
  long long ppb;  // pixels per block, a multiple of p
};

// ~2048 blocks across the chip, each confined to one image and holding at
// least about one 256-vector step; stripes are whole steps, so only the
// last block of an image that has pixels sees a partial step, and blocks
// past it ((bpi - 1) * ppb >= HW) have an empty stripe.
static GnPlan gn_plan(long long B, long long HW, long long C) {
  GnPlan pl;
  const int V = (int)(C / 8);
  pl.ns = (V + GN_THREADS - 1) / GN_THREADS;
  pl.th = (V + pl.ns - 1) / pl.ns;
  pl.p = GN_THREADS / pl.th;
  pl.threads = (pl.p * pl.th + 63) / 64 * 64;
  const long long nvec = HW * V;
  pl.bpi = (int)std::min<long long>(
      std::max<long long>(1, 2048 / std::max<long long>(B, 1)),
      std::max<long long>(1, nvec / GN_THREADS));
  const long long per = (HW + pl.bpi - 1) / pl.bpi;
  pl.ppb = std::max<long long>(1, (per + pl.p - 1) / pl.p) * pl.p;
  return pl;
}

// bf16_rne(x + a) as fp32: what torch's bf16 add leaves in memory
__device__ __forceinline__ float gn_add_bf16(float x, uint16_t a) {
  return bf16_bits_to_f32(f32_to_bf16_bits(x + bf16_bits_to_f32(a)));
}

template <bool ADD>
__device__ __forceinline__ void gn_accum(const ushort8_t& vec,
                                         const ushort8_t& av, int cut,
                                         float4_t& acc) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float f = bf16_bits_to_f32(vec[j]);
    if (ADD) f = gn_add_bf16(f, av[j]);
    if (j < cut) {
      acc[0] += f;
      acc[1] += f * f;
    } else {
      acc[2] += f;
      acc[3] += f * f;
    }
  }
}

template <int NS, bool ADD>
__global__ __launch_bounds__(GN_THREADS) void gn_stats_kernel(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ addend,
    float* __restrict__ partial,  // [B, bpi, G, 2]
    int C, int G, long long HW, int TH, int P, long long ppb) {
  const int b = blockIdx.y;
  const int V = C >> 3;
  const int Cg = C / G;
  const int t = threadIdx.x;
  const int prow = t / TH;
  const int sl = t - prow * TH;
  const long long p0 = (long long)blockIdx.x * ppb;
  const long long p1 = min(p0 + ppb, HW);
  const long long step = (long long)P * C;  // elements between a lane's loads

  __shared__ float4_t s_part[NS * GN_THREADS];  // [k][prow][sl]
  __shared__ float4_t s_slot[NS * GN_THREADS];  // [slot]

#pragma unroll
  for (int k = 0; k < NS; ++k) {
    float4_t acc = {0.f, 0.f, 0.f, 0.f};
    const int s = sl + k * TH;
    if (prow < P && s < V) {
      const int c0 = s << 3;
      const int g0 = c0 / Cg;
      const int cut = min((g0 + 1) * Cg - c0, 8);  // elements in the first run
      ushort8_t av = {0, 0, 0, 0, 0, 0, 0, 0};
      if (ADD)
        av = *reinterpret_cast<const ushort8_t*>(addend + (long long)b * C + c0);
      long long p = p0 + prow;
      const uint16_t* px = x + ((long long)b * HW + p) * C + c0;
      for (; p + 3 * P < p1; p += 4 * P, px += 4 * step) {
        ushort8_t v0 = *reinterpret_cast<const ushort8_t*>(px);
        ushort8_t v1 = *reinterpret_cast<const ushort8_t*>(px + step);
        ushort8_t v2 = *reinterpret_cast<const ushort8_t*>(px + 2 * step);
        ushort8_t v3 = *reinterpret_cast<const ushort8_t*>(px + 3 * step);
        gn_accum<ADD>(v0, av, cut, acc);
        gn_accum<ADD>(v1, av, cut, acc);
        gn_accum<ADD>(v2, av, cut, acc);
        gn_accum<ADD>(v3, av, cut, acc);
      }
      // up to three pixels left: their loads go out together as well
      const int rem = (p < p1) + (p + P < p1) + (p + 2 * P < p1);
      if (rem > 0) {
        ushort8_t v0 = *reinterpret_cast<const ushort8_t*>(px);
        ushort8_t v1 = v0, v2 = v0;
        if (rem > 1) v1 = *reinterpret_cast<const ushort8_t*>(px + step);
        if (rem > 2) v2 = *reinterpret_cast<const ushort8_t*>(px + 2 * step);
        gn_accum<ADD>(v0, av, cut, acc);
        if (rem > 1) gn_accum<ADD>(v1, av, cut, acc);
        if (rem > 2) gn_accum<ADD>(v2, av, cut, acc);
      }
    }
    s_part[k * GN_THREADS + t] = acc;
  }
  __syncthreads();
  // pixel rows of one slot, in row order
  for (int u = t; u < NS * TH; u += blockDim.x) {
    const int k = u / TH;
    const int base = k * GN_THREADS + (u - k * TH);
    float4_t tot = s_part[base];
    for (int r = 1; r < P; ++r) {
      const float4_t o = s_part[base + r * TH];
      tot[0] += o[0]; tot[1] += o[1]; tot[2] += o[2]; tot[3] += o[3];
    }
    s_slot[u] = tot;  // u == slot index: slot s lives at k = s / TH
  }
  __syncthreads();
  // slots of one group, in channel order; a slot holds the group either as
  // its first run (g0 == g) or as its second
  if (t < G) {
    const int sa = (t * Cg) >> 3;
    const int sb = ((t + 1) * Cg - 1) >> 3;
    float sum = 0.f, sq = 0.f;
    for (int s = sa; s <= sb; ++s) {
      const float4_t o = s_slot[s];
      const bool first = ((s << 3) / Cg) == t;
      sum += first ? o[0] : o[2];
      sq += first ? o[1] : o[3];
    }
    float* dst = partial + (((long long)b * gridDim.x + blockIdx.x) * G + t) * 2;
    dst[0] = sum;
    dst[1] = sq;
  }
}

// One block per image: sums the bpi partial pairs of every group in block
// order (256 / 2G contiguous chunks, then the chunks in order) and writes
// (mean, rstd). var = E[x^2] - mean^2 in fp32, clamped at 0.
__global__ __launch_bounds__(GN_THREADS) void gn_finalize_kernel(
    const float* __restrict__ partial, float* __restrict__ stats,  // [B, G, 2]
    int G, int bpi, float inv_count, float eps) {
  const int b = blockIdx.x;
  const int n2 = 2 * G;
  const int nparts = GN_THREADS / n2;
  const int t = threadIdx.x;
  const int part = t / n2;
  const int e = t - part * n2;
  __shared__ float s_acc[GN_THREADS];
  __shared__ float s_tot[2 * GN_MAXG];
  float acc = 0.f;
  if (part < nparts) {
    const int chunk = (bpi + nparts - 1) / nparts;
    const int k0 = part * chunk;
    const int k1 = min(k0 + chunk, bpi);
    const float* src = partial + ((long long)b * bpi + k0) * n2 + e;
    // eight loads in flight, added in block order (a masked slot adds 0)
    for (int k = k0; k < k1; k += 8, src += 8 * n2) {
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = (k + i < k1) ? src[i * n2] : 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc += v[i];
    }
  }
  s_acc[t] = acc;
  __syncthreads();
  if (t < n2) {
    float tot = s_acc[t];
    for (int p = 1; p < nparts; ++p) tot += s_acc[p * n2 + t];
    s_tot[t] = tot;
  }
  __syncthreads();
  if (t < G) {
    const float mean = s_tot[2 * t] * inv_count;
    const float var = s_tot[2 * t + 1] * inv_count - mean * mean;
    stats[((long long)b * G + t) * 2 + 0] = mean;
    stats[((long long)b * G + t) * 2 + 1] = rsqrtf(fmaxf(var, 0.f) + eps);
  }
}

// Pass 2: ((x - mean) * rstd) * w + b, then SiLU, one bf16 rounding on the
// store. The SiLU divide is a reciprocal (v_rcp_f32, 1 ulp in fp32): the
// IEEE division sequence is a third of the pass's vector instructions.
template <bool FUSE_SILU, bool ADD>
__device__ __forceinline__ ushort8_t gn_apply_vec(
    const ushort8_t& vec, const ushort8_t& av, int cut, float m0, float r0,
    float m1, float r1, const float (&w)[8], const float (&bs)[8]) {
  ushort8_t out;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float f = bf16_bits_to_f32(vec[j]);
    if (ADD) f = gn_add_bf16(f, av[j]);
    f = (f - (j < cut ? m0 : m1)) * (j < cut ? r0 : r1);
    f = f * w[j] + bs[j];
    if (FUSE_SILU) f = f * __builtin_amdgcn_rcpf(1.0f + __expf(-f));
    out[j] = f32_to_bf16_bits(f);
  }
  return out;
}

template <int NS, bool FUSE_SILU, bool ADD>
__global__ __launch_bounds__(GN_THREADS) void gn_apply_kernel(
    const uint16_t* __restrict__ x, uint16_t* __restrict__ y,
    const uint16_t* __restrict__ addend,
    const float* __restrict__ stats,  // [B, G, 2] (mean, rstd)
    const float* __restrict__ weight, const float* __restrict__ bias,
    int C, int G, long long HW, int TH, int P, long long ppb) {
  const int b = blockIdx.y;
  const int V = C >> 3;
  const int Cg = C / G;
  const int t = threadIdx.x;
  const int prow = t / TH;
  const int sl = t - prow * TH;
  if (prow >= P) return;
  const long long p0 = (long long)blockIdx.x * ppb;
  const long long p1 = min(p0 + ppb, HW);
  const long long step = (long long)P * C;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int s = sl + k * TH;
    if (s >= V) break;
    const int c0 = s << 3;
    const int g0 = c0 / Cg;
    const int g1 = (c0 + 7) / Cg;
    const int cut = min((g0 + 1) * Cg - c0, 8);
    const float* st = stats + (long long)b * G * 2;
    const float m0 = st[2 * g0], r0 = st[2 * g0 + 1];
    const float m1 = st[2 * g1], r1 = st[2 * g1 + 1];
    float w[8], bs[8];
    {
      const float4_t wa = *reinterpret_cast<const float4_t*>(weight + c0);
      const float4_t wb = *reinterpret_cast<const float4_t*>(weight + c0 + 4);
      const float4_t ba = *reinterpret_cast<const float4_t*>(bias + c0);
      const float4_t bb = *reinterpret_cast<const float4_t*>(bias + c0 + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        w[j] = wa[j]; w[j + 4] = wb[j];
        bs[j] = ba[j]; bs[j + 4] = bb[j];
      }
    }
    ushort8_t av = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ADD)
      av = *reinterpret_cast<const ushort8_t*>(addend + (long long)b * C + c0);
    long long p = p0 + prow;
    const long long off = ((long long)b * HW + p) * C + c0;
    const uint16_t* px = x + off;
    uint16_t* py = y + off;
    for (; p + 3 * P < p1; p += 4 * P, px += 4 * step, py += 4 * step) {
      ushort8_t v0 = *reinterpret_cast<const ushort8_t*>(px);
      ushort8_t v1 = *reinterpret_cast<const ushort8_t*>(px + step);
      ushort8_t v2 = *reinterpret_cast<const ushort8_t*>(px + 2 * step);
      ushort8_t v3 = *reinterpret_cast<const ushort8_t*>(px + 3 * step);
      *reinterpret_cast<ushort8_t*>(py) =
          gn_apply_vec<FUSE_SILU, ADD>(v0, av, cut, m0, r0, m1, r1, w, bs);
      *reinterpret_cast<ushort8_t*>(py + step) =
          gn_apply_vec<FUSE_SILU, ADD>(v1, av, cut, m0, r0, m1, r1, w, bs);
      *reinterpret_cast<ushort8_t*>(py + 2 * step) =
          gn_apply_vec<FUSE_SILU, ADD>(v2, av, cut, m0, r0, m1, r1, w, bs);
      *reinterpret_cast<ushort8_t*>(py + 3 * step) =
          gn_apply_vec<FUSE_SILU, ADD>(v3, av, cut, m0, r0, m1, r1, w, bs);
    }
    const int rem = (p < p1) + (p + P < p1) + (p + 2 * P < p1);
    if (rem > 0) {
      ushort8_t v0 = *reinterpret_cast<const ushort8_t*>(px);
      ushort8_t v1 = v0, v2 = v0;
      if (rem > 1) v1 = *reinterpret_cast<const ushort8_t*>(px + step);
      if (rem > 2) v2 = *reinterpret_cast<const ushort8_t*>(px + 2 * step);
      *reinterpret_cast<ushort8_t*>(py) =
          gn_apply_vec<FUSE_SILU, ADD>(v0, av, cut, m0, r0, m1, r1, w, bs);
      if (rem > 1)
        *reinterpret_cast<ushort8_t*>(py + step) =
            gn_apply_vec<FUSE_SILU, ADD>(v1, av, cut, m0, r0, m1, r1, w, bs);
      if (rem > 2)
        *reinterpret_cast<ushort8_t*>(py + 2 * step) =
            gn_apply_vec<FUSE_SILU, ADD>(v2, av, cut, m0, r0, m1, r1, w, bs);
    }
  }
}

// The three launches of one two-pass GroupNorm.
template <int NS, bool ADD>
static void gn_two_pass(const GnPlan& pl, const uint16_t* x, uint16_t* y,
                        const uint16_t* addend, float* partial, float* stats,
                        const float* w, const float* b, int B, int C, int G,
                        long long HW, float eps, bool fuse_silu,
                        hipStream_t stream) {
  dim3 grid((unsigned)pl.bpi, (unsigned)B), block(pl.threads);
  hipLaunchKernelGGL((gn_stats_kernel<NS, ADD>), grid, block, 0, stream, x,
                     addend, partial, C, G, HW, pl.th, pl.p, pl.ppb);
  const float inv_count = 1.f / ((float)HW * (C / G));
  hipLaunchKernelGGL(gn_finalize_kernel, dim3(B), dim3(GN_THREADS), 0, stream,
                     partial, stats, G, pl.bpi, inv_count, eps);
  with_bool(fuse_silu, [&](auto SILU) {
    hipLaunchKernelGGL((gn_apply_kernel<NS, decltype(SILU)::value, ADD>), grid,
                       block, 0, stream, x, y, addend, stats, w, b, C, G, HW,
                       pl.th, pl.p, pl.ppb);
  });
}

// (B, HW, C) -> (threads, pixels per step, slots per lane, blocks per image,
// pixels per block) of the two-pass kernels; launches nothing.
std::vector<int64_t> group_norm_nhwc_plan(int64_t B, int64_t HW, int64_t C) {
  TORCH_CHECK(B > 0 && HW > 0 && C > 0 && C % 8 == 0
              && C / 8 <= GN_MAX_SLOTS * GN_THREADS);
  const GnPlan pl = gn_plan(B, HW, C);
  return {pl.threads, pl.p, pl.ns, pl.bpi, pl.ppb};
}

torch::Tensor group_norm_nhwc(torch::Tensor x, int64_t groups,
                              torch::Tensor weight, torch::Tensor bias,
                              double eps, bool fuse_silu,
                              c10::optional<torch::Tensor> addend) {
  // x: [B, H, W, C] bf16 contiguous; addend: [B, C] bf16, added per sample
  // (rounded to bf16) before the statistics
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && x.scalar_type() == at::kBFloat16
              && x.is_contiguous());
  const int B = x.size(0), C = x.size(3);
  const long long HW = (long long)x.size(1) * x.size(2);
  TORCH_CHECK(groups > 0 && C % groups == 0);
  const int G = (int)groups, Cg = C / G;
  auto w = param_f32(weight, x, C, "weight");
  auto b = param_f32(bias, x, C, "bias");
  auto aligned16 = [](const torch::Tensor& t) {
    return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
  };
  // The two-pass kernels read x, weight, bias and addend 16 bytes at a time,
  // and a vector may span at most two groups: Cg >= 8, or Cg == 4, where
  // each aligned 8-element vector covers exactly two complete groups (the
  // VAE's C = 128 / G = 32 stages, the per-(n, g) kernel's worst case).
  const bool two_pass = C % 8 == 0 && (Cg >= 8 || Cg == 4) && G <= GN_MAXG
                        && C / 8 <= GN_MAX_SLOTS * GN_THREADS
                        && B > 0 && B <= 65535 && HW > 0
                        && aligned16(x) && aligned16(w) && aligned16(b);
  const bool has_add = addend.has_value() && addend->defined();
  if (has_add) {
    TORCH_CHECK(addend->is_cuda() && addend->scalar_type() == at::kBFloat16
                && addend->dim() == 2 && addend->size(0) == B
                && addend->size(1) == C, "addend must be bf16 [B, C]");
    if (!two_pass)  // the per-(n, g) kernel takes the summed tensor
      x = (x + addend->view({B, 1, 1, C})).contiguous();
  }
  auto y = torch::empty_like(x);
  if (!two_pass) {
    gn_per_group_launch(
        [](auto SILU) { return groupnorm_nhwc_kernel<decltype(SILU)::value>; },
        x, y, w, b, B, C, G, HW, eps, fuse_silu);
    return y;
  }
  const GnPlan pl = gn_plan(B, HW, C);
  auto fopt = x.options().dtype(at::kFloat);
  auto partial = torch::empty({B, pl.bpi, G, 2}, fopt);
  auto stats = torch::empty({B, G, 2}, fopt);
  torch::Tensor ac;
  const uint16_t* ap = nullptr;
  if (has_add) {
    ac = addend->contiguous();
    if (!aligned16(ac)) ac = ac.clone();
    ap = (const uint16_t*)ac.data_ptr();
  }
  auto run = has_add
      ? (pl.ns == 1 ? gn_two_pass<1, true> : gn_two_pass<2, true>)
      : (pl.ns == 1 ? gn_two_pass<1, false> : gn_two_pass<2, false>);
  run(pl, (const uint16_t*)x.data_ptr(), (uint16_t*)y.data_ptr(), ap,
      partial.data_ptr<float>(), stats.data_ptr<float>(),
      w.data_ptr<float>(), b.data_ptr<float>(), B, C, G, HW, (float)eps,
      fuse_silu, at::hip::getCurrentHIPStream());
  HIP_CHECK_LAUNCH();
  return y;
}

// ---------------------------------------------------------------------------
// LayerNorm over the last dim. x: [T, C] bf16 (rows = flattened tokens),
// gamma/beta fp32. One wave per row at every C: a lane strides the row in
// 16-byte vectors and re-reads it for the normalize pass.
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
  // tail (C not a multiple of 8): scalar, one element per low lane
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
  const int C = x.size(-1);
  auto g = param_f32(gamma, x, C, "gamma");
  auto b = param_f32(beta, x, C, "beta");
  auto xc = x.contiguous();
  const long long T = xc.numel() / C;
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

// SiLU, or GELU in its tanh form (0.7978845608 = sqrt(2 / pi))
template <bool GELU>
__device__ __forceinline__ float act_f(float x) {
  return GELU ? 0.5f * x * (1.f + tanhf(0.7978845608f * (x + 0.044715f * x * x * x)))
              : silu_f(x);
}

// One element of the 8-wide body. The loop over a vector's elements stays in
// each kernel: inside a helper of any form (vector returned, stored through a
// pointer, written out without a loop) the GELU kernels compile to packed
// v_pk_mul_f32 / v_pk_add_f32 pairs, not to the instructions that were
// measured (profiles/r13_norms.md).
template <bool GELU>
__device__ __forceinline__ uint16_t act_mul1(uint16_t a, uint16_t b) {
  float act = act_f<GELU>(bf16_bits_to_f32(b));
  return f32_to_bf16_bits(bf16_bits_to_f32(a) * act);
}

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
    for (int j = 0; j < 8; ++j) o[j] = act_mul1<GELU>(va[j], vb[j]);
    *reinterpret_cast<ushort8_t*>(y + i) = o;
  }
  // tail: n % 8 elements, by the first threads of block 0 (b[k] is loaded
  // first; as arguments of act_mul1 the two loads would swap)
  if (blockIdx.x == 0 && threadIdx.x < 8) {
    for (long long k = (n / 8) * 8 + threadIdx.x; k < n; k += 8) {
      float act = act_f<GELU>(bf16_bits_to_f32(b[k]));
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
    for (int j = 0; j < 8; ++j) o[j] = act_mul1<GELU>(va[j], vb[j]);
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
  auto stream = at::hip::getCurrentHIPStream();
  long long pitch_a = 0, pitch_b = 0;
  if (!(a.is_contiguous() && b.is_contiguous())
      && act_mul_row_view(a, &pitch_a) && act_mul_row_view(b, &pitch_b)
      && a.numel() / 8 < (1LL << 32)) {
    const long long cols = a.size(-1);
    const long long nvec = a.numel() / 8;
    auto y = torch::empty(a.sizes(), a.options());
    int blocks = (int)std::min<long long>((nvec + 255) / 256, 2048);
    with_bool(gelu, [&](auto GELU) {
      hipLaunchKernelGGL((act_mul_rows_kernel<decltype(GELU)::value>),
                         dim3(blocks), dim3(256), 0, stream,
                         (const uint16_t*)a.data_ptr(),
                         (const uint16_t*)b.data_ptr(), (uint16_t*)y.data_ptr(),
                         (unsigned)nvec, (unsigned)(cols / 8), pitch_a, pitch_b);
    });
    HIP_CHECK_LAUNCH();
    return y;
  }
  auto ac = a.contiguous(), bc = b.contiguous();
  auto y = torch::empty_like(ac);
  long long n = ac.numel();
  int blocks = (int)std::min<long long>((n / 8 + 255) / 256 + 1, 2048);
  with_bool(gelu, [&](auto GELU) {
    hipLaunchKernelGGL((act_mul_kernel<decltype(GELU)::value>), dim3(blocks),
                       dim3(256), 0, stream, (const uint16_t*)ac.data_ptr(),
                       (const uint16_t*)bc.data_ptr(), (uint16_t*)y.data_ptr(), n);
  });
  HIP_CHECK_LAUNCH();
  return y;
}
