// Hand-written CDNA4 convolution kernels for the VAE decode path.
//
// Implicit-GEMM formulation on MFMA 16x16x32 bf16: output pixels are GEMM
// rows (M = B*H*W), output channels are GEMM columns (N = K), the reduction
// runs over (r, s, c) with the channel dim innermost (NHWC activations, so
// every A fragment is a contiguous 16-byte load; no im2col materialization,
// no NCHW<->NHWC transposes). Weights are host-repacked once per module to
// W_t[k_out][(r*3+s)*C + c] so B fragments are contiguous too.
//
// Covers: 3x3 stride-1 pad-1 and 1x1 convs with C % 32 == 0, K % 16 == 0 —
// the whole VAE decoder trunk (512/256/128 channels). Odd-channel edges
// (conv_in from 4 latents, conv_out to RGB) stay on MIOpen.
//
// Reference counterpart: the VAEDecode ComfyUI op the reference calls per
// tile.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define ZERO8_C short8{0, 0, 0, 0, 0, 0, 0, 0}

// Tile geometry: BM=64 pixels x BN=64 channels per workgroup, 4 waves in a
// 2x2 grid (each wave owns a 32x32 sub-tile = 2x2 MFMA fragments).
#define CBM 64
#define CBN 64

template <int RS>  // 9 for 3x3, 1 for 1x1
__global__ __launch_bounds__(256) void conv_nhwc_kernel(
    const uint16_t* __restrict__ x,   // [B, H, W, C]
    const uint16_t* __restrict__ wt,  // [K, RS*C] repacked
    const float* __restrict__ bias,   // [K] or nullptr
    uint16_t* __restrict__ y,         // [B, H, W, K]
    int B, int H, int W, int C, int K, int fuse_silu) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wm = wave >> 1;          // wave row (0..1)
  const int wn = wave & 1;           // wave col (0..1)
  const long long HW = (long long)H * W;
  const long long M = (long long)B * HW;

  const long long m_base = (long long)blockIdx.x * CBM + wm * 32;
  const int n_base = blockIdx.y * CBN + wn * 32;

  // accumulators: 2x2 fragments of 16x16
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // per-lane A row (pixel) and B row (output channel)
  const int fr = lane & 15;          // fragment row/col index
  const int kgrp = lane >> 4;        // k-group: elements kgrp*8..+8

  // decompose the two pixel rows this lane loads for A
  long long m_row[2];
  int px_y[2], px_x[2], px_b[2];
  bool m_ok[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    m_row[i] = m_base + i * 16 + fr;
    m_ok[i] = m_row[i] < M;
    long long mm = m_ok[i] ? m_row[i] : 0;
    px_b[i] = (int)(mm / HW);
    int rem = (int)(mm - (long long)px_b[i] * HW);
    px_y[i] = rem / W;
    px_x[i] = rem % W;
  }
  const int n_col[2] = {n_base + fr, n_base + 16 + fr};

  const int csteps = C / 32;
  for (int rs = 0; rs < RS; ++rs) {
    const int r = RS == 1 ? 0 : rs / 3;
    const int s = RS == 1 ? 0 : rs % 3;
    // source pixel offsets for this tap (pad 1 for 3x3)
    int sy[2], sx[2];
    bool tap_ok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      sy[i] = px_y[i] + (RS == 1 ? 0 : r - 1);
      sx[i] = px_x[i] + (RS == 1 ? 0 : s - 1);
      tap_ok[i] = m_ok[i] && sy[i] >= 0 && sy[i] < H && sx[i] >= 0 && sx[i] < W;
    }
    for (int cs = 0; cs < csteps; ++cs) {
      const int c0 = cs * 32 + kgrp * 8;
      // A fragments (2 pixel rows x 8 contiguous channels)
      short8 a[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (tap_ok[i]) {
          const uint16_t* p = x + (((long long)px_b[i] * H + sy[i]) * W + sx[i]) * C + c0;
          a[i] = *reinterpret_cast<const short8*>(p);
        } else {
          a[i] = short8{0, 0, 0, 0, 0, 0, 0, 0};
        }
      }
      // B fragments (2 output channels x 8 contiguous k-elements)
      const int kdim = rs * C + cs * 32 + kgrp * 8;
      short8 bfr[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int n = n_col[j];
        bfr[j] = (n < K)
            ? *reinterpret_cast<const short8*>(wt + (long long)n * (RS * C) + kdim)
            : short8{0, 0, 0, 0, 0, 0, 0, 0};
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], bfr[j],
                                                              acc[i][j], 0, 0, 0);
    }
  }

  // epilogue: bias + optional SiLU, store NHWC
  const int out_col = lane & 15;
  const int rgrp = lane >> 4;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n_base + j * 16 + out_col;
      if (n >= K) continue;
      const float bval = bias ? bias[n] : 0.f;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const long long m = m_base + i * 16 + rgrp * 4 + rr;
        if (m >= M) continue;
        float v = acc[i][j][rr] + bval;
        if (fuse_silu) v = silu_f(v);
        y[m * K + n] = f32_to_bf16_bits(v);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// v2: 128x128 tile, 8 waves (2M x 4N wave grid, each wave 64x32 output),
// weights LDS-staged per 32-deep k-step in a conflict-free 80-byte-pitch
// image shared by all waves; A fragments stream from global (L1/L2-cached:
// consecutive k-steps walk a pixel row sequentially).
// ---------------------------------------------------------------------------

#define C2BM 128
#define C2BN 128
#define W_PITCH 40  // elements per LDS weight row (32 + 8 pad = 80 B)

template <int RS>
__global__ __launch_bounds__(512) void conv_nhwc2_kernel(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ wt,
    const float* __restrict__ bias, uint16_t* __restrict__ y, int B, int H,
    int W, int C, int K, int fuse_silu) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wm = wave >> 2;  // 0..1  (M strip of 64)
  const int wn = wave & 3;   // 0..3  (N strip of 32)
  const long long HW = (long long)H * W;
  const long long M = (long long)B * HW;

  const long long m_base = (long long)blockIdx.x * C2BM + wm * 64;
  const int n_base = blockIdx.y * C2BN + wn * 32;

  __shared__ __align__(16) uint16_t w_lds[C2BN][W_PITCH];

  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15;
  const int kgrp = lane >> 4;

  long long m_row[4];
  int px_y[4], px_x[4], px_b[4];
  bool m_ok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    m_row[i] = m_base + i * 16 + fr;
    m_ok[i] = m_row[i] < M;
    long long mm = m_ok[i] ? m_row[i] : 0;
    px_b[i] = (int)(mm / HW);
    int rem = (int)(mm - (long long)px_b[i] * HW);
    px_y[i] = rem / W;
    px_x[i] = rem % W;
  }

  const int csteps = C / 32;
  for (int rs = 0; rs < RS; ++rs) {
    const int r = RS == 1 ? 0 : rs / 3;
    const int s = RS == 1 ? 0 : rs % 3;
    int sy[4], sx[4];
    bool tap_ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sy[i] = px_y[i] + (RS == 1 ? 0 : r - 1);
      sx[i] = px_x[i] + (RS == 1 ? 0 : s - 1);
      tap_ok[i] = m_ok[i] && sy[i] >= 0 && sy[i] < H && sx[i] >= 0 && sx[i] < W;
    }
    for (int cs = 0; cs < csteps; ++cs) {
      const int kdim = rs * C + cs * 32;
      // ---- stage the 128x32 weight chunk (one 16B piece per thread) ----
      __syncthreads();
      {
        const int n = blockIdx.y * C2BN + (threadIdx.x >> 2);      // 128 rows
        const int koff = (threadIdx.x & 3) * 8;                     // 4 pieces
        short8 wv = (n < K)
            ? *reinterpret_cast<const short8*>(wt + (long long)n * (RS * C) + kdim + koff)
            : short8{0, 0, 0, 0, 0, 0, 0, 0};
        *reinterpret_cast<short8*>(&w_lds[threadIdx.x >> 2][koff]) = wv;
      }
      __syncthreads();

      const int c0 = cs * 32 + kgrp * 8;
      short8 a[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (tap_ok[i]) {
          const uint16_t* p =
              x + (((long long)px_b[i] * H + sy[i]) * W + sx[i]) * C + c0;
          a[i] = *reinterpret_cast<const short8*>(p);
        } else {
          a[i] = short8{0, 0, 0, 0, 0, 0, 0, 0};
        }
      }
      short8 bfr[2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
        bfr[j] = *reinterpret_cast<const short8*>(
            &w_lds[wn * 32 + j * 16 + fr][kgrp * 8]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], bfr[j],
                                                              acc[i][j], 0, 0, 0);
    }
  }

  const int out_col = lane & 15;
  const int rgrp = lane >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n_base + j * 16 + out_col;
      if (n >= K) continue;
      const float bval = bias ? bias[n] : 0.f;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const long long m = m_base + i * 16 + rgrp * 4 + rr;
        if (m >= M) continue;
        float v = acc[i][j][rr] + bval;
        if (fuse_silu) v = silu_f(v);
        y[m * K + n] = f32_to_bf16_bits(v);
      }
    }
  }
}

template <int RS>
__global__ void conv_nhwc3_kernel(const uint16_t*, const uint16_t*,
                                  const float*, uint16_t*, int, int, int,
                                  int, int, int);

torch::Tensor conv_nhwc(torch::Tensor x, torch::Tensor wt, torch::Tensor bias,
                        int64_t B, int64_t H, int64_t W, int64_t C, int64_t K,
                        int64_t rs, bool fuse_silu) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.is_contiguous());
  TORCH_CHECK(wt.is_cuda() && wt.scalar_type() == at::kBFloat16 && wt.is_contiguous());
  TORCH_CHECK(C % 32 == 0, "C must be a multiple of 32");
  TORCH_CHECK(rs == 9 || rs == 1, "only 3x3 and 1x1");
  auto y = torch::empty({B, H, W, K}, x.options());
  const long long M = B * H * W;
  auto stream = at::hip::getCurrentHIPStream();
  const float* bptr = nullptr;
  torch::Tensor bf;
  if (bias.defined() && bias.numel() > 0) {
    bf = bias.contiguous().to(at::kFloat);
    bptr = bf.data_ptr<float>();
  }
  // v3 (64-deep k-steps) is opt-in until GPU-validated; v2 (LDS-staged
  // weights, 128x128 tile) when the N dim fills it; v1 otherwise. M tail
  // handled by in-kernel bounds in all variants.
  static const bool v3_enabled = [] {
    const char* e = getenv("DISTGPU_CONV_V3");
    return e && e[0] == '1';
  }();
  if (v3_enabled && (K % C2BN == 0) && (C % 64 == 0) && (M >= C2BM)) {
    dim3 grid((unsigned)((M + C2BM - 1) / C2BM), (unsigned)(K / C2BN));
    dim3 block(512);
    if (rs == 9)
      hipLaunchKernelGGL((conv_nhwc3_kernel<9>), grid, block, 0, stream,
                         (const uint16_t*)x.data_ptr(), (const uint16_t*)wt.data_ptr(),
                         bptr, (uint16_t*)y.data_ptr(), (int)B, (int)H, (int)W,
                         (int)C, (int)K, fuse_silu ? 1 : 0);
    else
      hipLaunchKernelGGL((conv_nhwc3_kernel<1>), grid, block, 0, stream,
                         (const uint16_t*)x.data_ptr(), (const uint16_t*)wt.data_ptr(),
                         bptr, (uint16_t*)y.data_ptr(), (int)B, (int)H, (int)W,
                         (int)C, (int)K, fuse_silu ? 1 : 0);
    HIP_CHECK_LAUNCH();
    return y;
  }
  const bool use_v2 = (K % C2BN == 0) && (M >= C2BM);
  if (use_v2) {
    dim3 grid((unsigned)((M + C2BM - 1) / C2BM), (unsigned)(K / C2BN));
    dim3 block(512);
    if (rs == 9)
      hipLaunchKernelGGL((conv_nhwc2_kernel<9>), grid, block, 0, stream,
                         (const uint16_t*)x.data_ptr(), (const uint16_t*)wt.data_ptr(),
                         bptr, (uint16_t*)y.data_ptr(), (int)B, (int)H, (int)W,
                         (int)C, (int)K, fuse_silu ? 1 : 0);
    else
      hipLaunchKernelGGL((conv_nhwc2_kernel<1>), grid, block, 0, stream,
                         (const uint16_t*)x.data_ptr(), (const uint16_t*)wt.data_ptr(),
                         bptr, (uint16_t*)y.data_ptr(), (int)B, (int)H, (int)W,
                         (int)C, (int)K, fuse_silu ? 1 : 0);
    HIP_CHECK_LAUNCH();
    return y;
  }
  dim3 grid((unsigned)((M + CBM - 1) / CBM), (unsigned)((K + CBN - 1) / CBN));
  dim3 block(256);
  if (rs == 9)
    hipLaunchKernelGGL((conv_nhwc_kernel<9>), grid, block, 0, stream,
                       (const uint16_t*)x.data_ptr(), (const uint16_t*)wt.data_ptr(),
                       bptr, (uint16_t*)y.data_ptr(), (int)B, (int)H, (int)W,
                       (int)C, (int)K, fuse_silu ? 1 : 0);
  else
    hipLaunchKernelGGL((conv_nhwc_kernel<1>), grid, block, 0, stream,
                       (const uint16_t*)x.data_ptr(), (const uint16_t*)wt.data_ptr(),
                       bptr, (uint16_t*)y.data_ptr(), (int)B, (int)H, (int)W,
                       (int)C, (int)K, fuse_silu ? 1 : 0);
  HIP_CHECK_LAUNCH();
  return y;
}

// ---------------------------------------------------------------------------
// v3 (experimental, env-gated DISTGPU_CONV_V3=1 until GPU-validated):
// like v2 but with 64-deep k-steps — one barrier pair covers TWO 32-deep
// MFMA sub-steps (the CDNA4 guide measures BK 32->64 at +16% on the
// equivalent GEMM structure: fewer barrier drains per MFMA).
// ---------------------------------------------------------------------------

#define W3_PITCH 72  // 64 elements + 8 pad = 144 B rows (16B-aligned,
                     // 36-dword stride -> conflict-free b128 lane groups)

template <int RS>
__global__ __launch_bounds__(512) void conv_nhwc3_kernel(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ wt,
    const float* __restrict__ bias, uint16_t* __restrict__ y, int B, int H,
    int W, int C, int K, int fuse_silu) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wm = wave >> 2;
  const int wn = wave & 3;
  const long long HW = (long long)H * W;
  const long long M = (long long)B * HW;

  const long long m_base = (long long)blockIdx.x * C2BM + wm * 64;
  const int n_base = blockIdx.y * C2BN + wn * 32;

  __shared__ __align__(16) uint16_t w_lds[C2BN][W3_PITCH];

  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15;
  const int kgrp = lane >> 4;

  long long m_row[4];
  int px_y[4], px_x[4], px_b[4];
  bool m_ok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    m_row[i] = m_base + i * 16 + fr;
    m_ok[i] = m_row[i] < M;
    long long mm = m_ok[i] ? m_row[i] : 0;
    px_b[i] = (int)(mm / HW);
    int rem = (int)(mm - (long long)px_b[i] * HW);
    px_y[i] = rem / W;
    px_x[i] = rem % W;
  }

  const int csteps2 = C / 64;  // 64-deep k-steps per tap
  for (int rs = 0; rs < RS; ++rs) {
    const int r = RS == 1 ? 0 : rs / 3;
    const int s = RS == 1 ? 0 : rs % 3;
    int sy[4], sx[4];
    bool tap_ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sy[i] = px_y[i] + (RS == 1 ? 0 : r - 1);
      sx[i] = px_x[i] + (RS == 1 ? 0 : s - 1);
      tap_ok[i] = m_ok[i] && sy[i] >= 0 && sy[i] < H && sx[i] >= 0 && sx[i] < W;
    }
    for (int cs = 0; cs < csteps2; ++cs) {
      const int kdim = rs * C + cs * 64;
      // ---- stage the 128x64 weight chunk (two 16B pieces per thread) ----
      __syncthreads();
      {
        const int row = threadIdx.x >> 2;           // 128 rows
        const int piece = threadIdx.x & 3;          // 4 x 16B = 64B half
        const int n = blockIdx.y * C2BN + row;
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
          const int koff = h2 * 32 + piece * 8;
          short8 wv = (n < K)
              ? *reinterpret_cast<const short8*>(
                    wt + (long long)n * (RS * C) + kdim + koff)
              : ZERO8_C;
          *reinterpret_cast<short8*>(&w_lds[row][koff]) = wv;
        }
      }
      __syncthreads();

      // ---- two 32-deep MFMA sub-steps under one barrier pair ----
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int c0 = cs * 64 + half * 32 + kgrp * 8;
        short8 a[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (tap_ok[i]) {
            const uint16_t* p =
                x + (((long long)px_b[i] * H + sy[i]) * W + sx[i]) * C + c0;
            a[i] = *reinterpret_cast<const short8*>(p);
          } else {
            a[i] = ZERO8_C;
          }
        }
        short8 bfr[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
          bfr[j] = *reinterpret_cast<const short8*>(
              &w_lds[wn * 32 + j * 16 + fr][half * 32 + kgrp * 8]);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a[i], bfr[j], acc[i][j], 0, 0, 0);
      }
    }
  }

  const int out_col = lane & 15;
  const int rgrp = lane >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n_base + j * 16 + out_col;
      if (n >= K) continue;
      const float bval = bias ? bias[n] : 0.f;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const long long m = m_base + i * 16 + rgrp * 4 + rr;
        if (m >= M) continue;
        float v = acc[i][j][rr] + bval;
        if (fuse_silu) v = silu_f(v);
        y[m * K + n] = f32_to_bf16_bits(v);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Small-C conv (the UNet/VAE stem: C_in <= 8, e.g. 4 latents -> 320).
// MIOpen/CK fall back to very slow paths for NHWC C=4; this is a simple
// HBM-bound kernel: 32 pixels x 8 k-slots per 256-thread block, weights
// staged in LDS, per-pixel taps read once and reused across the k-slots
// via L1.
// ---------------------------------------------------------------------------

#define SC_KSLOTS 8

template <int RS, int C>
__global__ __launch_bounds__(256) void conv_smallc_kernel(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ wt,
    const float* __restrict__ bias, uint16_t* __restrict__ y, int B, int H,
    int W, int K, int fuse_silu) {
  constexpr int KD = RS * C;
  extern __shared__ __align__(16) uint16_t w_sm[];  // [K][KD]
  for (int i = threadIdx.x; i < K * KD; i += blockDim.x) w_sm[i] = wt[i];
  __syncthreads();

  const long long HW = (long long)H * W;
  const long long M = (long long)B * HW;
  const int kper = (K + SC_KSLOTS - 1) / SC_KSLOTS;
  const int pix_local = threadIdx.x / SC_KSLOTS;   // 0..31
  const int kslot = threadIdx.x % SC_KSLOTS;
  const long long p = (long long)blockIdx.x * 32 + pix_local;
  if (p >= M) return;
  const int b = (int)(p / HW);
  const int rem = (int)(p - (long long)b * HW);
  const int py = rem / W, px = rem % W;

  // taps fully unrolled -> registers (a runtime-indexed array would live
  // in scratch: 5x slowdown)
  float taps[KD];
#pragma unroll
  for (int rs = 0; rs < RS; ++rs) {
    const int r = RS == 1 ? 0 : rs / 3;
    const int s = RS == 1 ? 0 : rs % 3;
    const int sy = py + (RS == 1 ? 0 : r - 1);
    const int sx = px + (RS == 1 ? 0 : s - 1);
    const bool ok = sy >= 0 && sy < H && sx >= 0 && sx < W;
    const uint16_t* src =
        x + (((long long)b * H + sy) * W + sx) * C;
#pragma unroll
    for (int c = 0; c < C; ++c)
      taps[rs * C + c] = ok ? bf16_bits_to_f32(src[c]) : 0.f;
  }

  const int k0 = kslot * kper;
  const int k1 = min(k0 + kper, K);
  uint16_t* dst = y + p * K;
  for (int k = k0; k < k1; ++k) {
    const uint16_t* wrow = &w_sm[k * KD];
    float acc = bias ? bias[k] : 0.f;
#pragma unroll
    for (int i = 0; i < KD; ++i)
      acc += taps[i] * bf16_bits_to_f32(wrow[i]);
    if (fuse_silu) acc = silu_f(acc);
    dst[k] = f32_to_bf16_bits(acc);
  }
}

torch::Tensor conv_smallc(torch::Tensor x, torch::Tensor wt, torch::Tensor bias,
                          int64_t B, int64_t H, int64_t W, int64_t C,
                          int64_t K, int64_t rs, bool fuse_silu) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.is_contiguous());
  TORCH_CHECK(C <= 8, "conv_smallc is for C <= 8");
  TORCH_CHECK(rs == 9 || rs == 1);
  auto y = torch::empty({B, H, W, K}, x.options());
  const long long M = B * H * W;
  dim3 grid((unsigned)((M + 31) / 32));
  dim3 block(256);
  const size_t smem = (size_t)K * rs * C * sizeof(uint16_t);
  TORCH_CHECK(smem <= 64 * 1024, "weights exceed LDS budget");
  auto stream = at::hip::getCurrentHIPStream();
  const float* bptr = nullptr;
  torch::Tensor bf;
  if (bias.defined() && bias.numel() > 0) {
    bf = bias.contiguous().to(at::kFloat);
    bptr = bf.data_ptr<float>();
  }
#define SC_LAUNCH(RS_, C_)                                                     \
  hipLaunchKernelGGL((conv_smallc_kernel<RS_, C_>), grid, block, smem, stream,\
                     (const uint16_t*)x.data_ptr(),                           \
                     (const uint16_t*)wt.data_ptr(), bptr,                    \
                     (uint16_t*)y.data_ptr(), (int)B, (int)H, (int)W, (int)K, \
                     fuse_silu ? 1 : 0)
  TORCH_CHECK(C == 3 || C == 4 || C == 8, "conv_smallc supports C in {3,4,8}");
  if (rs == 9) {
    if (C == 3) SC_LAUNCH(9, 3);
    else if (C == 4) SC_LAUNCH(9, 4);
    else SC_LAUNCH(9, 8);
  } else {
    if (C == 3) SC_LAUNCH(1, 3);
    else if (C == 4) SC_LAUNCH(1, 4);
    else SC_LAUNCH(1, 8);
  }
#undef SC_LAUNCH
  HIP_CHECK_LAUNCH();
  return y;
}

// ---------------------------------------------------------------------------
// NHWC fused GroupNorm(+SiLU): one block per (n, g); channels of a group are
// contiguous within each pixel (span Cg*2 bytes).
// ---------------------------------------------------------------------------

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

  __shared__ float scratch[16];
  __shared__ float s_mean, s_rstd;

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
  sum = block_reduce(sum, scratch, SumOp{}, 0.f);
  sumsq = block_reduce(sumsq, scratch, SumOp{}, 0.f);
  if (threadIdx.x == 0) {
    const float count = (float)HW * Cg;
    float mean = sum / count;
    float var = sumsq / count - mean * mean;
    s_mean = mean;
    s_rstd = rsqrtf(fmaxf(var, 0.f) + eps);
  }
  __syncthreads();
  const float mean = s_mean, rstd = s_rstd;

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
        float f = (bf16_bits_to_f32(v[j]) - mean) * rstd;
        f = f * weight[ch] + bias[ch];
        if (FUSE_SILU) f = silu_f(f);
        o[j] = f32_to_bf16_bits(f);
      }
      *reinterpret_cast<ushort8_t*>(py + c) = o;
    }
    for (; c < Cg; ++c) {
      const int ch = g * Cg + c;
      float f = (bf16_bits_to_f32(px[c]) - mean) * rstd;
      f = f * weight[ch] + bias[ch];
      if (FUSE_SILU) f = silu_f(f);
      py[c] = f32_to_bf16_bits(f);
    }
  }
}

// ---------------------------------------------------------------------------
// v2 GroupNorm: two fully-coalesced passes. The v1 kernel above (one block
// per (n, g)) reads each pixel's Cg*2 bytes at C*2-byte stride — ~6% of a
// 128-byte line useful at Cg=4..10, and rocprof r01 showed it at 13.4% of
// flagship kernel time (391 us avg). v2 streams the tensor linearly twice
// (stats, then fused normalize+affine+SiLU): 3 x bytes of traffic total,
// which is the memory-bound floor for an unfused GN.
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
// IEEE division sequence was a third of the pass's vector instructions.
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
  if (fuse_silu)
    hipLaunchKernelGGL((gn_apply_kernel<NS, true, ADD>), grid, block, 0,
                       stream, x, y, addend, stats, w, b, C, G, HW, pl.th,
                       pl.p, pl.ppb);
  else
    hipLaunchKernelGGL((gn_apply_kernel<NS, false, ADD>), grid, block, 0,
                       stream, x, y, addend, stats, w, b, C, G, HW, pl.th,
                       pl.p, pl.ppb);
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
  TORCH_CHECK(C % groups == 0);
  const int G = (int)groups, Cg = C / G;
  auto w = weight.contiguous().to(at::kFloat);
  auto b = bias.contiguous().to(at::kFloat);
  TORCH_CHECK(w.numel() == C && b.numel() == C);
  auto aligned16 = [](const torch::Tensor& t) {
    return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
  };
  // the two-pass kernels read x, weight, bias and addend 16 bytes at a time
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
  auto stream = at::hip::getCurrentHIPStream();
  // Cg == 4 also satisfies the <=2-groups-per-16B-vector invariant (each
  // aligned 8-element vector covers exactly two complete groups); the VAE
  // C=128/G=32 stages live here and were the v1 kernel's worst case.
  if (two_pass) {
    const GnPlan pl = gn_plan(B, HW, C);
    auto fopt = x.options().dtype(at::kFloat);
    auto partial = torch::empty({B, pl.bpi, G, 2}, fopt);
    auto stats = torch::empty({B, G, 2}, fopt);
    const uint16_t* xp = (const uint16_t*)x.data_ptr();
    uint16_t* yp = (uint16_t*)y.data_ptr();
    if (has_add) {
      auto ac = addend->contiguous();
      if (!aligned16(ac)) ac = ac.clone();
      const uint16_t* ap = (const uint16_t*)ac.data_ptr();
      if (pl.ns == 1)
        gn_two_pass<1, true>(pl, xp, yp, ap, partial.data_ptr<float>(),
                             stats.data_ptr<float>(), w.data_ptr<float>(),
                             b.data_ptr<float>(), B, C, G, HW, (float)eps,
                             fuse_silu, stream);
      else
        gn_two_pass<2, true>(pl, xp, yp, ap, partial.data_ptr<float>(),
                             stats.data_ptr<float>(), w.data_ptr<float>(),
                             b.data_ptr<float>(), B, C, G, HW, (float)eps,
                             fuse_silu, stream);
    } else {
      if (pl.ns == 1)
        gn_two_pass<1, false>(pl, xp, yp, nullptr, partial.data_ptr<float>(),
                              stats.data_ptr<float>(), w.data_ptr<float>(),
                              b.data_ptr<float>(), B, C, G, HW, (float)eps,
                              fuse_silu, stream);
      else
        gn_two_pass<2, false>(pl, xp, yp, nullptr, partial.data_ptr<float>(),
                              stats.data_ptr<float>(), w.data_ptr<float>(),
                              b.data_ptr<float>(), B, C, G, HW, (float)eps,
                              fuse_silu, stream);
    }
    HIP_CHECK_LAUNCH();
    return y;
  }
  // fallback (odd channel counts): v1 per-(n,g) kernel
  dim3 grid(B * (int)groups);
  const long long per_group = (long long)(C / groups) * HW;
  dim3 block(B * groups >= 128 ? 256 : (per_group > (1 << 20) ? 1024 : 256));
  if (fuse_silu)
    hipLaunchKernelGGL((groupnorm_nhwc_kernel<true>), grid, block, 0, stream,
                       (const uint16_t*)x.data_ptr(), (uint16_t*)y.data_ptr(),
                       w.data_ptr<float>(), b.data_ptr<float>(), C,
                       (int)groups, HW, (float)eps);
  else
    hipLaunchKernelGGL((groupnorm_nhwc_kernel<false>), grid, block, 0, stream,
                       (const uint16_t*)x.data_ptr(), (uint16_t*)y.data_ptr(),
                       w.data_ptr<float>(), b.data_ptr<float>(), C,
                       (int)groups, HW, (float)eps);
  HIP_CHECK_LAUNCH();
  return y;
}
