// FP8 (OCP e4m3fn) Linear path for the WAN / Flux transformer blocks:
// a per-row activation quantiser and a 256x256x128 block-scaled-MFMA GEMM.
//
//   quant_rows_fp8   x [M,K] bf16 -> q [M,K] e4m3, scale [M] fp32
//                    scale = max(amax, 2^-126 * 448) * (1/448)   (one fp32
//                    multiply, so the host reproduces it bit for bit)
//                    q = rne_e4m3(clamp(x * (1/scale), +-448))
//   gemm_fp8         Y[M,N] = act((Qa . Qw^T) * sa[m] * sw[n] + bias[n]), bf16
//
// The GEMM runs on the 256-tile skeleton of gemm_tile.h, shared with gemm.hip's
// gemm256_kernel: thread constants, both glds stages and the K-tile interleave
// come from the header; this file has the fp8 `cluster` and the epilogue. A
// K-tile is 128 fp8 = the same 128 bytes per row as 64 bf16; each pair of
// 16x16x32 bf16 MFMAs becomes one v_mfma_scale_f32_16x16x128_f8f6f4 with every
// hardware block scale 1.0.
//
// Fragment k order: a lane's 32-byte operand is the concatenation of the two
// 16-byte fragments the bf16 kernel reads for its k-steps 0 and 1. A and B
// go through the same lane->k map and all block scales are 1, so whatever k
// permutation the instruction applies inside the tile, the same products are
// summed. tests/test_fp8_linear_gpu.py checks that with exact integer data.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "gemm_tile.h"

#define QBM TILE_BM
#define QBN 256
#define QBK 128          // fp8 elements = bytes per tile row

enum { ACT_NONE = 0, ACT_SILU = 1, ACT_GELU = 2 };

// ---------------------------------------------------------------------------
// quantiser: one wave per row. Pass 1 takes the row absmax (lane-local max,
// then __shfl_xor); pass 2 re-reads the row, which is at most 32 KiB and was
// just pulled through L2 by the same wave, instead of holding up to 128
// VGPRs of it. 16-byte loads, 8-byte fp8 stores. No LDS, no atomics.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
quant_rows_fp8_kernel(const uint16_t* __restrict__ x, uint8_t* __restrict__ q,
                      float* __restrict__ scale, int K, long long nrows) {
  const long long row =
      (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= nrows) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const uint16_t* xr = x + row * K;

  float amax = 0.f;
  for (int i = lane * 8; i < K; i += 512)
    amax = fp8_absmax8(*reinterpret_cast<const ushort8_t*>(xr + i), amax);
  amax = wave_reduce_max(amax);

  const float s = fp8_row_scale(amax);
  const float inv = fp8_row_inv_scale(s);
  if (lane == 0) scale[row] = s;

  uint8_t* qr = q + row * K;
  for (int i = lane * 8; i < K; i += 512)
    *reinterpret_cast<u32x2_t*>(qr + i) =
        fp8_quant8(*reinterpret_cast<const ushort8_t*>(xr + i), inv);
}

// ---------------------------------------------------------------------------
// GEMM
// ---------------------------------------------------------------------------

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

template <int BN, int ACT>
__global__ __launch_bounds__(512, 1) void gemm_fp8_kernel(
    const uint8_t* __restrict__ A,    // [M, K] e4m3
    const uint8_t* __restrict__ Bw,   // [N, K] e4m3
    const float* __restrict__ sa,     // [M] row scales
    const float* __restrict__ sw,     // [N] output-channel scales
    const float* __restrict__ bias,   // [N] or nullptr
    const uint8_t* __restrict__ zero_page,  // >= 16 B of zeros
    uint16_t* __restrict__ Y,         // [M, N] bf16
    long long M, int N, int Kdim) {
  static_assert(BN == 256, "only the 256-wide N-tile is built");
  constexpr int NF = BN / 64;   // 16-column fragments per wave
  constexpr int NB = BN / 64;   // B glds instructions per K-tile
  constexpr unsigned B_TILE = BN * 128u;
  const TileThread t = tile_thread();
  // scalar copies for the lambdas to capture: through the struct the code is
  // the same but every register is numbered differently (r11_gemm_tile.md)
  const int wave = t.wave, wm = t.wm, wn = t.wn, fr = t.fr, kgrp = t.kgrp,
            r0 = t.r0;

  // A images then B images, one object (a second __shared__ de-pipelines
  // the glds)
  __shared__ __align__(16) uint8_t lds[65536 + 2 * BN * 128];

  const long long m_blk = (long long)blockIdx.x * QBM;
  const int n_blk = blockIdx.y * BN;

  // ---- per-thread glds chunk descriptors (K-invariant; the chunk map is in
  // gemm_tile.h). An fp8 element is a byte, so c_byte is the element offset.
  const int bn0 = n_blk + r0;
  const long long b_off = (long long)bn0 * Kdim + t.c_byte;
  long long a_off[2][2];   // [a_piece][instr]; -1 = row past M
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int pc = 0; pc < 2; ++pc) {
      const long long m = t.a_row(m_blk, pc, i);
      a_off[pc][i] = m < M ? m * (long long)Kdim + t.c_byte : -1;
    }

  f32x4_t acc[8][NF];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int kt_end = Kdim / QBK;

  // fragment read addresses: image row (wave's 64-row group + fr), 16-byte
  // k-group kgrp, swizzled once. A quarter qq = mq*2 + wm is rows qq*64..;
  // a wave's B strip is rows wn*64..
  unsigned a_lane = swz((unsigned)((wm * 64 + fr) * 128 + kgrp * 16));
  unsigned b_lane =
      swz((unsigned)((wn * (BN / 4) + fr) * 128 + kgrp * 16));
  // opaque, so the reads stay one address register + immediate offsets
  asm volatile("" : "+v"(a_lane), "+v"(b_lane));
  const uint8_t* lds_a = lds + TILE_ABUF + a_lane;
  const uint8_t* lds_b = lds + TILE_BBUF + b_lane;

  auto stage_b = [&](int kt, int p, auto J0, auto JN) {
    tile_stage_b<false, decltype(J0)::value, decltype(JN)::value>(
        Bw, zero_page, b_off, bn0, N, Kdim, kt * QBK,
        lds + (unsigned)TILE_BBUF + p * B_TILE, wave);
  };

  auto stage_a = [&](int kt, int p, int pc) {
    tile_stage_a(A, zero_page,
                 [&](int i, long long& off) {
                   off = a_off[pc][i];
                   return off >= 0;
                 },
                 kt * QBK,
                 lds + (unsigned)TILE_ABUF + p * TILE_IMG + pc * 16384u,
                 wave);
  };

  // one cluster: A rows of half mq x fragments [nf0, nf0+nfn) over the
  // K-tile's 128-deep K: 4*nfn MFMAs
  auto cluster = [&](int p, auto MQ, auto NF0, auto NFN) {
    constexpr int mq = decltype(MQ)::value;
    constexpr int nf0 = decltype(NF0)::value;
    constexpr int nfn = decltype(NFN)::value;
    // per-lane swizzled base + compile-time offsets: swz only touches bit 5
    // from bit 9 (fr bit 2), and the mq / mf / nf / k-half terms are bits
    // 6 and >= 11, so they add to the lane address outside the swizzle
    // keep this cluster's reads behind the previous cluster's MFMAs: hoisted,
    // two clusters' fragments are live at once and the accumulators spill
    __builtin_amdgcn_sched_barrier(0);
    const uint8_t* ap = lds_a + p * TILE_IMG;
    const uint8_t* bp = lds_b + p * B_TILE;
    i32x8_t af[4], bfr[nfn];
#pragma unroll
    for (int mf = 0; mf < 4; ++mf) {
      constexpr unsigned base = mq * 16384u;
      const i32x4_t h0 =
          *reinterpret_cast<const i32x4_t*>(ap + base + mf * 2048u);
      const i32x4_t h1 =
          *reinterpret_cast<const i32x4_t*>(ap + base + mf * 2048u + 64u);
      af[mf] = i32x8_t{h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
    }
#pragma unroll
    for (int nf = 0; nf < nfn; ++nf) {
      const i32x4_t h0 =
          *reinterpret_cast<const i32x4_t*>(bp + (nf0 + nf) * 2048u);
      const i32x4_t h1 =
          *reinterpret_cast<const i32x4_t*>(bp + (nf0 + nf) * 2048u + 64u);
      bfr[nf] = i32x8_t{h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int mf = 0; mf < 4; ++mf)
#pragma unroll
      for (int nf = 0; nf < nfn; ++nf)
        // operands swapped (W fragment first): the 16x16 result is the
        // transposed tile, a lane holds 4 adjacent COLUMNS n = kgrp*4 + reg
        // of row m = fr. cbsz = blgp = 0: e4m3 for both; E8M0 scale bytes
        // 0x7f = 1.0
        acc[mq * 4 + mf][nf0 + nf] =
            __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                bfr[nf], af[mf], acc[mq * 4 + mf][nf0 + nf], 0, 0, 0,
                0x7f7f7f7f, 0, 0x7f7f7f7f);
    __builtin_amdgcn_s_setprio(0);
  };

  // ---- main loop: prologue stage, then one tile_ktile per K-tile ---------
  stage_b(0, 0, ic<0>{}, ic<NB>{});
  stage_a(0, 0, 0);
  stage_a(0, 0, 1);
  // The staging is unconditional (std::true_type): the last K-tile stages
  // itself once more into the idle buffer (in bounds, never read). With an
  // `if (more)` around each stage the loop body is nine basic blocks, and the
  // compiler sinks all 32 MFMAs below the last of them, behind the fragment
  // reads of all four clusters: 200+ bytes/lane of scratch.
  for (int kt = 0; kt < kt_end; ++kt) {
    const int ktn = kt + 1 < kt_end ? kt + 1 : kt;
    tile_ktile<BN>(kt & 1, ktn, std::true_type{}, stage_b, stage_a, cluster);
  }
  // the last tile's redundant stage must land before the workgroup's LDS
  // can be handed to another
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // ---- epilogue: row scale, channel scale, bias, activation, bf16 store --
  const long long m_wave = m_blk + wm * 128;
  const int n_wave = n_blk + wn * (BN / 4);
  const bool vec4 = (N & 3) == 0;

#pragma unroll
  for (int mf = 0; mf < 8; ++mf) {
    const long long m = m_wave + mf * 16 + fr;
    if (m >= M) continue;
    const float s_m = sa[m];
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
      const int n0 = n_wave + nf * 16 + kgrp * 4;
      if (n0 >= N) continue;
      if (vec4) {
        const f32x4_t s_n = *reinterpret_cast<const f32x4_t*>(sw + n0);
        f32x4_t v = acc[mf][nf] * s_m * s_n;
        if (bias) v += *reinterpret_cast<const f32x4_t*>(bias + n0);
        u16x4_t o;
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = f32_to_bf16_bits(act_q<ACT>(v[c]));
        *reinterpret_cast<u16x4_t*>(Y + m * N + n0) = o;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (n0 + c >= N) break;
          float v = acc[mf][nf][c] * s_m * sw[n0 + c];
          if (bias) v += bias[n0 + c];
          Y[m * N + n0 + c] = f32_to_bf16_bits(act_q<ACT>(v));
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

std::tuple<torch::Tensor, torch::Tensor> quant_rows_fp8(torch::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous(),
              "x must be contiguous [M, K] on device");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "x must be bf16");
  const long long M = x.size(0), K = x.size(1);
  TORCH_CHECK(K % 128 == 0 && K >= 128 && K <= 16384,
              "K must be a multiple of 128 in [128, 16384], got ", K);
  TORCH_CHECK((reinterpret_cast<uintptr_t>(x.data_ptr()) & 15) == 0,
              "x must be 16-byte aligned");
  auto q = torch::empty({M, K}, x.options().dtype(at::kFloat8_e4m3fn));
  auto scale = torch::empty({M}, x.options().dtype(at::kFloat));
  if (M == 0) return {q, scale};
  const int waves_per_block = 4;
  const long long nblocks = (M + waves_per_block - 1) / waves_per_block;
  TORCH_CHECK(nblocks < (1LL << 31), "quant_rows_fp8: too many rows");
  hipLaunchKernelGGL(quant_rows_fp8_kernel, dim3((unsigned)nblocks),
                     dim3(64 * waves_per_block), 0,
                     at::hip::getCurrentHIPStream(),
                     (const uint16_t*)x.data_ptr(), (uint8_t*)q.data_ptr(),
                     scale.data_ptr<float>(), (int)K, M);
  HIP_CHECK_LAUNCH();
  return {q, scale};
}

torch::Tensor gemm_fp8(torch::Tensor qa, torch::Tensor sa, torch::Tensor qw,
                       torch::Tensor sw, torch::Tensor bias, int64_t act) {
  // qa [M, K] e4m3, sa [M] fp32, qw [N, K] e4m3 (torch Linear layout),
  // sw [N] fp32, bias [N] (any float dtype) or empty -> y [M, N] bf16
  TORCH_CHECK(qa.is_cuda() && qa.dim() == 2 && qa.is_contiguous() &&
                  qa.scalar_type() == at::kFloat8_e4m3fn,
              "qa must be a contiguous float8_e4m3fn [M, K] on device");
  TORCH_CHECK(qw.is_cuda() && qw.dim() == 2 && qw.is_contiguous() &&
                  qw.scalar_type() == at::kFloat8_e4m3fn,
              "qw must be a contiguous float8_e4m3fn [N, K] on device");
  const long long M = qa.size(0);
  const long long K = qa.size(1), N = qw.size(0);
  TORCH_CHECK(qw.size(1) == K, "qa and qw disagree on K");
  TORCH_CHECK(K % QBK == 0 && K >= QBK, "K must be a multiple of 128, got ", K);
  TORCH_CHECK(N >= 1 && N < (1LL << 31) && K < (1LL << 31));
  TORCH_CHECK(sa.is_cuda() && sa.scalar_type() == at::kFloat &&
                  sa.is_contiguous() && sa.numel() == M,
              "sa must be contiguous fp32 [M]");
  TORCH_CHECK(sw.is_cuda() && sw.scalar_type() == at::kFloat &&
                  sw.is_contiguous() && sw.numel() == N,
              "sw must be contiguous fp32 [N]");
  TORCH_CHECK(act >= ACT_NONE && act <= ACT_GELU,
              "act must be 0 (none), 1 (SiLU) or 2 (GELU-tanh)");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(qa.data_ptr()) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(qw.data_ptr()) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(sw.data_ptr()) & 15) == 0,
              "qa, qw and sw must be 16-byte aligned");
  auto y = torch::empty({M, N}, qa.options().dtype(at::kBFloat16));
  if (M == 0) return y;
  torch::Tensor bf32;
  TORCH_CHECK(!bias.defined() || bias.numel() == 0 ||
                  (bias.is_cuda() && bias.numel() == N),
              "bias must be [N]");
  const float* bptr = bias_f32_ptr(bias, bf32);
  TORCH_CHECK((reinterpret_cast<uintptr_t>(bptr) & 15) == 0,
              "bias must be 16-byte aligned");
  const long long gx = (M + QBM - 1) / QBM, gy = (N + QBN - 1) / QBN;
  TORCH_CHECK(gx < (1LL << 31) && gy < 65536, "gemm_fp8: grid too large");
  dim3 grid((unsigned)gx, (unsigned)gy);
  auto stream = at::hip::getCurrentHIPStream();
  const uint8_t* zp = (const uint8_t*)device_zero_page(qa);
#define LAUNCH_Q(ACTV)                                                        \
  hipLaunchKernelGGL((gemm_fp8_kernel<QBN, ACTV>), grid, dim3(512), 0,        \
                     stream, (const uint8_t*)qa.data_ptr(),                   \
                     (const uint8_t*)qw.data_ptr(), sa.data_ptr<float>(),     \
                     sw.data_ptr<float>(), bptr, zp, (uint16_t*)y.data_ptr(), \
                     M, (int)N, (int)K)
  if (act == ACT_SILU) LAUNCH_Q(ACT_SILU);
  else if (act == ACT_GELU) LAUNCH_Q(ACT_GELU);
  else LAUNCH_Q(ACT_NONE);
#undef LAUNCH_Q
  HIP_CHECK_LAUNCH();
  return y;
}
