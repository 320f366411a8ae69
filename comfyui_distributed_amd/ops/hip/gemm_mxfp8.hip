// MXFP8 activation rows (OCP microscaling: e4m3 codes, one E8M0 power-of-two
// scale per 32 adjacent K-elements of a row) for the FP8 Linear path:
//
//   quant_rows_mxfp8   x [M,K] bf16 -> q [M,K] e4m3, e [M,K/32] E8M0 bytes
//   gemm_mxfp8         Y[m][n] = act((sum_kb 2^exp[m][kb] *
//                          dot32(qa[m][kb], qw[n][kb])) * sw[n] + bias[n])
//                      as bf16 [M,N], or (EMIT) as the MX rows
//                      quant_rows_mxfp8 makes of that bf16 result
//
// Block exponent (mx_scale_byte): the smallest power of two 2^exp with
// amax * 2^-exp <= 448, from the bits of amax: exp = E - 8 for a mantissa up
// to 1.75, E - 7 above it, clamped to the E8M0 range; codes are
// rne_e4m3(clamp(x * 2^-exp, +-448)). dispatch.py has the same definition in
// torch and the tests compare the two bit for bit.
//
// The weights stay what gemm_fp8 reads (e4m3, one fp32 scale per output
// channel, hardware block scale 1.0), so the GEMM is the 256-tile skeleton of
// gemm_tile.h again. It differs from gemm_fp8_kernel in three places:
//
// 1. Which scale meets which 32 K-elements. The scale byte that the lanes of
//    k-group b (lanes 16b .. 16b+15) supply is applied to K-elements
//    [32b, 32b+32) of the instruction's K order, not to the 32 bytes those
//    lanes hold: in that order a lane of k-group g holds [16g, 16g+16) in its
//    first four registers and [64+16g, 64+16g+16) in the last four. That is
//    the operand gemm_fp8_kernel already builds from LDS slots g and 4+g, so
//    the stage, the images and the conflict-free fragment reads are the
//    parent's unchanged, and lane (fr, b) supplies row fr's scale of block b.
//    (Permuting the rows so that a lane holds [32g, 32g+32) puts every second
//    half-block under a neighbour's scale: tests/test_mxfp8_gpu.py's integer
//    test tells the two apart.)
// 2. Scale bytes. A lane (row fr, k-group g) needs byte g of the dword
//    e[m][4kt..4kt+3] for each of its 8 A rows. The 8 dwords of K-tile kt+1
//    are loaded into registers right after K-tile kt's barrier (all 4 k-group
//    lanes of a row read the same dword), so they land under a whole tile of
//    MFMAs, and are shifted by 8g when they become current: op_sel stays 0.
//    Rows past M read row M-1; their codes come from the zero page.
// 3. EMIT: the epilogue rounds to bf16 in registers and quantises that. With
//    swapped operands a lane holds 4 adjacent columns per fragment, a wave's
//    strip is 64 columns from a multiple of 64, so a 32-column block is the
//    fragment pair (2j, 2j+1) across the 4 lanes fr + 16g: lane-local max of
//    8, two cross-lane steps, two 4-byte code stores, one scale byte.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "gemm_tile.h"
#include "fp8_act.h"

#define MXBM TILE_BM
#define MXBN 256
#define MXBK 128         // fp8 elements = bytes per tile row = 4 MX blocks

// E8M0 byte (exp + 127) of a block with absmax `amax` >= 0. be - 127 = E; a
// zero or subnormal amax has be = 0 and clamps to byte 0 = 2^-127.
__device__ __forceinline__ unsigned mx_scale_byte(float amax) {
  const unsigned bits = __float_as_uint(amax);
  const int e = (int)(bits >> 23) - 8 + ((bits & 0x7fffffu) > 0x600000u);
  return (unsigned)min(max(e, 0), 254);
}

// 2^-exp = 2^(127 - byte). byte <= 247 (the largest finite amax), so this is
// a normal fp32 and x * 2^-exp is exact
__device__ __forceinline__ float mx_inv_scale(unsigned byte) {
  return __uint_as_float((254u - byte) << 23);
}

// ---------------------------------------------------------------------------
// quantiser: one wave per row, one pass. A lane's 16-byte load is a quarter of
// a block, so the block absmax is the lane-local max and two xor steps inside
// groups of 4 lanes; the scale is known then, no second read of the row.
// 8-byte code stores; the 4 scale bytes of 16 lanes go out as one dword. K %
// 128 == 0 keeps every group of 16 lanes wholly inside or outside the loop.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) FP8_NO_PK_F32
quant_rows_mxfp8_kernel(const uint16_t* __restrict__ x, uint8_t* __restrict__ q,
                        uint8_t* __restrict__ e, int K, long long nrows) {
  const long long row =
      (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= nrows) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const uint16_t* xr = x + row * K;
  uint8_t* qr = q + row * K;
  uint8_t* er = e + row * (K >> 5);

  for (int i = lane * 8; i < K; i += 512) {
    const ushort8_t v = *reinterpret_cast<const ushort8_t*>(xr + i);
    float amax = fp8_absmax8(v, 0.f);
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
    const unsigned eb = mx_scale_byte(amax);
    *reinterpret_cast<u32x2_t*>(qr + i) = fp8_quant8(v, mx_inv_scale(eb));
    // bytes of lanes L, L+4, L+8, L+12 -> one dword in lane L = 0 mod 16
    unsigned g = eb | ((unsigned)__shfl_xor((int)eb, 4, 64) << 8);
    g |= (unsigned)__shfl_xor((int)g, 8, 64) << 16;
    if ((lane & 15) == 0) *reinterpret_cast<unsigned*>(er + (i >> 5)) = g;
  }
}

// ---------------------------------------------------------------------------
// GEMM
// ---------------------------------------------------------------------------
// One 256 x BN output tile over the whole K. A function of its own, inlined
// into the kernel below: the lambdas then belong to a function with the
// default target features and inline into it; written in the __global__, whose
// target attribute they do not inherit, they stay calls.
template <int BN, int ACT, bool EMIT>
__device__ __forceinline__ void gemm_mxfp8_tile(
    const uint8_t* __restrict__ A,    // [M, K] e4m3
    const uint8_t* __restrict__ Bw,   // [N, K] e4m3
    const uint8_t* __restrict__ Ea,   // [M, K/32] E8M0 block scales of A
    const float* __restrict__ sw,     // [N] output-channel scales
    const float* __restrict__ bias,   // [N] or nullptr
    const uint8_t* __restrict__ zero_page,  // >= 16 B of zeros
    uint16_t* __restrict__ Y,         // !EMIT: [M, N] bf16
    uint8_t* __restrict__ Qo,         // EMIT: [M, N] e4m3
    uint8_t* __restrict__ Eo,         // EMIT: [M, N/32] E8M0
    int M, int N, int Kdim) {
  static_assert(BN == 256, "only the 256-wide N-tile is built");
  static_assert(ACT != ACT_GEGLU, "no GEGLU epilogue here");
  constexpr int NF = BN / 64;   // 16-column fragments per wave
  constexpr int NB = BN / 64;   // B glds instructions per K-tile
  constexpr unsigned B_TILE = BN * 128u;
  const TileThread t = tile_thread();
  const int wave = t.wave, wm = t.wm, wn = t.wn, fr = t.fr, kgrp = t.kgrp,
            r0 = t.r0;

  __shared__ __align__(16) uint8_t lds[65536 + 2 * BN * 128];

  const int m_blk = blockIdx.x * MXBM;
  const int n_blk = blockIdx.y * BN;

  // ---- glds chunk descriptors, as in gemm_fp8_kernel
  const int bn0 = n_blk + r0;
  const long long b_off = (long long)bn0 * Kdim + t.c_byte;
  long long a_off[2][2];   // [a_piece][instr]; -1 = row past M
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int pc = 0; pc < 2; ++pc) {
      const int m = t.a_row(m_blk, pc, i);
      a_off[pc][i] = m < M ? m * (long long)Kdim + t.c_byte : -1;
    }

  f32x4_t acc[8][NF];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int kt_end = Kdim / MXBK;

  unsigned a_lane = swz((unsigned)((wm * 64 + fr) * 128 + kgrp * 16));
  unsigned b_lane =
      swz((unsigned)((wn * (BN / 4) + fr) * 128 + kgrp * 16));
  asm volatile("" : "+v"(a_lane), "+v"(b_lane));
  const uint8_t* lds_a = lds + TILE_ABUF + a_lane;
  const uint8_t* lds_b = lds + TILE_BBUF + b_lane;

  // ---- block scales of this lane's 8 A rows m_blk + wm*128 + 16*i + fr:
  // sc_next holds the raw dwords e[m][4kt..4kt+3] of the K-tile being staged,
  // sc the current tile's, shifted so that byte 0 is this lane's block kgrp.
  // The row offsets are recomputed per K-tile (3 VALU each) instead of held
  // in 8 more registers; the launcher keeps M * K/32 below 2^31.
  const int m_lane = m_blk + wm * 128 + fr;
  const unsigned sc_shift = (unsigned)kgrp * 8u;
  unsigned sc[8], sc_next[8];
  auto load_scales = [&](int kt) {
    int m0 = m_lane;
    asm volatile("" : "+v"(m0));  // not loop-invariant to the compiler
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const unsigned off =
          ((unsigned)min(m0 + 16 * i, M - 1) * (unsigned)kt_end + kt) * 4u;
      sc_next[i] = *reinterpret_cast<const unsigned*>(Ea + off);
    }
  };

  auto stage_b = [&](int kt, int p, auto J0, auto JN) {
    // the first stage call of a K-tile follows its barrier: the scale loads
    // go first and have the whole tile to land
    if constexpr (decltype(J0)::value == 0) load_scales(kt);
    tile_stage_b<false, decltype(J0)::value, decltype(JN)::value>(
        Bw, zero_page, b_off, bn0, N, Kdim, kt * MXBK,
        lds + (unsigned)TILE_BBUF + p * B_TILE, wave);
  };

  auto stage_a = [&](int kt, int p, int pc) {
    tile_stage_a(A, zero_page,
                 [&](int i, long long& off) {
                   off = a_off[pc][i];
                   return off >= 0;
                 },
                 kt * MXBK,
                 lds + (unsigned)TILE_ABUF + p * TILE_IMG + pc * 16384u,
                 wave);
  };

  // one cluster, as gemm_fp8_kernel's: A rows of half mq x fragments
  // [nf0, nf0+nfn); the A operand carries the lane's block scale
  auto cluster = [&](int p, auto MQ, auto NF0, auto NFN) {
    constexpr int mq = decltype(MQ)::value;
    constexpr int nf0 = decltype(NF0)::value;
    constexpr int nfn = decltype(NFN)::value;
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
        // operands swapped (W fragment first, scale 1.0 = 0x7f); the second
        // operand's scale is byte 0 of sc: 2^exp of row fr, block kgrp of
        // the K-tile
        acc[mq * 4 + mf][nf0 + nf] =
            __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                bfr[nf], af[mf], acc[mq * 4 + mf][nf0 + nf], 0, 0, 0,
                0x7f7f7f7f, 0, (int)sc[mq * 4 + mf]);
    __builtin_amdgcn_s_setprio(0);
  };

  // ---- main loop (unconditional staging, as in gemm_fp8_kernel) ----------
  stage_b(0, 0, ic<0>{}, ic<NB>{});
  stage_a(0, 0, 0);
  stage_a(0, 0, 1);
  for (int kt = 0; kt < kt_end; ++kt) {
    const int ktn = kt + 1 < kt_end ? kt + 1 : kt;
#pragma unroll
    for (int i = 0; i < 8; ++i) sc[i] = sc_next[i] >> sc_shift;
    tile_ktile<BN>(kt & 1, ktn, std::true_type{}, stage_b, stage_a, cluster);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // ---- epilogue ----------------------------------------------------------
  const int m_wave = m_blk + wm * 128;
  const int n_wave = n_blk + wn * (BN / 4);

  if constexpr (EMIT) {
    // N % 32 == 0: a block is whole or absent, wave-uniformly, so the
    // shuffles run with every lane; only the stores look at the row
    const int nblk = N >> 5;
#pragma unroll
    for (int mf = 0; mf < 8; ++mf) {
      const int m = m_wave + mf * 16 + fr;
#pragma unroll
      for (int j = 0; j < NF / 2; ++j) {
        const int nb0 = n_wave + 32 * j;
        if (nb0 >= N) continue;
        const int n0 = nb0 + kgrp * 4;
        ushort8_t hb;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          f32x4_t v = acc[mf][2 * j + h] *
                      *reinterpret_cast<const f32x4_t*>(sw + n0 + 16 * h);
          if (bias) v += *reinterpret_cast<const f32x4_t*>(bias + n0 + 16 * h);
#pragma unroll
          for (int c = 0; c < 4; ++c)
            hb[4 * h + c] = f32_to_bf16_bits(act_q<ACT>(v[c]));
        }
        float amax = fp8_absmax8(hb, 0.f);
        amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
        amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
        const unsigned eb = mx_scale_byte(amax);
        const u32x2_t w = fp8_quant8(hb, mx_inv_scale(eb));
        if (m < M) {
          uint8_t* qp = Qo + (long long)m * N + n0;
          *reinterpret_cast<unsigned*>(qp) = w[0];
          *reinterpret_cast<unsigned*>(qp + 16) = w[1];
          if (kgrp == 0) Eo[(long long)m * nblk + (nb0 >> 5)] = (uint8_t)eb;
        }
      }
    }
    return;
  }

  const bool vec4 = (N & 3) == 0;
#pragma unroll
  for (int mf = 0; mf < 8; ++mf) {
    const int m = m_wave + mf * 16 + fr;
    if (m >= M) continue;
    uint16_t* yr = Y + (long long)m * N;
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
      const int n0 = n_wave + nf * 16 + kgrp * 4;
      if (n0 >= N) continue;
      if (vec4) {
        f32x4_t v = acc[mf][nf] * *reinterpret_cast<const f32x4_t*>(sw + n0);
        if (bias) v += *reinterpret_cast<const f32x4_t*>(bias + n0);
        u16x4_t o;
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = f32_to_bf16_bits(act_q<ACT>(v[c]));
        *reinterpret_cast<u16x4_t*>(yr + n0) = o;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (n0 + c >= N) break;
          float v = acc[mf][nf][c] * sw[n0 + c];
          if (bias) v += bias[n0 + c];
          yr[n0 + c] = f32_to_bf16_bits(act_q<ACT>(v));
        }
      }
    }
  }
}

// Without packed fp32 arithmetic, as gemm_fp8_geglu_kernel: the epilogues
// would otherwise pair their scale / bias arithmetic into v_pk_*_f32.
template <int BN, int ACT, bool EMIT>
__global__ __launch_bounds__(512, 1) FP8_NO_PK_F32 void gemm_mxfp8_kernel(
    const uint8_t* __restrict__ A, const uint8_t* __restrict__ Bw,
    const uint8_t* __restrict__ Ea, const float* __restrict__ sw,
    const float* __restrict__ bias, const uint8_t* __restrict__ zero_page,
    uint16_t* __restrict__ Y, uint8_t* __restrict__ Qo,
    uint8_t* __restrict__ Eo, int M, int N, int Kdim) {
  gemm_mxfp8_tile<BN, ACT, EMIT>(A, Bw, Ea, sw, bias, zero_page, Y, Qo, Eo, M,
                                 N, Kdim);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

std::tuple<torch::Tensor, torch::Tensor> quant_rows_mxfp8(torch::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous(),
              "x must be contiguous [M, K] on device");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "x must be bf16");
  const long long M = x.size(0), K = x.size(1);
  TORCH_CHECK(K % 128 == 0 && K >= 128 && K <= 16384,
              "K must be a multiple of 128 in [128, 16384], got ", K);
  TORCH_CHECK((reinterpret_cast<uintptr_t>(x.data_ptr()) & 15) == 0,
              "x must be 16-byte aligned");
  auto q = torch::empty({M, K}, x.options().dtype(at::kFloat8_e4m3fn));
  auto e = torch::empty({M, K / 32}, x.options().dtype(at::kByte));
  if (M == 0) return {q, e};
  const int waves_per_block = 4;
  const long long nblocks = (M + waves_per_block - 1) / waves_per_block;
  TORCH_CHECK(nblocks < (1LL << 31), "quant_rows_mxfp8: too many rows");
  hipLaunchKernelGGL(quant_rows_mxfp8_kernel, dim3((unsigned)nblocks),
                     dim3(64 * waves_per_block), 0,
                     at::hip::getCurrentHIPStream(),
                     (const uint16_t*)x.data_ptr(), (uint8_t*)q.data_ptr(),
                     (uint8_t*)e.data_ptr(), (int)K, M);
  HIP_CHECK_LAUNCH();
  return {q, e};
}

// qa [M, K] e4m3, ea [M, K/32] uint8, qw [N, K] e4m3 (torch Linear layout),
// sw [N] fp32, bias [N] (any float dtype) or empty. emit = false: {y [M, N]
// bf16}; emit = true (N % 32 == 0): {q [M, N] e4m3, e [M, N/32] uint8}
static std::vector<torch::Tensor> gemm_mxfp8_run(
    const torch::Tensor& qa, const torch::Tensor& ea, const torch::Tensor& qw,
    const torch::Tensor& sw, const torch::Tensor& bias, int act, bool emit) {
  TORCH_CHECK(act >= ACT_NONE && act <= ACT_GELU,
              "act must be 0 (none), 1 (SiLU) or 2 (GELU-tanh)");
  TORCH_CHECK(qa.is_cuda() && qa.dim() == 2 && qa.is_contiguous() &&
                  qa.scalar_type() == at::kFloat8_e4m3fn,
              "qa must be a contiguous float8_e4m3fn [M, K] on device");
  TORCH_CHECK(qw.is_cuda() && qw.dim() == 2 && qw.is_contiguous() &&
                  qw.scalar_type() == at::kFloat8_e4m3fn,
              "qw must be a contiguous float8_e4m3fn [N, K] on device");
  const long long M = qa.size(0);
  const long long K = qa.size(1), N = qw.size(0);
  TORCH_CHECK(qw.size(1) == K, "qa and qw disagree on K");
  TORCH_CHECK(K % MXBK == 0 && K >= MXBK && K <= 16384,
              "K must be a multiple of 128 in [128, 16384], got ", K);
  TORCH_CHECK(N >= 1 && N < (1LL << 31));
  TORCH_CHECK(ea.is_cuda() && ea.scalar_type() == at::kByte &&
                  ea.is_contiguous() && ea.dim() == 2 && ea.size(0) == M &&
                  ea.size(1) == K / 32,
              "ea must be contiguous uint8 [M, K/32]");
  // the kernel indexes rows and scale dwords in 32 bits
  TORCH_CHECK(M * (K / 32) < (1LL << 31) && M + MXBM < (1LL << 31),
              "gemm_mxfp8: M * K / 32 must be below 2^31");
  TORCH_CHECK(sw.is_cuda() && sw.scalar_type() == at::kFloat &&
                  sw.is_contiguous() && sw.numel() == N,
              "sw must be contiguous fp32 [N]");
  TORCH_CHECK(!emit || N % 32 == 0,
              "emit: N must be a multiple of 32, got ", N);
  TORCH_CHECK((reinterpret_cast<uintptr_t>(qa.data_ptr()) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(qw.data_ptr()) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(sw.data_ptr()) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(ea.data_ptr()) & 3) == 0,
              "qa, qw and sw must be 16-byte aligned, ea 4-byte aligned");
  std::vector<torch::Tensor> out;
  if (emit) {
    out.push_back(torch::empty({M, N}, qa.options()));
    out.push_back(torch::empty({M, N / 32}, qa.options().dtype(at::kByte)));
  } else {
    out.push_back(torch::empty({M, N}, qa.options().dtype(at::kBFloat16)));
  }
  if (M == 0) return out;
  torch::Tensor bf32;
  TORCH_CHECK(!bias.defined() || bias.numel() == 0 ||
                  (bias.is_cuda() && bias.numel() == N),
              "bias must be [N]");
  const float* bptr = bias_f32_ptr(bias, bf32);
  TORCH_CHECK((reinterpret_cast<uintptr_t>(bptr) & 15) == 0,
              "bias must be 16-byte aligned");
  const long long gx = (M + MXBM - 1) / MXBM, gy = (N + MXBN - 1) / MXBN;
  TORCH_CHECK(gy < 65536, "gemm_mxfp8: grid too large");
  dim3 grid((unsigned)gx, (unsigned)gy);
  auto stream = at::hip::getCurrentHIPStream();
  const uint8_t* zp = (const uint8_t*)device_zero_page(qa);
  uint16_t* yp = emit ? nullptr : (uint16_t*)out[0].data_ptr();
  uint8_t* qp = emit ? (uint8_t*)out[0].data_ptr() : nullptr;
  uint8_t* ep = emit ? (uint8_t*)out[1].data_ptr() : nullptr;
#define LAUNCH_MX(ACT, EMIT)                                                  \
  hipLaunchKernelGGL((gemm_mxfp8_kernel<MXBN, ACT, EMIT>), grid, dim3(512),   \
                     0, stream, (const uint8_t*)qa.data_ptr(),                \
                     (const uint8_t*)qw.data_ptr(),                           \
                     (const uint8_t*)ea.data_ptr(), sw.data_ptr<float>(),     \
                     bptr, zp, yp, qp, ep, (int)M, (int)N, (int)K)
#define LAUNCH_MX_ACT(EMIT)                                  \
  do {                                                       \
    if (act == ACT_SILU) LAUNCH_MX(ACT_SILU, EMIT);          \
    else if (act == ACT_GELU) LAUNCH_MX(ACT_GELU, EMIT);     \
    else LAUNCH_MX(ACT_NONE, EMIT);                          \
  } while (0)
  if (emit) LAUNCH_MX_ACT(true);
  else LAUNCH_MX_ACT(false);
#undef LAUNCH_MX_ACT
#undef LAUNCH_MX
  HIP_CHECK_LAUNCH();
  return out;
}

torch::Tensor gemm_mxfp8(torch::Tensor qa, torch::Tensor ea, torch::Tensor qw,
                         torch::Tensor sw, torch::Tensor bias, int64_t act) {
  return gemm_mxfp8_run(qa, ea, qw, sw, bias, (int)act, false)[0];
}

std::tuple<torch::Tensor, torch::Tensor> gemm_mxfp8_emit(
    torch::Tensor qa, torch::Tensor ea, torch::Tensor qw, torch::Tensor sw,
    torch::Tensor bias, int64_t act) {
  auto out = gemm_mxfp8_run(qa, ea, qw, sw, bias, (int)act, true);
  return {out[0], out[1]};
}
