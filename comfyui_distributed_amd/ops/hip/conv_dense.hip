// Dense-block convolution for the RRDBNet (ESRGAN) upscale model: 3x3,
// stride 1, pad 1, NHWC bf16, narrow K_out (1..64), operands that are channel
// slices of wider NHWC buffers.
//
//   t   = sum_{r,s,c<C_in} x[b, y+r-1, x+s-1, c] * w[k, r, s, c] + bias[k]
//   t   = t > 0 ? t : slope * t                          (lrelu)
//   out = bf16(alpha * t + beta1 * res1 + res2)          (one rounding)
//
// The shape class: N = K_out <= 64 gives no reuse of the activations across
// output columns, so the reuse there is lies in the nine taps. A workgroup of
// 8 waves owns an 8 x 32-pixel output tile and walks C_in in 32-channel
// chunks. Per chunk it stages, in LDS,
//   - the 10 x 34 halo patch of the tile (340 pixels x 64 B), read from global
//     once instead of nine times (1.33x the input in all), and
//   - the chunk's 9 x NF*16 x 32 weights beside it,
// both at an 80-byte row pitch (32 channels + 16 B pad): the 16 rows of a
// ds_read_b128 fragment read then start 20 banks apart and cover the 64 banks
// once, the pitch conv.hip's staged weights use. The nine taps are nine
// shifted fragment reads out of the patch: tap (r, s) of the wave's tile row
// `wave` is patch row wave + r from column s on.
//
// Chunks are staged through registers one chunk ahead (as attention.hip stages
// K and V): the 16-byte pieces of chunk i+1 are loaded from global before the
// MFMAs of chunk i and committed to LDS between the two barriers at the top of
// the next trip. Out-of-image halo pixels, channels of the weight past K_out
// and piece slots past the end are zero registers, decided once per thread
// before the loop (an offset of -1), so there is no bounds arithmetic and no
// zero page in the loop. One LDS image, 38 / 49 / 72 KB at NF = 1 / 2 / 4:
// two to four workgroups per CU cover each other's barriers.
//
// Each wave holds 2 x NF accumulators (its tile row's 32 pixels x NF*16
// channels). The MFMA operands are swapped (weights as A, pixels as B), which
// leaves 4 adjacent output channels of one pixel on a lane: 8-byte epilogue
// loads of res1 / res2 and 8-byte stores; the masked N tail (K_out = 3) goes
// element by element.
//
// Addressing: the image and tile-row base of every operand is a 64-bit
// pointer computed once per workgroup; inside the workgroup 32-bit element
// offsets of at most 10 rows are added (the launcher checks 10 * W * pitch
// < 2^31), so operands above 2 GiB work. `up2` reads source pixel
// (y >> 1, x >> 1) with bounds on the upsampled size; the upsampled tensor is
// never written.
//
// Aliasing: out may be elementwise identical to res1 or res2 (the lane that
// stores an element is the one that loaded it); out may share a buffer with x
// when their channel ranges are disjoint (dispatch.conv3x3_dense checks).
// No atomics, no memset, no workspace, no scratch: capture-safe.
//
// Reference counterpart: the ImageUpscaleWithModel step of the reference's
// distributed-upscale workflow (spandrel's RRDBNet on the host application).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) short short4v;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define CD_ZERO8 short8{0, 0, 0, 0, 0, 0, 0, 0}
#define CD_TH 8                      // tile rows = waves
#define CD_TW 32                     // tile columns = 2 fragments
#define CD_PH (CD_TH + 2)
#define CD_PW (CD_TW + 2)
#define CD_PITCH 40                  // elements per LDS row (32 + 8 pad = 80 B)
#define CD_THREADS (CD_TH * 64)
#define CD_PATCH_PIECES (CD_PH * CD_PW * 4)   // 16-byte pieces of a patch chunk
#define CD_PSLOTS ((CD_PATCH_PIECES + CD_THREADS - 1) / CD_THREADS)

struct DenseArgs {
  const uint16_t* x;      // (b, 0, 0, 0) of the source view
  const uint16_t* wt;     // [K, 9 * C]
  const float* bias;      // [K] or nullptr
  uint16_t* out;
  const uint16_t* res1;   // or nullptr
  const uint16_t* res2;   // or nullptr
  long long x_pitch, out_pitch, r1_pitch, r2_pitch;   // elements per pixel
  int Hs, Ws;             // source size
  int Ho, Wo;             // output size (2x the source with up2)
  int C, K;
  int tiles_x, tiles_y;
  int up2, lrelu;
  float slope, alpha, beta1;
};

// the epilogue's multiply-adds must not pair into v_pk_*_f32
#if defined(__HIP_DEVICE_COMPILE__)  // the host pass does not know the feature
#define CD_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define CD_NO_PK_F32
#endif

template <int NF>
__global__ __launch_bounds__(CD_THREADS, 4) CD_NO_PK_F32 void conv_dense_kernel(
    const DenseArgs a) {
  constexpr int NK = NF * 16;                  // weight rows per tap
  constexpr int W_PIECES = 9 * NK * 4;
  constexpr int WSLOTS = (W_PIECES + CD_THREADS - 1) / CD_THREADS;
  __shared__ __align__(16) uint16_t lds[(CD_PH * CD_PW + 9 * NK) * CD_PITCH];
  uint16_t* const patch = lds;
  uint16_t* const wl = lds + CD_PH * CD_PW * CD_PITCH;

  const uint16_t* const wt = a.wt;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int fr = lane & 15;
  const int kgrp = lane >> 4;

  unsigned bid = blockIdx.x;
  const int tx = (int)(bid % (unsigned)a.tiles_x);
  bid /= (unsigned)a.tiles_x;
  const int ty = (int)(bid % (unsigned)a.tiles_y);
  const int b = (int)(bid / (unsigned)a.tiles_y);
  const int ox0 = tx * CD_TW, oy0 = ty * CD_TH;

  // ---- per-thread staging plan: source offsets (or -1) and LDS slots ------
  const int oy_first = oy0 > 0 ? oy0 - 1 : 0;
  const int sy_base = a.up2 ? oy_first >> 1 : oy_first;
  const uint16_t* const xb =
      a.x + ((long long)b * a.Hs + sy_base) * a.Ws * a.x_pitch;
  int poff[CD_PSLOTS];
#pragma unroll
  for (int k = 0; k < CD_PSLOTS; ++k) {
    const int id = tid + k * CD_THREADS;
    const int pix = id >> 2;
    const int py = pix / CD_PW, px = pix - py * CD_PW;
    const int oy = oy0 - 1 + py, ox = ox0 - 1 + px;
    const bool ok = id < CD_PATCH_PIECES && oy >= 0 && oy < a.Ho && ox >= 0 &&
                    ox < a.Wo;
    const int sy = ok ? (a.up2 ? oy >> 1 : oy) : sy_base;
    const int sx = ok ? (a.up2 ? ox >> 1 : ox) : 0;
    poff[k] = ok ? ((sy - sy_base) * a.Ws + sx) * (int)a.x_pitch + (id & 3) * 8
                 : -1;
  }
  int woff[WSLOTS];
#pragma unroll
  for (int k = 0; k < WSLOTS; ++k) {
    const int id = tid + k * CD_THREADS;
    const int row = id >> 2;
    const int tap = row / NK, kk = row - tap * NK;
    const bool ok = id < W_PIECES && kk < a.K;
    woff[k] = ok ? kk * 9 * a.C + tap * a.C + (id & 3) * 8 : -1;
  }

  // the 16-byte pieces of one chunk, global -> registers -> LDS (macros: as
  // lambdas capturing the arrays by reference they were kept in scratch)
  short8 pr[CD_PSLOTS], wr[WSLOTS];
#define CD_FETCH(c0)                                                          \
  do {                                                                        \
    _Pragma("unroll") for (int k = 0; k < CD_PSLOTS; ++k)                     \
      pr[k] = poff[k] >= 0                                                    \
                  ? *reinterpret_cast<const short8*>(xb + poff[k] + (c0))     \
                  : CD_ZERO8;                                                 \
    _Pragma("unroll") for (int k = 0; k < WSLOTS; ++k)                        \
      wr[k] = woff[k] >= 0                                                    \
                  ? *reinterpret_cast<const short8*>(wt + woff[k] + (c0))     \
                  : CD_ZERO8;                                                 \
  } while (0)
#define CD_COMMIT()                                                           \
  do {                                                                        \
    _Pragma("unroll") for (int k = 0; k < CD_PSLOTS; ++k) {                   \
      const int id = tid + k * CD_THREADS;                                    \
      if (id < CD_PATCH_PIECES)                                               \
        *reinterpret_cast<short8*>(patch + (id >> 2) * CD_PITCH +             \
                                   (id & 3) * 8) = pr[k];                     \
    }                                                                         \
    _Pragma("unroll") for (int k = 0; k < WSLOTS; ++k) {                      \
      const int id = tid + k * CD_THREADS;                                    \
      if (id < W_PIECES)                                                      \
        *reinterpret_cast<short8*>(wl + (id >> 2) * CD_PITCH +                \
                                   (id & 3) * 8) = wr[k];                     \
    }                                                                         \
  } while (0)

  f32x4 acc[2][NF];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragment read origins: pixel (wave, fr) of the patch, weight row fr
  const uint16_t* const a_rd = patch + (wave * CD_PW + fr) * CD_PITCH + kgrp * 8;
  const uint16_t* const b_rd = wl + fr * CD_PITCH + kgrp * 8;

  const int chunks = a.C >> 5;
  CD_FETCH(0);
  for (int ch = 0; ch < chunks; ++ch) {
    __syncthreads();          // every wave is done reading the previous chunk
    CD_COMMIT();
    __syncthreads();
    if (ch + 1 < chunks) CD_FETCH((ch + 1) << 5);   // in flight under the MFMAs
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int r = tap / 3, s = tap % 3;
      short8 px[2], wf[NF];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        px[i] = *reinterpret_cast<const short8*>(
            a_rd + (r * CD_PW + s + i * 16) * CD_PITCH);
#pragma unroll
      for (int j = 0; j < NF; ++j)
        wf[j] = *reinterpret_cast<const short8*>(
            b_rd + (tap * NK + j * 16) * CD_PITCH);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              wf[j], px[i], acc[i][j], 0, 0, 0);
    }
  }

  // ---- epilogue: lane = pixel fr of a fragment, channels kgrp*4 .. +3 ------
  const int oy = oy0 + wave;
  if (oy >= a.Ho) return;
  const long long row0 = ((long long)b * a.Ho + oy0) * a.Wo;
  uint16_t* const ob = a.out + row0 * a.out_pitch;
  const uint16_t* const r1b = a.res1 ? a.res1 + row0 * a.r1_pitch : nullptr;
  const uint16_t* const r2b = a.res2 ? a.res2 + row0 * a.r2_pitch : nullptr;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int ox = ox0 + i * 16 + fr;
    if (ox >= a.Wo) continue;
    const int pix = wave * a.Wo + ox;
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      const int n0 = j * 16 + kgrp * 4;
      if (n0 >= a.K) continue;
      const bool full = n0 + 4 <= a.K;
      float v[4];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        float t = acc[i][j][rr];
        if (a.bias && n0 + rr < a.K) t += a.bias[n0 + rr];
        if (a.lrelu) t = t > 0.f ? t : a.slope * t;
        v[rr] = a.alpha * t;
      }
      if (r1b) {
        const uint16_t* p = r1b + pix * (int)a.r1_pitch + n0;
        if (full) {
          const short4v q = *reinterpret_cast<const short4v*>(p);
#pragma unroll
          for (int rr = 0; rr < 4; ++rr)
            v[rr] = fmaf(a.beta1, bf16_bits_to_f32((uint16_t)q[rr]), v[rr]);
        } else {
#pragma unroll
          for (int rr = 0; rr < 4; ++rr)
            if (n0 + rr < a.K)
              v[rr] = fmaf(a.beta1, bf16_bits_to_f32(p[rr]), v[rr]);
        }
      }
      if (r2b) {
        const uint16_t* p = r2b + pix * (int)a.r2_pitch + n0;
        if (full) {
          const short4v q = *reinterpret_cast<const short4v*>(p);
#pragma unroll
          for (int rr = 0; rr < 4; ++rr)
            v[rr] += bf16_bits_to_f32((uint16_t)q[rr]);
        } else {
#pragma unroll
          for (int rr = 0; rr < 4; ++rr)
            if (n0 + rr < a.K) v[rr] += bf16_bits_to_f32(p[rr]);
        }
      }
      uint16_t* dst = ob + pix * (int)a.out_pitch + n0;
      if (full) {
        short4v q;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) q[rr] = (short)f32_to_bf16_bits(v[rr]);
        *reinterpret_cast<short4v*>(dst) = q;
      } else {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
          if (n0 + rr < a.K) dst[rr] = f32_to_bf16_bits(v[rr]);
      }
    }
  }
}

// A [B, H, W, C] bf16 view as the kernel addresses it: channels contiguous,
// pixels `pitch` elements apart, rows and images packed at that pitch, pitch
// and start multiples of 8 elements. Returns the pitch.
static long long dense_view(const torch::Tensor& t, const char* name,
                            int64_t B, int64_t H, int64_t W, int64_t C) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16, name,
              ": bf16 tensor on the GPU expected");
  TORCH_CHECK(t.dim() == 4 && t.size(0) == B && t.size(1) == H &&
                  t.size(2) == W && t.size(3) == C,
              name, ": expected [", B, ", ", H, ", ", W, ", ", C, "], got ",
              t.sizes());
  // a single pixel has no pitch: any aligned value does
  const int64_t pitch = W > 1 ? t.stride(2) : (H > 1 ? t.stride(1) : (
      B > 1 ? t.stride(0) : (C + 7) / 8 * 8));
  TORCH_CHECK(C == 1 || t.stride(3) == 1, name, ": channels not contiguous");
  TORCH_CHECK(pitch >= C && pitch % 8 == 0, name, ": pixel pitch ", pitch,
              " is not a multiple of 8 covering C");
  TORCH_CHECK((H == 1 || t.stride(1) == W * pitch) &&
                  (B == 1 || t.stride(0) == H * W * pitch),
              name, ": rows / images not packed at the pixel pitch");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
              ": start is not 16-byte aligned");
  TORCH_CHECK(10 * W * pitch < (1ll << 31), name,
              ": 10 rows exceed the 32-bit in-tile offsets");
  return pitch;
}

void conv_dense(torch::Tensor x, torch::Tensor wt, torch::Tensor bias,
                torch::Tensor out, c10::optional<torch::Tensor> res1,
                c10::optional<torch::Tensor> res2, bool lrelu, double slope,
                double alpha, double beta1, bool up2) {
  TORCH_CHECK(x.dim() == 4 && out.dim() == 4, "x, out: [B, H, W, C] views");
  const int64_t B = x.size(0), Hs = x.size(1), Ws = x.size(2), C = x.size(3);
  const int64_t K = out.size(3);
  const int64_t Ho = up2 ? 2 * Hs : Hs, Wo = up2 ? 2 * Ws : Ws;
  TORCH_CHECK(C % 32 == 0 && C >= 32 && C <= 512, "C_in % 32, 32..512");
  TORCH_CHECK(K >= 1 && K <= 64, "K_out in 1..64");
  TORCH_CHECK(B >= 1 && Hs >= 1 && Ws >= 1, "empty input");
  TORCH_CHECK(wt.is_cuda() && wt.scalar_type() == at::kBFloat16 &&
                  wt.is_contiguous() && wt.dim() == 2 && wt.size(0) == K &&
                  wt.size(1) == 9 * C,
              "weight: contiguous bf16 [K, 9 * C_in]");
  DenseArgs a{};
  a.x_pitch = dense_view(x, "x", B, Hs, Ws, C);
  a.out_pitch = dense_view(out, "out", B, Ho, Wo, K);
  a.x = (const uint16_t*)x.data_ptr();
  a.out = (uint16_t*)out.data_ptr();
  if (res1.has_value() && res1->defined()) {
    a.r1_pitch = dense_view(*res1, "res1", B, Ho, Wo, K);
    a.res1 = (const uint16_t*)res1->data_ptr();
  }
  if (res2.has_value() && res2->defined()) {
    a.r2_pitch = dense_view(*res2, "res2", B, Ho, Wo, K);
    a.res2 = (const uint16_t*)res2->data_ptr();
  }
  torch::Tensor bf;
  if (bias.defined() && bias.numel()) {
    TORCH_CHECK(bias.is_cuda() && bias.numel() == K, "bias: [K] on the GPU");
    a.bias = bias_f32_ptr(bias, bf);
  }
  a.wt = (const uint16_t*)wt.data_ptr();
  a.Hs = (int)Hs; a.Ws = (int)Ws; a.Ho = (int)Ho; a.Wo = (int)Wo;
  a.C = (int)C; a.K = (int)K;
  a.tiles_x = (int)((Wo + CD_TW - 1) / CD_TW);
  a.tiles_y = (int)((Ho + CD_TH - 1) / CD_TH);
  a.up2 = up2; a.lrelu = lrelu;
  a.slope = (float)slope; a.alpha = (float)alpha; a.beta1 = (float)beta1;
  const long long blocks = (long long)a.tiles_x * a.tiles_y * B;
  TORCH_CHECK(blocks < (1ll << 31), "too many tiles for one grid");
  auto stream = at::hip::getCurrentHIPStream();
  const dim3 grid((unsigned)blocks), block(CD_THREADS);
  if (K <= 16)
    hipLaunchKernelGGL(conv_dense_kernel<1>, grid, block, 0, stream, a);
  else if (K <= 32)
    hipLaunchKernelGGL(conv_dense_kernel<2>, grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL(conv_dense_kernel<4>, grid, block, 0, stream, a);
  HIP_CHECK_LAUNCH();
}
