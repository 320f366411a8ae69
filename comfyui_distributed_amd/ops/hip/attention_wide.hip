// Flash-attention forward for wide heads, 160 < D <= 512 (MI355X/gfx950):
// the single-head mid-block attention of the autoencoder-KL VAE (D = 512)
// and DiT head dims up to 256. attention.hip serves D <= 160.
//
// Why another kernel: attn_fwd_kernel gives one wave "16 q rows x all of D"
// for both products. At D = 512 that is 128 VGPRs of O accumulators, 64 of
// resident Q, 64 of K/V staging and 32 of scores/P per lane, ~300 against
// the 256 of two waves per SIMD, and 150 KB of K + V^T images per 64 keys.
//
// Split: the 8-wave workgroup owns 64 q rows as 4 row groups x 2 D-halves.
// Wave (rg, dh) holds the Q fragments and the O accumulators of columns
// [dh*D_PAD/2, (dh+1)*D_PAD/2) of q rows rg*16 .. rg*16+15 only. Per 32-key
// tile it computes the scores of its row group over ITS half of D; the two
// waves of a pair swap those partial sums through a 16 x 32 fp32 LDS slab
// (one barrier) and add them. fp32 addition commutes, so both waves hold
// the same bits and run the same softmax (same running max, same P); each
// then multiplies P into its own half of V^T. Scores and P never leave the
// CU; O is normalised and rounded once on store.
//
// Kept from attention.hip: K rows and V^T columns staged through LDS once
// per workgroup from registers loaded one tile ahead; every global load
// unconditional (rows past Nq/Nk and the d >= D tail redirect to the zero
// page, the key tail is masked); swapped QK^T so a lane's scores sit on one
// q row and cvt_pk of them IS the PV A operand (V^T keys permuted to
// match); exp2-domain online softmax with defer-max; the XCD renumbering.
// No atomics, no workspace: capture-safe and bit-identical call to call.
//
// LDS map (one object, bytes), D_PAD = 512 | 256:
//   K    [32][D_PAD + 16] bf16      33792 | 17408   pitch 66 | 34 slots
//   V^T  [D_PAD][32 + 16] bf16      49152 | 24576   pitch 6 slots
//   X    [8 waves][8][64] fp32      16384 | 16384   score exchange
//   total                           99328 | 58368
// Both pitches are 2 mod 4 in 16-byte slots: the ds_read_b128 fragment
// reads are conflict-free (the rule derived in attention.hip).
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), see
// profiles/r19_attention_wide.md: both instantiations 0 scratch.
//
// Rejected: both waves of a pair computing the full-D scores. No exchange
// and one barrier fewer per tile, but QK^T runs twice (1.5x the MFMAs and
// 1.5x the LDS fragment reads, which is what bounds the tile) and Q costs
// 64 resident VGPRs instead of 32. Also rejected: one wave per SIMD with a
// 512-VGPR budget, where nothing covers a wave's softmax.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define W_NWAVES 8
#define W_NTHREADS (W_NWAVES * 64)
#define W_QROWS 64  // q rows per workgroup: 4 row groups x 16
#define W_KT 32     // keys per tile
#define W_KFRAG (W_KT / 16)
#define W_VT_PITCH (W_KT + 16)
#define W_DEFER_THR 8.0f
#define W_LOG2E 1.4426950408889634f

// Everything below is compiled without the packed fp32 instructions
// (v_pk_add_f32, v_pk_mul_f32, v_pk_fma_f32), which the rescale and row-sum
// code would otherwise pair into. A function with the attribute cannot
// inline one without it, so the few helpers the kernel needs (shuffle,
// ballot, barrier, bf16 rounding) are defined here, inside the region,
// instead of taken from the HIP headers and common.h.
#if defined(__HIP_DEVICE_COMPILE__)  // the host pass does not know the feature
#pragma clang attribute push(                                              \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// two f32 -> packed bf16 pair (RNE), lo in bits 15:0
__device__ __forceinline__ uint32_t cvt_pk_bf16(float lo, float hi) {
  uint32_t r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

// value of `v` in lane `src` (ds_bpermute: no LDS storage involved)
__device__ __forceinline__ float w_shfl(float v, int src) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute(src << 2, __builtin_bit_cast(int, v)));
}

// workgroup barrier that orders LDS accesses, as __syncthreads()
__device__ __forceinline__ void w_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// one workgroup per CU (LDS), two waves per SIMD: up to 256 VGPRs
template <int D_PAD>  // 256 or 512
__global__ __launch_bounds__(W_NTHREADS)
__attribute__((amdgpu_waves_per_eu(2, 2))) void attn_wide_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, uint16_t* __restrict__ o,
    const uint16_t* __restrict__ zp,  // >= 16 B of zeros
    int Nq, int Nk, int D, int H, int Hkv, float scale, long long q_bstride,
    long long q_hstride, long long q_rstride, long long k_bstride,
    long long k_hstride, long long k_rstride, long long o_bstride,
    long long o_hstride, long long o_rstride) {
  constexpr int DH = D_PAD / 2;    // columns of one D-half
  constexpr int DKH = DH / 32;     // QK^T k-steps per wave
  constexpr int DNH = DH / 16;     // O fragments per wave
  constexpr int K_PITCH = D_PAD + 16;
  constexpr int KCH = D_PAD / 8;   // 16-byte pieces per K / V row
  constexpr int KROWS = W_NTHREADS / KCH;  // K rows one slot covers
  constexpr int KSLOTS = W_KT / KROWS;
  constexpr int VDP = W_NTHREADS / W_KT;   // V d-pieces one slot covers
  constexpr int VSLOTS = KCH / VDP;
  constexpr int K_ELEMS = W_KT * K_PITCH;
  constexpr int V_ELEMS = D_PAD * W_VT_PITCH;
  static_assert(D_PAD == 256 || D_PAD == 512, "two D-halves of 128 or 256");
  static_assert(KSLOTS * KROWS == W_KT && VSLOTS * VDP == KCH,
                "every staging slot is full: no guards on the commits");
  static_assert((K_PITCH / 8) % 4 == 2 && (W_VT_PITCH / 8) % 4 == 2,
                "ds_read_b128 bank rule");

  __shared__ __align__(16) uint16_t
      lds[K_ELEMS + V_ELEMS + W_NTHREADS * 8 * 2];
  uint16_t* const k_lds = lds;            // [W_KT][K_PITCH]
  uint16_t* const v_t = lds + K_ELEMS;    // [D_PAD][W_VT_PITCH]
  float* const xch = reinterpret_cast<float*>(lds + K_ELEMS + V_ELEMS);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int dh = wave & 1;   // D-half
  const int rgw = wave >> 1; // row group
  // XCD j walks heads j, j+8, ... with all q-blocks of a head back to back
  // (attention.hip); placement only changes speed, never the result
  int bh = blockIdx.x, qblk = blockIdx.y;
  if ((gridDim.x & 7) == 0) {
    const unsigned lin = blockIdx.y * gridDim.x + blockIdx.x;
    const unsigned idx = lin >> 3;
    bh = (int)(idx / gridDim.y) * 8 + (int)(lin & 7);
    qblk = (int)(idx % gridDim.y);
  }
  const int b = bh / H;
  const int h = bh % H;
  const int hk = h / (H / Hkv);
  const int q_row0 = qblk * W_QROWS + rgw * 16;
  const int dbase = dh * DH;

  const uint16_t* qbase = q + b * q_bstride + h * q_hstride;
  const uint16_t* kbase = k + b * k_bstride + hk * k_hstride;
  const uint16_t* vbase = v + b * k_bstride + hk * k_hstride;
  uint16_t* obase = o + b * o_bstride + h * o_hstride;

  const int kd0 = (lane >> 4) * 8;

  // ---- Q fragments of this D-half, resident -----------------------------
  short8 qfrag[DKH];
  {
    const int row = q_row0 + (lane & 15);
    const bool row_ok = row < Nq;
#pragma unroll
    for (int kk = 0; kk < DKH; ++kk) {
      const int d = dbase + kk * 32 + kd0;
      const uint16_t* src = (row_ok && d + 8 <= D)
          ? qbase + (long long)row * q_rstride + d : zp;
      qfrag[kk] = *reinterpret_cast<const short8*>(src);
    }
  }

  // softmax state of q row (lane & 15) in the exp2 domain; the two waves of
  // a pair carry identical copies. l_run is the lane's partial row sum.
  const float c = scale * W_LOG2E;
  float m_run = -1e30f, l_run = 0.f;
  f32x4 oacc[DNH];
#pragma unroll
  for (int n = 0; n < DNH; ++n) oacc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int ntiles = (Nk + W_KT - 1) / W_KT;

  // ---- K/V register staging ---------------------------------------------
  // K slot s: key tid/KCH + s*KROWS, columns (tid%KCH)*8.. (coalesced rows).
  // V slot s: key tid%32, d-piece tid/32 + s*VDP; key 16h+4g+r lands in
  // V^T column 8g+4h+r, the k-slot where the PV A operand holds its P.
  // d >= D pieces point at the zero page with a zero step.
  const int kkey0 = tid / KCH;
  const int kcol = (tid % KCH) * 8;
  const int vkey = tid & (W_KT - 1);
  const int vdp0 = tid / W_KT;
  const int vcol = ((vkey & 12) << 1) | ((vkey & 16) >> 2) | (vkey & 3);
  const uint16_t* kptr[KSLOTS];
  long long kstep[KSLOTS];
#pragma unroll
  for (int s = 0; s < KSLOTS; ++s) {
    const bool ok = kcol + 8 <= D;
    kptr[s] = ok ? kbase + (long long)(kkey0 + s * KROWS) * k_rstride + kcol
                 : zp;
    kstep[s] = ok ? (long long)W_KT * k_rstride : 0ll;
  }
  const uint16_t* vptr[VSLOTS];
  long long vstep[VSLOTS];
#pragma unroll
  for (int s = 0; s < VSLOTS; ++s) {
    const int d0 = (vdp0 + s * VDP) * 8;
    const bool ok = d0 + 8 <= D;
    vptr[s] = ok ? vbase + (long long)vkey * k_rstride + d0 : zp;
    vstep[s] = ok ? (long long)W_KT * k_rstride : 0ll;
  }

  short8 kreg[KSLOTS], vreg[VSLOTS];
  auto prefetch = [&](int key0) {
    const uint16_t* ks[KSLOTS];
    const uint16_t* vs[VSLOTS];
#pragma unroll
    for (int s = 0; s < KSLOTS; ++s) ks[s] = kptr[s];
#pragma unroll
    for (int s = 0; s < VSLOTS; ++s) vs[s] = vptr[s];
    if (key0 + W_KT > Nk) {  // workgroup-uniform: the partial tile only
#pragma unroll
      for (int s = 0; s < KSLOTS; ++s)
        if (key0 + kkey0 + s * KROWS >= Nk) ks[s] = zp;
#pragma unroll
      for (int s = 0; s < VSLOTS; ++s)
        if (key0 + vkey >= Nk) vs[s] = zp;
    }
#pragma unroll
    for (int s = 0; s < KSLOTS; ++s) {
      kreg[s] = *reinterpret_cast<const short8*>(ks[s]);
      kptr[s] += kstep[s];
    }
#pragma unroll
    for (int s = 0; s < VSLOTS; ++s) {
      vreg[s] = *reinterpret_cast<const short8*>(vs[s]);
      vptr[s] += vstep[s];
    }
  };
  prefetch(0);

  for (int t = 0; t < ntiles; ++t) {
    const int key0 = t * W_KT;

    // ---- commit the prefetched tile (everyone is done with the last one)
    w_sync();
#pragma unroll
    for (int s = 0; s < KSLOTS; ++s)
      *reinterpret_cast<short8*>(
          &k_lds[(kkey0 + s * KROWS) * K_PITCH + kcol]) = kreg[s];
#pragma unroll
    for (int s = 0; s < VSLOTS; ++s) {
      const int d0 = (vdp0 + s * VDP) * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v_t[(d0 + j) * W_VT_PITCH + vcol] = (uint16_t)vreg[s][j];
    }
    if (t + 1 < ntiles) prefetch(key0 + W_KT);
    w_sync();

    // ---- partial scores over this wave's D-half, SWAPPED (S^T = K Q^T):
    // s[f][r] = score(key0 + f*16 + (lane>>4)*4 + r, q row lane&15)
    f32x4 s[W_KFRAG];
#pragma unroll
    for (int f = 0; f < W_KFRAG; ++f) s[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < DKH; ++kk) {
      short8 kf[W_KFRAG];
#pragma unroll
      for (int f = 0; f < W_KFRAG; ++f)
        kf[f] = *reinterpret_cast<const short8*>(
            &k_lds[(f * 16 + (lane & 15)) * K_PITCH + dbase + kk * 32 + kd0]);
#pragma unroll
      for (int f = 0; f < W_KFRAG; ++f)
        s[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[f], qfrag[kk], s[f],
                                                       0, 0, 0);
    }

    // ---- the pair swaps its halves: slab [wave][f*4+r][lane], lane-major
    // so both the writes and the reads are conflict-free. The slab is
    // rewritten two barriers after it was last read.
#pragma unroll
    for (int f = 0; f < W_KFRAG; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        xch[(wave * 8 + f * 4 + r) * 64 + lane] = s[f][r];
    w_sync();
#pragma unroll
    for (int f = 0; f < W_KFRAG; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        s[f][r] += xch[((wave ^ 1) * 8 + f * 4 + r) * 64 + lane];

    if (key0 + W_KT > Nk) {  // workgroup-uniform: the key tail
#pragma unroll
      for (int f = 0; f < W_KFRAG; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = key0 + f * 16 + (lane >> 4) * 4 + r;
          if (key >= Nk) s[f][r] = -1e30f;
        }
    }

    // ---- online softmax on raw scores; c > 0 so max commutes with it ----
    float mt = s[0][0];
#pragma unroll
    for (int f = 0; f < W_KFRAG; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r) mt = fmaxf(mt, s[f][r]);
    mt = fmaxf(mt, w_shfl(mt, lane ^ 16));
    mt = fmaxf(mt, w_shfl(mt, lane ^ 32));
    mt *= c;

    // decide, rescale O and l, THEN exponentiate against the max the
    // decision left behind; the deferred P stays below e^8
    const bool need = (mt - m_run) > W_DEFER_THR * W_LOG2E;
    if (__builtin_amdgcn_ballot_w64(need) != 0ull) {
      const float m_new = fmaxf(m_run, mt);
      const float a = __builtin_amdgcn_exp2f(m_run - m_new);
      m_run = m_new;
      l_run *= a;
      // O fragment rows are (lane>>4)*4+r: fetch each row's alpha from a
      // lane holding that row's state (same 16-lane group, col == row)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int src = (lane & 48) | (((lane >> 4) * 4 + r) & 15);
        const float ar = w_shfl(a, src);
#pragma unroll
        for (int n = 0; n < DNH; ++n) oacc[n][r] *= ar;
      }
    }
    float p[W_KFRAG][4];
#pragma unroll
    for (int f = 0; f < W_KFRAG; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p[f][r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[f][r], c, -m_run));
        l_run += p[f][r];
      }

    // ---- PV over this wave's D-half, P straight from registers: lane
    // (g = lane>>4) holds keys 16h + 4g + r in p[h][r]; as A-operand
    // element 4h + r that is k-slot 8g + 4h + r, the V^T column of that key
    union { uint32_t u[4]; short8 v8; } pf;
    pf.u[0] = cvt_pk_bf16(p[0][0], p[0][1]);
    pf.u[1] = cvt_pk_bf16(p[0][2], p[0][3]);
    pf.u[2] = cvt_pk_bf16(p[1][0], p[1][1]);
    pf.u[3] = cvt_pk_bf16(p[1][2], p[1][3]);
#pragma unroll
    for (int n0 = 0; n0 < DNH; n0 += 4) {
      short8 vfrag[4];
#pragma unroll
      for (int n = 0; n < 4; ++n)
        vfrag[n] = *reinterpret_cast<const short8*>(
            &v_t[(dbase + (n0 + n) * 16 + (lane & 15)) * W_VT_PITCH + kd0]);
#pragma unroll
      for (int n = 0; n < 4; ++n)
        oacc[n0 + n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            pf.v8, vfrag[n], oacc[n0 + n], 0, 0, 0);
    }
  }

  // ---- epilogue: this wave's D-half of its 16 rows ----------------------
  {
    const int col = lane & 15;
    const int rg = lane >> 4;
    l_run += w_shfl(l_run, lane ^ 16);
    l_run += w_shfl(l_run, lane ^ 32);
    const float rl_own = __builtin_amdgcn_rcpf(l_run);
    float rl[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int src = (lane & 48) | ((rg * 4 + r) & 15);
      rl[r] = w_shfl(rl_own, src);
    }
#pragma unroll
    for (int n = 0; n < DNH; ++n) {
      const int d = dbase + n * 16 + col;
      if (d >= D) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = q_row0 + rg * 4 + r;
        if (row >= Nq) continue;
        obase[(long long)row * o_rstride + d] =
            (uint16_t)cvt_pk_bf16(oacc[n][r] * rl[r], 0.f);
      }
    }
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// Called by launch_attn_raw (attention.hip) for 160 < D <= 512 with the
// same strided description of q/k/v and the packed output it uses itself.
void launch_attn_wide(const uint16_t* qp, const uint16_t* kp,
                      const uint16_t* vp, uint16_t* op, const uint16_t* zp,
                      int H, int Hkv, int Nq, int Nk, int D, float scale,
                      long long qb, long long qh, long long qr, long long kb,
                      long long kh, long long kr, long long ob, long long oh,
                      long long orr, int batch) {
  TORCH_CHECK(D > 160 && D <= 512 && D % 8 == 0,
              "wide attention serves head dims %8 in (160, 512], got ", D);
  TORCH_CHECK(Nq >= 1 && Nk >= 1 && Hkv >= 1 && H % Hkv == 0);
  dim3 grid(batch * H, (Nq + W_QROWS - 1) / W_QROWS);
  dim3 block(W_NTHREADS);
  auto stream = at::hip::getCurrentHIPStream();
#define LAUNCH_W(DP)                                                          \
  hipLaunchKernelGGL((attn_wide_kernel<DP>), grid, block, 0, stream, qp, kp,  \
                     vp, op, zp, Nq, Nk, D, H, Hkv, scale, qb, qh, qr, kb,    \
                     kh, kr, ob, oh, orr)
  if (D <= 256) LAUNCH_W(256); else LAUNCH_W(512);
#undef LAUNCH_W
  HIP_CHECK_LAUNCH();
}
