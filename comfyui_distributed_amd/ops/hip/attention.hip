// Flash-attention forward for diffusion UNet/DiT blocks (MI355X/gfx950).
//
// Hand-written CDNA4 kernel, v5: generalized strided addressing so the
// kernel consumes the QKV projections' natural packed layout
// [B, N, H*D] directly — no pad, no permute, no copies on the host side.
// The head dim D only needs to be a multiple of 8: staged rows are
// zero-filled at 8-element granularity up to the padded compute width.
//
// Structure per 64-key tile (see profiles/ for measurements):
//   * 8-wave workgroup owns 128 q rows; the K tile (row-major) and the V^T
//     tile are staged through LDS ONCE per workgroup: every thread loads its
//     16-byte pieces one tile ahead into registers and commits them between
//     the two tile-start barriers; workgroups are renumbered so that an XCD
//     works through one head's q-blocks before the next head's (K/V stays
//     in that XCD's L2);
//   * swapped QK^T keeps each lane's 16 scores on one q row; P goes from
//     the score registers straight into the PV A operand (V^T is stored
//     with its keys permuted to match), never through LDS;
//   * online softmax in the exp2 domain (scale*log2e folded into one fma),
//     defer-max (T13), lane-local row sums reduced once in the epilogue.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define QROWS_PER_WAVE 16
#define NWAVES 8
#define NTHREADS (NWAVES * 64)
#define QROWS_PER_BLOCK (QROWS_PER_WAVE * NWAVES)  // 128
#define KT 64
#define KFRAG (KT / 16)
// V^T row pitch: 10 16-byte slots (== 2 mod 4), the same bank rule as the
// K rows below — the B-fragment ds_read_b128 is conflict-free
#define VT_PITCH (KT + 16)
#define DEFER_THR 8.0f
#define LOG2E 1.4426950408889634f

// two f32 -> packed bf16 pair (RNE), lo in bits 15:0
__device__ __forceinline__ uint32_t cvt_pk_bf16(float lo, float hi) {
  uint32_t r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

// waves_per_eu(2, 4): two workgroups per CU is the target, so the scheduler
// may spend up to 128 VGPRs on keeping a k-step's fragment reads in flight
// ahead of its MFMAs instead of squeezing toward a fifth wave
template <int D_PAD>  // multiple of 16; QK^T K-depth rounds up to 32s
__global__ __launch_bounds__(NTHREADS)
__attribute__((amdgpu_waves_per_eu(2, 4))) void attn_fwd_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, uint16_t* __restrict__ o,
    const uint16_t* __restrict__ zp,  // >=16B zeros: OOB loads redirect
                                      // here so every load is UNconditional
                                      // (a per-lane branchy load makes
                                      // hipcc emit vmcnt(0) per cluster —
                                      // guide §5 trap (c) — serializing
                                      // the whole prefetch pipeline)
    int Nq, int Nk,
    int D, int H, int Hkv, float scale, long long q_bstride,
    long long q_hstride, long long q_rstride, long long k_bstride,
    long long k_hstride, long long k_rstride, long long o_bstride,
    long long o_hstride, long long o_rstride) {
  constexpr int DK = (D_PAD + 31) / 32;
  constexpr int DN = D_PAD / 16;
  // K rows hold DK*32 columns (d >= D zero-filled) + 16 pad: the row pitch
  // is (4*DK+2) 16-byte slots, == 2 mod 4, so the 16 rows x {g, g+1}
  // column slots of every ds_read_b128 lane group cover all 16 slots of
  // the 256-byte bank row exactly once (conflict-free A-fragment reads)
  constexpr int K_PITCH = DK * 32 + 16;
  constexpr int KCH = DK * 4;  // 16-byte pieces per K row
  constexpr int KSLOTS = (KT * KCH + NTHREADS - 1) / NTHREADS;
  constexpr int VCH = D_PAD / 8;  // 16-byte pieces per V row
  constexpr int VSLOTS = (KT * VCH + NTHREADS - 1) / NTHREADS;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  // Workgroups are handed to the 8 XCDs round-robin in linear-id order, x
  // fastest, so the plain (bh, q-block) = (x, y) grid has every head of the
  // launch in flight at once and each head's K/V leaves L2 between its
  // q-blocks. Renumber so that XCD j walks heads j, j+8, ... one after the
  // other, all q-blocks of a head back to back: the few heads an XCD has in
  // flight fit its L2. Placement only changes speed, never the result.
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
  const int q_row0 = qblk * QROWS_PER_BLOCK + wave * QROWS_PER_WAVE;

  const uint16_t* qbase = q + b * q_bstride + h * q_hstride;
  const uint16_t* kbase = k + b * k_bstride + hk * k_hstride;
  const uint16_t* vbase = v + b * k_bstride + hk * k_hstride;
  uint16_t* obase = o + b * o_bstride + h * o_hstride;

  __shared__ __align__(16) uint16_t k_lds[KT][K_PITCH];
  __shared__ __align__(16) uint16_t v_t[D_PAD][VT_PITCH];

  const int kd0 = (lane >> 4) * 8;

  // T5 static priority (microarch guide, two-waves-per-SIMD item 4): the
  // second-dispatched wave half loses issue arbitration on every segment;
  // ONE setprio for that half — and no per-segment flips — removes its
  // start-of-segment penalty
  if (wave >= NWAVES / 2) __builtin_amdgcn_s_setprio(1);

  // ---- Q fragments resident (OOB rows/d -> zero page) -------------------
  short8 qfrag[DK];
  {
    const int row = q_row0 + (lane & 15);
    const bool row_ok = row < Nq;
#pragma unroll
    for (int kk = 0; kk < DK; ++kk) {
      const int d = kk * 32 + kd0;
      const uint16_t* src = (row_ok && d + 8 <= D)
          ? qbase + (long long)row * q_rstride + d : zp;
      qfrag[kk] = *reinterpret_cast<const short8*>(src);
    }
  }

  // per-lane softmax state for q row (lane & 15), kept in the exp2 domain:
  // m_run = c * (running max of the raw scores), c = scale*log2e > 0.
  // l_run is this lane's PARTIAL row sum (its own 16 keys per tile); the
  // four lanes of a row share m_run, so one alpha rescales all of them
  const float c = scale * LOG2E;
  float m_run = -1e30f, l_run = 0.f;
  f32x4 oacc[DN];
#pragma unroll
  for (int n = 0; n < DN; ++n) oacc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int ntiles = (Nk + KT - 1) / KT;

  // ---- K/V register staging: piece c of a tile belongs to thread c%512.
  // Source pointers are built once (the d >= D pieces point at the zero
  // page with a zero step) and advance one tile per prefetch; the key-tail
  // redirect is needed only while prefetching the partial last tile.
  // K piece c: key c/KCH, columns (c%KCH)*8.. -> coalesced row reads.
  // V piece c: key c%64 (== lane), d (c/64)*8.. -> conflict-light V^T
  // scatter; key 16h+4g+r of each 32-key chunk lands in column 8g+4h+r,
  // the k-slot where the PV A operand holds that key's P (see below).
  const uint16_t* kptr[KSLOTS];
  long long kstep[KSLOTS];
  int kkey[KSLOTS];
#pragma unroll
  for (int s = 0; s < KSLOTS; ++s) {
    const int pc = (int)threadIdx.x + s * NTHREADS;
    kkey[s] = pc / KCH;
    const int d0 = (pc % KCH) * 8;
    const bool ok = pc < KT * KCH && d0 + 8 <= D;
    kptr[s] = ok ? kbase + (long long)kkey[s] * k_rstride + d0 : zp;
    kstep[s] = ok ? (long long)KT * k_rstride : 0ll;
  }
  const uint16_t* vptr[VSLOTS];
  long long vstep[VSLOTS];
#pragma unroll
  for (int s = 0; s < VSLOTS; ++s) {
    const int pc = (int)threadIdx.x + s * NTHREADS;
    const int d0 = (pc / KT) * 8;
    const bool ok = pc < KT * VCH && d0 + 8 <= D;
    vptr[s] = ok ? vbase + (long long)lane * k_rstride + d0 : zp;
    vstep[s] = ok ? (long long)KT * k_rstride : 0ll;
  }
  const int vcol = (lane & 32) | ((lane & 12) << 1) | ((lane & 16) >> 2)
                 | (lane & 3);

  short8 kreg[KSLOTS], vreg[VSLOTS];
  auto prefetch = [&](int key0) {
    const uint16_t* ks[KSLOTS];
    const uint16_t* vs[VSLOTS];
#pragma unroll
    for (int s = 0; s < KSLOTS; ++s) ks[s] = kptr[s];
#pragma unroll
    for (int s = 0; s < VSLOTS; ++s) vs[s] = vptr[s];
    if (key0 + KT > Nk) {  // wave-uniform: the partial tile only
#pragma unroll
      for (int s = 0; s < KSLOTS; ++s)
        if (key0 + kkey[s] >= Nk) ks[s] = zp;
#pragma unroll
      for (int s = 0; s < VSLOTS; ++s)
        if (key0 + lane >= Nk) vs[s] = zp;
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
    const int key0 = t * KT;

    // ---- commit the prefetched K rows and V^T columns (barrier-bracketed;
    // the loads were issued one full tile ago) -----------------------------
    __syncthreads();
#pragma unroll
    for (int s = 0; s < KSLOTS; ++s) {
      const int pc = (int)threadIdx.x + s * NTHREADS;
      if (pc < KT * KCH)
        *reinterpret_cast<short8*>(&k_lds[pc / KCH][(pc % KCH) * 8]) = kreg[s];
    }
#pragma unroll
    for (int s = 0; s < VSLOTS; ++s) {
      const int pc = (int)threadIdx.x + s * NTHREADS;
      if (pc < KT * VCH) {
        const int d0 = (pc / KT) * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) v_t[d0 + j][vcol] = (uint16_t)vreg[s][j];
      }
    }
    // staging registers are free again: tile t+1's loads fly under all of
    // tile t's compute (plain loads survive the barrier)
    if (t + 1 < ntiles) prefetch(key0 + KT);
    __syncthreads();

    // ---- scores, SWAPPED: S^T = mfma(K, Q) so each lane's 16 score
    // values all belong to ONE q row (col = lane&15) — softmax becomes
    // in-register with only 2 cross-lane steps (guide's swapped-QK^T
    // idiom).  s[f][r] = score(key = key0 + f*16 + (lane>>4)*4 + r,
    //                          qrow = lane&15)
    f32x4 s[KFRAG];
#pragma unroll
    for (int f = 0; f < KFRAG; ++f) s[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < DK; ++kk) {
      // all four reads in flight before the first MFMA waits on one
      short8 kf[KFRAG];
#pragma unroll
      for (int f = 0; f < KFRAG; ++f)
        kf[f] = *reinterpret_cast<const short8*>(
            &k_lds[f * 16 + (lane & 15)][kk * 32 + kd0]);
#pragma unroll
      for (int f = 0; f < KFRAG; ++f)
        s[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[f], qfrag[kk], s[f],
                                                       0, 0, 0);
    }

    if (key0 + KT > Nk) {  // wave-uniform: only the last tile has a tail
#pragma unroll
      for (int f = 0; f < KFRAG; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = key0 + f * 16 + (lane >> 4) * 4 + r;
          if (key >= Nk) s[f][r] = -1e30f;
        }
    }

    // ---- online softmax on raw scores; c > 0 so max commutes with it ----
    float mt = s[0][0];
#pragma unroll
    for (int f = 0; f < KFRAG; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r) mt = fmaxf(mt, s[f][r]);
    mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    mt *= c;

    // textbook order (T13 hazard): decide, rescale O and l, THEN
    // exponentiate this tile against the max the decision left behind.
    // Threshold in the exp2 domain keeps the deferred P bound at e^8.
    const bool need = (mt - m_run) > DEFER_THR * LOG2E;
    if (__ballot(need) != 0ull) {
      const float m_new = fmaxf(m_run, mt);
      const float a = __builtin_amdgcn_exp2f(m_run - m_new);
      m_run = m_new;
      l_run *= a;
      // O fragment rows are (lane>>4)*4+r: fetch each row's alpha from a
      // lane holding that row's state (same 16-lane group, col == row)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int src = (lane & 48) | (((lane >> 4) * 4 + r) & 15);
        const float ar = __shfl(a, src, 64);
#pragma unroll
        for (int n = 0; n < DN; ++n) oacc[n][r] *= ar;
      }
    }
    float p[KFRAG][4];
#pragma unroll
    for (int f = 0; f < KFRAG; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p[f][r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[f][r], c, -m_run));
        l_run += p[f][r];
      }

    // ---- PV, P straight from registers: for 32-key chunk kc this lane
    // (g = lane>>4) holds keys 16h + 4g + r in p[2kc+h][r]; as A-operand
    // element 4h + r that is k-slot 8g + 4h + r — the column V^T was
    // committed to. The sum over keys does not care about the order.
#pragma unroll
    for (int kc = 0; kc < KT / 32; ++kc) {
      union { uint32_t u[4]; short8 v8; } pf;
      pf.u[0] = cvt_pk_bf16(p[2 * kc][0], p[2 * kc][1]);
      pf.u[1] = cvt_pk_bf16(p[2 * kc][2], p[2 * kc][3]);
      pf.u[2] = cvt_pk_bf16(p[2 * kc + 1][0], p[2 * kc + 1][1]);
      pf.u[3] = cvt_pk_bf16(p[2 * kc + 1][2], p[2 * kc + 1][3]);
      short8 vfrag[DN];
#pragma unroll
      for (int n = 0; n < DN; ++n)
        vfrag[n] = *reinterpret_cast<const short8*>(
            &v_t[n * 16 + (lane & 15)][kc * 32 + kd0]);
#pragma unroll
      for (int n = 0; n < DN; ++n)
        oacc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf.v8, vfrag[n],
                                                          oacc[n], 0, 0, 0);
    }
  }

  // ---- epilogue ---------------------------------------------------------
  {
    const int col = lane & 15;
    const int rg = lane >> 4;
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    const float rl_own = __builtin_amdgcn_rcpf(l_run);
    float rl[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int src = (lane & 48) | ((rg * 4 + r) & 15);
      rl[r] = __shfl(rl_own, src, 64);
    }
#pragma unroll
    for (int n = 0; n < DN; ++n) {
      const int d = n * 16 + col;
      if (d >= D) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = q_row0 + rg * 4 + r;
        if (row >= Nq) continue;
        obase[(long long)row * o_rstride + d] =
            f32_to_bf16_bits(oacc[n][r] * rl[r]);
      }
    }
  }
}

static torch::Tensor launch_attn_raw(const uint16_t* qp, const uint16_t* kp,
                                     const uint16_t* vp, torch::Tensor o,
                                     int H, int Hkv, int Nq, int Nk, int D,
                                     float scale, long long qb, long long qh,
                                     long long qr, long long kb, long long kh,
                                     long long kr, int batch) {
  const uint16_t* zp = (const uint16_t*)device_zero_page(o);
  // D=40 (SD1.5's hot dim) pads to 48, not 64: PV runs 3 d-fragments
  // instead of 4 and the V^T stage shrinks 25% on the dominant kernel
  const int dpad = D <= 48 ? 48
                 : (D <= 64 ? 64 : (D <= 96 ? 96 : (D <= 128 ? 128 : 160)));
  TORCH_CHECK(D % 8 == 0 && D <= 160, "head dim must be %8 and <=160, got ", D);
  // the kernel takes the tile max on raw scores and scales it afterwards
  TORCH_CHECK(scale > 0.f, "attention scale must be positive, got ", scale);
  // output is always a fresh packed [B, Nq, H*D] tensor
  const long long ob = (long long)Nq * H * D, oh = D, orr = (long long)H * D;
  dim3 grid(batch * H, (Nq + QROWS_PER_BLOCK - 1) / QROWS_PER_BLOCK);
  dim3 block(NTHREADS);
  auto stream = at::hip::getCurrentHIPStream();
#define LAUNCH_D(DP)                                                          \
  hipLaunchKernelGGL((attn_fwd_kernel<DP>), grid, block, 0, stream, qp, kp,   \
                     vp, (uint16_t*)o.data_ptr(), zp, Nq, Nk, D, H, Hkv,      \
                     scale, qb, qh, qr, kb, kh, kr, ob, oh, orr)
  switch (dpad) {
    case 48: LAUNCH_D(48); break;
    case 64: LAUNCH_D(64); break;
    case 96: LAUNCH_D(96); break;
    case 128: LAUNCH_D(128); break;
    case 160: LAUNCH_D(160); break;
  }
#undef LAUNCH_D
  HIP_CHECK_LAUNCH();
  return o;
}

// Legacy layout: q [B*H, N, D] contiguous (one head per batch row).
torch::Tensor attn_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                       int64_t heads, int64_t kv_heads, int64_t nk_real,
                       double scale) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kBFloat16);
  TORCH_CHECK(q.dim() == 3 && q.is_contiguous() && k.is_contiguous()
              && v.is_contiguous());
  const int D = q.size(2);
  const int Nq = q.size(1), Nk = (int)nk_real;
  const int BH = q.size(0);
  TORCH_CHECK(BH % heads == 0);
  const int batch = BH / (int)heads;
  const long long qr = D, qh = (long long)Nq * D,
                  qb = (long long)heads * Nq * D;
  const long long kr = D, kh = (long long)k.size(1) * D,
                  kb = (long long)kv_heads * k.size(1) * D;
  auto o = torch::empty({batch, Nq, heads * D}, q.options());
  launch_attn_raw((const uint16_t*)q.data_ptr(), (const uint16_t*)k.data_ptr(),
                  (const uint16_t*)v.data_ptr(), o, (int)heads, (int)kv_heads,
                  Nq, Nk, D, (float)scale, qb, qh, qr, kb, kh, kr, batch);
  // packed output [B, Nq, H*D] -> legacy [B*H, Nq, D] view requires a
  // permute copy; callers of the legacy API accept it (tests, WAN path)
  return o.reshape({batch, Nq, (int)heads, D})
      .permute({0, 2, 1, 3})
      .reshape({BH, Nq, D})
      .contiguous();
}

// Packed layout: q [B, Nq, H*D], k/v [B, Nk, Hkv*D] — the natural output of
// fused QKV projections; zero host-side reshapes.
torch::Tensor attn_fwd_packed(torch::Tensor q, torch::Tensor k,
                              torch::Tensor v, int64_t heads,
                              int64_t kv_heads, double scale) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kBFloat16);
  TORCH_CHECK(q.dim() == 3 && q.is_contiguous() && k.is_contiguous()
              && v.is_contiguous());
  const int B = q.size(0), Nq = q.size(1), Nk = k.size(1);
  const int D = q.size(2) / (int)heads;
  TORCH_CHECK((int)(heads * D) == q.size(2), "q last dim must be H*D");
  TORCH_CHECK((int)(kv_heads * D) == k.size(2), "k last dim must be Hkv*D");
  const long long qr = (long long)heads * D, qh = D,
                  qb = (long long)Nq * heads * D;
  const long long kr = (long long)kv_heads * D, kh = D,
                  kb = (long long)Nk * kv_heads * D;
  auto o = torch::empty_like(q);
  launch_attn_raw((const uint16_t*)q.data_ptr(), (const uint16_t*)k.data_ptr(),
                  (const uint16_t*)v.data_ptr(), o, (int)heads, (int)kv_heads,
                  Nq, Nk, D, (float)scale, qb, qh, qr, kb, kh, kr, B);
  return o;
}

// Fused self-attention: qkv [B, N, 3*H*D] from one projection GEMM; the
// kernel reads q/k/v through strides — zero splits, zero copies.
torch::Tensor attn_fwd_qkv(torch::Tensor qkv, int64_t heads, double scale) {
  TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16);
  TORCH_CHECK(qkv.dim() == 3 && qkv.is_contiguous());
  const int B = qkv.size(0), N = qkv.size(1);
  const int HD = qkv.size(2) / 3;
  const int D = HD / (int)heads;
  TORCH_CHECK(3 * HD == qkv.size(2) && (int)heads * D == HD);
  const long long rstride = 3LL * HD, hstride = D,
                  bstride = (long long)N * 3 * HD;
  auto o = torch::empty({B, N, HD}, qkv.options());
  const uint16_t* base = (const uint16_t*)qkv.data_ptr();
  launch_attn_raw(base, base + HD, base + 2 * HD, o, (int)heads, (int)heads,
                  N, N, D, (float)scale, bstride, hstride, rstride, bstride,
                  hstride, rstride, B);
  return o;
}

// Fused cross-attention: q [B, Nq, H*D], kv [B, Nk, 2*H*D].
torch::Tensor attn_fwd_q_kv(torch::Tensor q, torch::Tensor kv, int64_t heads,
                            double scale) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kBFloat16);
  TORCH_CHECK(q.is_contiguous() && kv.is_contiguous());
  const int B = q.size(0), Nq = q.size(1), Nk = kv.size(1);
  const int HD = q.size(2);
  const int D = HD / (int)heads;
  TORCH_CHECK(2 * HD == kv.size(2));
  const long long qr = HD, qh = D, qb = (long long)Nq * HD;
  const long long kr = 2LL * HD, kh = D, kb = (long long)Nk * 2 * HD;
  auto o = torch::empty_like(q);
  const uint16_t* kvp = (const uint16_t*)kv.data_ptr();
  launch_attn_raw((const uint16_t*)q.data_ptr(), kvp, kvp + HD, o, (int)heads,
                  (int)heads, Nq, Nk, D, (float)scale, qb, qh, qr, kb, kh, kr,
                  B);
  return o;
}
