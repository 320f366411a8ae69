// FP8 (OCP e4m3fn) flash-attention forward for head dim 128 (WAN, Flux) on
// MI355X/gfx950, and the quantiser that prepares its operands.
//
//   attn_quant_fp8(q, k, v, heads) -> q codes [B,Nq,H*128] + scale [B,Nq,H]
//                                     k codes [B,H,Nkp,128] + scale [B,H,Nkp/128]
//                                     v codes [B,H,128,Nkp] + scale [B,H,128]
//                                     k mean  [B,H*128]
//   attn_fwd_fp8(those, Nk, scale) -> o [B,Nq,H*128] bf16
//   attn_fwd_fp8_sparse(those, Nk, scale, idx, cnt) -> the same over a list
//                                     of key tiles per 256-row q-block
//                                     (attn_fp8_kernel_t, below)
//
// Nkp = Nk rounded up to 128; pad keys are zero codes. K has its per-(batch,
// head, channel) mean over the keys removed before it is quantised (softmax
// does not see a per-row constant; the e4m3 range is not spent on channel
// offsets). V is stored transposed, and inside every 128-key tile position
// 64a + 16g + 4f + r holds key 64a + 16f + 4g + r: the order in which the PV
// A operand holds a lane's P values (below). So the attention kernel stages K
// rows and V^T rows with straight 16-byte copies.
//
// Quantiser, four launches, no atomics, no memset, fixed summation order:
//   attn_col_partial_kernel  per 64-key chunk and column: sum of K, absmax of
//                            V, rows added one after the other in key order
//   attn_col_final_kernel    chunk partials added in chunk order; mean =
//                            sum * fl(1/Nk); V scale = max(amax, floor)/448
//   attn_quant_q_kernel      16 lanes per (token, head): absmax, scale, codes
//   attn_quant_kv_kernel     one workgroup per (head, 128-key block), z = 0:
//                            K - mean, block absmax, codes; z = 1: V codes,
//                            transposed and permuted through LDS
//   code = rne_e4m3(clamp(x * (1 / scale), +-448)) throughout.
//
// attn_fp8_kernel. Both products are v_mfma_scale_f32_16x16x128_f8f6f4 with
// all E8M0 scales 1.0. A lane of k-group g = lane >> 4 supplies the
// instruction with K-elements [16g, 16g+16) and [64+16g, 64+16g+16).
//   * Work split: 8 waves x 32 q rows = 256 q rows per workgroup, key tile
//     128. A wave holds two Q fragments (16 VGPRs), so every K fragment and
//     every V^T fragment it reads from LDS feeds two MFMAs: 32 KB of fragment
//     reads per tile for 32 MFMAs, where 16 rows per wave would read the same
//     32 KB for 16. Scores 64 + O 64 + Q 16 + staging 16 + P 16 registers fit
//     the 256 of two waves per SIMD with 0 scratch, once the staging loads
//     are buffer loads (a scalar descriptor and one 32-bit lane offset per
//     image, where global loads kept three 64-bit address pairs per lane) and
//     the lane bookkeeping of the tail mask and the epilogue is taken again
//     where it is used. Rejected: 16 rows per wave (LDS reads per MFMA doubled, the likely limit at the fp8 MFMA rate); 64 rows per wave
//     (scores and O alone take 256 registers).
//   * QK^T swapped: S^T = mfma(K frag, Q frag), one instruction contracts all
//     of D for 16 keys x 16 q rows; a lane's 32 scores per Q fragment are keys
//     16f + 4g + r of q row lane & 15. Q and K go through the same lane->k
//     map, so the order inside D does not matter.
//   * Softmax in the exp2 domain on the raw code products: the tile max is
//     taken on the MFMA outputs and multiplied once by sq[row] * scale *
//     log2e (per lane) * sk[tile] (per tile); every score then takes one fma
//     and one exp2. P carries the power-of-two scale 2^ATTN_FP8_SP (SP = 6)
//     in the fma's addend. The running max is raised only when a tile max
//     leads it by more than DEFER = 2 (log2 units), so
//     p' <= 2^(SP + DEFER) * (1 + 2^-20) = 256 < 448: the e4m3 conversion
//     never saturates and needs no clamp, p = 1 sits two binades under the
//     top of the range and weights down to 2^-12 keep a normal mantissa.
//     Row sums are fp32 sums of the unrounded p'. When the maximum rises by
//     more than SP + DEFER + 10, all weights already in O are under half of
//     e4m3's smallest step in the new frame and O restarts from zero, as the
//     definition (which rounds against the final maximum) has them. This is
//     fidelity to the definition, not accuracy: without it the kernel would
//     keep those contributions, which the row sum still counts. N such keys
//     carry at most N * 2^-18 of a row's weight between them (1/8 at 32k
//     keys, all of them 18 binades under the maximum); the bound's subnormal
//     term covers exactly this.
//   * P -> PV operand in registers: v_cvt_pk_fp8_f32 packs p[f][0..3] into
//     dword f, so byte 4f + r of the lane's 32-byte A operand is key
//     16f + 4g + r, which the instruction treats as K-element 64(f>>2) + 16g +
//     4(f&3) + r: the position the quantiser gave that key in V^T.
//   * K and V^T tiles (16 KB each, contiguous rows) are staged once per
//     workgroup through registers into double-buffered LDS, one barrier per
//     tile: the loads of tile t+2 fly under the compute of tile t+1. LDS rows
//     have a pitch of 160 bytes = 10 sixteen-byte slots (== 2 mod 4), the
//     conflict-free ds_read_b128 rule of attention.hip. Rejected for now:
//     global_load_lds, which writes 1 KB contiguous per wave instruction and
//     would need the swizzled, unpadded image of gemm_tile.h.
//   * Key tail masked on the last tile only (pad codes are zero, but a zero
//     logit is not a masked one). Epilogue: one reciprocal of the row sum,
//     the V channel scale, one bf16 rounding.
//   * Workgroups renumbered per XCD as in attn_fwd_kernel when B*H % 8 == 0;
//     64-bit row bases; no atomics, no workspace.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

#define AF8_D 128
#define AF8_KT 128
#define AF8_WAVES 8
#define AF8_QROWS (AF8_WAVES * 32)  // q rows per workgroup
#define AF8_THREADS (AF8_WAVES * 64)
#define AF8_PITCH 160               // LDS row pitch in bytes
#define AF8_TILE (AF8_KT * AF8_PITCH)
#define AF8_SP 6.0f
#define AF8_DEFER 2.0f
#define AF8_LOG2E 1.4426950408889634f
#define AF8_CHUNK 64                // keys per column-pass partial

// 8 fp32 values times inv -> 8 e4m3 bytes, value j in byte j (fp8_quant8 of
// common.h for values that are no longer bf16)
__device__ __forceinline__ u32x2_t af8_quant8(const float* x, float inv) {
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
    f[j] = fminf(fmaxf(x[j] * inv, -E4M3_MAX), E4M3_MAX);
  int w0 = 0, w1 = 0;
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], w0, false);
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w0, true);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], w1, false);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], w1, true);
  return u32x2_t{(unsigned)w0, (unsigned)w1};
}

// ---------------------------------------------------------------------------
// column pass: K channel sums and V channel absmax, per 64-key chunk
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
attn_col_partial_kernel(const uint16_t* __restrict__ k,
                        const uint16_t* __restrict__ v,
                        float* __restrict__ psum, float* __restrict__ pmax,
                        int N, int HD, int nchunk) {
  const int c0 = (blockIdx.x * 256 + threadIdx.x) * 8;
  if (c0 >= HD) return;
  const int chunk = blockIdx.y, b = blockIdx.z;
  const int r0 = chunk * AF8_CHUNK;
  const int r1 = min(N, r0 + AF8_CHUNK);
  const long long base = ((long long)b * N + r0) * HD + c0;
  float s[8], m[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = m[j] = 0.f;
  for (int r = 0; r < r1 - r0; ++r) {
    const ushort8_t kv = *reinterpret_cast<const ushort8_t*>(
        k + base + (long long)r * HD);
    const ushort8_t vv = *reinterpret_cast<const ushort8_t*>(
        v + base + (long long)r * HD);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s[j] += bf16_bits_to_f32(kv[j]);
      m[j] = fmaxf(m[j], fabsf(bf16_bits_to_f32(vv[j])));
    }
  }
  const long long o = ((long long)b * nchunk + chunk) * HD + c0;
  *reinterpret_cast<f32x4_t*>(psum + o) = f32x4_t{s[0], s[1], s[2], s[3]};
  *reinterpret_cast<f32x4_t*>(psum + o + 4) = f32x4_t{s[4], s[5], s[6], s[7]};
  *reinterpret_cast<f32x4_t*>(pmax + o) = f32x4_t{m[0], m[1], m[2], m[3]};
  *reinterpret_cast<f32x4_t*>(pmax + o + 4) = f32x4_t{m[4], m[5], m[6], m[7]};
}

__global__ void __launch_bounds__(256)
attn_col_final_kernel(const float* __restrict__ psum,
                      const float* __restrict__ pmax,
                      float* __restrict__ kmean, float* __restrict__ vscale,
                      int HD, int nchunk, float inv_n) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= HD) return;
  const int b = blockIdx.y;
  float s = 0.f, m = 0.f;
  for (int j = 0; j < nchunk; ++j) {
    const long long o = ((long long)b * nchunk + j) * HD + c;
    s += psum[o];
    m = fmaxf(m, pmax[o]);
  }
  kmean[(long long)b * HD + c] = s * inv_n;
  vscale[(long long)b * HD + c] = fp8_row_scale(m);
}

// ---------------------------------------------------------------------------
// convert pass
// ---------------------------------------------------------------------------

// Q: thread = 8 adjacent elements, 16 threads = one (token, head) row
__global__ void __launch_bounds__(256)
attn_quant_q_kernel(const uint16_t* __restrict__ x, uint8_t* __restrict__ q,
                    float* __restrict__ scale, long long nvec) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool ok = i < nvec;
  ushort8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
  if (ok) v = *reinterpret_cast<const ushort8_t*>(x + i * 8);
  float amax = fp8_absmax8(v, 0.f);
#pragma unroll
  for (int off = 8; off > 0; off >>= 1)
    amax = fmaxf(amax, __shfl_xor(amax, off, 64));
  const float s = fp8_row_scale(amax);
  if (!ok) return;
  if ((threadIdx.x & 15) == 0) scale[i >> 4] = s;
  *reinterpret_cast<u32x2_t*>(q + i * 8) = fp8_quant8(v, fp8_row_inv_scale(s));
}

// K (blockIdx.z == 0) and V (1) of one (batch, head, 128-key block). Thread
// (krow = tid >> 4, c = tid & 15) takes channels 8c.. of keys 16p + krow.
__global__ void __launch_bounds__(256)
attn_quant_kv_kernel(const uint16_t* __restrict__ k,
                     const uint16_t* __restrict__ v,
                     const float* __restrict__ kmean,
                     const float* __restrict__ vscale,
                     uint8_t* __restrict__ kq, float* __restrict__ kscale,
                     uint8_t* __restrict__ vq, int N, int Np, int H) {
  __shared__ float red[8];
  __shared__ __align__(16) uint8_t vt[AF8_D][AF8_KT + 16];
  const int blk = blockIdx.x, bh = blockIdx.y;
  const int b = bh / H, h = bh % H;
  const int HD = H * AF8_D;
  const int d0 = (threadIdx.x & 15) * 8, krow = threadIdx.x >> 4;
  const long long src0 = (long long)b * N * HD + h * AF8_D + d0;
  const long long cbase = (long long)b * HD + h * AF8_D + d0;

  if (blockIdx.z == 0) {
    float mean[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) mean[j] = kmean[cbase + j];
    float x[8][8];
    float amax = 0.f;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const int key = blk * AF8_KT + p * 16 + krow;
      if (key < N) {
        const ushort8_t u = *reinterpret_cast<const ushort8_t*>(
            k + src0 + (long long)key * HD);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          x[p][j] = bf16_bits_to_f32(u[j]) - mean[j];
          amax = fmaxf(amax, fabsf(x[p][j]));
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) x[p][j] = 0.f;  // pad key: zero code
      }
    }
    amax = block_reduce(amax, red, MaxOp{}, 0.f);
    const float s = fp8_row_scale(amax);
    const float inv = fp8_row_inv_scale(s);
    if (threadIdx.x == 0) kscale[(long long)bh * (Np / AF8_KT) + blk] = s;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const int key = blk * AF8_KT + p * 16 + krow;
      *reinterpret_cast<u32x2_t*>(
          kq + ((long long)bh * Np + key) * AF8_D + d0) = af8_quant8(x[p], inv);
    }
    return;
  }

  float inv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) inv[j] = fp8_row_inv_scale(vscale[cbase + j]);
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int kl = p * 16 + krow;  // key inside the tile
    const int key = blk * AF8_KT + kl;
    ushort8_t u = {0, 0, 0, 0, 0, 0, 0, 0};
    if (key < N)
      u = *reinterpret_cast<const ushort8_t*>(v + src0 + (long long)key * HD);
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      f[j] = fminf(fmaxf(bf16_bits_to_f32(u[j]) * inv[j], -E4M3_MAX), E4M3_MAX);
    int w0 = 0, w1 = 0;
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], w0, false);
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w0, true);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], w1, false);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], w1, true);
    // key 64a + 16f + 4g + r -> position 64a + 16g + 4f + r
    const int pos = (kl & 0x43) | ((kl & 0x30) >> 2) | ((kl & 0x0c) << 2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      vt[d0 + j][pos] = (uint8_t)((unsigned)w0 >> (8 * j));
      vt[d0 + 4 + j][pos] = (uint8_t)((unsigned)w1 >> (8 * j));
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int pc = threadIdx.x + i * 256;
    const int d = pc >> 3, slot = pc & 7;
    *reinterpret_cast<i32x4_t*>(
        vq + ((long long)bh * AF8_D + d) * Np + blk * AF8_KT + slot * 16) =
        *reinterpret_cast<const i32x4_t*>(&vt[d][slot * 16]);
  }
}

// ---------------------------------------------------------------------------
// the flash forward
// ---------------------------------------------------------------------------

// Compiled without the packed fp32 instructions, as attention_wide.hip: paired
// into v_pk_*_f32 the rescale and softmax arithmetic needs aligned register
// pairs and the kernel spills (84 VGPRs). A function with the attribute cannot
// inline one without it, so the helpers the kernel needs are defined inside
// the region and the staging steps are macros, not lambdas.
#if defined(__HIP_DEVICE_COMPILE__)  // the host pass does not know the feature
#pragma clang attribute push(                                              \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// value of `v` in lane `src` (ds_bpermute: no LDS storage involved)
__device__ __forceinline__ float af8_shfl(float v, int src) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute(src << 2, __builtin_bit_cast(int, v)));
}

// workgroup barrier that orders LDS accesses, as __syncthreads()
__device__ __forceinline__ void af8_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// 16 bytes at base + voff + soff through a buffer descriptor: the base stays
// in SGPRs, the lane offset is one 32-bit register and the tile offset a
// scalar, where a global load keeps a 64-bit address pair per lane and piece
__device__ __forceinline__ i32x4_t af8_load16(__amdgpu_buffer_rsrc_t rsrc,
                                              unsigned voff, unsigned soff) {
  return __builtin_bit_cast(
      i32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 0));
}

// f32 -> bf16 bits, round to nearest even
__device__ __forceinline__ uint16_t af8_bf16(float x) {
  uint32_t r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %1" : "=v"(r) : "v"(x));
  return (uint16_t)r;
}

// key-tile number at position `pos` of a q-block's list, as a wave-uniform
// scalar, clamped to the tiles the K scales cover: a bad list gives wrong
// numbers, not a read outside sk (the K / V^T loads are bounded by their
// descriptors either way). `pos` past the row reads the row's last entry.
__device__ __forceinline__ int af8_list_tile(const int* __restrict__ lst,
                                             int pos, int maxc, int ntiles) {
  const int t = __builtin_amdgcn_readfirstlane(lst[min(pos, maxc - 1)]);
  return min(max(t, 0), ntiles - 1);
}

// the thread id from the wave number (a scalar) and the hardware lane count;
// volatile, so that it is taken where it is used and not kept in a register
__device__ __forceinline__ unsigned af8_tid(int wave_s) {
  unsigned l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0"
               : "=v"(l));
  return (unsigned)wave_s * 64u + l;
}

// Two kernels from one body. attn_fp8_kernel = attn_fp8_kernel_t<false> walks
// the key tiles 0..Np/128 and ignores idx, cnt and maxc (null).
// attn_fp8_sparse_kernel = attn_fp8_kernel_t<true> is the block-sparse form:
// for q-block y = row / 256 it walks the ascending key-tile numbers
// idx[y][0 .. cnt[y]) of idx [gridDim.y, maxc]; one list per q-block, shared
// by every batch and head. What differs is confined to scalars:
//   * tile numbers are read with uniform (scalar) loads two list positions
//     ahead of the compute, since position i + 2's loads are issued in
//     iteration i, and stay in SGPRs; each is clamped to [0, Np/128 - 1]
//   * the tile number of the position replaces the loop counter in the K /
//     V^T prefetch offsets, in sk[] and in the key-tail test: all keyed by
//     tile, never by position
//   * the trip count is cnt[y]; 1 and 2 are the dense kernel's ntiles 1 and 2
//   * the few more scalars in flight move the register allocation of a
//     kernel that sits at 256 VGPRs: the sparse form rebuilds the thread id,
//     and the staging offsets that derive from it, where they are used
//     (af8_tid), which keeps it at 0 scratch
// Two instantiations of a template, not two wrappers around an inlined body:
// inlined, the same source compiled to a dense kernel with 2 spilled VGPRs.
// Grid, XCD renumbering, LDS images, softmax and epilogue are shared; no
// atomics, workspace or memset, so the output is the same bits every call.
template <bool SPARSE>
__global__ __launch_bounds__(AF8_THREADS)
__attribute__((amdgpu_waves_per_eu(2, 2))) void attn_fp8_kernel_t(
    const uint8_t* __restrict__ q,    // [B, Nq, H*128] e4m3
    const float* __restrict__ sq,     // [B, Nq, H]
    const uint8_t* __restrict__ kq,   // [B*H, Np, 128] e4m3
    const float* __restrict__ sk,     // [B*H, Np/128]
    const uint8_t* __restrict__ vq,   // [B*H, 128, Np] e4m3, keys permuted
    const float* __restrict__ sv,     // [B*H, 128]
    uint16_t* __restrict__ o,         // [B, Nq, H*128] bf16
    const uint8_t* __restrict__ zp,   // 128 zero bytes: rows past Nq
    const int* __restrict__ idx,      // [gridDim.y, maxc] key-tile numbers
    const int* __restrict__ cnt,      // [gridDim.y] valid entries, >= 1
    int maxc, int Nq, int Nk, int Np, int H, float scale) {
  __shared__ __align__(16) uint8_t lds[2][2][AF8_TILE];  // [buffer][K | V^T]

  int wave_s = 0;
  if constexpr (SPARSE)
    wave_s = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int fr = lane & 15, g = lane >> 4;
  // XCD renumbering of attn_fwd_kernel: placement only
  int bh = blockIdx.x, qblk = blockIdx.y;
  if ((gridDim.x & 7) == 0) {
    const unsigned lin = blockIdx.y * gridDim.x + blockIdx.x;
    const unsigned idx = lin >> 3;
    bh = (int)(idx / gridDim.y) * 8 + (int)(lin & 7);
    qblk = (int)(idx % gridDim.y);
  }
  const int b = bh / H, h = bh % H;
  const int q_row0 = qblk * AF8_QROWS + wave * 32;
  const int ntiles = Np / AF8_KT;

  // ---- Q fragments and the per-lane logit constants ----------------------
  i32x8_t qf[2];
  float cq[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int row = q_row0 + a * 16 + fr;
    const bool ok = row < Nq;
    const long long rh = ((long long)b * Nq + (ok ? row : 0)) * H + h;
    const uint8_t* src = ok ? q + rh * AF8_D : zp;
    const i32x4_t h0 = *reinterpret_cast<const i32x4_t*>(src + 16 * g);
    const i32x4_t h1 = *reinterpret_cast<const i32x4_t*>(src + 64 + 16 * g);
    qf[a] = i32x8_t{h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
    cq[a] = sq[rh] * scale * AF8_LOG2E;
  }

  // ---- staging: piece pc = tid + 512 s of a 16 KB tile is row pc >> 3,
  // slot pc & 7, for K rows (128 contiguous bytes each) and V^T rows alike
  // (the second piece is 64 rows further). Uniform 64-bit bases + one 32-bit
  // lane offset each: Np * 128 < 2^31 is checked by the launcher
  // descriptors of this head's K and V^T images (Np * 128 bytes each; 0x20000:
  // raw 32-bit data format): a load past the image would return zeros
  const __amdgpu_buffer_rsrc_t k_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(kq + (long long)bh * Np * AF8_D), 0, Np * AF8_D,
      0x00020000);
  const __amdgpu_buffer_rsrc_t v_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(vq + (long long)bh * Np * AF8_D), 0, Np * AF8_D,
      0x00020000);
  const unsigned k_off = threadIdx.x * 16;
  const unsigned v_off = (threadIdx.x >> 3) * Np + (threadIdx.x & 7) * 16;
  const unsigned st_off = (threadIdx.x >> 3) * AF8_PITCH + (threadIdx.x & 7) * 16;
  i32x4_t kreg[2], vreg[2];
#define AF8_PREFETCH(T)                                                       \
  {                                                                           \
    unsigned ko_ = k_off, vo_ = v_off;                                        \
    if constexpr (SPARSE) {                                                   \
      const unsigned tid_ = af8_tid(wave_s);                                  \
      ko_ = tid_ * 16;                                                        \
      vo_ = (tid_ >> 3) * Np + (tid_ & 7) * 16;                               \
    }                                                                         \
    _Pragma("unroll") for (int s_ = 0; s_ < 2; ++s_) {                        \
      kreg[s_] = af8_load16(k_rsrc, ko_,                                      \
                            (unsigned)(T) * (AF8_KT * AF8_D) +                \
                                (unsigned)s_ * (AF8_THREADS * 16));           \
      vreg[s_] = af8_load16(v_rsrc, vo_,                                      \
                            (unsigned)(T) * AF8_KT +                          \
                                (unsigned)s_ * 64u * (unsigned)Np);           \
    }                                                                         \
  }
#define AF8_COMMIT(P)                                                         \
  _Pragma("unroll") for (int s_ = 0; s_ < 2; ++s_) {                          \
    *reinterpret_cast<i32x4_t*>(                                              \
        &lds[P][0][st_off + s_ * 64 * AF8_PITCH]) = kreg[s_];                 \
    *reinterpret_cast<i32x4_t*>(                                              \
        &lds[P][1][st_off + s_ * 64 * AF8_PITCH]) = vreg[s_];                 \
  }

  float m_run[2] = {-1e30f, -1e30f}, l_run[2] = {0.f, 0.f};
  f32x4_t oacc[2][8];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int n = 0; n < 8; ++n) oacc[a][n] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // nt list positions are walked. Sparse: tc and tn are the tile numbers of
  // positions i and i + 1, scalars taken from the list two positions ahead
  // of the compute, since position i + 2's loads are issued in iteration i
  int nt = ntiles, tc = 0, tn = 1;
  const int* lst = nullptr;
  if constexpr (SPARSE) {
    lst = idx + (long long)qblk * maxc;
    nt = min(max(__builtin_amdgcn_readfirstlane(cnt[qblk]), 1), maxc);
    tc = af8_list_tile(lst, 0, maxc, ntiles);
    tn = af8_list_tile(lst, 1, maxc, ntiles);
  }

  AF8_PREFETCH(tc)
  AF8_COMMIT(0)
  if (nt > 1) AF8_PREFETCH(tn)
  af8_sync();

  const unsigned frag_off = fr * AF8_PITCH + 16 * g;

  for (int i = 0; i < nt; ++i) {
    const int p = i & 1;
    int t = i, t2 = i + 2;  // tile numbers of positions i and i + 2
    if constexpr (SPARSE) {
      t = tc;
      t2 = af8_list_tile(lst, i + 2, maxc, ntiles);
    }
    const int key0 = t * AF8_KT;
    const uint8_t* kl = &lds[p][0][frag_off];
    const uint8_t* vl = &lds[p][1][frag_off];

    // ---- S^T = K Q^T on the codes: s[a][f][r] = key 16f + 4g + r, q row fr
    f32x4_t s[2][8];
#pragma unroll
    for (int f = 0; f < 8; ++f) {
      // at most four fragments' reads in flight: hoisted all eight, they
      // take 64 registers beside the scores and O, and the kernel spills
      if ((f & 1) == 0) __builtin_amdgcn_sched_barrier(0);
      const i32x4_t h0 =
          *reinterpret_cast<const i32x4_t*>(kl + f * 16 * AF8_PITCH);
      const i32x4_t h1 =
          *reinterpret_cast<const i32x4_t*>(kl + f * 16 * AF8_PITCH + 64);
      const i32x8_t kf =
          i32x8_t{h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
#pragma unroll
      for (int a = 0; a < 2; ++a)
        s[a][f] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            kf, qf[a], f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0, 0x7f7f7f7f, 0,
            0x7f7f7f7f);
    }

    __builtin_amdgcn_sched_barrier(0);
    if (key0 + AF8_KT > Nk) {  // wave-uniform: the last tile's key tail
      // the lane's k-group from the hardware lane count, on this one tile
      // (volatile: hoisted out of the loop it would be a register, or a
      // spill slot, kept through every tile)
      int lm;
      asm volatile(
          "v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0"
          : "=v"(lm));
      const int gm = lm >> 4;
#pragma unroll
      for (int f = 0; f < 8; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (key0 + f * 16 + gm * 4 + r >= Nk)
            s[0][f][r] = s[1][f][r] = -__builtin_inff();
    }

    // ---- online softmax; the logit factor is positive, so the max is taken
    // on the raw products and scaled once
    const float skt = sk[(long long)bh * ntiles + t];
    float ct[2], mt[2];
    bool need = false;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      float m = s[a][0][0];
#pragma unroll
      for (int f = 0; f < 8; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) m = fmaxf(m, s[a][f][r]);
      m = fmaxf(m, af8_shfl(m, lane ^ 16));
      m = fmaxf(m, af8_shfl(m, lane ^ 32));
      // kept a normal positive number (an all-zero K block has the floor
      // scale 2^-126): -inf * ct stays -inf for the masked keys
      ct[a] = fmaxf(cq[a] * skt, 0x1p-126f);
      mt[a] = m * ct[a];
      need |= (mt[a] - m_run[a]) > AF8_DEFER;
    }
    if (__builtin_amdgcn_ballot_w64(need) != 0ull) {
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const float m_new = fmaxf(m_run[a], mt[a]);
        const float al = __builtin_amdgcn_exp2f(m_run[a] - m_new);
        // Under 2^-(SP + DEFER + 10) every weight summed into O so far is,
        // against the new maximum, below 2^-10: half of e4m3's smallest
        // step, which the definition rounds to zero. O drops them too (the
        // row sum, taken from unrounded weights, keeps them).
        const float al_o =
            m_run[a] - m_new < -(AF8_SP + AF8_DEFER + 10.f) ? 0.f : al;
        m_run[a] = m_new;
        l_run[a] *= al;
        // O rows are 4g + r: their alpha is held by lane (g-group, fr == row)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float ar = af8_shfl(al_o, (lane & 48) | (g * 4 + r));
#pragma unroll
          for (int n = 0; n < 8; ++n) oacc[a][n][r] *= ar;
        }
      }
    }

    // ---- p' = 2^(SP + logit - m_run) -> e4m3, straight into the PV operand
    i32x8_t pf[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const float add = AF8_SP - m_run[a];
#pragma unroll
      for (int f = 0; f < 8; ++f) {
        float e[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          e[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[a][f][r], ct[a], add));
          l_run[a] += e[r];
        }
        int w = 0;
        w = __builtin_amdgcn_cvt_pk_fp8_f32(e[0], e[1], w, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(e[2], e[3], w, true);
        pf[a][f] = w;
      }
    }

    // ---- O += P V: V^T fragment n is channels 16n + fr, keys in P's order
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      if ((n & 3) == 0) __builtin_amdgcn_sched_barrier(0);
      const i32x4_t h0 =
          *reinterpret_cast<const i32x4_t*>(vl + n * 16 * AF8_PITCH);
      const i32x4_t h1 =
          *reinterpret_cast<const i32x4_t*>(vl + n * 16 * AF8_PITCH + 64);
      const i32x8_t vf =
          i32x8_t{h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
#pragma unroll
      for (int a = 0; a < 2; ++a)
        oacc[a][n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            pf[a], vf, oacc[a][n], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
    }

    // ---- position i+1's tile into the other buffer (last read during
    // position i-1, before the previous barrier), then position i+2's loads
    if (i + 1 < nt) {
      AF8_COMMIT(p ^ 1)
      if (i + 2 < nt) AF8_PREFETCH(t2)
    }
    af8_sync();
    if constexpr (SPARSE) {
      tc = tn;
      tn = t2;
    }
  }

  // ---- epilogue: 1 / row sum, V channel scale, one bf16 rounding ---------
  // lane bookkeeping taken again from the thread id, so that none of it
  // has to live in a register through the tile loop
  int tid_e = threadIdx.x;
  if constexpr (SPARSE) tid_e = (int)af8_tid(wave_s);
  asm volatile("" : "+v"(tid_e));
  const int fr_e = tid_e & 15, g_e = (tid_e >> 4) & 3;
  const int lane_e = tid_e & 63;
  const int q_row_e = qblk * AF8_QROWS + (tid_e >> 6) * 32;
  float svd[8];
#pragma unroll
  for (int n = 0; n < 8; ++n)
    svd[n] = sv[(long long)bh * AF8_D + n * 16 + fr_e];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    float l = l_run[a];
    l += af8_shfl(l, lane_e ^ 16);
    l += af8_shfl(l, lane_e ^ 32);
    const float rl_own = __builtin_amdgcn_rcpf(l);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float rl = af8_shfl(rl_own, (lane_e & 48) | (g_e * 4 + r));
      const int row = q_row_e + a * 16 + g_e * 4 + r;
      if (row >= Nq) continue;
      uint16_t* orow =
          o + (((long long)b * Nq + row) * H + h) * AF8_D + fr_e;
#pragma unroll
      for (int n = 0; n < 8; ++n)
        orow[n * 16] = af8_bf16(oacc[a][n][r] * rl * svd[n]);
    }
  }
}

#undef AF8_PREFETCH
#undef AF8_COMMIT
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// the names the launchers, the documents and the profiles use
static constexpr auto attn_fp8_kernel = attn_fp8_kernel_t<false>;
static constexpr auto attn_fp8_sparse_kernel = attn_fp8_kernel_t<true>;

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

int64_t attn_fp8_qrows() { return AF8_QROWS; }
int64_t attn_fp8_sp() { return (int64_t)AF8_SP; }

static void check_packed_bf16(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 3 && t.is_contiguous() &&
                  t.scalar_type() == at::kBFloat16,
              name, " must be a contiguous bf16 [B, N, H*128] on device");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0, name,
              " must be 16-byte aligned");
}

// -> (q codes, q scale, k codes, k scale, v codes, v scale, k mean)
std::vector<torch::Tensor> attn_quant_fp8(torch::Tensor q, torch::Tensor k,
                                          torch::Tensor v, int64_t heads) {
  check_packed_bf16(q, "q");
  check_packed_bf16(k, "k");
  check_packed_bf16(v, "v");
  const long long B = q.size(0), Nq = q.size(1), N = k.size(1);
  const long long H = heads, HD = H * AF8_D;
  TORCH_CHECK(H >= 1 && q.size(2) == HD && k.size(2) == HD,
              "last dim must be heads * 128");
  TORCH_CHECK(k.size(0) == B && v.sizes() == k.sizes(),
              "q, k and v disagree on the batch or k and v on the shape");
  TORCH_CHECK(B >= 1 && Nq >= 1 && N >= 1 && B * H < 65536 && B < 65536 &&
                  N < (1LL << 30) && Nq < (1LL << 30),
              "attn_quant_fp8: shape out of range");
  const long long Np = (N + AF8_KT - 1) / AF8_KT * AF8_KT;
  const long long nchunk = (N + AF8_CHUNK - 1) / AF8_CHUNK;
  TORCH_CHECK(nchunk < 65536, "attn_quant_fp8: too many keys");
  auto f8 = q.options().dtype(at::kFloat8_e4m3fn);
  auto f32 = q.options().dtype(at::kFloat);
  auto qq = torch::empty({B, Nq, HD}, f8);
  auto qs = torch::empty({B, Nq, H}, f32);
  auto kc = torch::empty({B, H, Np, AF8_D}, f8);
  auto ks = torch::empty({B, H, Np / AF8_KT}, f32);
  auto vc = torch::empty({B, H, AF8_D, Np}, f8);
  auto vs = torch::empty({B, H, AF8_D}, f32);
  auto km = torch::empty({B, HD}, f32);
  auto psum = torch::empty({B, nchunk, HD}, f32);
  auto pmax = torch::empty({B, nchunk, HD}, f32);
  auto stream = at::hip::getCurrentHIPStream();
  const uint16_t* kp = (const uint16_t*)k.data_ptr();
  const uint16_t* vp = (const uint16_t*)v.data_ptr();

  hipLaunchKernelGGL(attn_col_partial_kernel,
                     dim3((unsigned)((HD / 8 + 255) / 256), (unsigned)nchunk,
                          (unsigned)B),
                     dim3(256), 0, stream, kp, vp, psum.data_ptr<float>(),
                     pmax.data_ptr<float>(), (int)N, (int)HD, (int)nchunk);
  hipLaunchKernelGGL(attn_col_final_kernel,
                     dim3((unsigned)((HD + 255) / 256), (unsigned)B), dim3(256),
                     0, stream, psum.data_ptr<float>(), pmax.data_ptr<float>(),
                     km.data_ptr<float>(), vs.data_ptr<float>(), (int)HD,
                     (int)nchunk, (float)(1.0 / (double)N));
  const long long nvec = B * Nq * HD / 8;
  TORCH_CHECK((nvec + 255) / 256 < (1LL << 31), "attn_quant_fp8: q too large");
  hipLaunchKernelGGL(attn_quant_q_kernel, dim3((unsigned)((nvec + 255) / 256)),
                     dim3(256), 0, stream, (const uint16_t*)q.data_ptr(),
                     (uint8_t*)qq.data_ptr(), qs.data_ptr<float>(), nvec);
  hipLaunchKernelGGL(attn_quant_kv_kernel,
                     dim3((unsigned)(Np / AF8_KT), (unsigned)(B * H), 2),
                     dim3(256), 0, stream, kp, vp, km.data_ptr<float>(),
                     vs.data_ptr<float>(), (uint8_t*)kc.data_ptr(),
                     ks.data_ptr<float>(), (uint8_t*)vc.data_ptr(), (int)N,
                     (int)Np, (int)H);
  HIP_CHECK_LAUNCH();
  return {qq, qs, kc, ks, vc, vs, km};
}

// idx / cnt: the block lists of attn_fp8_sparse_kernel, or null for the dense
// kernel
static torch::Tensor attn_fwd_fp8_launch(
    const torch::Tensor& qq, const torch::Tensor& qs, const torch::Tensor& kc,
    const torch::Tensor& ks, const torch::Tensor& vc, const torch::Tensor& vs,
    int64_t nk, double scale, const torch::Tensor* idx,
    const torch::Tensor* cnt) {
  auto is_f8 = [](const torch::Tensor& t) {
    return t.is_cuda() && t.is_contiguous() &&
           t.scalar_type() == at::kFloat8_e4m3fn &&
           (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0;
  };
  auto is_f32 = [](const torch::Tensor& t) {
    return t.is_cuda() && t.is_contiguous() && t.scalar_type() == at::kFloat;
  };
  TORCH_CHECK(is_f8(qq) && is_f8(kc) && is_f8(vc),
              "codes must be contiguous, 16-byte aligned float8_e4m3fn");
  TORCH_CHECK(is_f32(qs) && is_f32(ks) && is_f32(vs),
              "scales must be contiguous fp32");
  TORCH_CHECK(qq.dim() == 3 && kc.dim() == 4 && vc.dim() == 4,
              "q codes [B,Nq,H*128], k codes [B,H,Np,128], v codes "
              "[B,H,128,Np]");
  const long long B = qq.size(0), Nq = qq.size(1), H = kc.size(1),
                  Np = kc.size(2);
  TORCH_CHECK(kc.size(0) == B && kc.size(3) == AF8_D && qq.size(2) == H * AF8_D,
              "q and k codes disagree");
  TORCH_CHECK(vc.size(0) == B && vc.size(1) == H && vc.size(2) == AF8_D &&
                  vc.size(3) == Np,
              "v codes must be [B,H,128,Np]");
  TORCH_CHECK(Np >= AF8_KT && Np % AF8_KT == 0 && nk >= 1 && nk <= Np &&
                  nk > Np - AF8_KT && Np < (1LL << 24),
              "key count ", nk, " does not belong to a buffer of ", Np);
  TORCH_CHECK(qs.numel() == B * Nq * H && ks.numel() == B * H * (Np / AF8_KT) &&
                  vs.numel() == B * H * AF8_D,
              "scale shapes disagree with the codes");
  TORCH_CHECK(scale > 0.0, "attention scale must be positive, got ", scale);
  TORCH_CHECK(B >= 1 && Nq >= 1 && Nq < (1LL << 30) && B * H < (1LL << 31));
  auto o = torch::empty({B, Nq, H * AF8_D}, qq.options().dtype(at::kBFloat16));
  const long long gy = (Nq + AF8_QROWS - 1) / AF8_QROWS;
  TORCH_CHECK(gy < 65536, "attn_fwd_fp8: too many q rows");
  const dim3 grid((unsigned)(B * H), (unsigned)gy);
  if (idx == nullptr) {
    hipLaunchKernelGGL(attn_fp8_kernel, grid, dim3(AF8_THREADS), 0,
                       at::hip::getCurrentHIPStream(),
                       (const uint8_t*)qq.data_ptr(), qs.data_ptr<float>(),
                       (const uint8_t*)kc.data_ptr(), ks.data_ptr<float>(),
                       (const uint8_t*)vc.data_ptr(), vs.data_ptr<float>(),
                       (uint16_t*)o.data_ptr(),
                       (const uint8_t*)device_zero_page(qq),
                       (const int*)nullptr, (const int*)nullptr, 0, (int)Nq,
                       (int)nk, (int)Np, (int)H, (float)scale);
  } else {
    auto is_i32 = [&](const torch::Tensor& t) {
      return t.is_cuda() && t.device() == qq.device() && t.is_contiguous() &&
             t.scalar_type() == at::kInt;
    };
    TORCH_CHECK(is_i32(*idx) && is_i32(*cnt) && idx->dim() == 2 &&
                    cnt->dim() == 1,
                "idx [nqb, maxc] and cnt [nqb] must be contiguous int32 on "
                "the operands' device");
    TORCH_CHECK(cnt->numel() == gy && idx->size(0) == gy,
                "block lists are for ", cnt->numel(), " (cnt) and ",
                idx->size(0), " (idx) q-blocks of ", AF8_QROWS,
                " rows, the queries have ", gy);
    const long long maxc = idx->size(1);
    TORCH_CHECK(maxc >= 1 && maxc < (1LL << 24), "idx has ", maxc,
                " list positions per q-block, needs 1 .. 2^24 - 1");
    hipLaunchKernelGGL(attn_fp8_sparse_kernel, grid, dim3(AF8_THREADS), 0,
                       at::hip::getCurrentHIPStream(),
                       (const uint8_t*)qq.data_ptr(), qs.data_ptr<float>(),
                       (const uint8_t*)kc.data_ptr(), ks.data_ptr<float>(),
                       (const uint8_t*)vc.data_ptr(), vs.data_ptr<float>(),
                       (uint16_t*)o.data_ptr(),
                       (const uint8_t*)device_zero_page(qq),
                       (const int*)idx->data_ptr<int>(),
                       (const int*)cnt->data_ptr<int>(), (int)maxc, (int)Nq,
                       (int)nk, (int)Np, (int)H, (float)scale);
  }
  HIP_CHECK_LAUNCH();
  return o;
}

torch::Tensor attn_fwd_fp8(torch::Tensor qq, torch::Tensor qs,
                           torch::Tensor kc, torch::Tensor ks,
                           torch::Tensor vc, torch::Tensor vs, int64_t nk,
                           double scale) {
  return attn_fwd_fp8_launch(qq, qs, kc, ks, vc, vs, nk, scale, nullptr,
                             nullptr);
}

// attn_fwd_fp8 over the key tiles idx[y][0 .. cnt[y]) for q-block y. The
// values are the caller's to validate (dispatch.attn_blocks); the kernel
// clamps them, so a bad list gives wrong numbers, never a fault.
torch::Tensor attn_fwd_fp8_sparse(torch::Tensor qq, torch::Tensor qs,
                                  torch::Tensor kc, torch::Tensor ks,
                                  torch::Tensor vc, torch::Tensor vs,
                                  int64_t nk, double scale, torch::Tensor idx,
                                  torch::Tensor cnt) {
  return attn_fwd_fp8_launch(qq, qs, kc, ks, vc, vs, nk, scale, &idx, &cnt);
}
