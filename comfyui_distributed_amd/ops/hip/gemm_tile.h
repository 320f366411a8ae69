// The 256-row tile skeleton shared by gemm256_kernel (gemm.hip, bf16) and
// gemm_fp8_kernel (gemm_fp8.hip, e4m3): what depends only on the BYTE layout
// of a tile row, 128 bytes in both (64 bf16 or 128 e4m3). 8 waves (2M x 4N),
// BM = 256, BN = 128 / 256 / 320, both operands staged HBM->LDS with
// global_load_lds (glds) into double-buffered, st_16x32 XOR-swizzled images in
// ONE __shared__ object (a second one de-pipelines glds, guide §5 trap (a)),
// B before A, one vmcnt(0) + raw barrier per K-tile, MFMA operands swapped so
// a lane holds 4 adjacent output columns. Each kernel keeps its `cluster`
// (they differ for measured reasons); the conv address mode stays in gemm.hip.
#pragma once

#include <type_traits>
#include "common.h"

typedef __attribute__((ext_vector_type(8))) short s16x8_t;  // bf16 MFMA operand
typedef __attribute__((ext_vector_type(4))) int i32x4_t;
typedef __attribute__((ext_vector_type(8))) int i32x8_t;    // fp8 MFMA operand
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) uint16_t u16x4_t;

#define TILE_BM 256  // LDS: A[2][256][128 B] at ABUF, B[2][BN][128 B] at BBUF
#define TILE_ABUF 0
#define TILE_BBUF 65536
#define TILE_IMG 32768  // one 256-row A image; a B image is BN*128 bytes

template <int V>
using ic = std::integral_constant<int, V>;

// st_16x32 swizzle within each 1 KiB subtile: ds_read_b128 lane groups go to
// four 32 B slots, not two (applied on the glds SOURCE address, guide §5)
__device__ __forceinline__ unsigned swz(unsigned byte_off) {
  return byte_off ^ (((byte_off >> 9) & 1u) << 5);
}

// one 16 B/lane HBM->LDS DMA; LDS destination is wave-uniform base + lane*16,
// the GLOBAL side is per-lane (guide §5)
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_dst) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) uint32_t*)gsrc,
      (__attribute__((address_space(3))) uint32_t*)lds_dst, 16, 0, 0);
}

// ---- per-thread constants (K-invariant) ----------------------------------
// Staging per K-tile is the B image (BN/64 glds of 8 KiB) then the A image
// (2 pieces of 16 KiB, 2 glds each), row-permuted so piece 0 holds the mq=0
// rows of BOTH wave halves: quarter qq = mq*2 + wm -> (qq&1)*128+(qq>>1)*64+r.
// A slot (piece, instr i) is chunk tid + i*512 at logical byte swz(piece_off +
// chunk*16); B instr j covers rows j*64..+64 at swz((tid + j*512)*16). swz
// flips bit 5 by bit 9, so the 8 KiB chunk offsets pass through it: every
// slot of a thread has the same byte offset c_byte in the 128-byte row and the
// same row r0 in its 64-row group. That is 3 registers per A slot and 3 for
// the B image, which lets the 160-accumulator BN = 320 variant fit 256 VGPRs.
struct TileThread {
  int lane, wave;
  int wm;           // 0..1: M half (128 rows)
  int wn;           // 0..3: N strip (BN/4 cols)
  int fr, kgrp;     // MFMA fragment row and 16-byte k-group of this lane
  int r0;           // 0..63: row of this thread's chunk in a 64-row group
  int c_byte;       // byte offset of the chunk within the 128-byte row
  // base + the row within the 256-row tile that A slot (piece pc, instr i)
  // stages; summed in base's type, left to right
  template <typename I>
  __device__ __forceinline__ I a_row(I base, int pc, int i) const {
    return base + i * 128 + pc * 64 + r0;
  }
};

__device__ __forceinline__ TileThread tile_thread(int tid = threadIdx.x) {
  TileThread t;
  t.lane = tid & 63;
  t.wave = tid >> 6;
  t.wm = t.wave >> 2;
  t.wn = t.wave & 3;
  t.fr = t.lane & 15;
  t.kgrp = t.lane >> 4;
  const unsigned y0 = swz((unsigned)tid * 16u);
  t.c_byte = (int)(y0 & 127u);
  t.r0 = (int)(y0 >> 7);
  return t;
}

// The stage functions take operands BY REFERENCE (pointer type deduced, with
// its __restrict__): in the callers' lambdas each is then loaded where it is
// used, as in a hand-written body; by value the compiler reassociates the K
// loop's row addresses differently (profiles/r11_gemm_tile.md, whose
// section 1 has to be run again if these signatures change).

// ---- glds stage of B instrs [J0, J0+JN) into the B image at `img` --------
// B is row-major [N][K]; instr j reads row bn0 + 64*j: b_off = bn0*Kdim + the
// thread's element offset in the row. Rows past N read the zero page (glds
// cannot conditionally zero, but its per-lane SOURCE address is free). FENCE
// (BN = 320): keep the row addresses of the 5 instrs out of registers.
template <bool FENCE, int J0, int JN, typename P>
__device__ __forceinline__ void tile_stage_b(
    const P& Bw, const P& zero_page, const long long& b_off, const int& bn0,
    const int& N, const int& Kdim, int kbase, uint8_t* img, const int& wave) {
  long long b_off_k = b_off;
  if constexpr (FENCE) asm volatile("" : "+v"(b_off_k));
#pragma unroll
  for (int j = J0; j < J0 + JN; ++j) {
    const P src = (bn0 + 64 * j < N)
                      ? Bw + b_off_k + (long long)(64 * j) * Kdim + kbase
                      : zero_page;
    glds16(src, img + (wave * 64u + j * 512u) * 16u);
  }
}

// ---- glds stage of one 16 KiB A piece (2 instrs), plain-GEMM mode --------
// A is row-major [M][K]. row(i, off) gives instr i's element offset at k = 0
// and returns whether its row is below M; rows past M read the zero page
template <typename P, typename Row>
__device__ __forceinline__ void tile_stage_a(const P& A, const P& zero_page,
                                             const Row& row, int kbase,
                                             uint8_t* piece, const int& wave) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    long long off;
    const bool live = row(i, off);
    glds16(live ? A + off + kbase : zero_page,
           piece + (wave * 64u + i * 512u) * 16u);
  }
}

// ---- one K-tile of the main loop -----------------------------------------
// Raw s_barrier (guide §5: __syncthreads with glds in flight drains vmcnt(0)
// mid-tile). One drain + barrier per K-tile; the next tile's glds are issued
// between the MFMA clusters of buffer p, B image first, then A0, then A1:
//   BN 256: [B0 B1] q(0,0) [B2 B3]    q(0,1) [A0] q(1,0) [A1] q(1,1)
//   BN 320: [B0 B1] 3 frag [B2 B3 B4] 2 frag [A0] 3 frag [A1] 2 frag
//   BN 128: [B0 B1 A0] both fragments of mq=0 [A1] both fragments of mq=1
// The tile's glds were issued a whole K-tile ago, so the full drain is cheap,
// and the barrier AFTER it makes every wave's staging visible (a counted
// per-wave vmcnt cannot order OTHER waves' DMA against this wave's ds_reads).
// `more`: stage tile ktn into buffer 1-p? A runtime bool stages conditionally,
// std::true_type always (gemm_fp8.hip). Callables: stage_b(kt, p, J0, JN),
// stage_a(kt, p, pc), cluster(p, MQ, NF0, NFN).
template <int BN, typename More, typename StageB, typename StageA,
          typename Cluster>
__device__ __forceinline__ void tile_ktile(int p, int ktn, More more,
                                           const StageB& stage_b,
                                           const StageA& stage_a,
                                           const Cluster& cluster) {
  constexpr int NF = BN / 64;        // 16-column fragments per wave
  constexpr int NB = BN / 64;        // B glds instructions per K-tile
  constexpr int NFA = (NF + 1) / 2;  // fragments in the first N cluster
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if constexpr (BN == 128) {
    if (more) {
      stage_b(ktn, 1 - p, ic<0>{}, ic<NB>{});
      stage_a(ktn, 1 - p, 0);
    }
    cluster(p, ic<0>{}, ic<0>{}, ic<NF>{});
    if (more) stage_a(ktn, 1 - p, 1);
    cluster(p, ic<1>{}, ic<0>{}, ic<NF>{});
  } else {
    if (more) stage_b(ktn, 1 - p, ic<0>{}, ic<2>{});
    cluster(p, ic<0>{}, ic<0>{}, ic<NFA>{});
    if (more) stage_b(ktn, 1 - p, ic<2>{}, ic<NB - 2>{});
    cluster(p, ic<0>{}, ic<NFA>{}, ic<NF - NFA>{});
    if (more) stage_a(ktn, 1 - p, 0);
    cluster(p, ic<1>{}, ic<0>{}, ic<NFA>{});
    if (more) stage_a(ktn, 1 - p, 1);
    cluster(p, ic<1>{}, ic<NFA>{}, ic<NF - NFA>{});
  }
}
