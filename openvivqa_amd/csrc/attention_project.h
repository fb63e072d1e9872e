// The projection loop of the fused attention kernels of attention_mfma.hip (included by that file only): a small GEMM
// main loop  acc[j][i] += W[wr * NJ * 16 + j * 16 ..][k] . x[wc * NI * 16 + i * 16 ..][k]  like gemm_mfma.hip's --
// v_mfma_f32_16x16x32_bf16 on a direct-to-LDS ring of NBUF stages of BKF-deep K tiles, XOR-swizzled [rows][BKF] images --
// in ONE implementation: the geometry, the swizzle, the ring with its s_waitcnt counts and the MFMA order live here and
// nowhere else.  The kernels differ in the geometry (the template parameters) and in where their rows come from (the two
// callables of setup()); what each of them does around the loop, and in which order, stays with the kernel.  One
// exception: attn_qkv_fwd_mfma_kernel repeats setup()'s per-piece loop in its own body (it keeps its registers that way,
// see there) -- a change to how a lane's pieces map to rows and chunks has to be made in both.
#pragma once
#include "attention_frags.h"

namespace {

typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void gbl_void;

// NW waves stage, per K step, WROWS weight rows and XROWS x rows of BKF bf16 (BKF = 32 or 64) into stage kt % NBUF, in
// 1-KiB pieces (one global_load_lds of a wave); a wave multiplies NJ x NI units of 16 x 16: NW = (WROWS / (NJ * 16)) row
// slabs `wr` of the weights x (XROWS / (NI * 16)) row slabs `wc` of x.
template <int NJ, int NI, int BKF, int NBUF, int NW, int WROWS, int XROWS>
struct ProjLoop {
  static constexpr int PROWS = 1024 / (BKF * 2);                      // rows of a piece: 16 (64-B rows) or 8 (128-B rows)
  static constexpr int CHR = BKF / 8;                                 // 16-byte chunks per row: 4 or 8
  static constexpr int WCH = WROWS / PROWS, XCH = XROWS / PROWS;      // pieces of the W / x tiles
  static constexpr int PCS = WCH + XCH;                               // pieces per stage
  static constexpr int PER = (PCS + NW - 1) / NW;                     // per wave: PER pieces, the last one only for waves < FULL
  static constexpr int FULL = PCS - NW * (PER - 1);                   // waves with PER pieces
  static constexpr bool RAGGED = PCS % NW != 0;                       // (only then is the `full` path compiled)
  static constexpr int STAGE = PCS * 1024;                            // bytes of one stage: W pieces, then x pieces
  static constexpr int RING_BYTES = NBUF * STAGE;                     // what a launcher reserves for the loop
  static_assert(BKF == 32 || BKF == 64, "K steps of 32 or 64");
  static_assert(NBUF >= 2, "a ring has a stage in flight next to the one being read");
  static_assert(WROWS % PROWS == 0 && XROWS % PROWS == 0, "tiles are whole pieces");
  static_assert((WROWS / (NJ * 16)) * (XROWS / (NI * 16)) == NW, "the waves' units tile the stage exactly");

  // [rows][32] bf16 image, 64 B per row: chunk ch of row r sits in 16-byte slot ch ^ g((r >> 2) & 3), g = {0, 2, 3, 1}.
  // ds_read_b128 serves the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... (MI355X_MICROARCH.md, LDS): with
  // lane -> (row base + (lane & 15), chunk lane >> 4) a group holds rows {0-3, 12-15} of one chunk and rows {4-11} of
  // the next, and this g puts their 16 slots on 16 distinct 16-byte bank columns (the plain (r >> 2) & 3 is 2-way
  // conflicting: 1.5 M conflict cycles per launch).  A staging piece is 16 rows = 1 KiB; lane l of the loading wave
  // fills slot l & 3 of row l >> 2, i.e. fetches global chunk (l & 3) ^ g.
  // (128-byte rows, BKF = 64: the GEMM kernels' slot = chunk ^ (row & 7))
  static __device__ __forceinline__ int swz(int row) { return BKF == 32 ? (0x78 >> (2 * ((row >> 2) & 3))) & 3 : (row & 7); }
  // byte offset of 16-byte chunk `ch` of row `row` of a staged tile
  static __device__ __forceinline__ int off(int row, int ch) { return row * (BKF * 2) + ((ch ^ swz(row)) << 4); }

  const bf16* src[PER];  // this lane's source row (+ chunk) of each of its pieces, K offset 0

  static __device__ __forceinline__ void zero(f32x4 (&acc)[NJ][NI]) {
#pragma unroll
    for (int j = 0; j < NJ; j++)
#pragma unroll
      for (int i = 0; i < NI; i++) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // Zeroes the accumulators and takes the source pointers: wrow(row) / xrow(row) = global address of weight row / x row
  // `row` of the stage at K offset 0 (the caller's perm32, head offset and row clamping live in them).  Separate from
  // run() because some kernels request other loads in between, and where those go is measured.
  // (attn_qkv_fwd_mfma_kernel writes src[] with this code of its own: see there)
  template <typename WF, typename XF>
  __device__ __forceinline__ void setup(f32x4 (&acc)[NJ][NI], int wave, int lane, WF wrow, XF xrow) {
    zero(acc);
#pragma unroll
    for (int i = 0; i < PER; i++) {
      const int ci = wave + NW * i;
      const int prow = lane / CHR, pch = lane % CHR;
      if (ci < WCH) {
        const int row = ci * PROWS + prow;
        src[i] = wrow(row) + ((pch ^ swz(row)) << 3);
      } else {
        const int row = (ci - WCH) * PROWS + prow;
        src[i] = xrow(row) + ((pch ^ swz(row)) << 3);
      }
    }
  }

  __device__ __forceinline__ void issue(char* smem, int wave, bool full, int kt) const {
    char* buf = smem + (kt % NBUF) * STAGE;
#pragma unroll
    for (int i = 0; i < PER; i++) {
      if (RAGGED && i == PER - 1 && !full) break;
      __builtin_amdgcn_global_load_lds((gbl_void*)(src[i] + kt * BKF), (lds_void*)(buf + (wave + NW * i) * 1024), 16, 0, 0);
    }
  }

  // The ring over nkt K steps, staged at smem[0 .. RING_BYTES).  Ends without a barrier: the caller synchronises before
  // it reuses the ring's memory.
  __device__ __forceinline__ void run(f32x4 (&acc)[NJ][NI], char* smem, int wave, int lane, int wr, int wc, int nkt) const {
    const bool full = !RAGGED || wave < FULL;  // wave-uniform
#pragma unroll
    for (int p = 0; p < NBUF - 1; p++)
      if (p < nkt) issue(smem, wave, full, p);
    for (int kt = 0; kt < nkt; kt++) {
      // stage kt has landed once at most the loads of the NBUF - 2 younger stages are outstanding (in-order return)
      if (kt + NBUF - 2 >= nkt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      } else if (full) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER * (NBUF - 2)) : "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((PER - 1) * (NBUF - 2)) : "memory");
      }
      __builtin_amdgcn_s_barrier();
      if (kt + NBUF - 1 < nkt) issue(smem, wave, full, kt + NBUF - 1);
      const char* Ws = smem + (kt % NBUF) * STAGE;
      const char* Xs = Ws + WCH * 1024;
#pragma unroll
      for (int ks = 0; ks < BKF / 32; ks++) {
        bf16x8 pf[NJ], qf[NI];
#pragma unroll
        for (int j = 0; j < NJ; j++)
          pf[j] = *reinterpret_cast<const bf16x8*>(Ws + off(wr * (NJ * 16) + j * 16 + (lane & 15), ks * 4 + (lane >> 4)));
#pragma unroll
        for (int i = 0; i < NI; i++)
          qf[i] = *reinterpret_cast<const bf16x8*>(Xs + off(wc * (NI * 16) + i * 16 + (lane & 15), ks * 4 + (lane >> 4)));
#pragma unroll
        for (int j = 0; j < NJ; j++)
#pragma unroll
          for (int i = 0; i < NI; i++) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf[j], qf[i], acc[j][i], 0, 0, 0);
      }
    }
  }
};

// acc0 / acc1 (features f .. f+3 / f+4 .. f+7 of one row) + their bias values, rounded to the 8 bf16 a lane stores
__device__ __forceinline__ bf16x8 pack_bias8(const f32x4& a0, const f32x4& a1, const float4& c0, const float4& c1) {
  bf16x8 o8;
  o8[0] = (bf16)(a0[0] + c0.x); o8[1] = (bf16)(a0[1] + c0.y); o8[2] = (bf16)(a0[2] + c0.z); o8[3] = (bf16)(a0[3] + c0.w);
  o8[4] = (bf16)(a1[0] + c1.x); o8[5] = (bf16)(a1[1] + c1.y); o8[6] = (bf16)(a1[2] + c1.z); o8[7] = (bf16)(a1[3] + c1.w);
  return o8;
}

// The backward kernels' dO image (bf16 [rows][64], the layout of img_off) from the accumulators of a 2 x NI projection:
// the wave's rows row0 + i * 16 + (lane & 15), features col0 + (lane >> 4) * 8 ..+7; rows beyond nq are zero (p = 0 there
// anyway), rounded as the separate GEMM would have stored dO.
template <int NI>
__device__ __forceinline__ void store_do_image(char* Gs, const f32x4 (&acc)[2][NI], int row0, int col0, int nq, int lane) {
#pragma unroll
  for (int i = 0; i < NI; i++) {
    const int r = row0 + i * 16 + (lane & 15);
    const int col = col0 + (lane >> 4) * 8;
    bf16x8 o8;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      o8[e] = r < nq ? (bf16)acc[0][i][e] : (bf16)0.f;
      o8[4 + e] = r < nq ? (bf16)acc[1][i][e] : (bf16)0.f;
    }
    *reinterpret_cast<bf16x8*>(Gs + img_off(r, col >> 3)) = o8;
  }
}

}  // namespace
