// Fragment helpers shared by the LDS-resident (attention_mfma.hip) and streaming (attention_stream.hip) MFMA attention
// kernels: the swizzled [rows][D] bf16 image, the 32x32x16 operand fragments read from it, the accumulator row order,
// the packed hi / lo probability and the 4-element dropout multipliers.
// (What the backward kernels of both files share on top of these: attention_bwd_tile.h.)
#pragma once
#include "common.h"

namespace {

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
constexpr float LOG2E = 1.4426950408889634f;
// raw v_exp_f32: the arguments are <= ~0 (score minus row maximum / log-sum-exp), results in [0, 1]; the libm
// exp2f wraps the instruction in denormal-range fix-ups (~4 extra VALU ops per element of a VALU-bound softmax)
__device__ __forceinline__ float exp2_fast(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ int xs(int row) { return ((row >> 2) & 3) | (((row >> 1) & 1) << 2); }
// Head size D (64, 96 or 128 features): an image row holds D bf16 in a pitch of 128 B (D = 64) or 256 B (D = 96, 128: one
// full 64-bank row per image row; the 96-feature image leaves its last 4 chunk slots unused).  With the 256-B pitch the
// XOR pattern takes the row's parity as a fourth bit: the 16 rows of a ds_read_b128 lane group then land on 16 distinct
// 16-byte slots, and the 4 rows x 4 chunks x 2 halves of a transposing read cover the bank row exactly once -- both
// read kinds stay conflict free, as with the 128-B pitch (where parity selects the half of the bank row instead).
template <int D> struct Img {
  static constexpr int PITCH = D <= 64 ? 128 : 256;
  static constexpr int CH = D / 8;   // 16-byte chunks of a row
  static constexpr int KS = D / 16;  // k steps of a 32x32x16 product over the features
  static constexpr int DT = D / 32;  // 32-feature output tiles
  static __device__ __forceinline__ int sw(int row) { return D <= 64 ? xs(row) : (xs(row) | ((row & 1) << 3)); }
  // byte offset of 16-byte chunk `ch` of row `row`
  static __device__ __forceinline__ int off(int row, int ch) { return row * PITCH + ((ch ^ sw(row)) << 4); }
};
__device__ __forceinline__ int img_off(int row, int ch) { return Img<64>::off(row, ch); }

// k-contiguous 32-row operand fragment (A or B of 32x32x16): lane -> row base+(lane&31), k = 16*ks + 8*(lane>>5) + j
template <int D = 64>
__device__ __forceinline__ bf16x8 frag_rows(const char* img, int base, int ks, int lane) {
  return *reinterpret_cast<const bf16x8*>(img + Img<D>::off(base + (lane & 31), 2 * ks + (lane >> 5)));
}
// transposed operand fragment from a [k rows][64] image: lane -> column cbase+(lane&31),
// element j <-> k row  kbase + 8*(j>>2) + 4*(lane>>5) + (j&3)   (the order an accumulator tile has)
template <int D = 64>
__device__ __forceinline__ bf16x8 frag_tr(const char* img, int kbase, int cbase, int lane) {
  const int row = kbase + 4 * (lane >> 5) + ((lane >> 2) & 3);
  const int col = cbase + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  const int ch = col >> 3, sub = (col & 7) * 2;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(img + Img<D>::off(row, ch) + sub));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(img + Img<D>::off(row + 8, ch) + sub));
  bf16x8 f;
  f[0] = lo[0]; f[1] = lo[1]; f[2] = lo[2]; f[3] = lo[3];
  f[4] = hi[0]; f[5] = hi[1]; f[6] = hi[2]; f[7] = hi[3];
  return f;
}

__device__ __forceinline__ int acc_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// A probability as two bf16 in one 32-bit register: low half = bf16(p), high half = bf16(p - bf16(p)).
__device__ __forceinline__ float pack_hi_lo(float p) {
  const bf16 hb = (bf16)p;
  const bf16 lb = (bf16)(p - (float)hb);
  return __uint_as_float((uint32_t)__builtin_bit_cast(unsigned short, hb) |
                         ((uint32_t)__builtin_bit_cast(unsigned short, lb) << 16));
}
__device__ __forceinline__ bf16 packed_hi(float v) {
  return __builtin_bit_cast(bf16, (unsigned short)(__float_as_uint(v) & 0xffffu));
}
__device__ __forceinline__ bf16 packed_lo(float v) {
  return __builtin_bit_cast(bf16, (unsigned short)(__float_as_uint(v) >> 16));
}

// Dropout multipliers (keep / (1 - p) or 0) of the 4 consecutive flat elements idx .. idx+3: the run of keys a lane owns in
// one group of a 32x32 accumulator tile (acc_row(4*g4 + e) = key0 + e).  Same decisions as drop_keep(): element 2m / 2m+1
// takes the low / high 16 bits of the hash of pair m.  Two hashes when idx is even; an odd idx (odd n_k, odd row) straddles
// three pairs.
__device__ __forceinline__ void drop_mul4(const DropState& s, uint32_t idx, float (&m)[4]) {
  const uint32_t pr = idx >> 1;
  const uint32_t h0 = drop_pair_hash(s, pr), h1 = drop_pair_hash(s, pr + 1);
  uint32_t f[4];
  if ((idx & 1u) == 0) {
    f[0] = h0 & 0xFFFFu; f[1] = h0 >> 16; f[2] = h1 & 0xFFFFu; f[3] = h1 >> 16;
  } else {
    const uint32_t h2 = drop_pair_hash(s, pr + 2);
    f[0] = h0 >> 16; f[1] = h1 & 0xFFFFu; f[2] = h1 >> 16; f[3] = h2 & 0xFFFFu;
  }
#pragma unroll
  for (int e = 0; e < 4; e++) m[e] = f[e] >= s.thresh ? s.inv_keep : 0.f;
}

template <typename K>
int ensure_lds(K kernel, size_t bytes, const char* what) {
  if (bytes > 160 * 1024) {
    ovqa_set_error("%s: needs %zu B of LDS", what, bytes);
    return OVQA_ERR_UNSUPPORTED;
  }
  if (bytes > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) {
      ovqa_set_error("%s: hipFuncSetAttribute: %s", what, hipGetErrorString(e));
      return OVQA_ERR_LAUNCH;
    }
  }
  return OVQA_OK;
}

}  // namespace
