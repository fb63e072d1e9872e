// Pieces of a tile step of the MFMA attention backward shared by the LDS-resident kernels (attention_mfma.hip: the two-kernel
// form attn_bwd_dq / attn_bwd_dkv, the merged small-n_k form smallk_bwd_compute, the role-split form attn_bwd_roles) and the
// streaming ones (attention_stream.hip).  Every one of them works on 32 x 32 tiles in one or both of two orientations:
//   transposed (lane = query):  S^T, dP^T -> dS^T = P^T (dP^T keep/(1-p) - delta_q) -> dQ^T += K^T dS^T
//   direct     (lane = key):    S, dP -> P, dS = P (dP keep/(1-p) - delta_row)      -> dV^T += dO^T P~, dK^T += Q^T dS
// and ends with the store of transposed accumulators below.  The steps in between are still written out per kernel:
// profiles/README.md ("One tile step for the attention backward kernels") has the register and scratch figures of the
// attempt to share them.
//
// The probability is recomputed in one of two forms, and the two stay two:
//   log2 units     p = exp2(s * scale2 + (m - lse)),  scale2 = scale * log2 e, with the mask row and lse staged in LDS already
//                  multiplied by log2 e: smallk_bwd_compute and attn_bwd_roles_mfma_kernel (D = 64, no dropout), latency
//                  chains that count instructions -- one fma and one exp2 per element;
//   natural units  p = exp2((s * scale + m - lse) * log2 e): attn_bwd_dq / attn_bwd_dkv_mfma_kernel and the streaming
//                  kernels, which read mask and lse as the forward stored them.
// Under -ffp-contract=fast the first is one fma onto an already rounded (m - lse) * log2 e, the second an fma, a subtraction
// and a multiplication: the arguments of exp2 differ in their last bits, so merging the forms would change dQ / dK / dV of
// whichever kernels gave theirs up.
#pragma once
#include "attention_frags.h"

namespace {

// Store of transposed accumulators (lane = output row, registers = features, in acc_row order): 32 features at `row`
__device__ __forceinline__ void store_acc_tile(bf16* row, const f32x16& acc, float mul, int lane) {
#pragma unroll
  for (int g4 = 0; g4 < 4; g4++) {
    bf16x4 o4;
#pragma unroll
    for (int e = 0; e < 4; e++) o4[e] = (bf16)(acc[4 * g4 + e] * mul);
    *reinterpret_cast<bf16x4*>(row + 8 * g4 + 4 * (lane >> 5)) = o4;
  }
}
// the D features of a row: dQ (mul = scale)
template <int D>
__device__ __forceinline__ void store_acc_rows(bf16* row, const f32x16 (&acc)[Img<D>::DT], float mul, int lane) {
#pragma unroll
  for (int d = 0; d < Img<D>::DT; d++) store_acc_tile(row + d * 32, acc[d], mul, lane);
}
// dK (times mulk) and dV rows in one loop: the two store streams interleave
template <int D>
__device__ __forceinline__ void store_acc_rows(bf16* dkrow, const f32x16 (&dkt)[Img<D>::DT], float mulk, bf16* dvrow,
                                               const f32x16 (&dvt)[Img<D>::DT], int lane) {
#pragma unroll
  for (int d = 0; d < Img<D>::DT; d++)
#pragma unroll
    for (int g4 = 0; g4 < 4; g4++) {
      bf16x4 k4, v4;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        k4[e] = (bf16)(dkt[d][4 * g4 + e] * mulk);
        v4[e] = (bf16)dvt[d][4 * g4 + e];
      }
      *reinterpret_cast<bf16x4*>(dkrow + d * 32 + 8 * g4 + 4 * (lane >> 5)) = k4;
      *reinterpret_cast<bf16x4*>(dvrow + d * 32 + 8 * g4 + 4 * (lane >> 5)) = v4;
    }
}

}  // namespace
