// Streaming MFMA attention for gfx950 (bf16 storage, fp32 softmax), d_k = d_v in {64, 96, 128}, any sequence length: the
// shapes the LDS-resident kernels of attention_mfma.hip cannot hold (n_k, or n_q in the backward, above 256 / 192).
//
// Same operand layout as attn_fwd_mfma_kernel: S^T = K Q^T on v_mfma_f32_32x32x16_bf16, so a lane owns ONE query and the
// running max / sum of the online softmax are per-lane scalars plus one lane ^ 32 shuffle; P^T stays in registers as the B
// operand of O^T = V^T P^T, V^T comes through ds_read_b64_tr_b16 from the swizzled image (Img<D>).  What changes is that
// the other side is streamed: a workgroup (4 waves, 128 rows of its own side, one (batch, head)) walks the other side in
// tiles of KT = 64 rows through a two-stage LDS ring.  The global loads of tile t + 1 are issued into registers before the
// MFMAs of tile t and written to the free stage after them, so one barrier per tile separates the stages.  The wave's own
// operand fragments (Q, dO; K, V in the dK / dV kernel) are read once from global memory into registers.
//
// LDS per workgroup: two stages of two [64][D] images + 512 B of side values = 33 KiB (D = 64) / 65 KiB (D = 96, 128),
// so at least two workgroups fit a CU's 160 KiB.
//
// Backward (FlashAttention-2 form, with the forward's lse and delta = dO . (o + o_lo) as in attention_mfma.hip):
//   attn_stream_bwd_dq_kernel  -- owns 128 queries, streams K | V tiles: dQ^T += K^T dS^T; writes delta first.
//   attn_stream_bwd_dkv_kernel -- owns 128 keys, streams Q | dO tiles (+ lse, delta): dV^T += dO^T P~, dK^T += Q^T dS.
// Every output element is written by exactly one lane and accumulated in a fixed order: no atomics, results are
// bit-identical from run to run.
#include "common.h"
#include "kernels.h"
#include "attention_frags.h"
#include "attention_bwd_tile.h"

namespace {

constexpr int KT = 64;   // rows of one streamed tile (two 32-row MFMA sub-tiles)
constexpr int QB = 128;  // rows of its own side a workgroup owns: 4 waves x 32

template <int D> struct Ring {
  static constexpr int IMG = KT * Img<D>::PITCH;  // one [KT][D] image
  static constexpr int SIDE = 2 * KT * 4;         // fp32 side values of a tile: mask row, or lse | delta
  static constexpr int STAGE = 2 * IMG + SIDE;
  static constexpr int BYTES = 2 * STAGE;
  static constexpr int PER = KT * Img<D>::CH / 256;  // 16-byte loads per thread per image and tile (2, 3 or 4)
};

// Rows r0 .. r0 + KT - 1 of two row-major bf16 sources (beyond `rows`: zeros) into registers; NI = 1: the first only.
template <int D, int NI>
__device__ __forceinline__ void tile_fetch(uint4 (&v)[2 * Ring<D>::PER], const bf16* s0, int64_t ld0, const bf16* s1,
                                           int64_t ld1, int r0, int rows, int tid) {
  constexpr int CH = Img<D>::CH, PER = Ring<D>::PER;
#pragma unroll
  for (int u = 0; u < NI * PER; u++) {
    const int e = tid + (u % PER) * 256;
    const int row = e / CH, ch = e % CH;
    v[u] = make_uint4(0u, 0u, 0u, 0u);
    if (r0 + row < rows) {
      const bf16* src = u < PER ? s0 + (int64_t)(r0 + row) * ld0 : s1 + (int64_t)(r0 + row) * ld1;
      v[u] = *reinterpret_cast<const uint4*>(src + ch * 8);
    }
  }
}
template <int D, int NI>
__device__ __forceinline__ void tile_store(const uint4 (&v)[2 * Ring<D>::PER], char* stage, int tid) {
  constexpr int CH = Img<D>::CH, PER = Ring<D>::PER;
#pragma unroll
  for (int u = 0; u < NI * PER; u++) {
    const int e = tid + (u % PER) * 256;
    *reinterpret_cast<uint4*>(stage + (u < PER ? 0 : Ring<D>::IMG) + Img<D>::off(e / CH, e % CH)) = v[u];
  }
}

// The streaming loop shared by the kernels: stage tile 0, then per tile t fetch t + 1 into registers, run `body` on
// stage t & 1, store t + 1 into the other stage, barrier.  `side(t, tid)` returns the fp32 side value thread tid (< 2 KT)
// stages with tile t (threads >= 2 KT: ignored).  All waves run the loop (idle waves keep the barriers company).
template <int D, int NI, typename Side, typename Body>
__device__ __forceinline__ void stream_tiles(char* smem, const bf16* s0, int64_t ld0, const bf16* s1, int64_t ld1,
                                             int rows, int tid, Side side, Body body) {
  const int ntile = (rows + KT - 1) / KT;
  uint4 v[2 * Ring<D>::PER];
  float sv = 0.f;
  tile_fetch<D, NI>(v, s0, ld0, s1, ld1, 0, rows, tid);
  if (tid < 2 * KT) sv = side(0, tid);
  tile_store<D, NI>(v, smem, tid);
  if (tid < 2 * KT) reinterpret_cast<float*>(smem + 2 * Ring<D>::IMG)[tid] = sv;
  __syncthreads();
  for (int t = 0; t < ntile; t++) {
    const bool more = t + 1 < ntile;
    if (more) {
      tile_fetch<D, NI>(v, s0, ld0, s1, ld1, (t + 1) * KT, rows, tid);
      if (tid < 2 * KT) sv = side(t + 1, tid);
    }
    body(t, (const char*)(smem + (t & 1) * Ring<D>::STAGE));
    if (more) {
      char* nx = smem + ((t + 1) & 1) * Ring<D>::STAGE;
      tile_store<D, NI>(v, nx, tid);
      if (tid < 2 * KT) reinterpret_cast<float*>(nx + 2 * Ring<D>::IMG)[tid] = sv;
    }
    __syncthreads();
  }
}

// 32-row k-contiguous operand fragment straight from global memory (row `row`, head column base already applied)
template <int D>
__device__ __forceinline__ bf16x8 frag_global(const bf16* rowp, int ks, int lane) {
  return *reinterpret_cast<const bf16x8*>(rowp + 16 * ks + 8 * (lane >> 5));
}

// ------------------------------------------------------------------------------------------ forward
// grid (B*H, ceil(n_q / 128)); wave w: queries 128 blockIdx.y + 32 w ...  ROWMASK: the mask is one row per (b, h)
// (msq == 0, or none), staged per tile as a side value (-inf beyond n_k) and combined with the prefix-LM corner (a.tail);
// otherwise per-element reads of the mask row of the query.  DROP as attn_fwd_mfma_kernel: max, sum and lse are those of
// the undropped P, the P.V operand is p keep / (1 - p).  a.att: a second sweep over the K tiles writes P~ under the final
// max and sum.  Online softmax with a running max m: a tile raises m to m', the accumulators and the running sum are
// scaled by exp(m - m'); while no finite score has been seen the exponent base is 0 (no inf - inf), and a row that
// ends with m = -inf (every key masked with -inf) gives NaN o / lse / att, as the LDS-resident kernel does.
template <int D, bool ROWMASK, bool DROP>
__global__ __launch_bounds__(256) void attn_stream_fwd_kernel(ovqa::AttnArgs a) {
  constexpr int KS = Img<D>::KS, DT = Img<D>::DT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nk = a.nk, nq = a.nq;
  const int pid = blockIdx.x, b = pid / a.H, h = pid % a.H;
  const int q0 = blockIdx.y * QB + wave * 32;
  const bool active = q0 < nq;  // wave-uniform
  const int q = q0 + (lane & 31);
  const bool qok = q < nq;
  const int qc = qok ? q : nq - 1;
  const float* mbase = a.mask ? a.mask + (int64_t)b * a.msb + (int64_t)h * a.msh : nullptr;
  const float* mrow = mbase ? mbase + (int64_t)qc * a.msq : nullptr;
  const bf16* kg = (const bf16*)a.k + (int64_t)b * nk * a.ldk + h * D;
  const bf16* vg = (const bf16*)a.v + (int64_t)b * nk * a.ldv + h * D;
  const bool want_lo = a.o_lo != nullptr;
  DropState dst{};
  uint32_t rbase = 0;
  if constexpr (DROP) {
    dst = drop_init(a.drop);
    rbase = (uint32_t)((((int64_t)b * a.H + h) * nq + qc) * nk);
  }

  bf16x8 qf[KS];
  {
    const bf16* qrow = (const bf16*)a.q + ((int64_t)b * nq + qc) * a.ldq + h * D;
#pragma unroll
    for (int ks = 0; ks < KS; ks++) qf[ks] = frag_global<D>(qrow, ks, lane);
  }
  auto mask_side = [&](int t, int i) -> float {  // key-row mask value of key t KT + i (i < KT; the rest unused)
    const int j = t * KT + i;
    return j < nk ? (mbase ? mbase[j] : 0.f) : -INFINITY;
  };
  // S^T tile (2 x 32 keys) -> scaled, masked scores in st
  auto scores = [&](int t, const char* stg, f32x16 (&st)[2]) {
    const float* ml = reinterpret_cast<const float*>(stg + 2 * Ring<D>::IMG);
#pragma unroll
    for (int sub = 0; sub < 2; sub++) {
#pragma unroll
      for (int r = 0; r < 16; r++) st[sub][r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ks++)
        st[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<D>(stg, sub * 32, ks, lane), qf[ks], st[sub], 0, 0, 0);
#pragma unroll
      for (int g4 = 0; g4 < 4; g4++) {
        const int i0 = sub * 32 + 8 * g4 + 4 * (lane >> 5), key0 = t * KT + i0;
        if constexpr (ROWMASK) {
          const float4 m4 = *reinterpret_cast<const float4*>(ml + i0);
          const float mm[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
          for (int e = 0; e < 4; e++) {
            float sv = st[sub][4 * g4 + e] * a.scale + mm[e];
            if (a.tail && key0 + e > q && q >= nq - a.tail) sv = -INFINITY;  // prefix-LM corner (see attn_fwd_core)
            st[sub][4 * g4 + e] = sv;
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; e++) {
            const int key = key0 + e;
            st[sub][4 * g4 + e] = key < nk ? st[sub][4 * g4 + e] * a.scale + (mrow ? mrow[key] : 0.f) : -INFINITY;
          }
        }
      }
    }
  };

  float m = -INFINITY, l = 0.f;
  f32x16 acc[DT];
#pragma unroll
  for (int d = 0; d < DT; d++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[d][r] = 0.f;

  stream_tiles<D, 2>(smem, kg, a.ldk, vg, a.ldv, nk, tid, [&](int t, int i) { return ROWMASK && i < KT ? mask_side(t, i) : 0.f; },
                     [&](int t, const char* stg) {
    if (!active) return;
    f32x16 st[2];
    scores(t, stg, st);
    float mt = -INFINITY;
#pragma unroll
    for (int sub = 0; sub < 2; sub++)
#pragma unroll
      for (int r = 0; r < 16; r++) mt = fmaxf(mt, st[sub][r]);
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const float mn = fmaxf(m, mt);
    const float mu = mn == -INFINITY ? 0.f : mn;
    const float alpha = exp2_fast((m - mu) * LOG2E);  // m = -inf: 0
    m = mn;
    l *= alpha;
#pragma unroll
    for (int d = 0; d < DT; d++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[d][r] *= alpha;
#pragma unroll
    for (int sub = 0; sub < 2; sub++)
#pragma unroll
      for (int g4 = 0; g4 < 4; g4++) {
        float dm[4] = {1.f, 1.f, 1.f, 1.f};
        if constexpr (DROP) {
          const int key0 = t * KT + sub * 32 + 8 * g4 + 4 * (lane >> 5);
          dm[0] = dm[1] = dm[2] = dm[3] = 0.f;
          if (qok && key0 < nk) drop_mul4(dst, rbase + (uint32_t)key0, dm);
        }
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const float p = exp2_fast((st[sub][4 * g4 + e] - mu) * LOG2E);
          l += p;
          st[sub][4 * g4 + e] = pack_hi_lo(DROP ? p * dm[e] : p);
        }
      }
    // O^T += V^T P^T (hi halves; training: the lo halves into the same fp32 accumulators, o + o_lo = P V to ~16 bits)
#pragma unroll
    for (int sub = 0; sub < 2; sub++)
#pragma unroll
      for (int s = 0; s < 2; s++) {
        bf16x8 pb;
#pragma unroll
        for (int j = 0; j < 8; j++) pb[j] = packed_hi(st[sub][8 * s + j]);
#pragma unroll
        for (int d = 0; d < DT; d++)
          acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr<D>(stg + Ring<D>::IMG, sub * 32 + 16 * s, d * 32, lane), pb,
                                                           acc[d], 0, 0, 0);
        if (want_lo) {
#pragma unroll
          for (int j = 0; j < 8; j++) pb[j] = packed_lo(st[sub][8 * s + j]);
#pragma unroll
          for (int d = 0; d < DT; d++)
            acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr<D>(stg + Ring<D>::IMG, sub * 32 + 16 * s, d * 32, lane),
                                                             pb, acc[d], 0, 0, 0);
        }
      }
  });

  float inv = 0.f;
  if (active) {
    l += __shfl_xor(l, 32, 64);
    const bool dead = m == -INFINITY;
    inv = dead ? NAN : 1.f / l;
    const float lse = dead ? NAN : m + __logf(l);
    if (qok && a.lse && lane < 32) a.lse[((int64_t)b * a.H + h) * nq + q] = lse;
    if (qok) {
      bf16* orow = (bf16*)a.o + ((int64_t)b * nq + q) * a.ldo + h * D;
      bf16* lrow = (bf16*)a.o_lo + ((int64_t)b * nq + q) * a.ldo + h * D;
#pragma unroll
      for (int d = 0; d < DT; d++)
#pragma unroll
        for (int g4 = 0; g4 < 4; g4++) {
          bf16x4 o4, l4;
#pragma unroll
          for (int e = 0; e < 4; e++) {
            const float of = acc[d][4 * g4 + e] * inv;
            o4[e] = (bf16)of;
            l4[e] = (bf16)(of - (float)o4[e]);
          }
          const int c = d * 32 + 8 * g4 + 4 * (lane >> 5);
          *reinterpret_cast<bf16x4*>(orow + c) = o4;
          if (want_lo) *reinterpret_cast<bf16x4*>(lrow + c) = l4;
        }
    }
  }
  if (a.att == nullptr) return;  // launch-uniform
  // ---- second sweep: P~ = exp(s - m) / l keep / (1 - p) under the final max and sum (K tiles only).  Not exp(s - lse): an
  // lse near -1e5 (a row padded with the reference's -1e5) carries an absolute rounding of 2^-7, i.e. 2^-8 relative in P.
  stream_tiles<D, 1>(smem, kg, a.ldk, vg, a.ldv, nk, tid, [&](int t, int i) { return ROWMASK && i < KT ? mask_side(t, i) : 0.f; },
                     [&](int t, const char* stg) {
    if (!active) return;
    f32x16 st[2];
    scores(t, stg, st);
    if (!qok) return;
    bf16* arow = (bf16*)a.att + (((int64_t)b * a.H + h) * nq + q) * (int64_t)nk;
#pragma unroll
    for (int sub = 0; sub < 2; sub++)
#pragma unroll
      for (int g4 = 0; g4 < 4; g4++) {
        const int key0 = t * KT + sub * 32 + 8 * g4 + 4 * (lane >> 5);
        float dm[4] = {1.f, 1.f, 1.f, 1.f};
        if constexpr (DROP) {
          dm[0] = dm[1] = dm[2] = dm[3] = 0.f;
          if (key0 < nk) drop_mul4(dst, rbase + (uint32_t)key0, dm);
        }
#pragma unroll
        for (int e = 0; e < 4; e++)
          if (key0 + e < nk) arow[key0 + e] = (bf16)(exp2_fast((st[sub][4 * g4 + e] - m) * LOG2E) * inv * dm[e]);
      }
  });
}

// ------------------------------------------------------------------------------------------ backward
// dQ: grid (B*H, ceil(n_q / 128)), wave w owns 32 queries; per K | V tile (2 x 32 keys):
//   S^T = K Q^T, dP^T = V dO^T, P^T = exp(S^T scale + mask - lse), dS^T = P^T (dP^T keep / (1 - p) - delta),
//   dQ^T += K^T dS^T  (K^T through transposing reads of the staged K image).
// delta = dO . (o + o_lo) is computed here, stored for the dK / dV kernel (launched after this one).
template <int D, bool ROWMASK, bool DROP>
__global__ __launch_bounds__(256) void attn_stream_bwd_dq_kernel(ovqa::AttnBwdArgs a) {
  constexpr int KS = Img<D>::KS, DT = Img<D>::DT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nk = a.nk, nq = a.nq;
  const int pid = blockIdx.x, b = pid / a.H, h = pid % a.H;
  const int q0 = blockIdx.y * QB + wave * 32;
  const bool active = q0 < nq;
  const int q = q0 + (lane & 31);
  const bool qok = q < nq;
  const int qc = qok ? q : nq - 1;
  const float* mbase = a.mask ? a.mask + (int64_t)b * a.msb + (int64_t)h * a.msh : nullptr;
  const float* mrow = mbase ? mbase + (int64_t)qc * a.msq : nullptr;
  const bf16* kg = (const bf16*)a.k + (int64_t)b * nk * a.ldk + h * D;
  const bf16* vg = (const bf16*)a.v + (int64_t)b * nk * a.ldv + h * D;

  float delta = 0.f, lse = 0.f;
  bf16x8 qf[KS], gf[KS];
  if (active) {
    const bf16* gr = (const bf16*)a.d_o + ((int64_t)b * nq + qc) * a.lddo + h * D;
    const bf16* qr = (const bf16*)a.q + ((int64_t)b * nq + qc) * a.ldq + h * D;
#pragma unroll
    for (int ks = 0; ks < KS; ks++) {
      qf[ks] = frag_global<D>(qr, ks, lane);
      gf[ks] = frag_global<D>(gr, ks, lane);
    }
    // delta over this lane's half of the D features, combined with the partner half-wave (as attn_bwd_dq_mfma_kernel)
    const bf16* gh = gr + (D / 2) * (lane >> 5);
    const bf16* orow = (const bf16*)a.o + ((int64_t)b * nq + qc) * a.ldo + h * D + (D / 2) * (lane >> 5);
    const bf16* lrow = a.o_lo ? (const bf16*)a.o_lo + ((int64_t)b * nq + qc) * a.ldo + h * D + (D / 2) * (lane >> 5) : nullptr;
#pragma unroll
    for (int c = 0; c < D / 16; c++) {
      const bf16x8 g8 = *reinterpret_cast<const bf16x8*>(gh + 8 * c);
      const bf16x4 oa = *reinterpret_cast<const bf16x4*>(orow + 8 * c);
      const bf16x4 ob = *reinterpret_cast<const bf16x4*>(orow + 8 * c + 4);
#pragma unroll
      for (int e = 0; e < 4; e++) delta += (float)g8[e] * (float)oa[e] + (float)g8[4 + e] * (float)ob[e];
      if (lrow) {
        const bf16x4 la = *reinterpret_cast<const bf16x4*>(lrow + 8 * c);
        const bf16x4 lb = *reinterpret_cast<const bf16x4*>(lrow + 8 * c + 4);
#pragma unroll
        for (int e = 0; e < 4; e++) delta += (float)g8[e] * (float)la[e] + (float)g8[4 + e] * (float)lb[e];
      }
    }
    delta += __shfl_xor(delta, 32, 64);
    lse = a.lse[((int64_t)b * a.H + h) * nq + qc];
    if (qok && lane < 32) a.delta[((int64_t)b * a.H + h) * nq + q] = delta;
  }
  // prefix-LM corner (a.tail, key-row masks only): this lane's query sees no key > qlim (as attn_bwd_dq_mfma_kernel)
  const int qlim = (ROWMASK && a.tail && q >= nq - a.tail) ? q : 0x7fffffff;
  DropState dst{};
  uint32_t rbase = 0;
  if constexpr (DROP) {
    dst = drop_init(a.drop);
    rbase = (uint32_t)((((int64_t)b * a.H + h) * nq + qc) * nk);
  }
  f32x16 dqt[DT];
#pragma unroll
  for (int d = 0; d < DT; d++)
#pragma unroll
    for (int r = 0; r < 16; r++) dqt[d][r] = 0.f;

  stream_tiles<D, 2>(smem, kg, a.ldk, vg, a.ldv, nk, tid,
                     [&](int t, int i) {
                       const int j = t * KT + i;
                       return ROWMASK && i < KT ? (j < nk ? (mbase ? mbase[j] : 0.f) : -INFINITY) : 0.f;
                     },
                     [&](int t, const char* stg) {
    if (!active) return;
    const float* ml = reinterpret_cast<const float*>(stg + 2 * Ring<D>::IMG);
#pragma unroll
    for (int sub = 0; sub < 2; sub++) {
      f32x16 st, dp;
#pragma unroll
      for (int r = 0; r < 16; r++) { st[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
      for (int ks = 0; ks < KS; ks++) {
        st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<D>(stg, sub * 32, ks, lane), qf[ks], st, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<D>(stg + Ring<D>::IMG, sub * 32, ks, lane), gf[ks], dp, 0, 0, 0);
      }
      float ds[16];
#pragma unroll
      for (int g4 = 0; g4 < 4; g4++) {
        const int i0 = sub * 32 + 8 * g4 + 4 * (lane >> 5), key0 = t * KT + i0;
        float dm[4] = {1.f, 1.f, 1.f, 1.f};
        if constexpr (DROP) {
          dm[0] = dm[1] = dm[2] = dm[3] = 0.f;
          if (qok && key0 < nk) drop_mul4(dst, rbase + (uint32_t)key0, dm);
        }
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const int r = 4 * g4 + e, key = key0 + e;
          float p;
          if constexpr (ROWMASK) {
            p = key > qlim ? 0.f : exp2_fast((st[r] * a.scale + ml[i0 + e] - lse) * LOG2E);  // -inf beyond n_k -> 0
          } else {
            p = 0.f;
            if (key < nk) p = exp2_fast((st[r] * a.scale + (mrow ? mrow[key] : 0.f) - lse) * LOG2E);
          }
          ds[r] = p * ((DROP ? dp[r] * dm[e] : dp[r]) - delta);
        }
      }
#pragma unroll
      for (int s = 0; s < 2; s++) {
        bf16x8 db;
#pragma unroll
        for (int j = 0; j < 8; j++) db[j] = (bf16)ds[8 * s + j];
#pragma unroll
        for (int d = 0; d < DT; d++)
          dqt[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr<D>(stg, sub * 32 + 16 * s, d * 32, lane), db, dqt[d], 0, 0, 0);
      }
    }
  });
  if (active && qok) store_acc_rows<D>((bf16*)a.dq + ((int64_t)b * nq + q) * a.lddq + h * D, dqt, a.scale, lane);
}

// dK / dV: grid (B*H, ceil(n_k / 128)), wave w owns 32 keys (columns); per Q | dO tile (2 x 32 queries, with their lse and
// delta as side values: lse = +inf beyond n_q, so those rows give P = 0):
//   S = Q K^T, dP = dO V^T, P = exp(S scale + mask - lse), dS = P (dP keep / (1 - p) - delta),
//   dV^T += dO^T P~,  dK^T += Q^T dS  (dO^T / Q^T through transposing reads).
// DROP: a lane walks a key column, its 4 consecutive accumulator rows are queries n_k elements apart: each element hashes
// its own pair (as attn_bwd_dkv_mfma_kernel).
// TAIL (key-row masks only; the prefix-LM corner of a.tail): queries nq - tail <= qi < key do not see this lane's key, P is
// exactly 0 there (as exp2 of a dense mask's -inf), so nothing reaches dV or dS.  A compile-time form of its own,
// attn_stream_bwd_dkv_tail_kernel: as a run-time field the test cost attn_stream_bwd_dkv_kernel<128, true, *> 80 / 60 bytes
// of scratch per lane, and the calls without a tail keep the code they had.
template <int D, bool ROWMASK, bool DROP, bool TAIL>
__device__ __forceinline__ void stream_bwd_dkv_body(const ovqa::AttnBwdArgs& a) {
  static_assert(ROWMASK || !TAIL, "the prefix-LM corner goes with a key-row mask");
  constexpr int KS = Img<D>::KS, DT = Img<D>::DT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nk = a.nk, nq = a.nq;
  const int pid = blockIdx.x, b = pid / a.H, h = pid % a.H;
  const int k0 = blockIdx.y * QB + wave * 32;
  const bool active = k0 < nk;
  const int key = k0 + (lane & 31);
  const bool kok = key < nk;
  const int kc = kok ? key : nk - 1;
  const float* mcol = a.mask ? a.mask + (int64_t)b * a.msb + (int64_t)h * a.msh + kc : nullptr;
  const float mconst = (ROWMASK && mcol) ? mcol[0] : 0.f;
  const int qlo = TAIL ? nq - a.tail : nq;
  const int64_t prob = (int64_t)b * a.H + h;
  const bf16* qg = (const bf16*)a.q + (int64_t)b * nq * a.ldq + h * D;
  const bf16* gg = (const bf16*)a.d_o + (int64_t)b * nq * a.lddo + h * D;
  DropState dst{};
  uint32_t pbase = 0;  // element (qi, key) is pbase + qi * nk
  if constexpr (DROP) {
    dst = drop_init(a.drop);
    pbase = (uint32_t)(prob * nq * nk + kc);
  }
  bf16x8 kf[KS], vf[KS];
  {
    const bf16* kr = (const bf16*)a.k + ((int64_t)b * nk + kc) * a.ldk + h * D;
    const bf16* vr = (const bf16*)a.v + ((int64_t)b * nk + kc) * a.ldv + h * D;
#pragma unroll
    for (int ks = 0; ks < KS; ks++) {
      kf[ks] = frag_global<D>(kr, ks, lane);
      vf[ks] = frag_global<D>(vr, ks, lane);
    }
  }
  f32x16 dvt[DT], dkt[DT];
#pragma unroll
  for (int d = 0; d < DT; d++)
#pragma unroll
    for (int r = 0; r < 16; r++) { dvt[d][r] = 0.f; dkt[d][r] = 0.f; }

  stream_tiles<D, 2>(smem, qg, a.ldq, gg, a.lddo, nq, tid,
                     [&](int t, int i) {
                       const int j = t * KT + (i & (KT - 1));
                       if (i < KT) return j < nq ? a.lse[prob * nq + j] : INFINITY;
                       return j < nq ? a.delta[prob * nq + j] : 0.f;
                     },
                     [&](int t, const char* stg) {
    if (!active) return;
    const float* ls = reinterpret_cast<const float*>(stg + 2 * Ring<D>::IMG);
#pragma unroll
    for (int sub = 0; sub < 2; sub++) {
      f32x16 s_, dp;
#pragma unroll
      for (int r = 0; r < 16; r++) { s_[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
      for (int ks = 0; ks < KS; ks++) {
        s_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<D>(stg, sub * 32, ks, lane), kf[ks], s_, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<D>(stg + Ring<D>::IMG, sub * 32, ks, lane), vf[ks], dp, 0, 0, 0);
      }
      float p[16], ds[16];
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int li = sub * 32 + acc_row(r, lane), qi = t * KT + li;
        float mv = mconst;
        if constexpr (!ROWMASK) mv = (mcol && qi < nq) ? mcol[(int64_t)qi * a.msq] : 0.f;
        float pv = exp2_fast((s_[r] * a.scale + mv - ls[li]) * LOG2E);
        if constexpr (TAIL) pv = (qi >= qlo && qi < key) ? 0.f : pv;
        if constexpr (DROP) {
          const float mk = (qi < nq && kok && drop_keep(dst, pbase + (uint32_t)qi * (uint32_t)nk)) ? dst.inv_keep : 0.f;
          p[r] = pv * mk;
          ds[r] = pv * (dp[r] * mk - ls[KT + li]);
        } else {
          p[r] = pv;
          ds[r] = pv * (dp[r] - ls[KT + li]);
        }
      }
#pragma unroll
      for (int s = 0; s < 2; s++) {
        bf16x8 pb, db;
#pragma unroll
        for (int j = 0; j < 8; j++) { pb[j] = (bf16)p[8 * s + j]; db[j] = (bf16)ds[8 * s + j]; }
#pragma unroll
        for (int d = 0; d < DT; d++) {
          dvt[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr<D>(stg + Ring<D>::IMG, sub * 32 + 16 * s, d * 32, lane), pb,
                                                           dvt[d], 0, 0, 0);
          dkt[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr<D>(stg, sub * 32 + 16 * s, d * 32, lane), db, dkt[d], 0, 0, 0);
        }
      }
    }
  });
  if (active && kok)
    store_acc_rows<D>((bf16*)a.dk_ + ((int64_t)b * nk + key) * a.lddk + h * D, dkt, a.scale,
                      (bf16*)a.dv_ + ((int64_t)b * nk + key) * a.lddv + h * D, dvt, lane);
}

template <int D, bool ROWMASK, bool DROP>
__global__ __launch_bounds__(256) void attn_stream_bwd_dkv_kernel(ovqa::AttnBwdArgs a) {
  stream_bwd_dkv_body<D, ROWMASK, DROP, false>(a);
}
template <int D, bool DROP>
__global__ __launch_bounds__(256) void attn_stream_bwd_dkv_tail_kernel(ovqa::AttnBwdArgs a) {
  stream_bwd_dkv_body<D, true, DROP, true>(a);
}

// ------------------------------------------------------------------------------------------ launchers
template <int D, bool ROWMASK, bool DROP>
int launch_stream_fwd_t(const ovqa::AttnArgs& a, hipStream_t st) {
  constexpr size_t lds = Ring<D>::BYTES;
  int rc = ensure_lds(attn_stream_fwd_kernel<D, ROWMASK, DROP>, lds, "attention_fwd(mfma-stream)");
  if (rc != OVQA_OK) return rc;
  const dim3 grid((unsigned)((int64_t)a.B * a.H), (unsigned)((a.nq + QB - 1) / QB));
  OVQA_LAUNCH_TIMED((attn_stream_fwd_kernel<D, ROWMASK, DROP>), grid, dim3(256), lds, st, a);
  return ovqa_check_launch("attention_fwd(mfma-stream)");
}

template <int D>
int launch_stream_fwd(const ovqa::AttnArgs& a, hipStream_t st) {
  const bool rowmask = a.msq == 0, drop = a.drop.p > 0.f;
  if (rowmask) return drop ? launch_stream_fwd_t<D, true, true>(a, st) : launch_stream_fwd_t<D, true, false>(a, st);
  return drop ? launch_stream_fwd_t<D, false, true>(a, st) : launch_stream_fwd_t<D, false, false>(a, st);
}

template <int D, bool ROWMASK, bool DROP>
int launch_stream_bwd_t(const ovqa::AttnBwdArgs& a, hipStream_t st) {
  constexpr size_t lds = Ring<D>::BYTES;
  const unsigned nprob = (unsigned)((int64_t)a.B * a.H);
  int rc = ensure_lds(attn_stream_bwd_dq_kernel<D, ROWMASK, DROP>, lds, "attention_bwd(mfma-stream,dq)");
  if (rc != OVQA_OK) return rc;
  OVQA_LAUNCH_TIMED((attn_stream_bwd_dq_kernel<D, ROWMASK, DROP>), dim3(nprob, (unsigned)((a.nq + QB - 1) / QB)), dim3(256),
                    lds, st, a);
  rc = ovqa_check_launch("attention_bwd(mfma-stream,dq)");
  if (rc != OVQA_OK) return rc;
  const dim3 kgrid(nprob, (unsigned)((a.nk + QB - 1) / QB));
  if constexpr (ROWMASK) {
    if (a.tail > 0) {  // prefix-LM corner
      rc = ensure_lds(attn_stream_bwd_dkv_tail_kernel<D, DROP>, lds, "attention_bwd(mfma-stream,dkv)");
      if (rc != OVQA_OK) return rc;
      OVQA_LAUNCH_TIMED((attn_stream_bwd_dkv_tail_kernel<D, DROP>), kgrid, dim3(256), lds, st, a);
      return ovqa_check_launch("attention_bwd(mfma-stream,dkv)");
    }
  }
  rc = ensure_lds(attn_stream_bwd_dkv_kernel<D, ROWMASK, DROP>, lds, "attention_bwd(mfma-stream,dkv)");
  if (rc != OVQA_OK) return rc;
  OVQA_LAUNCH_TIMED((attn_stream_bwd_dkv_kernel<D, ROWMASK, DROP>), kgrid, dim3(256), lds, st, a);
  return ovqa_check_launch("attention_bwd(mfma-stream,dkv)");
}

template <int D>
int launch_stream_bwd(const ovqa::AttnBwdArgs& a, hipStream_t st) {
  const bool rowmask = a.msq == 0, drop = a.drop.p > 0.f;
  if (rowmask) return drop ? launch_stream_bwd_t<D, true, true>(a, st) : launch_stream_bwd_t<D, true, false>(a, st);
  return drop ? launch_stream_bwd_t<D, false, true>(a, st) : launch_stream_bwd_t<D, false, false>(a, st);
}

}  // namespace

namespace ovqa {

// The conditions of mfma_attention_supported / mfma_attention_bwd_supported without their length caps.
bool stream_attention_supported(const AttnArgs& a) {
  auto al = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  const bool d_ok = a.dk == a.dv && (a.dk == 64 || a.dk == 96 || a.dk == 128);
  return d_ok && a.nk >= 1 && a.nq >= 1 && a.ldq % 8 == 0 && a.ldk % 8 == 0 && a.ldv % 8 == 0 && a.ldo % 4 == 0 &&
         al(a.q) && al(a.k) && al(a.v) && (((uintptr_t)a.o & 7) == 0);
}

bool stream_attention_bwd_supported(const AttnBwdArgs& a) {
  auto al = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  auto al8 = [](const void* p) { return ((uintptr_t)p & 7) == 0; };
  const bool d_ok = a.dk == a.dv && (a.dk == 64 || a.dk == 96 || a.dk == 128);
  return a.d_att == nullptr && a.d_lse == nullptr && d_ok && a.nk >= 1 && a.nq >= 1 && a.ldq % 8 == 0 && a.ldk % 8 == 0 &&
         a.ldv % 8 == 0 && a.lddo % 8 == 0 && a.ldo % 4 == 0 && a.lddq % 4 == 0 && a.lddk % 4 == 0 && a.lddv % 4 == 0 &&
         al(a.q) && al(a.k) && al(a.v) && al(a.d_o) && al8(a.o) && al8(a.dq) && al8(a.dk_) && al8(a.dv_) && a.lse && a.delta;
}

int stream_attention_fwd(const AttnArgs& a, hipStream_t st) {
  if (a.dk == 96) return launch_stream_fwd<96>(a, st);
  if (a.dk == 128) return launch_stream_fwd<128>(a, st);
  return launch_stream_fwd<64>(a, st);
}

int stream_attention_bwd(const AttnBwdArgs& a, hipStream_t st) {
  if (a.dk == 96) return launch_stream_bwd<96>(a, st);
  if (a.dk == 128) return launch_stream_bwd<128>(a, st);
  return launch_stream_bwd<64>(a, st);
}

}  // namespace ovqa
