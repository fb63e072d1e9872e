// Single-query attention for autoregressive decoding (models/modules/attentions.py:314-327 with one new
// query per sequence, decoders.py:46-63, beam_search.py:41-62): o[r] = softmax(q[r] K[r / group]^T * scale + mask[r]) V[r / group].
//
//   * one WAVE per (row r, head h): no 32-query MFMA tile padded around a single query; K and V of the (sample, head)
//     are streamed exactly once per wave, 16 bytes per lane;
//   * the K / V caches are [rows_kv, Lmax, H*d] buffers written in place by the projection GEMMs (row stride Lmax * H*d):
//     nothing is concatenated; `n` keys are live;
//   * `group` consecutive query rows share one cache row (the beams of a sample attend to the SAME encoder positions:
//     the projected encoder K / V are kept once per sample, beam_search.py:19-34 would gather them into every beam);
//   * scores: 4 lanes per key (16 features each, two 16-byte loads), 16 keys per pass, fp32; softmax over LDS-resident
//     scores with DPP wave reductions; P.V: a lane owns a feature pair, the two half-waves take alternate keys.
// HBM-bound byte streaming (d = 64: 256 B per key and head), VALU arithmetic: the roofline is the cache bytes.
#include <stdlib.h>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int LMAX_KEYS = 512;  // keys of ONE window: a wave's scores for one query live in a fixed LDS slot (512 floats,
                                // 128 per wave in the split form); longer key lists are walked window by window
constexpr int MAX_KEYS = 1 << 30;  // key indices (and a window's end, j + 16 * 4 passes) are 32-bit ints
constexpr int DECODE_MAX_SPLITS = 32;  // slices of the key split across workgroups (a merge lane per slice; 2048 keys / 64)
// the automatic rule's constants (MEASURED at H = 8, d = 64, bf16, B in 1 .. 32: DESIGN section 18)
constexpr int AUTO_MIN_SLICE = 128;   // keys of a slice: shorter slices bought nothing (the split form's floor is two launches)
constexpr int AUTO_MAX_SPLITS = 16;   // 32 slices were slower than 16 in every cell
constexpr int AUTO_MIN_SPLITS = 4;    // 2 slices lose at 577 / 617 keys and win under 6 % at 1024
constexpr int AUTO_WGS_PER_CU = 1;    // workgroups per CU the split may reach: at 2 per CU, 128 problems of one query lost

template <typename T> struct Vec16;  // 16 bytes of T
template <> struct Vec16<bf16> { typedef bf16x8 type; static constexpr int N = 8; };
template <> struct Vec16<float> { typedef f32x4 type; static constexpr int N = 4; };

// G = query rows per wave: beams of a sample (G divides group, G <= 8: K and V of the sample's head are read ONCE for
// all of them; launch_decode picks it) or 1.  Scores: 4 lanes per key, 16 keys per pass; P.V: 16-byte chunks of a V row per lane, 64 / chunks
// keys per pass, partial sums of the key groups reduced with xor shuffles at the end.
// SPLIT = false: a wave owns a (row group, head) -- 4 independent problems per workgroup (short key lists: the
// self-attention prefix).  SPLIT = true: the 4 waves of a workgroup share ONE (row group, head) and take a quarter of the
// keys each (the 237 encoder positions: a lone wave streams its 60 KB at the latency of its own dependent round trips,
// 28 us measured; four waves and twice the workgroups cut the chain to a quarter), partial softmaxes merged through LDS
// (running maximum / sum, flash-decoding style).
// WIN = false: the wave's keys fit its LDS slot (n <= 512), one pass: scores, softmax, P.V.  WIN = true (n > 512): the
// wave walks its keys in windows of SLOT keys and carries a running maximum M, a running sum S and the UNNORMALISED
// output accumulators across them (online softmax): a window's numerators are taken against max(M, window maximum),
// and S and the accumulators are rescaled by exp(M_old - M_new) when the maximum rises (exp(-inf) = 0 before the first
// window).  Masks are additive and FINITE, so a window of masked keys has a finite maximum and never poisons M; a wave
// without keys runs no window and hands (-inf, 0, 0) to the merge.  The first V rows of window w + 1 are requested
// before the softmax of window w starts, as the first window's are requested next to its K rows: one round trip per
// window.  WIN is a separate instantiation so that the one-window form keeps its registers and its arithmetic.
// G = 5 .. 8 exist in the SPLIT form only (LDS: 4 waves x 8 queries x 128 floats = 16 KiB) and keep fewer loads in
// flight per lane (UK, UV below: batching of loads, not the order of any sum).
//
// The body is one function for two kernels.  attn_decode_kernel hands it all keys, [0, n), and gets o stored.
// attn_decode_part_kernel (PART = true, the SPLIT forms only) hands workgroup (problem, slice s) the keys [k_lo, k_hi) of
// slice s: the four waves take a quarter of the SLICE each and merge through LDS as above, and instead of dividing and
// storing o the workgroup writes its merged (M, S, unnormalised o[D]) as fp32 into record (row, head, s) of `ws` (layout at
// decode_split_workspace_bytes); attn_decode_merge_kernel, the next launch in the stream, merges the records.
template <typename T, int D, int G, bool SPLIT, bool WIN, bool PART>
__device__ __forceinline__ void attn_decode_body(const ovqa::AttnDecodeArgs& a, const int wg, const int k_lo, const int k_hi,
                                                 float* __restrict__ ws, const int slices, const int slice) {
  static_assert(G <= 4 || SPLIT, "more than 4 queries per wave: split form only");
  static_assert(!WIN || SPLIT, "past one window the four waves always share the problem");
  static_assert(!WIN || G <= 6, "windowed forms of 7 and 8 queries measured slower than the forms they would replace");
  static_assert(!PART || SPLIT, "a partial is what the four waves of a workgroup merged");
  constexpr int SLOT = SPLIT ? LMAX_KEYS / 4 : LMAX_KEYS;  // scores a wave keeps per query
  __shared__ float sc[4][G][SLOT];
  __shared__ float red_m[4][G], red_s[4][G];
  __shared__ float red_o[SPLIT ? 4 : 1][G][D];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wid = SPLIT ? wg : wg * 4 + wave;
  const int rows_g = a.R / G;
  const bool live = wid < rows_g * a.H;
  if (!SPLIT && !live) return;  // (whole waves; the non-split form has no workgroup barrier)
  const int rg = live ? wid / a.H : 0, h = live ? wid - rg * a.H : 0;
  const int r0 = rg * G;  // first query row
  // this wave's keys [j_lo, j_hi): everything, or a quarter rounded up to whole 16-key passes
  const int quarter = ((k_hi - k_lo + 3) / 4 + 15) & ~15;
  const int j_lo = SPLIT ? min(k_lo + wave * quarter, k_hi) : k_lo;
  const int j_hi = SPLIT ? min(j_lo + quarter, k_hi) : k_hi;
  const int64_t kvrow = (int64_t)(r0 / a.group) * a.kv_batch_stride;
  const T* kb = (const T*)a.k + kvrow + h * D;
  const T* vb = (const T*)a.v + kvrow + h * D;
  constexpr int PER = D / 4;                      // features per lane of a key's 4-lane group
  constexpr int NV = Vec16<T>::N, NL = PER / NV;  // 16-byte loads per lane and key
  static_assert(PER % NV == 0, "a lane's share of a key is a whole number of 16-byte loads");
  typedef typename Vec16<T>::type vec_t;
  const int part = lane & 3, kk = lane >> 2;
  float qf[G][PER];
#pragma unroll
  for (int g = 0; g < G; g++) {
    const T* q = (const T*)a.q + (int64_t)(r0 + g) * a.ldq + h * D;
#pragma unroll
    for (int l = 0; l < NL; l++) {
      const vec_t v = *reinterpret_cast<const vec_t*>(q + part * PER + l * NV);
#pragma unroll
      for (int e = 0; e < NV; e++) qf[g][l * NV + e] = to_f32<T>(v[e]) * a.scale;
    }
  }
  // ---- the first V rows this lane will need are requested NOW, next to the K rows: they do not depend on the scores, and
  // the wave's time is its chain of dependent memory round trips (K -> scores -> softmax -> V -> o was two of them + one
  // more per further 32 keys; a quarter of 237 keys is now ONE round trip for K and V together)
  constexpr int CH = D * (int)sizeof(T) / 16;  // 16-byte chunks per V row: 8 (bf16, d = 64)
  constexpr int KG = 64 / CH;                  // keys in flight per pass
  static_assert(CH >= 1 && CH <= 64 && 64 % CH == 0, "chunks per row divide the wave");
  const int c = lane % CH, kg = lane / CH;
  constexpr int UV = G > 4 ? 4 : 8;  // V rows in flight per lane
  vec_t vpre[UV];
#pragma unroll
  for (int u = 0; u < UV; u++)
    vpre[u] = *reinterpret_cast<const vec_t*>(vb + (int64_t)min(j_lo + kg + KG * u, max(j_hi - 1, 0)) * a.ldv + c * NV);
  float inv[G], wmax[G];
  float acc[G][NV];  // o = P V: lane -> 16-byte chunk c of key group kg
#pragma unroll
  for (int g = 0; g < G; g++) {
    wmax[g] = -INFINITY;  // (WIN: the running maximum and the running sum)
    inv[g] = 0.f;
#pragma unroll
    for (int e = 0; e < NV; e++) acc[g][e] = 0.f;
  }
  // ---- the wave's windows [w0, n) of its keys [j_lo, j_hi): exactly one when !WIN
  for (int w0 = j_lo; WIN ? w0 < j_hi : w0 == j_lo; w0 += SLOT) {
  const int n = WIN ? min(w0 + SLOT, j_hi) : j_hi;
  // ---- scores: 16 keys per pass, every key row loaded once for the G queries
  float mx[G];
#pragma unroll
  for (int g = 0; g < G; g++) mx[g] = -INFINITY;
  constexpr int UK = G > 4 ? 2 : 4;  // passes in flight: the loads of 64 keys are issued before the first dot product
  for (int j0 = w0; j0 < n; j0 += 16 * UK) {
    vec_t kv[UK][NL];
    float mk[UK][G];  // the additive mask of these keys: requested with the K rows, not one dependent load per use
#pragma unroll
    for (int u = 0; u < UK; u++) {
      const int j = min(j0 + 16 * u + kk, n - 1);  // (clamped: always a valid row; results beyond n are dropped)
      const T* kr = kb + (int64_t)j * a.ldk + part * PER;
#pragma unroll
      for (int l = 0; l < NL; l++) kv[u][l] = *reinterpret_cast<const vec_t*>(kr + l * NV);
#pragma unroll
      for (int g = 0; g < G; g++) mk[u][g] = a.mask ? a.mask[(int64_t)(r0 + g) * a.ldmask + j] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < UK; u++) {
      const int j = j0 + 16 * u + kk;
      float dot[G];
#pragma unroll
      for (int g = 0; g < G; g++) dot[g] = 0.f;
#pragma unroll
      for (int l = 0; l < NL; l++)
#pragma unroll
        for (int e = 0; e < NV; e++) {
          const float kf = to_f32<T>(kv[u][l][e]);
#pragma unroll
          for (int g = 0; g < G; g++) dot[g] = fmaf(qf[g][l * NV + e], kf, dot[g]);
        }
#pragma unroll
      for (int g = 0; g < G; g++) {
        dot[g] += __shfl_xor(dot[g], 1, 64);
        dot[g] += __shfl_xor(dot[g], 2, 64);
        if (j < n) {
          const float sv = dot[g] + mk[u][g];
          if (part == 0) sc[wave][g][j - w0] = sv;
          mx[g] = fmaxf(mx[g], sv);
        }
      }
    }
  }
  // (WIN) the first V rows of the NEXT window: on their way while this window's softmax and P.V run
  vec_t vnxt[WIN ? UV : 1];
  if constexpr (WIN) {
#pragma unroll
    for (int u = 0; u < UV; u++)
      vnxt[u] = *reinterpret_cast<const vec_t*>(vb + (int64_t)min(n + kg + KG * u, j_hi - 1) * a.ldv + c * NV);
  }
  // ---- softmax numerators (the wave's own LDS rows: written and read by this wave only)
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the score stores of every lane have landed
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int g = 0; g < G; g++) {
    float m = wave_max(mx[g]);
    float resc = 0.f;
    if constexpr (WIN) {  // against the running maximum; what was summed under the old one is scaled down to the new
      m = fmaxf(m, wmax[g]);
      resc = __expf(wmax[g] - m);  // (0 before the first window; 1 while the maximum stands)
    }
    float sum = 0.f;
    for (int j = w0 + lane; j < n; j += 64) {
      const float p = __expf(sc[wave][g][j - w0] - m);
      sc[wave][g][j - w0] = p;
      sum += p;
    }
    sum = wave_sum(sum);
    wmax[g] = m;
    if constexpr (WIN) {
      inv[g] = fmaf(inv[g], resc, sum);
#pragma unroll
      for (int e = 0; e < NV; e++) acc[g][e] *= resc;
    } else {
      inv[g] = SPLIT ? sum : 1.f / sum;  // (split: the row sum itself, merged below)
    }
  }
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_wave_barrier();
  // ---- o += P V
  if constexpr (!WIN) {
#pragma unroll
    for (int g = 0; g < G; g++)
#pragma unroll
      for (int e = 0; e < NV; e++) acc[g][e] = 0.f;
  }
  bool first = true;
  for (int j0 = w0 + kg; j0 < n; j0 += KG * UV, first = false) {
    vec_t vv[UV];
    if (first) {  // (the first trip's rows are already here)
#pragma unroll
      for (int u = 0; u < UV; u++) vv[u] = vpre[u];
    } else {
#pragma unroll
      for (int u = 0; u < UV; u++)
        vv[u] = *reinterpret_cast<const vec_t*>(vb + (int64_t)min(j0 + KG * u, n - 1) * a.ldv + c * NV);
    }
#pragma unroll
    for (int u = 0; u < UV; u++) {
      const int j = j0 + KG * u;
      if (j < n) {
#pragma unroll
        for (int g = 0; g < G; g++) {
          const float p = sc[wave][g][j - w0];
#pragma unroll
          for (int e = 0; e < NV; e++) acc[g][e] = fmaf(p, to_f32<T>(vv[u][e]), acc[g][e]);
        }
      }
    }
  }
  if constexpr (WIN) {
#pragma unroll
    for (int u = 0; u < UV; u++) vpre[u] = vnxt[u];
    __builtin_amdgcn_s_waitcnt(0xC07F);  // this window's numerators are read before the next window's scores land on them
    __builtin_amdgcn_wave_barrier();
  }
  }  // windows
#pragma unroll
  for (int g = 0; g < G; g++) {
#pragma unroll
    for (int e = 0; e < NV; e++) {
      float v = acc[g][e];
#pragma unroll
      for (int off = CH; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
      acc[g][e] = v;
    }
    if constexpr (!SPLIT) {
      if (kg == 0) {
        T* orow = (T*)a.o + (int64_t)(r0 + g) * a.ldo + h * D + c * NV;
        vec_t ov;
#pragma unroll
        for (int e = 0; e < NV; e++) ov[e] = from_f32<T>(acc[g][e] * inv[g]);
        *reinterpret_cast<vec_t*>(orow) = ov;
      }
    } else {
      if (kg == 0) {
#pragma unroll
        for (int e = 0; e < NV; e++) red_o[wave][g][c * NV + e] = acc[g][e];
      }
      if (lane == 0) {
        red_m[wave][g] = wmax[g];  // -inf for a wave without keys: its terms vanish in the merge
        red_s[wave][g] = inv[g];
      }
    }
  }
  if constexpr (SPLIT) {
    __syncthreads();
    for (int t = threadIdx.x; t < G * D; t += 256) {
      const int g = t / D, f = t - g * D;
      float M = red_m[0][g];
#pragma unroll
      for (int w = 1; w < 4; w++) M = fmaxf(M, red_m[w][g]);
      float S = 0.f, o = 0.f;
#pragma unroll
      for (int w = 0; w < 4; w++) {
        const float e = __expf(red_m[w][g] - M);  // exp(-inf) = 0: empty quarters drop out
        S = fmaf(red_s[w][g], e, S);
        o = fmaf(red_o[w][g][f], e, o);
      }
      if constexpr (PART) {  // the slice's record: what the four waves merged to, left unnormalised
        const int64_t rec = ((int64_t)(r0 + g) * a.H + h) * slices + slice;
        if (live) {
          ws[rec * D + f] = o;
          if (f == 0) {
            float* ms = ws + (int64_t)a.R * a.H * slices * D + 2 * rec;
            ms[0] = M;
            ms[1] = S;
          }
        }
      } else {
        if (live) ((T*)a.o)[(int64_t)(r0 + g) * a.ldo + h * D + f] = from_f32<T>(o / S);
      }
    }
  }
}

template <typename T, int D, int G, bool SPLIT, bool WIN>
__global__ __launch_bounds__(256) void attn_decode_kernel(ovqa::AttnDecodeArgs a) {
  attn_decode_body<T, D, G, SPLIT, WIN, false>(a, (int)blockIdx.x, 0, a.n, nullptr, 1, 0);
}

// ---- the key split ACROSS workgroups (small batches: 8 workgroups of B = 1, H = 8 leave 248 CUs idle and each wave walks
// its keys as a chain of round trips).  Two launches, ordered by the stream and by nothing else: no counters, no flags.
// Workgroup b of the first = (problem b / slices, slice b % slices), keys [slice * chunk, min(+ chunk, n)): never empty,
// a multiple of 64 keys from the start (decode_split_slices).  WIN: chunk > 512, a wave's quarter of a slice exceeds its LDS slot.
template <typename T, int D, int G, bool WIN>
__global__ __launch_bounds__(256) void attn_decode_part_kernel(ovqa::AttnDecodeArgs a, float* __restrict__ ws, int chunk,
                                                               int slices) {
  const int wg = (int)blockIdx.x / slices, slice = (int)blockIdx.x - wg * slices;
  const int k_lo = slice * chunk;
  attn_decode_body<T, D, G, true, WIN, true>(a, wg, k_lo, min(k_lo + chunk, a.n), ws, slices, slice);
}

// One wave per (row, head): M = max of the slices' maxima, every record scaled by exp(m_s - M) -- the formulas of the
// in-workgroup merge; a slice whose keys are all masked has a finite maximum near -1e5 and drops out by underflow -- then
// o / S stored with the caller's row stride.  Lane s holds slice s's (m, S) (slices <= 32); for o a lane owns a 16-byte
// chunk of a record and the wave's 64 / (D / 4) lane groups take alternate slices, 4 loads in flight per lane.  The order
// of every sum is fixed: same bits on every run.
template <typename T, int D>
__global__ __launch_bounds__(256) void attn_decode_merge_kernel(const float* __restrict__ ws, T* __restrict__ o, int64_t ldo,
                                                                int RH, int H, int slices) {
  const int lane = threadIdx.x & 63, p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= RH) return;  // (whole waves)
  const int r = p / H, h = p - r * H;
  const float* wo = ws + (int64_t)p * slices * D;
  const float* wms = ws + (int64_t)RH * slices * D + (int64_t)p * slices * 2;
  const float m = lane < slices ? wms[2 * lane] : -INFINITY;
  const float s = lane < slices ? wms[2 * lane + 1] : 0.f;
  const float M = wave_max(m);
  const float e = __expf(m - M);  // exp(-inf) = 0 for the lanes past the last slice
  const float S = wave_sum(s * e);
  constexpr int CH = D / 4, NG = 64 / CH, U = 4;
  const int c = lane % CH, sg = lane / CH;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int s0 = 0; s0 < slices; s0 += NG * U) {
    f32x4 part[U];
#pragma unroll
    for (int u = 0; u < U; u++)
      part[u] = *reinterpret_cast<const f32x4*>(wo + (int64_t)min(s0 + NG * u + sg, slices - 1) * D + c * 4);
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int sl = s0 + NG * u + sg;
      const float w = __shfl(e, min(sl, slices - 1), 64);
      if (sl < slices) {
#pragma unroll
        for (int i = 0; i < 4; i++) acc[i] = fmaf(part[u][i], w, acc[i]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    float v = acc[i];
#pragma unroll
    for (int off = CH; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
    acc[i] = v;
  }
  if (sg == 0) {
    T* orow = o + (int64_t)r * ldo + h * D + c * 4;
#pragma unroll
    for (int i = 0; i < 4; i++) orow[i] = from_f32<T>(acc[i] / S);
  }
}

// ---- the k best of every row (k <= 8): candidate selection of a beam-search step (beam_search.py:36-39 sorts all
// cur_beam * |V| candidates; any of the overall best `beam` is among the best `beam` of its own beam's |V| words).
// One wave per row: every lane keeps the best k of its strided share in registers (sorted, insertion), then k rounds
// of a wave-wide arg-max pop the winners.  Ties: the smaller index first.
template <int K>
__global__ __launch_bounds__(256) void topk_rows_kernel(const float* __restrict__ x, int64_t ldx, int R, int V,
                                                        float* __restrict__ vals, int64_t* __restrict__ idx) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const float* xr = x + (int64_t)row * ldx;
  float bv[K];
  int bi[K];
#pragma unroll
  for (int t = 0; t < K; t++) { bv[t] = -INFINITY; bi[t] = 0x7fffffff; }
  auto offer = [&](float v, int i) {
    // (a lane visits its indices in increasing order: '>' keeps the smaller index on ties; an empty slot takes anything)
    if (v > bv[K - 1] || bi[K - 1] == 0x7fffffff) {
#pragma unroll
      for (int t = 0; t < K; t++) {
        const bool take = v > bv[t] || bi[t] == 0x7fffffff;
        const float ov = bv[t];
        const int oi = bi[t];
        bv[t] = take ? v : ov;
        bi[t] = take ? i : oi;
        v = take ? ov : v;
        i = take ? oi : i;
      }
    }
  };
  // 16-byte loads, four of them in flight per lane (one load per step left the wave at the latency of ~60 round trips)
  const bool vec = (((uintptr_t)xr | (uintptr_t)(ldx * 4)) & 15) == 0;
  const int V4 = vec ? V / 4 : 0;
  for (int c0 = lane; c0 < V4; c0 += 64 * 4) {
    float4 q[4];
#pragma unroll
    for (int u = 0; u < 4; u++) q[u] = *reinterpret_cast<const float4*>(xr + 4 * min(c0 + 64 * u, V4 - 1));
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int c = c0 + 64 * u;
      if (c < V4) {
        offer(q[u].x, 4 * c); offer(q[u].y, 4 * c + 1); offer(q[u].z, 4 * c + 2); offer(q[u].w, 4 * c + 3);
      }
    }
  }
  for (int j = 4 * V4 + lane; j < V; j += 64) offer(xr[j], j);
#pragma unroll
  for (int t = 0; t < K; t++) {
    const float best = wave_max(bv[0]);
    // among the lanes that hold `best` at their head, the smallest index wins
    int cand = bv[0] == best ? bi[0] : 0x7fffffff;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) cand = min(cand, __shfl_xor(cand, off, 64));
    if (lane == 0) {
      vals[(int64_t)row * K + t] = best;
      idx[(int64_t)row * K + t] = cand;
    }
    if (bv[0] == best && bi[0] == cand) {  // pop the winner's head
#pragma unroll
      for (int u = 0; u < K - 1; u++) { bv[u] = bv[u + 1]; bi[u] = bi[u + 1]; }
      bv[K - 1] = -INFINITY;
      bi[K - 1] = 0x7fffffff;
    }
  }
}

}  // namespace

namespace ovqa {

int topk_rows(const float* x, int64_t ldx, int64_t R, int64_t V, int k, float* vals, int64_t* idx, hipStream_t st) {
  if (R == 0) return OVQA_OK;
  const dim3 grid((unsigned)((R + 3) / 4)), block(256);
#define OVQA_TK(KV) hipLaunchKernelGGL((topk_rows_kernel<KV>), grid, block, 0, st, x, ldx, (int)R, (int)V, vals, idx)
  switch (k) {
    case 1: OVQA_TK(1); break;
    case 2: OVQA_TK(2); break;
    case 3: OVQA_TK(3); break;
    case 4: OVQA_TK(4); break;
    case 5: OVQA_TK(5); break;
    case 6: OVQA_TK(6); break;
    case 7: OVQA_TK(7); break;
    default: OVQA_TK(8);
  }
#undef OVQA_TK
  return ovqa_check_launch("topk_rows");
}

bool attention_decode_supported(const AttnDecodeArgs& a, int esize) {
  const auto al = [&](const void* p) { return ((uintptr_t)p & 15) == 0; };
  return (a.d == 64 || a.d == 32 || a.d == 128) && a.n >= 1 && a.n <= MAX_KEYS && a.group >= 1 && al(a.q) && al(a.k) &&
         al(a.v) && (a.ldq * esize) % 16 == 0 && (a.ldk * esize) % 16 == 0 && (a.ldv * esize) % 4 == 0 &&
         (a.ldv * esize) % 16 == 0 && (a.kv_batch_stride * esize) % 16 == 0 && (a.ldo * esize) % 16 == 0 && al(a.o);
}

#define OVQA_DEC(SPLITV, WINV)                                                                          \
  do {                                                                                                  \
    OVQA_NOTE_LAUNCH((attn_decode_kernel<T, D, G, SPLITV, WINV>));                                      \
    hipLaunchKernelGGL((attn_decode_kernel<T, D, G, SPLITV, WINV>), grid, dim3(256), 0, st, a);         \
  } while (0)
template <typename T, int D, int G>
static void launch_form(bool split, bool win, dim3 grid, const AttnDecodeArgs& a, hipStream_t st) {
  if constexpr (G <= 4) {
    if (!split) {
      OVQA_DEC(false, false);
      return;
    }
  }
  if constexpr (G <= 6) {
    if (win) {
      OVQA_DEC(true, true);
      return;
    }
  }
  OVQA_DEC(true, false);
}
#undef OVQA_DEC

static int device_cus() {
  static int cus = -1;
  if (cus < 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      cus = 256;
  }
  return cus;
}

static int decode_group_max() {
  static int group_max = -1;
  if (group_max < 0) {
    const char* e = getenv("OVQA_DECODE_GROUP_MAX");  // (A/B: 4 = the forms before groups of 5 .. 8, 1 = no sharing)
    group_max = e ? atoi(e) : 8;
  }
  return group_max;
}

template <typename T, int D>
static int launch_decode(const AttnDecodeArgs& a, hipStream_t st) {
  static int split_min = -1;
  if (split_min < 0) {
    const char* e = getenv("OVQA_DECODE_SPLIT_MIN");
    split_min = e ? atoi(e) : 64;
  }
  const bool win = a.n > LMAX_KEYS;  // more keys than the waves' LDS slots: the windowed instantiation (split form only)
  const bool split = win || a.n >= split_min;  // long key lists: the four waves of a workgroup share one problem
  // G queries per wave: the beams of a sample share its K / V rows (group in 2 .. 8 and R a multiple of it): G is the
  // largest divisor of the group that has a form here, so that the G rows of a wave belong to one sample (group 8 past
  // 512 keys runs as two waves of 4).  The forms of 5 .. 8 queries (every choice MEASURED):
  //   * exist in the split form only (LDS), i.e. from OVQA_DECODE_SPLIT_MIN keys on;
  //   * are taken only where they still put two workgroups on every CU: a wave's time is its chain of round trips plus
  //     G dot products per key, so with CUs to spare more workgroups of fewer queries win (B = 32: 256 workgroups of 5
  //     lose to 1280 of 1, whose re-reads of a sample's rows hit in L2; B = 64 wins);
  //   * windowed (n > 512) stop at 6: 7 and 8 queries need every VGPR plus AGPR copies at one wave per SIMD and measured
  //     no faster than per-row reads (7) and slower than two waves of 4 (8).
  // Past 8 beams, or R not a multiple of the group, every row reads for itself.  Same bits whichever form runs.
  const int group_max = decode_group_max();
  int G = 1;
  if (a.group >= 2 && a.group <= 8 && a.R % a.group == 0) {
    // the largest divisor of the group that has a form: the G rows of a wave then belong to one sample
    for (int g = a.group; g > 1; g--) {
      if (a.group % g != 0 || g > group_max) continue;
      if (g > 4 && (!split || (int64_t)(a.R / g) * a.H < 2 * (int64_t)device_cus() || (win && g > 6))) continue;
      G = g;
      break;
    }
  }
  const int64_t problems = (int64_t)(a.R / G) * a.H;
  const dim3 grid((unsigned)(split ? problems : (problems + 3) / 4));
  switch (G) {
    case 2: launch_form<T, D, 2>(split, win, grid, a, st); break;
    case 3: launch_form<T, D, 3>(split, win, grid, a, st); break;
    case 4: launch_form<T, D, 4>(split, win, grid, a, st); break;
    case 5: launch_form<T, D, 5>(split, win, grid, a, st); break;
    case 6: launch_form<T, D, 6>(split, win, grid, a, st); break;
    case 7: launch_form<T, D, 7>(split, win, grid, a, st); break;
    case 8: launch_form<T, D, 8>(split, win, grid, a, st); break;
    default: launch_form<T, D, 1>(split, win, grid, a, st);
  }
  return ovqa_check_launch("attention_decode");
}

int attention_decode(int dtype, const AttnDecodeArgs& a, hipStream_t st) {
  if (a.R == 0 || a.H == 0) return OVQA_OK;
  if (dtype == OVQA_BF16) {
    switch (a.d) {
      case 32: return launch_decode<bf16, 32>(a, st);
      case 64: return launch_decode<bf16, 64>(a, st);
      default: return launch_decode<bf16, 128>(a, st);
    }
  }
  switch (a.d) {
    case 32: return launch_decode<float, 32>(a, st);
    case 64: return launch_decode<float, 64>(a, st);
    default: return launch_decode<float, 128>(a, st);
  }
}

// ---- the key split across workgroups -------------------------------------------------------------------------------------
// Slice plan: chunk = ceil(n / splits) rounded up to 64 keys, slices = ceil(n / chunk) <= splits; slice s = keys
// [s * chunk, min((s + 1) * chunk, n)): none empty, every start a multiple of 64.
int64_t decode_split_slices(int64_t n, int64_t splits, int64_t* chunk) {
  if (n < 1 || n > MAX_KEYS || splits < 1 || splits > DECODE_MAX_SPLITS) return -1;
  const int64_t c = ((n + splits - 1) / splits + 63) / 64 * 64;
  if (chunk) *chunk = c;
  return (n + c - 1) / c;
}

// Workspace: fp32, record (row r, head h, slice s) = (r * H + h) * slices + s.  The unnormalised o of every record first
// ([R * H * slices][d]: 16-byte aligned rows for the merge's loads), then its (M, S) pair ([R * H * slices][2]).
// splits = 0 (the automatic rule): the size of the most slices that rule can pick.
int64_t decode_split_workspace_bytes(int64_t R, int64_t H, int64_t n, int64_t d, int64_t splits) {
  const int64_t slices = decode_split_slices(n, splits == 0 ? DECODE_MAX_SPLITS : splits, nullptr);
  if (slices < 1 || R < 1 || H < 1 || d < 1) return -1;
  return (R * H * slices * (d + 2) * (int64_t)sizeof(float) + 15) / 16 * 16;
}

// Queries per wave of the part kernel: the largest divisor of the group that is at most 4 (the forms of 5 .. 8 need two
// workgroups per CU, which is never the small-batch case), or 1: group 5 and 7 read per row, 8 runs as two waves of 4.
static int part_group(const int64_t R, const int64_t group) {
  if (group < 2 || group > 8 || R % group != 0) return 1;
  for (int g = 4; g > 1; g--)
    if (group % g == 0 && g <= decode_group_max()) return g;
  return 1;
}

// The automatic rule.  Fixed by the code: 1 whenever the unsplit launch already fills the chip twice
// (launch_decode's own criterion), and never more than n / 64 (the slice plan).  Measured: see the constants.
int64_t decode_auto_splits(int64_t R, int64_t H, int64_t group, int64_t n, int64_t d, int dtype) {
  (void)d;
  (void)dtype;
  if (R < 1 || H < 1 || n < 1) return 1;
  const int64_t problems = R / part_group(R, group) * H, cus = device_cus();
  // up to one window (512 keys) a wave of the unsplit call has ONE round trip: with beams 1 and 5 the second launch costs
  // more than is saved; the beam-3 cells at 512 keys won 0.6 us and are left unsplit (one threshold for every beam count)
  if (problems >= 2 * cus || n <= LMAX_KEYS) return 1;
  int64_t s = AUTO_WGS_PER_CU * cus / problems;
  if (s > n / AUTO_MIN_SLICE) s = n / AUTO_MIN_SLICE;
  if (s > AUTO_MAX_SPLITS) s = AUTO_MAX_SPLITS;
  return s < AUTO_MIN_SPLITS ? 1 : s;
}

#define OVQA_PART(WINV)                                                                                              \
  do {                                                                                                               \
    OVQA_NOTE_LAUNCH((attn_decode_part_kernel<T, D, G, WINV>));                                                      \
    hipLaunchKernelGGL((attn_decode_part_kernel<T, D, G, WINV>), grid, dim3(256), 0, st, a, ws, chunk, slices);      \
  } while (0)
template <typename T, int D, int G>
static void launch_part(const AttnDecodeArgs& a, float* ws, int chunk, int slices, hipStream_t st) {
  const dim3 grid((unsigned)((int64_t)(a.R / G) * a.H * slices));
  if (chunk > LMAX_KEYS)  // a wave's quarter of a slice exceeds its LDS slot: the windowed instantiation
    OVQA_PART(true);
  else
    OVQA_PART(false);
}
#undef OVQA_PART

template <typename T, int D>
static int launch_split(const AttnDecodeArgs& a, float* ws, int chunk, int slices, hipStream_t st) {
  switch (part_group(a.R, a.group)) {
    case 2: launch_part<T, D, 2>(a, ws, chunk, slices, st); break;
    case 3: launch_part<T, D, 3>(a, ws, chunk, slices, st); break;
    case 4: launch_part<T, D, 4>(a, ws, chunk, slices, st); break;
    default: launch_part<T, D, 1>(a, ws, chunk, slices, st);
  }
  int rc = ovqa_check_launch("attention_decode_split (partials)");
  if (rc != OVQA_OK) return rc;
  const int RH = a.R * a.H;
  OVQA_NOTE_LAUNCH((attn_decode_merge_kernel<T, D>));
  hipLaunchKernelGGL((attn_decode_merge_kernel<T, D>), dim3((unsigned)((RH + 3) / 4)), dim3(256), 0, st,
                     (const float*)ws, (T*)a.o, a.ldo, RH, a.H, slices);
  return ovqa_check_launch("attention_decode_split (merge)");
}

int attention_decode_split(int dtype, const AttnDecodeArgs& a, int chunk, int slices, float* ws, hipStream_t st) {
  if (a.R == 0 || a.H == 0) return OVQA_OK;
  if (dtype == OVQA_BF16) {
    switch (a.d) {
      case 32: return launch_split<bf16, 32>(a, ws, chunk, slices, st);
      case 64: return launch_split<bf16, 64>(a, ws, chunk, slices, st);
      default: return launch_split<bf16, 128>(a, ws, chunk, slices, st);
    }
  }
  switch (a.d) {
    case 32: return launch_split<float, 32>(a, ws, chunk, slices, st);
    case 64: return launch_split<float, 64>(a, ws, chunk, slices, st);
    default: return launch_split<float, 128>(a, ws, chunk, slices, st);
  }
}

}  // namespace ovqa
