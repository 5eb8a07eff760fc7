// Fused conditional-GRU decoder (training scan + one-step) for gfx950.
//
// Implements the reference's gru_cond_layer step (nats.py:498-572; kernel
// rows K10-K16 in SURVEY §2.4) as five fused stages per timestep driven
// by a C++ time loop (no python in the scan):
//   1. GRU_2          — the encoder cell (gru_kernels.h): nats_gru_step_fwd,
//                       or nats_gru2_gemm_splitk + nats_gru2_step_pointwise
//                       when Hpad >= 1024
//   2. pstate GEMM    — h1 @ W_att (cond_small_gemm_bt, split-K partials
//                       summed by stages 3 and 4)
//   3. attention 1    — cond_attn_fwd_chunk, one WG per (batch row,
//                       s-chunk): e-scores + distraction-over-weights,
//                       chunk-local masked softmax statistics (online
//                       softmax), unnormalised partial weighted context
//   4. attention 2    — cond_attn_combine_gate: global softmax statistics,
//                       combined context + distraction gate over content
//                       vectors + acc_ctx update, normalised alphas +
//                       acc_alpha update
//   5. GRU_1          — 4-output-group MFMA ([h1|ctx] packed operand) +
//                       gates/mask: cond_gru1_step_fwd, or
//                       cond_gru1_gemm_splitk + cond_gru1_step_pointwise
//                       when K1 >= 2048 (one MFMA phase, one finish)
// Backward, per step in reverse: cond_gru1_bwd_pointwise (GRU_1 gates +
// dctx passthrough), cond_bwd_gemm_dual_gate (dh1 and the dctx GEMM with
// the gate backward in its epilogue), cond_attn_bwd_dalpha (one wave per
// (b, s) context row), cond_attn_bwd_fused (one WG per (b, s-chunk):
// softmax backward, tanh backward into dpctx/acc_alpha, column sums through
// LDS), cond_dh1_att_gemm, nats_gru_step_bwd_pointwise (GRU_2 gates) and
// cond_dh_carry_gemm_split. The recurrent GEMMs share row_gemm
// (gru_kernels.h).
// The backward pass is the exact reverse chain with the running-sum
// accumulators' (acc_ctx/acc_alpha) gradients threaded backwards
// (SURVEY §7 "hard parts" (ii)); weight gradients that factor over time
// (dU_1, dW_1, dW_att, dWc_att, dU_con, ...) are computed as single
// time-batched GEMMs in python from the per-step buffers saved here.
//
// Occupancy design: at dim 1000 an output-tile grid is only ngrpH=63
// workgroups (a quarter of the 256 CUs), so every per-step GEMM splits
// its K dimension across extra grid dimensions and the elementwise
// reductions chunk their serial axis, with fp32 partials summed by the
// NEXT kernel in the chain rather than an extra pass (gru1/gru2 split-K
// -> pointwise combine; pstate split-K -> inline sums in both attention
// passes; attention s-chunks -> per-chunk (max, sum) pairs and partial
// contexts combined by pass 2; dh_carry split-K -> next step's GRU_1
// pointwise sums the halves). Every per-step scratch buffer is fully
// overwritten with plain stores by its producer, so the steady-state loop
// launches no memsets and no scratch needs re-zeroing. The only float
// atomics left in the attention chain are the per-chunk adds into
// dpstate; dD_wei / dU_att / dc_att accumulate over the time loop in one
// slot per (b, chunk) block and are summed once after it.
//
// Round-2 fusions (each GPU-measured; negatives reverted in history):
// the dctx passthrough merged into the GRU_1 backward pointwise; the
// distraction-gate backward plus the dU_con/dW_con column reductions live
// in the dctx GEMM's epilogue; dh1 += dpstate @ W_att converts fp32
// A-fragments in-register; the attention kernels stage the combined
// pstate + attention vectors in LDS. The chunked attention forward and
// the one-pass attention backward replaced seven kernels by three
// ("Decoder attention fusion"). Ladder and profiles in
// profiles/README.md.

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <algorithm>

#include "common.h"
#include "gru_kernels.h"

namespace {

// ---------------- small GEMM: pstate = h1 @ W_att ----------------
// A = [32][ldK] bf16 (zero-padded), Bt = [Npad][ldK] bf16. Split-K over
// grid.z into Cpart [KS][32][N] f32 partials (the unsplit version was 14
// waves on the whole chip, 11.3us of pure load latency): consumers
// (cond_attn_fwd_chunk inline, cond_attn_combine_gate for the saved
// pstate_all) sum the KS partials.
__global__ void cond_small_gemm_bt(const bf16_t* __restrict__ A,
                                   const bf16_t* __restrict__ Bt,
                                   float* __restrict__ Cpart, int B, int N,
                                   int ldK, int Kpad) {
  const int m0 = blockIdx.x * 16;
  const int n0 = blockIdx.y * 16;
  const KRange k = k_part(KRange{0, Kpad}, gridDim.z, blockIdx.z);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  // NB: Bt's row stride is Kpad (the packed weight width), NOT ldK.
  NATS_MFMA_KLOOP(acc, A, m0, ldK, Bt, n0, Kpad, k.beg, k.end);
  const int lane = threadIdx.x & (NATS_WAVE - 1);
  const int col = n0 + (lane & 15);
  const int rbase = m0 + (lane >> 4) * 4;
  if (col >= N) return;
  float* C = Cpart + (long)blockIdx.z * 32 * N;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = rbase + i;
    if (row < B) C[(long)row * N + col] = acc[i];
  }
}

// ---------------- attention: chunking of the source axis ----------------
// The forward and backward attention kernels run one 256-thread block per
// (batch row, contiguous s-chunk). A chunk holds at most ATT_CH_MAX source
// positions (the LDS tiles are sized for it).
constexpr int ATT_CH_MAX = 64;
constexpr int ATT_THREADS = 256;

// Chunk length: about one block per CU (256 of them) — B * Ts / 256
// positions per block — but never more than ATT_CH_MAX (the per-chunk
// partials stay ~3 % of the context traffic at 64) and never fewer than
// 16 (below that the [B][NCH][C] partials cost more than the context rows
// they summarise), rounded up to a multiple of 8. CNN/DM (B 20, Ts 801):
// 64 -> 13 chunks, 260 blocks; LCSTS (Ts 121) and one-step decode at a
// short source: 16 -> 8 chunks per row.
static inline int attn_chunk_len(int B, int Ts) {
  const long per = ((long)B * Ts + 255) / 256;
  const int ch = (int)std::min<long>(ATT_CH_MAX, std::max<long>(16, per));
  return (ch + 7) & ~7;
}

// Lanes that share one source position in the per-(s, i) loops: the
// largest power of two in [4, 16] that still gives every position of a
// chunk its own lane group (chunk 64 -> 4, 32 -> 8, 16 -> 16).
static inline int attn_lanes_per_s(int CH) {
  int lps = 4;
  while (lps < 16 && CH * lps * 2 <= ATT_THREADS) lps *= 2;
  return lps;
}

// Stage the combined pstate (sum of the split-K partials, or the saved
// combined row when PS_KS == 1 and ld == A) and the two attention vectors
// in LDS: [A] ps | [A] Dwei | [A] Uatt. Caller barriers.
__device__ __forceinline__ void attn_stage_vectors(
    float* sm, const float* __restrict__ ps_part, int PS_KS, long ks_stride,
    int b, const float* __restrict__ Dwei, const float* __restrict__ Uatt,
    int A) {
  for (int i = threadIdx.x; i < A; i += blockDim.x) {
    float ps = 0.f;
    for (int k = 0; k < PS_KS; ++k)
      ps += ps_part[(long)k * ks_stride + (long)b * A + i];
    sm[i] = ps;
    sm[A + i] = Dwei[i];
    sm[2 * A + i] = Uatt[i];
  }
}

// ---------------- attention forward, pass 1 (one block per (b, chunk)) ----
// e-scores of the chunk (all of A in the block: no A-split, no atomics),
// chunk-local softmax statistics, and the chunk's partial weighted context
// with the UNNORMALISED p = exp(e - m_c) * mask. cond_attn_combine_gate
// rescales by exp(m_c - M) / L. pstate arrives as [KS][32][A] split-K
// partials.
// With a row_src table (decode against a context kept once per sentence)
// row b reads source column row_src[b] of the S-column pctx / ctx_mask /
// ctx_bf; everything else stays per row. An entry outside [0, S) is never
// dereferenced: the row is treated as fully masked (p = 0, zero partial
// context), which the combine pass's L == 0 guard turns into alpha = 0.
__global__ __launch_bounds__(ATT_THREADS) void cond_attn_fwd_chunk(
    const float* __restrict__ pctx,      // [Ts][S][A]
    const float* __restrict__ ps_part,   // [KS][32][A] pstate partials
    int PS_KS,
    const float* __restrict__ accA,      // [B][Ts] (pre-update)
    const float* __restrict__ Dwei,      // [A]
    const float* __restrict__ Uatt,      // [A]
    const float* __restrict__ catt_p,    // [1]
    const float* __restrict__ ctx_mask,  // [Ts][S] or null
    const bf16_t* __restrict__ ctx_bf,   // [Ts][S][C]
    const int* __restrict__ row_src,     // [B] source column; null: identity
    int S,                               // context columns (B without table)
    float* __restrict__ alphas_t,        // [B][Ts] out: unnormalised p
    float* __restrict__ stats,           // [B][NCH][2] out: (m_c, l_c)
    float* __restrict__ ctx_part,        // [B][NCH][C] out
    int B, int Ts, int A, int C, int CH, int lps) {
  extern __shared__ __attribute__((aligned(16))) float sm_att[];  // [3A]
  __shared__ float sm_e[ATT_CH_MAX];
  __shared__ float sm_p[ATT_CH_MAX];
  const float* sm_ps = sm_att;
  const float* sm_dw = sm_att + A;
  const float* sm_ua = sm_att + 2 * A;
  const int b = blockIdx.x;
  const int src = (row_src != nullptr) ? row_src[b] : b;  // block-uniform
  const bool src_ok = src >= 0 && src < S;
  const int NCH = gridDim.y;
  const int sbeg = blockIdx.y * CH;
  const int n = min(CH, Ts - sbeg);  // >= 1: NCH = ceil(Ts / CH)
  attn_stage_vectors(sm_att, ps_part, PS_KS, (long)32 * A, b, Dwei, Uatt, A);
  __syncthreads();

  // e-scores: lps lanes share one s and walk its pctx row together
  const int gl = threadIdx.x % lps;
  const int ngrp = ATT_THREADS / lps;
  for (int ls = threadIdx.x / lps; ls < n; ls += ngrp) {
    const int s = sbeg + ls;
    // masked positions must not influence any max: they are zeroed AFTER
    // exp, but a padded position's e shifting a max changes rounding for
    // the real ones — decode results would then depend on how far the
    // source was padded (the graph-decode length bucketing pads to 64)
    const bool live =
        src_ok &&
        ((ctx_mask == nullptr) || ctx_mask[(long)s * S + src] != 0.f);
    float e = 0.f;
    if (live) {  // uniform over the lane group
      const float accAu = accA[(long)b * Ts + s];
      const float* prow = pctx + ((long)s * S + src) * A;
      if (A % 4 == 0) {
        for (int i = gl * 4; i < A; i += lps * 4) {
          const float4 p = *(const float4*)(prow + i);
          const float4 st = *(const float4*)(sm_ps + i);
          const float4 dw = *(const float4*)(sm_dw + i);
          const float4 ua = *(const float4*)(sm_ua + i);
          e += tanhf(p.x + st.x + accAu * dw.x) * ua.x +
               tanhf(p.y + st.y + accAu * dw.y) * ua.y +
               tanhf(p.z + st.z + accAu * dw.z) * ua.z +
               tanhf(p.w + st.w + accAu * dw.w) * ua.w;
        }
      } else {
        for (int i = gl; i < A; i += lps)
          e += tanhf(prow[i] + sm_ps[i] + accAu * sm_dw[i]) * sm_ua[i];
      }
    }
    for (int off = lps / 2; off > 0; off >>= 1) e += __shfl_xor(e, off);
    if (gl == 0) sm_e[ls] = live ? e + catt_p[0] : -INFINITY;
  }
  __syncthreads();

  // chunk-local statistics: n <= 64, so the first wave holds the chunk
  if (threadIdx.x < NATS_WAVE) {
    const int ls = threadIdx.x;
    const float e = (ls < n) ? sm_e[ls] : -INFINITY;
    float m = e;
#pragma unroll
    for (int off = NATS_WAVE / 2; off > 0; off >>= 1)
      m = fmaxf(m, __shfl_xor(m, off));
    float p = 0.f;
    if (e != -INFINITY) {  // live, hence m finite
      p = __expf(e - m);
      if (ctx_mask != nullptr) p *= ctx_mask[(long)(sbeg + ls) * S + src];
    }
    float l = p;
#pragma unroll
    for (int off = NATS_WAVE / 2; off > 0; off >>= 1) l += __shfl_xor(l, off);
    sm_p[ls] = p;
    if (ls < n) alphas_t[(long)b * Ts + sbeg + ls] = p;
    if (ls == 0) {
      stats[((long)b * NCH + blockIdx.y) * 2] = m;  // -inf: empty chunk
      stats[((long)b * NCH + blockIdx.y) * 2 + 1] = l;
    }
  }
  __syncthreads();

  // partial weighted context: each thread owns 8 consecutive c (one 16 B
  // load per source row), eight rows in flight per thread
  float* part = ctx_part + ((long)b * NCH + blockIdx.y) * C;
  if (!src_ok) {  // no source column to load from: the partial is zero
    for (int c = threadIdx.x; c < C; c += ATT_THREADS) part[c] = 0.f;
    return;
  }
  const long sstride = (long)S * C;
  const bf16_t* cbase = ctx_bf + ((long)sbeg * S + src) * C;
  const int C8 = C & ~7;
  for (int c0 = threadIdx.x * 8; c0 < C8; c0 += ATT_THREADS * 8) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const bf16_t* col = cbase + c0;
    int ls = 0;
    for (; ls + 8 <= n; ls += 8) {
      bf16x8 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        v[u] = *(const bf16x8*)(col + (long)(ls + u) * sstride);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float p = sm_p[ls + u];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += (float)v[u][k] * p;
      }
    }
    for (; ls < n; ++ls) {
      const bf16x8 v = *(const bf16x8*)(col + (long)ls * sstride);
      const float p = sm_p[ls];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += (float)v[k] * p;
    }
    if (C % 4 == 0) {  // rows of part are 16 B aligned
      *(float4*)(part + c0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
      *(float4*)(part + c0 + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) part[c0 + k] = acc[k];
    }
  }
  for (int c = C8 + threadIdx.x; c < C; c += ATT_THREADS) {  // C % 8 tail
    float acc = 0.f;
    for (int ls = 0; ls < n; ++ls)
      acc += (float)cbase[(long)ls * sstride + c] * sm_p[ls];
    part[c] = acc;
  }
}

// ---------------- attention forward, pass 2: combine + gate ----------------
// grid (B, ceil(C/256)). Every block derives its row's global softmax
// statistics from the NCH chunk pairs (serially, in chunk order: all blocks
// of a row agree bit for bit), combines the partial contexts with the
// per-chunk scale w_c = exp(m_c - M) / L, applies the distraction gate and
// the acc_ctx update, and finishes its share of the row's attention
// weights (alphas *= w_chunk, acc_alpha update). Block y == 0 also writes
// the combined pstate the backward reads.
__global__ __launch_bounds__(ATT_THREADS) void cond_attn_combine_gate(
    const float* __restrict__ stats,     // [B][NCH][2]
    const float* __restrict__ ctx_part,  // [B][NCH][C]
    int NCH, int CH,
    float* __restrict__ alphas_t,        // [B][Ts] in: p, out: alpha
    float* __restrict__ accA,            // [B][Ts] in/out
    float* __restrict__ accA_used_t,     // [B][Ts] out (pre-update copy)
    const float* __restrict__ ps_part,   // [KS][32][A] pstate partials
    int PS_KS,
    float* __restrict__ pstate_t,        // [B][A] combined (for backward)
    int A, int Ts,
    const float* __restrict__ Ucon, const float* __restrict__ Wcon,
    float* __restrict__ accC,            // [B][C] in/out
    bf16_t* __restrict__ accC_used_t,    // [B][C]
    bf16_t* __restrict__ ctxpre_t,       // [B][C] (saved pre-gate sum)
    float* __restrict__ ctxs_t,          // [B][C] (gated output)
    bf16_t* __restrict__ hc_bf,          // [32][K1] GRU_1 operand
    int ctx_off, int ldK1, const float* __restrict__ mask_t, int B, int C) {
  extern __shared__ float sm_w[];  // [NCH] per-chunk scale
  const int b = blockIdx.x;
  const float* st = stats + (long)b * NCH * 2;
  float M = -INFINITY;
  for (int k = 0; k < NCH; ++k) M = fmaxf(M, st[2 * k]);
  float L = 0.f;
  for (int k = 0; k < NCH; ++k) {
    const float l = st[2 * k + 1];
    if (l > 0.f) L += l * __expf(st[2 * k] - M);
  }
  // all-masked rows cannot occur (every sequence has >= 1 real token),
  // but guard the degenerate L = 0 anyway: such a row gets alpha = 0
  const float inv = (L > 0.f) ? 1.f / L : 0.f;
  for (int k = threadIdx.x; k < NCH; k += blockDim.x)
    sm_w[k] = (st[2 * k + 1] > 0.f) ? __expf(st[2 * k] - M) * inv : 0.f;
  __syncthreads();
  const float mm = (mask_t != nullptr) ? mask_t[b] : 1.f;

  const int c = blockIdx.y * blockDim.x + threadIdx.x;
  if (c < C) {
    const float* part = ctx_part + (long)b * NCH * C + c;
    float sum = 0.f;
#pragma unroll 4
    for (int k = 0; k < NCH; ++k) sum += sm_w[k] * part[(long)k * C];
    ctxpre_t[(long)b * C + c] = (bf16_t)sum;
    const float accCv = accC[(long)b * C + c];
    accC_used_t[(long)b * C + c] = (bf16_t)accCv;
    // distraction over input content vectors (nats.py:545-546)
    const float g = tanhf(Ucon[c] * sum + accCv * Wcon[c]);
    ctxs_t[(long)b * C + c] = g;
    hc_bf[(long)b * ldK1 + ctx_off + c] = (bf16_t)g;
    accC[(long)b * C + c] = accCv + mm * g;
  }

  // the row's blocks split the s range between them
  const int sper = (Ts + gridDim.y - 1) / gridDim.y;
  const int s0 = blockIdx.y * sper;
  const int s1 = min(Ts, s0 + sper);
  for (int s = s0 + threadIdx.x; s < s1; s += blockDim.x) {
    const float al = alphas_t[(long)b * Ts + s] * sm_w[s / CH];
    alphas_t[(long)b * Ts + s] = al;
    const float av = accA[(long)b * Ts + s];
    accA_used_t[(long)b * Ts + s] = av;
    accA[(long)b * Ts + s] = av + mm * al;
  }
  if (blockIdx.y == 0) {
    for (int i = threadIdx.x; i < A; i += blockDim.x) {
      float ps = 0.f;
      for (int k = 0; k < PS_KS; ++k) ps += ps_part[((long)k * 32 + b) * A + i];
      pstate_t[(long)b * A + i] = ps;
    }
  }
}

// ---------------- GRU_1 forward (fused, small-K path) ----------------
// 16 waves: wave w -> (m = w/8, g = (w%8)/2, ks = w%2) with output groups
// g0 = r2 (K = h1|ctx), g1 = u2 (K = h1|ctx), g2 = pxa (h1@Ux_1),
// g3 = pxb (ctx@Wx_1) — K-selectivity comes from zero blocks in W1pk.
// K is split across wave pairs (K1 is ~3H — the serial chain at 8 waves
// measured 34 us/launch, latency-bound). Split-K block ksb of KS takes K
// parts 2*ksb and 2*ksb+1 of 2*KS; the fused kernel is KS = 1.
__device__ __forceinline__ void gru1_mfma_phase(
    float (*pre)[2][32][JB + 1],  // [4][2][32][JB+1] out (caller barriers)
    const bf16_t* hc_bf, const bf16_t* W1pk, int K1, int wg, int ksb, int KS) {
  const int wave = threadIdx.x / NATS_WAVE;
  const int m = wave / 8;
  const int g = (wave % 8) / 2;
  const int ks = wave % 2;
  const KRange k = k_part(KRange{0, K1}, 2 * KS, 2 * ksb + ks);

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const bf16_t* brow = W1pk + (long)(wg * 4 + g) * JB * K1;
  NATS_MFMA_KLOOP(acc, hc_bf, 16 * m, K1, brow, 0, K1, k.beg, k.end);
  store_cd_lds(pre[g][ks], acc, 16 * m);
}

// GRU_1 finish of element (b, j) from the four summed preactivations:
// cell, h2 (fp32 + bf16 operand copy) and saved1 = (r2, u2, pxa, hbar).
__device__ __forceinline__ void gru1_fwd_finish(
    float p0, float p1, float pxa, float pxb, const float* h1_t,
    const float* b1, const float* bx1, const float* mask_t, float* h2_t,
    bf16_t* h2bf_out, int ld_h2bf, float* saved1_t, int H, int b, int j) {
  const long bj = (long)b * H + j;
  const GruCellFwd o = gru_cell_fwd(p0 + b1[j], p1 + b1[H + j], pxa + bx1[j],
                                    pxb, h1_t[bj], mask_t, b);
  h2_t[bj] = o.hnew;
  h2bf_out[(long)b * ld_h2bf + j] = (bf16_t)o.hnew;
  saved1_t[(long)b * 4 * H + j] = o.r;
  saved1_t[(long)b * 4 * H + H + j] = o.u;
  saved1_t[(long)b * 4 * H + 2 * H + j] = pxa;
  saved1_t[(long)b * 4 * H + 3 * H + j] = o.hbar;
}

__global__ __launch_bounds__(1024) void cond_gru1_step_fwd(
    const bf16_t* __restrict__ hc_bf,  // [32][K1] = [h1 | ctx_t] bf16
    const float* __restrict__ h1_t,    // [B][H] fp32
    const bf16_t* __restrict__ W1pk,   // [ngrp*4*16][K1]
    const float* __restrict__ b1,      // [2H]
    const float* __restrict__ bx1,     // [H]
    const float* __restrict__ mask_t,  // [B] or null
    float* __restrict__ h2_t,          // [B][H] out
    bf16_t* __restrict__ h2bf_out,     // [32][Hpad] out
    int ld_h2bf,
    float* __restrict__ saved1_t,      // [B][4H] (r2,u2,pxa,hbar)
    int B, int H, int K1) {
  __shared__ float pre[4][2][32][JB + 1];
  const int j0 = blockIdx.x * JB;
  gru1_mfma_phase(pre, hc_bf, W1pk, K1, blockIdx.x, 0, 1);
  __syncthreads();

  for (int idx = threadIdx.x; idx < B * JB; idx += blockDim.x) {
    const int b = idx / JB;
    const int c = idx % JB;
    const int j = j0 + c;
    if (j >= H) continue;
    gru1_fwd_finish(pre[0][0][b][c] + pre[0][1][b][c],
                    pre[1][0][b][c] + pre[1][1][b][c],
                    pre[2][0][b][c] + pre[2][1][b][c],
                    pre[3][0][b][c] + pre[3][1][b][c], h1_t, b1, bx1, mask_t,
                    h2_t, h2bf_out, ld_h2bf, saved1_t, H, b, j);
  }
}

// ---------------- GRU_1 forward (split-K) ----------------
// The single-kernel variant ran ngrpH (=63 at dim 1000) workgroups — a
// quarter of the chip — at 31.4us/step (profiles/
// cnn_kernel_stats_barrierv2.csv). Split-K: grid (ngrpH, KS) blocks each
// compute a K-quarter of all four gate GEMMs (16 waves: m x group x
// half-split as before) and store fp32 partials; a pointwise kernel sums
// the KS partials and applies the gate nonlinearities (nats.py:529-553).
__global__ __launch_bounds__(1024) void cond_gru1_gemm_splitk(
    const bf16_t* __restrict__ hc_bf,  // [32][K1] = [h1 | ctx_t] bf16
    const bf16_t* __restrict__ W1pk,   // [ngrp*4*16][K1]
    float* __restrict__ part,          // [KS][4][32][Hpad]
    int H, int K1, int Hpad) {
  __shared__ float pre[4][2][32][JB + 1];
  const int ksb = blockIdx.y;
  const int j0 = blockIdx.x * JB;
  gru1_mfma_phase(pre, hc_bf, W1pk, K1, blockIdx.x, ksb, gridDim.y);
  __syncthreads();

  float* dst = part + ((long)ksb * 4 + 0) * 32 * Hpad;
  for (int idx = threadIdx.x; idx < 4 * 32 * JB; idx += blockDim.x) {
    const int gg = idx / (32 * JB);
    const int b = (idx / JB) % 32;
    const int c = idx % JB;
    dst[((long)gg * 32 + b) * Hpad + j0 + c] =
        pre[gg][0][b][c] + pre[gg][1][b][c];
  }
}

__global__ void cond_gru1_step_pointwise(
    const float* __restrict__ part,    // [KS][4][32][Hpad]
    int KS,
    const float* __restrict__ h1_t,    // [B][H] fp32
    const float* __restrict__ b1,      // [2H]
    const float* __restrict__ bx1,     // [H]
    const float* __restrict__ mask_t,  // [B] or null
    float* __restrict__ h2_t,          // [B][H] out
    bf16_t* __restrict__ h2bf_out,     // [32][ld_h2bf] out
    int ld_h2bf,
    float* __restrict__ saved1_t,      // [B][4H] (r2,u2,pxa,hbar)
    int B, int H, int Hpad) {
  const long total = (long)B * H;
  for (long idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int b = idx / H;
    const int j = idx % H;
    float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
    const long bj = (long)b * Hpad + j;
    for (int k = 0; k < KS; ++k) {
      const float* pk = part + (long)k * 4 * 32 * Hpad;
      p0 += pk[bj];
      p1 += pk[(long)32 * Hpad + bj];
      p2 += pk[(long)2 * 32 * Hpad + bj];
      p3 += pk[(long)3 * 32 * Hpad + bj];
    }
    gru1_fwd_finish(p0, p1, p2, p3, h1_t, b1, bx1, mask_t, h2_t, h2bf_out,
                    ld_h2bf, saved1_t, H, b, j);
  }
}

// ---------------- backward kernels ----------------

// Fused per-step backward prologue: the GRU_1 pointwise and the
// independent dctx passthrough (upstream readout grad + acc-chain, formerly
// its own cond_dctx_dir launch) share one grid-stride index space.
__global__ void cond_gru1_bwd_pointwise(
    const float* __restrict__ dh_carry,   // [B][H] (split-K half 0)
    const float* __restrict__ dh_carry2,  // [B][H] half 1 or null
    const float* __restrict__ dh2_all_t,  // [B][H] or null
    const float* __restrict__ saved1_t,   // [B][4H]
    const float* __restrict__ h1_all_t,   // [B][H]
    const float* __restrict__ bx1,        // [H]
    const float* __restrict__ mask_t,     // [B] or null
    bf16_t* __restrict__ dstep1,          // [32][K3H] [dpr2|dpu2|dpxa_lin]
    bf16_t* __restrict__ dstepC,          // [32][K3H] [dpr2|dpu2|dpx2]
    int ldK3,
    float* __restrict__ ddirect_h1,       // [B][H]
    bf16_t* __restrict__ dpre1_t,         // [B][4H]
    const float* __restrict__ dctxs_t,    // [B][C] or null (upstream)
    const float* __restrict__ daccC,      // [B][C] (pre-update, read)
    float* __restrict__ dctx_dir,         // [B][C] out
    int C, int B, int H) {
  const long total = (long)B * H;
  const long total_all = total + (long)B * C;
  for (long idx2 = blockIdx.x * blockDim.x + threadIdx.x; idx2 < total_all;
       idx2 += (long)gridDim.x * blockDim.x) {
    if (idx2 >= total) {
      const long e = idx2 - total;
      const int b = e / C;
      const float mm = (mask_t != nullptr) ? mask_t[b] : 1.f;
      float v = mm * daccC[e];
      if (dctxs_t != nullptr) v += dctxs_t[e];
      dctx_dir[e] = v;
      continue;
    }
    const long idx = idx2;
    const int b = idx / H;
    const int j = idx % H;
    float dh2 = dh_carry[idx];
    if (dh_carry2 != nullptr) dh2 += dh_carry2[idx];
    if (dh2_all_t != nullptr) dh2 += dh2_all_t[idx];
    const float r2 = saved1_t[(long)b * 4 * H + j];
    const float u2 = saved1_t[(long)b * 4 * H + H + j];
    const float pxa = saved1_t[(long)b * 4 * H + 2 * H + j];
    const float hbar = saved1_t[(long)b * 4 * H + 3 * H + j];
    const float h1v = h1_all_t[idx];
    const float mm = (mask_t != nullptr) ? mask_t[b] : 1.f;
    const GruCellBwd o =
        gru_cell_bwd(dh2, r2, u2, pxa + bx1[j], hbar, h1v, mm);
    ddirect_h1[idx] = o.ddirect;
    dstep1[(long)b * ldK3 + j] = (bf16_t)o.dpr;
    dstep1[(long)b * ldK3 + H + j] = (bf16_t)o.dpu;
    dstep1[(long)b * ldK3 + 2 * H + j] = (bf16_t)o.dpxl;
    dstepC[(long)b * ldK3 + j] = (bf16_t)o.dpr;
    dstepC[(long)b * ldK3 + H + j] = (bf16_t)o.dpu;
    dstepC[(long)b * ldK3 + 2 * H + j] = (bf16_t)o.dpx;
    dpre1_t[(long)b * 4 * H + j] = (bf16_t)o.dpr;
    dpre1_t[(long)b * 4 * H + H + j] = (bf16_t)o.dpu;
    dpre1_t[(long)b * 4 * H + 2 * H + j] = (bf16_t)o.dpx;
    dpre1_t[(long)b * 4 * H + 3 * H + j] = (bf16_t)o.dpxl;
  }
}

// Dual recurrent-GEMM with the distraction-gate backward fused into the
// context side's epilogue. grid.y == 0: dh1 = ddirect_h1 + dstep1 @
// [U_1|Ux_1]^T (plain). grid.y == 1: the former dctx_buf value (dctx_dir
// + dstepC @ [W_1|Wx_1]^T) never touches memory — the gate backward
// (tanh', Ucon/Wcon splits, daccC accumulate; nats.py:545-546 reverse)
// is applied in-register, eliminating the separate cond_gate_bwd pass.
__global__ __launch_bounds__(384) void cond_bwd_gemm_dual_gate(
    const bf16_t* __restrict__ dstep1, const bf16_t* __restrict__ U1cat,
    const float* __restrict__ ddirect_h1, float* __restrict__ dh1_buf,
    int H, const bf16_t* __restrict__ dstepC,
    const bf16_t* __restrict__ W1cat, const float* __restrict__ dctx_dir,
    int C, int Kpad,
    const float* __restrict__ ctxs_t,   // [B][C] gated value
    const float* __restrict__ Ucon, const float* __restrict__ Wcon,
    float* __restrict__ daccC,          // [B][C] in/out
    float* __restrict__ dctxpre_f32,    // [B][C] out
    bf16_t* __restrict__ dctxpre_all_t, // [B][C] out
    const bf16_t* __restrict__ ctxpre_t,    // [B][C] (saved pre-gate sum)
    const bf16_t* __restrict__ accC_used_t, // [B][C] (saved acc state)
    float* __restrict__ gdUcon,         // [C] (+=, one atomic/col/step)
    float* __restrict__ gdWcon,         // [C]
    int B) {
  // dU_con[c] = sum_{t,b} dg*ctxpre and dW_con[c] = sum dg*accC_used
  // fold in here (block-local b-reduction + one atomic per column per
  // step) — the torch expression re-streamed three (T,B,C) buffers
  __shared__ float ucon_s[JB], wcon_s[JB];
  const bool ctx_side = (blockIdx.y == 1);
  if (ctx_side && threadIdx.x < JB) {
    ucon_s[threadIdx.x] = 0.f;
    wcon_s[threadIdx.x] = 0.f;
  }
  const int N = ctx_side ? C : H;
  if ((int)blockIdx.x * JB >= N) return;
  const bf16_t* dstep = ctx_side ? dstepC : dstep1;
  const bf16_t* Wt = ctx_side ? W1cat : U1cat;

  const int i0 = blockIdx.x * JB;
  row_gemm(dstep, Wt, i0, Kpad, KRange{0, Kpad}, B, N,
           [&](int b, int i, float sum) {
    const long bi = (long)b * N + i;
    if (!ctx_side) {
      dh1_buf[bi] = ddirect_h1[bi] + sum;
    } else {
      const float v = dctx_dir[bi] + sum;  // former dctx_buf value
      const float g = ctxs_t[bi];
      const float dg = v * (1.f - g * g);
      const float dpre = dg * Ucon[i];
      dctxpre_f32[bi] = dpre;
      dctxpre_all_t[bi] = (bf16_t)dpre;
      daccC[bi] += dg * Wcon[i];
      atomicAdd(ucon_s + (i - i0), dg * (float)ctxpre_t[bi]);
      atomicAdd(wcon_s + (i - i0), dg * (float)accC_used_t[bi]);
    }
  });
  if (ctx_side) {
    __syncthreads();
    if (threadIdx.x < JB && i0 + (int)threadIdx.x < N) {
      atomicAdd(gdUcon + i0 + threadIdx.x, ucon_s[threadIdx.x]);
      atomicAdd(gdWcon + i0 + threadIdx.x, wcon_s[threadIdx.x]);
    }
  }
}

// A-fragment built from an UNPADDED fp32 [Rows][Kcols] matrix with
// zero-fill outside (rows >= Rows, k >= Kcols) — lets the dh1 += dpstate
// @ W_att^T GEMM consume the atomically-reduced fp32 dpstate directly,
// without the former cond_dpstate_cast pass.
__device__ __forceinline__ bf16x8 frag_a_f32pad(const float* A, int row0,
                                                int ld, int k0, int Rows,
                                                int Kcols) {
  const int lane = threadIdx.x & (NATS_WAVE - 1);
  const int r = row0 + (lane & 15);
  const int kb = k0 + (lane >> 4) * 8;
  bf16x8 v;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int k = kb + i;
    v[i] = (bf16_t)((r < Rows && k < Kcols) ? A[(long)r * ld + k] : 0.f);
  }
  return v;
}

// dh_{t-1} carry GEMM with grid.y split-K and CONSUMER-side combine:
// the unsplit kernel ran 63 blocks (a quarter of the chip) at 12.6 us;
// round 1's atomic-combine split measured neutral (atomics + re-zero),
// so here each half writes its own [B][H] partial — full coverage, no
// zeroing — and the next step's GRU_1 pointwise sums the two.
__global__ __launch_bounds__(384) void cond_dh_carry_gemm_split(
    const bf16_t* __restrict__ dstep,  // [32][Kpad]
    const bf16_t* __restrict__ Wt,     // [ngrp*16][Kpad]
    const float* __restrict__ ddirect, // [B][H] (added by grid.y == 0)
    float* __restrict__ out,           // [2][B][H] partials
    int B, int H, int Kpad) {
  const int ks2 = blockIdx.y;        // K half
  float* o = out + (long)ks2 * B * H;
  row_gemm(dstep, Wt, blockIdx.x * JB, Kpad,
           k_part(KRange{0, Kpad}, 2, ks2), B, H,
           [&](int b, int i, float v) {
             if (ks2 == 0) v += ddirect[(long)b * H + i];
             o[(long)b * H + i] = v;
           });
}

// Same wave map and epilogue shape as row_gemm, kept written out: its A
// fragments are converted from fp32 in-register (frag_a_f32pad) under a
// plain K-loop, which row_gemm's pipelined bf16 loop cannot express.
__global__ __launch_bounds__(384) void cond_dh1_att_gemm(
    const float* __restrict__ dpstate_t,  // [B][A] fp32 (atomic-reduced)
    const bf16_t* __restrict__ WattB,     // [ngrpH*16][Apad]
    float* __restrict__ dh1_buf,          // [B][H] in/out (+=)
    int B, int H, int A, int Apad) {
  __shared__ float part[3][32][JB + 1];
  const int wg = blockIdx.x;
  const int wave = threadIdx.x / NATS_WAVE;
  const int m = wave / 3;
  const int ks = wave % 3;
  const int i0 = wg * JB;
  const KRange kr = k_part(KRange{0, Apad}, 3, ks);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k = kr.beg; k + 32 <= kr.end; k += 32) {
    bf16x8 a = frag_a_f32pad(dpstate_t, 16 * m, A, k, B, A);
    bf16x8 bfr = frag_bt_rowmajor(WattB, i0, Apad, k);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bfr, acc, 0, 0, 0);
  }
  store_cd_lds(part[ks], acc, 16 * m);
  __syncthreads();
  for (int idx = threadIdx.x; idx < B * JB; idx += blockDim.x) {
    const int b = idx / JB;
    const int cc = idx % JB;
    const int i = i0 + cc;
    if (i >= H) continue;
    dh1_buf[(long)b * H + i] +=
        part[0][b][cc] + part[1][b][cc] + part[2][b][cc];
  }
}

// attention backward, stage 1 (one WAVE per (b,s)): dalpha[b,s] =
// ctx[s,b,:] . dctxpre[b,:] (+ acc-chain and upstream alpha grads).
__global__ __launch_bounds__(256) void cond_attn_bwd_dalpha(
    const bf16_t* __restrict__ ctx_bf,      // [Ts][B][C]
    const float* __restrict__ dctxpre_f32,  // [B][C]
    const float* __restrict__ alphas_t,     // [B][Ts]
    const float* __restrict__ daccA,        // [B][Ts]
    const float* __restrict__ mask_t,       // [B] or null
    const float* __restrict__ dalphas_t,    // [B][Ts] or null
    float* __restrict__ dal_buf,            // [B][Ts]
    int B, int Ts, int C) {
  const int b = blockIdx.x;
  const int wave = threadIdx.x / NATS_WAVE;
  const int lane = threadIdx.x & (NATS_WAVE - 1);
  const int s = blockIdx.y * 4 + wave;
  if (s >= Ts) return;
  const bf16_t* crow = ctx_bf + ((long)s * B + b) * C;
  const float* drow = dctxpre_f32 + (long)b * C;
  float part = 0.f;
  const int C8 = C & ~7;
  for (int c = lane * 8; c < C8; c += NATS_WAVE * 8) {
    bf16x8 v = *(const bf16x8*)(crow + c);
    const float4 d0 = *(const float4*)(drow + c);
    const float4 d1 = *(const float4*)(drow + c + 4);
    part += (float)v[0] * d0.x + (float)v[1] * d0.y + (float)v[2] * d0.z +
            (float)v[3] * d0.w + (float)v[4] * d1.x + (float)v[5] * d1.y +
            (float)v[6] * d1.z + (float)v[7] * d1.w;
  }
  for (int c = C8 + lane; c < C; c += NATS_WAVE) {
    part += (float)crow[c] * drow[c];
  }
#pragma unroll
  for (int off = NATS_WAVE / 2; off > 0; off >>= 1)
    part += __shfl_down(part, off);
  if (lane == 0) {
    float dal = part;
    const float mm = (mask_t != nullptr) ? mask_t[b] : 1.f;
    dal += mm * daccA[(long)b * Ts + s];
    if (dalphas_t != nullptr) dal += dalphas_t[(long)b * Ts + s];
    dal_buf[(long)b * Ts + s] = dal;
    // NOTE: the dot(alpha, dal) fold was MEASURED OUT here twice — a
    // per-s atomicAdd serializes ~Ts adds on one address (~120us/step,
    // round 1), and a per-BLOCK atomic tree still serialized Ts/4 adds
    // per address (dalpha 9us -> 47.9us/call, prof_r2). Every block of
    // cond_attn_bwd_fused sums its row's dot itself instead.
  }
}

// attention backward, stage 2 (one block per (b, s-chunk), all of A in the
// block): the softmax-backward dot, the per-(s, i) tanh backward into
// dpctx_acc and the acc_alpha carry, and the chunk's column sums for
// dpstate / dD_wei / dU_att / dc_att, in one pass. The tanh values and
// their gradients go from the (s, i) loop to the column sums through an
// LDS tile, in fp32: 1 - pc^2 of a saturated pc has no relative precision
// left in a bf16 copy.
__global__ __launch_bounds__(ATT_THREADS) void cond_attn_bwd_fused(
    const float* __restrict__ alphas_t,     // [B][Ts]
    const float* __restrict__ dal_buf,      // [B][Ts]
    const float* __restrict__ pctx,         // [Ts][B][A]
    const float* __restrict__ pstate_t,     // [B][A]
    const float* __restrict__ accA_used_t,  // [B][Ts]
    const float* __restrict__ Dwei, const float* __restrict__ Uatt,
    float* __restrict__ daccA,              // [B][Ts] (+=)
    float* __restrict__ dpctx_acc,          // [Ts][B][A] (+=)
    float* __restrict__ dpstate_t,          // [B][A] (one atomic per block)
    float* __restrict__ gslot,              // [B][NCH][2A+1] (+=, own slot)
    int B, int Ts, int A, int CH, int lps) {
  // [3A] ps|Dwei|Uatt, then the [CH][A] dpc and pc tiles
  extern __shared__ __attribute__((aligned(16))) float sm_att[];
  __shared__ float sm_de[ATT_CH_MAX];
  __shared__ float sm_au[ATT_CH_MAX];
  const int A4 = (A + 3) & ~3;  // keeps the tiles 16 B aligned
  const float* sm_ps = sm_att;
  const float* sm_dw = sm_att + A;
  const float* sm_ua = sm_att + 2 * A;
  float* t_dpc = sm_att + 3 * A4;
  float* t_pc = t_dpc + (long)CH * A;
  const int b = blockIdx.x;
  const int NCH = gridDim.y;
  const int sbeg = blockIdx.y * CH;
  const int n = min(CH, Ts - sbeg);
  attn_stage_vectors(sm_att, pstate_t, 1, 0, b, Dwei, Uatt, A);

  // dot = sum_s alpha * dal over the WHOLE row, summed in a fixed order:
  // every block of the row gets the same bits
  float part = 0.f;
  for (int s = threadIdx.x; s < Ts; s += blockDim.x)
    part += alphas_t[(long)b * Ts + s] * dal_buf[(long)b * Ts + s];
  const float dot = block_reduce_sum(part);  // also orders the staging

  float dc = 0.f;
  if (threadIdx.x < NATS_WAVE) {
    const int ls = threadIdx.x;
    float de = 0.f, au = 0.f;
    if (ls < n) {
      const long bs = (long)b * Ts + sbeg + ls;
      de = alphas_t[bs] * (dal_buf[bs] - dot);
      au = accA_used_t[bs];
    }
    sm_de[ls] = de;
    sm_au[ls] = au;
    dc = de;
#pragma unroll
    for (int off = NATS_WAVE / 2; off > 0; off >>= 1)
      dc += __shfl_xor(dc, off);
  }
  __syncthreads();

  const int gl = threadIdx.x % lps;
  const int ngrp = ATT_THREADS / lps;
  for (int ls = threadIdx.x / lps; ls < n; ls += ngrp) {
    const int s = sbeg + ls;
    const float de = sm_de[ls];
    const float accAu = sm_au[ls];
    const float* prow = pctx + ((long)s * B + b) * A;
    float* dprow = dpctx_acc + ((long)s * B + b) * A;
    float* drow = t_dpc + (long)ls * A;
    float* crow = t_pc + (long)ls * A;
    float dacc = 0.f;
    if (A % 4 == 0) {
      for (int i = gl * 4; i < A; i += lps * 4) {
        const float4 p = *(const float4*)(prow + i);
        const float4 st = *(const float4*)(sm_ps + i);
        const float4 dw = *(const float4*)(sm_dw + i);
        const float4 ua = *(const float4*)(sm_ua + i);
        float4 dpv = *(const float4*)(dprow + i);
        float4 pc, d;
        pc.x = tanhf(p.x + st.x + accAu * dw.x);
        pc.y = tanhf(p.y + st.y + accAu * dw.y);
        pc.z = tanhf(p.z + st.z + accAu * dw.z);
        pc.w = tanhf(p.w + st.w + accAu * dw.w);
        d.x = de * (1.f - pc.x * pc.x) * ua.x;
        d.y = de * (1.f - pc.y * pc.y) * ua.y;
        d.z = de * (1.f - pc.z * pc.z) * ua.z;
        d.w = de * (1.f - pc.w * pc.w) * ua.w;
        dpv.x += d.x;
        dpv.y += d.y;
        dpv.z += d.z;
        dpv.w += d.w;
        *(float4*)(dprow + i) = dpv;
        dacc += d.x * dw.x + d.y * dw.y + d.z * dw.z + d.w * dw.w;
        *(float4*)(drow + i) = d;
        *(float4*)(crow + i) = pc;
      }
    } else {
      for (int i = gl; i < A; i += lps) {
        const float pc = tanhf(prow[i] + sm_ps[i] + accAu * sm_dw[i]);
        const float d = de * (1.f - pc * pc) * sm_ua[i];
        dprow[i] += d;
        dacc += d * sm_dw[i];
        drow[i] = d;
        crow[i] = pc;
      }
    }
    for (int off = lps / 2; off > 0; off >>= 1) dacc += __shfl_xor(dacc, off);
    // the block owns all of A for its s: plain +=
    if (gl == 0) daccA[(long)b * Ts + s] += dacc;
  }
  __syncthreads();

  // column sums over the chunk: thread i owns column i
  float* slot = gslot + ((long)b * NCH + blockIdx.y) * (2 * A + 1);
  for (int i = threadIdx.x; i < A; i += blockDim.x) {
    float sps = 0.f, sdw = 0.f, sua = 0.f;
    for (int ls = 0; ls < n; ++ls) {
      const float d = t_dpc[(long)ls * A + i];
      sps += d;
      sdw += d * sm_au[ls];
      sua += sm_de[ls] * t_pc[(long)ls * A + i];
    }
    atomicAdd(&dpstate_t[(long)b * A + i], sps);
    slot[i] += sdw;
    slot[A + i] += sua;
  }
  if (threadIdx.x == 0) slot[2 * A] += dc;
}

}  // namespace

// ================= host: forward =================
std::vector<torch::Tensor> cond_gru_fwd(
    torch::Tensor yg, torch::Tensor yc, c10::optional<torch::Tensor> mask,
    torch::Tensor init_state, torch::Tensor ctx_bf,
    c10::optional<torch::Tensor> ctx_mask, torch::Tensor pctx,
    torch::Tensor Upk2, torch::Tensor W1pk, torch::Tensor WattPk,
    torch::Tensor b1, torch::Tensor bx1, torch::Tensor Uatt,
    torch::Tensor catt, torch::Tensor Dwei, torch::Tensor Wcon,
    torch::Tensor Ucon,
    c10::optional<torch::Tensor> accC0, c10::optional<torch::Tensor> accA0,
    c10::optional<torch::Tensor> row_src) {
  const int T = yg.size(0), B = yg.size(1);
  const int H = yc.size(2);
  const int Ts = ctx_bf.size(0), C = ctx_bf.size(2);
  const int A = Uatt.size(0);
  TORCH_CHECK(B <= 32, "cond_gru: batch must be <= 32");
  check_scan_input(yg, torch::kBFloat16, "cond_gru yg");
  check_scan_input(ctx_bf, torch::kBFloat16, "cond_gru ctx");
  check_scan_input(pctx, torch::kFloat32, "cond_gru pctx");
  // decode against a context kept once per sentence: row b attends to
  // column row_src[b] of the S-column ctx / pctx / ctx_mask
  int S = B;
  const int* row_src_p = nullptr;
  if (row_src.has_value()) {
    check_scan_input(*row_src, torch::kInt32, "cond_gru row_src");
    S = ctx_bf.size(1);
    TORCH_CHECK(row_src->dim() == 1 && row_src->size(0) == B,
                "cond_gru: row_src must have one entry per row (", B, ")");
    TORCH_CHECK(ctx_bf.dim() == 3 && pctx.dim() == 3 && pctx.size(0) == Ts &&
                    pctx.size(1) == S && pctx.size(2) == A,
                "cond_gru: with row_src, pctx must be (Ts, S, A) next to a "
                "(Ts, S, C) ctx");
    TORCH_CHECK(!ctx_mask.has_value() ||
                    (ctx_mask->dim() == 2 && ctx_mask->size(0) == Ts &&
                     ctx_mask->size(1) == S),
                "cond_gru: with row_src, ctx_mask must be (Ts, S)");
    row_src_p = row_src->data_ptr<int>();
  }
  const int Hpad = Upk2.size(1);
  const int K1 = W1pk.size(1);
  const int ngrpH = cdiv(H, JB);
  check_packed_weight(Upk2, H, 3, "cond_gru Upk2");
  check_packed_weight(W1pk, H, 4, "cond_gru W1pk");

  auto optsF = yg.options().dtype(torch::kFloat32);
  auto optsB = yg.options();
  auto h2_all = torch::empty({T, B, H}, optsF);
  auto h1_all = torch::empty({T, B, H}, optsF);
  auto ctxs_all = torch::empty({T, B, C}, optsF);
  auto alphas_all = torch::empty({T, B, Ts}, optsF);
  auto saved2 = torch::empty({T, B, 3 * H}, optsB);
  // fp32: the backward forms 1 - u, u(1 - u), 1 - hbar^2 from these; from
  // bf16 copies a saturated gate loses all relative precision in them
  auto saved1 = torch::empty({T, B, 4 * H}, optsF);
  auto pstate_all = torch::empty({T, B, A}, optsF);
  auto ctxpre_all = torch::empty({T, B, C}, optsB);
  auto accA_used = torch::empty({T, B, Ts}, optsF);
  auto accC_used = torch::empty({T, B, C}, optsB);
  auto accA = accA0.has_value() ? accA0->contiguous().to(torch::kFloat32)
                                : torch::zeros({B, Ts}, optsF);
  auto accC = accC0.has_value() ? accC0->contiguous().to(torch::kFloat32)
                                : torch::zeros({B, C}, optsF);
  auto h2bf = torch::zeros({2, 32, Hpad}, optsB);
  const int GRU1_KS = 4;
  auto gru1_part = torch::empty({GRU1_KS, 4, 32, Hpad}, optsF);
  const int GRU2_KS = 4;
  auto gru2_part = torch::empty({GRU2_KS, 3, 32, Hpad}, optsF);
  auto hc_bf = torch::zeros({32, K1}, optsB);
  const int PS_KS = 4;
  auto ps_part = torch::empty({PS_KS, 32, A}, optsF);
  // attention chunking (rule at attn_chunk_len): every (b, chunk) block
  // writes its own statistics pair and partial context with plain stores,
  // so neither buffer needs zeroing
  const int CH = attn_chunk_len(B, Ts);
  const int NCH = cdiv(Ts, CH);
  const int lps = attn_lanes_per_s(CH);
  auto att_stats = torch::empty({B, NCH, 2}, optsF);
  auto ctx_part = torch::empty({B, NCH, C}, optsF);
  auto init_f = init_state.contiguous().to(torch::kFloat32);
  h2bf[0].slice(0, 0, B).slice(1, 0, H).copy_(init_f.to(torch::kBFloat16));

  const OptF32 mask_f(mask), cmask_f(ctx_mask);
  const float* cmask_p = cmask_f.p;

  auto stream = at::cuda::getCurrentCUDAStream().stream();
  const int Apad16 = cdiv(A, 16) * 16;
  const Steps<const bf16_t> yg_s(yg), yc_s(yc);
  const Steps<const float> mask_s(mask_f.t);
  const Steps<float> h1_s(h1_all), h2_s(h2_all), saved1_s(saved1),
      ctxs_s(ctxs_all), alphas_s(alphas_all), accA_used_s(accA_used),
      pstate_s(pstate_all);
  const Steps<bf16_t> saved2_s(saved2), accC_used_s(accC_used),
      ctxpre_s(ctxpre_all), h2bf_s(h2bf);  // h2bf: the ping-pong pair
  bf16_t* hc_bf_p = (bf16_t*)hc_bf.data_ptr();
  const bf16_t* Upk2_p = (const bf16_t*)Upk2.data_ptr();

  for (int t = 0; t < T; ++t) {
    const float* h2prev = t == 0 ? init_f.data_ptr<float>() : h2_s.at(t - 1);
    const float* mt = mask_s.at(t);
    // 1) GRU_2 -> h1 (bf16 into hc_bf cols [0,H)); split-K when K large
    if (Hpad >= 1024) {
      hipLaunchKernelGGL(nats_gru2_gemm_splitk, dim3(ngrpH, GRU2_KS),
                         dim3(384), 0, stream, h2bf_s.at(t % 2), Upk2_p,
                         gru2_part.data_ptr<float>(), Hpad);
      hipLaunchKernelGGL(nats_gru2_step_pointwise, dim3(cdiv(B * H, 256)),
                         dim3(256), 0, stream, gru2_part.data_ptr<float>(),
                         GRU2_KS, h2prev, yg_s.at(t), yc_s.at(t), mt,
                         h1_s.at(t), hc_bf_p, K1, saved2_s.at(t), B, H, Hpad);
    } else {
      hipLaunchKernelGGL(nats_gru_step_fwd, dim3(ngrpH), dim3(384), 0, stream,
                         h2bf_s.at(t % 2), h2prev, Upk2_p, yg_s.at(t),
                         yc_s.at(t), mt, h1_s.at(t), hc_bf_p, K1,
                         saved2_s.at(t), B, H, Hpad);
    }
    // 2) pstate = h1 @ W_att (split-K partials; summed by the consumers)
    hipLaunchKernelGGL(cond_small_gemm_bt, dim3(2, Apad16 / 16, PS_KS),
                       dim3(64), 0, stream, hc_bf_p,
                       (const bf16_t*)WattPk.data_ptr(),
                       ps_part.data_ptr<float>(), B, A, K1,
                       (int)WattPk.size(1));
    // 3) attention pass 1, one block per (b, s-chunk): e-scores,
    // chunk-local softmax statistics, unnormalised partial context
    hipLaunchKernelGGL(cond_attn_fwd_chunk, dim3(B, NCH), dim3(ATT_THREADS),
                       3 * A * sizeof(float), stream, pctx.data_ptr<float>(),
                       ps_part.data_ptr<float>(), PS_KS,
                       accA.data_ptr<float>(), Dwei.data_ptr<float>(),
                       Uatt.data_ptr<float>(), catt.data_ptr<float>(),
                       cmask_p, (const bf16_t*)ctx_bf.data_ptr(), row_src_p, S,
                       alphas_s.at(t), att_stats.data_ptr<float>(),
                       ctx_part.data_ptr<float>(), B, Ts, A, C, CH, lps);
    // 4) attention pass 2: global softmax statistics, combined context,
    // gate + acc_ctx, normalised alphas + acc_alpha, combined pstate
    hipLaunchKernelGGL(cond_attn_combine_gate, dim3(B, cdiv(C, ATT_THREADS)),
                       dim3(ATT_THREADS), NCH * sizeof(float), stream,
                       att_stats.data_ptr<float>(),
                       ctx_part.data_ptr<float>(), NCH, CH, alphas_s.at(t),
                       accA.data_ptr<float>(), accA_used_s.at(t),
                       ps_part.data_ptr<float>(), PS_KS, pstate_s.at(t), A,
                       Ts, Ucon.data_ptr<float>(), Wcon.data_ptr<float>(),
                       accC.data_ptr<float>(), accC_used_s.at(t),
                       ctxpre_s.at(t), ctxs_s.at(t), hc_bf_p, Hpad, K1, mt, B,
                       C);
    // 5) GRU_1 -> h2: split-K for large K (raises block parallelism 4x),
    // single fused kernel when K is small (split overhead dominates)
    if (K1 >= 2048) {
      hipLaunchKernelGGL(cond_gru1_gemm_splitk, dim3(ngrpH, GRU1_KS),
                         dim3(1024), 0, stream, hc_bf_p,
                         (const bf16_t*)W1pk.data_ptr(),
                         gru1_part.data_ptr<float>(), H, K1, Hpad);
      hipLaunchKernelGGL(cond_gru1_step_pointwise, dim3(cdiv(B * H, 256)),
                         dim3(256), 0, stream, gru1_part.data_ptr<float>(),
                         GRU1_KS, h1_s.at(t), b1.data_ptr<float>(),
                         bx1.data_ptr<float>(), mt, h2_s.at(t),
                         h2bf_s.at((t + 1) % 2), Hpad, saved1_s.at(t), B, H,
                         Hpad);
    } else {
      hipLaunchKernelGGL(cond_gru1_step_fwd, dim3(ngrpH), dim3(1024), 0,
                         stream, hc_bf_p, h1_s.at(t),
                         (const bf16_t*)W1pk.data_ptr(), b1.data_ptr<float>(),
                         bx1.data_ptr<float>(), mt, h2_s.at(t),
                         h2bf_s.at((t + 1) % 2), Hpad, saved1_s.at(t), B, H,
                         K1);
    }
  }
  HIP_CHECK(hipGetLastError());
  return {h2_all, ctxs_all, alphas_all, accC, accA, h1_all, saved2, saved1,
          pstate_all, ctxpre_all, accA_used, accC_used};
}

// ================= host: backward =================
std::vector<torch::Tensor> cond_gru_bwd(
    torch::Tensor dh2_all, c10::optional<torch::Tensor> dctxs_all,
    c10::optional<torch::Tensor> dalphas_all,
    c10::optional<torch::Tensor> daccC_f, c10::optional<torch::Tensor> daccA_f,
    // saved forward state
    torch::Tensor yc, torch::Tensor h1_all, torch::Tensor h2_all,
    torch::Tensor ctxs_all, torch::Tensor alphas_all, torch::Tensor saved2,
    torch::Tensor saved1, torch::Tensor pstate_all, torch::Tensor ctxpre_all,
    torch::Tensor accA_used, torch::Tensor accC_used, torch::Tensor ctx_bf,
    torch::Tensor pctx, torch::Tensor init_state,
    c10::optional<torch::Tensor> mask,
    // packed weights for the in-loop GEMMs
    torch::Tensor U1cat,   // [ngrpH*16][K3Hpad] = [U_1|Ux_1]
    torch::Tensor W1cat,   // [ngrpC*16][K3Hpad] = [W_1|Wx_1]
    torch::Tensor U2cat,   // [ngrpH*16][K3Hpad] = [U|Ux]
    torch::Tensor WattB,   // [ngrpH*16][Apad32] = W_att
    torch::Tensor bx1, torch::Tensor Dwei, torch::Tensor Uatt,
    torch::Tensor Ucon, torch::Tensor Wcon) {
  const int T = dh2_all.size(0), B = dh2_all.size(1), H = dh2_all.size(2);
  const int Ts = ctx_bf.size(0), C = ctx_bf.size(2);
  const int A = Uatt.size(0);
  const int K3Hpad = U1cat.size(1);
  const int Apad32 = WattB.size(1);
  const int ngrpH = cdiv(H, JB);
  const int ngrpC = cdiv(C, JB);
  // what cond_gru_fwd checks, for the tensors this side reads
  TORCH_CHECK(B <= 32, "cond_gru: batch must be <= 32");
  check_scan_input(yc, torch::kBFloat16, "cond_gru yc");
  check_scan_input(saved2, torch::kBFloat16, "cond_gru saved2");
  check_scan_input(ctx_bf, torch::kBFloat16, "cond_gru ctx");
  check_scan_input(pctx, torch::kFloat32, "cond_gru pctx");
  check_packed_weight(U1cat, H, 1, "cond_gru U1cat");
  check_packed_weight(W1cat, C, 1, "cond_gru W1cat");
  check_packed_weight(U2cat, H, 1, "cond_gru U2cat");
  check_packed_weight(WattB, H, 1, "cond_gru WattB");

  auto optsF = dh2_all.options().dtype(torch::kFloat32);
  auto optsB = dh2_all.options().dtype(torch::kBFloat16);
  auto dpre1_all = torch::empty({T, B, 4 * H}, optsB);
  auto dpre2_all = torch::empty({T, B, 4 * H}, optsB);
  auto dctxpre_all = torch::empty({T, B, C}, optsB);
  auto gdUcon = torch::zeros({C}, optsF);
  auto gdWcon = torch::zeros({C}, optsF);
  auto dpstate_all = torch::zeros({T, B, A}, optsF);  // per-chunk atomics
  auto dpctx_acc = torch::zeros({Ts, B, A}, optsF);
  // attention chunking as in the forward, the chunk further capped so the
  // two [CH][A] fp32 tiles fit 60 KB of LDS next to the staged vectors
  const int A4 = (A + 3) & ~3;
  const int lds_floats = 60 * 1024 / (int)sizeof(float);
  TORCH_CHECK(3 * A4 + 2 * 8 * A <= lds_floats,
              "cond_gru_bwd: dim_att too large for the attention tiles");
  const int CH = std::min(attn_chunk_len(B, Ts),
                          ((lds_floats - 3 * A4) / (2 * A)) & ~7);
  const int NCH = cdiv(Ts, CH);
  const int lps = attn_lanes_per_s(CH);
  // dD_wei | dU_att | dc_att: one slot per (b, chunk) block, accumulated
  // over the time loop with plain adds, summed once after it
  auto gslot = torch::zeros({B * NCH, 2 * A + 1}, optsF);

  auto dh_carry = torch::zeros({2, B, H}, optsF);
  auto dh1_buf = torch::zeros({B, H}, optsF);
  auto ddirect_h1 = torch::empty({B, H}, optsF);
  auto ddirect2 = torch::empty({B, H}, optsF);
  auto dctx_dir = torch::empty({B, C}, optsF);
  auto dctxpre_f32 = torch::empty({B, C}, optsF);
  auto daccA = daccA_f.has_value() ? daccA_f->contiguous().to(torch::kFloat32)
                                   : torch::zeros({B, Ts}, optsF);
  auto daccC = daccC_f.has_value() ? daccC_f->contiguous().to(torch::kFloat32)
                                   : torch::zeros({B, C}, optsF);
  auto dal_buf = torch::empty({B, Ts}, optsF);
  auto dstep1 = torch::zeros({32, K3Hpad}, optsB);
  auto dstepC = torch::zeros({32, K3Hpad}, optsB);
  auto dstep2 = torch::zeros({32, K3Hpad}, optsB);
  auto init_f = init_state.contiguous().to(torch::kFloat32);

  const OptF32 mask_f(mask), dctxs_f(dctxs_all), dalpha_f(dalphas_all);

  auto stream = at::cuda::getCurrentCUDAStream().stream();
  auto dh2_c = dh2_all.contiguous().to(torch::kFloat32);
  const int pwH = (int)std::min<long>(512, (((long)B * H) + 255) / 256);
  const int pwHC =
      (int)std::min<long>(512, (((long)B * (H + C)) + 255) / 256);
  const Steps<const float> mask_s(mask_f.t), dctxs_s(dctxs_f.t),
      dalpha_s(dalpha_f.t), dh2_s(dh2_c), h1_s(h1_all), h2_s(h2_all),
      saved1_s(saved1), ctxs_s(ctxs_all), alphas_s(alphas_all),
      pstate_s(pstate_all), accA_used_s(accA_used);
  const Steps<const bf16_t> yc_s(yc), saved2_s(saved2), ctxpre_s(ctxpre_all),
      accC_used_s(accC_used);
  const Steps<bf16_t> dpre1_s(dpre1_all), dpre2_s(dpre2_all),
      dctxpre_s(dctxpre_all);
  const Steps<float> dpstate_s(dpstate_all), dh_carry_s(dh_carry);  // K halves

  for (int t = T - 1; t >= 0; --t) {
    const float* mt = mask_s.at(t);
    const float* h2prev = t == 0 ? init_f.data_ptr<float>() : h2_s.at(t - 1);
    // b1 (fused): GRU_1 pointwise + dctx passthrough
    hipLaunchKernelGGL(cond_gru1_bwd_pointwise, dim3(pwHC), dim3(256), 0,
                       stream, dh_carry_s.at(0), dh_carry_s.at(1),
                       dh2_s.at(t), saved1_s.at(t), h1_s.at(t),
                       bx1.data_ptr<float>(), mt,
                       (bf16_t*)dstep1.data_ptr(), (bf16_t*)dstepC.data_ptr(),
                       K3Hpad, ddirect_h1.data_ptr<float>(), dpre1_s.at(t),
                       dctxs_s.at(t), daccC.data_ptr<float>(),
                       dctx_dir.data_ptr<float>(), C, B, H);
    // b2+b3+b4 fused launch: dh1 = ddirect_h1 + dstep1 @ [U_1|Ux_1]^T and
    // the dctx GEMM with the distraction-gate backward applied in the
    // epilogue (the former separate cond_gate_bwd pass)
    hipLaunchKernelGGL(cond_bwd_gemm_dual_gate,
                       dim3(std::max(ngrpH, ngrpC), 2), dim3(384), 0, stream,
                       (const bf16_t*)dstep1.data_ptr(),
                       (const bf16_t*)U1cat.data_ptr(),
                       ddirect_h1.data_ptr<float>(),
                       dh1_buf.data_ptr<float>(), H,
                       (const bf16_t*)dstepC.data_ptr(),
                       (const bf16_t*)W1cat.data_ptr(),
                       dctx_dir.data_ptr<float>(), C, K3Hpad, ctxs_s.at(t),
                       Ucon.data_ptr<float>(), Wcon.data_ptr<float>(),
                       daccC.data_ptr<float>(), dctxpre_f32.data_ptr<float>(),
                       dctxpre_s.at(t), ctxpre_s.at(t), accC_used_s.at(t),
                       gdUcon.data_ptr<float>(), gdWcon.data_ptr<float>(),
                       B);
    // b5: attention backward — wave-per-(b,s) dalpha, then one pass per
    // (b, s-chunk) block: softmax-bwd dot, dpctx/daccA, and the column
    // sums for dpstate/dD_wei/dU_att/dc_att through an LDS tile
    hipLaunchKernelGGL(cond_attn_bwd_dalpha, dim3(B, cdiv(Ts, 4)),
                       dim3(256), 0, stream,
                       (const bf16_t*)ctx_bf.data_ptr(),
                       dctxpre_f32.data_ptr<float>(), alphas_s.at(t),
                       daccA.data_ptr<float>(), mt, dalpha_s.at(t),
                       dal_buf.data_ptr<float>(), B, Ts, C);
    hipLaunchKernelGGL(cond_attn_bwd_fused, dim3(B, NCH), dim3(ATT_THREADS),
                       (3 * A4 + 2 * CH * A) * sizeof(float), stream,
                       alphas_s.at(t), dal_buf.data_ptr<float>(),
                       pctx.data_ptr<float>(), pstate_s.at(t),
                       accA_used_s.at(t), Dwei.data_ptr<float>(),
                       Uatt.data_ptr<float>(), daccA.data_ptr<float>(),
                       dpctx_acc.data_ptr<float>(), dpstate_s.at(t),
                       gslot.data_ptr<float>(), B, Ts, A, CH, lps);
    // b6a: dh1 += dpstate @ W_att^T — A fragments converted from the
    // fp32 dpstate in-register (no cond_dpstate_cast pass)
    hipLaunchKernelGGL(cond_dh1_att_gemm, dim3(ngrpH), dim3(384), 0, stream,
                       dpstate_s.at(t), (const bf16_t*)WattB.data_ptr(),
                       dh1_buf.data_ptr<float>(), B, H, A, Apad32);
    // b8: GRU_2 pointwise (dh1 -> gate preact grads)
    hipLaunchKernelGGL(nats_gru_step_bwd_pointwise, dim3(pwH), dim3(256), 0,
                       stream, dh1_buf.data_ptr<float>(), nullptr,
                       saved2_s.at(t), yc_s.at(t), h2prev, mt,
                       (bf16_t*)dstep2.data_ptr(), K3Hpad,
                       ddirect2.data_ptr<float>(), dpre2_s.at(t), B, H);
    // b9: dh_{t-1} = [dpr1|dpu1|dpxl1] @ [U|Ux]^T + passthrough, split
    // over K halves written as two partials (summed by the next step's
    // GRU_1 pointwise — no atomics, no zeroing)
    hipLaunchKernelGGL(cond_dh_carry_gemm_split, dim3(ngrpH, 2), dim3(384),
                       0, stream, (const bf16_t*)dstep2.data_ptr(),
                       (const bf16_t*)U2cat.data_ptr(),
                       ddirect2.data_ptr<float>(), dh_carry.data_ptr<float>(),
                       B, H, K3Hpad);
  }
  HIP_CHECK(hipGetLastError());
  auto dh_carry_sum = dh_carry[0] + dh_carry[1];
  auto gsum = gslot.sum(0);
  auto gdDwei = gsum.slice(0, 0, A).contiguous();
  auto gdUatt = gsum.slice(0, A, 2 * A).contiguous();
  auto gdcatt = gsum.slice(0, 2 * A, 2 * A + 1).contiguous();
  return {dpre1_all, dpre2_all, dctxpre_all, gdUcon, dpstate_all,
          dpctx_acc, gdDwei, gdUatt, gdcatt, dh_carry_sum, daccC, daccA,
          gdWcon};
}
