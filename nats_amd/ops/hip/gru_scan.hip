// Fused GRU scan (forward + backward) for CDNA4 / gfx950.
//
// Replaces the reference's per-timestep Theano scan body (gru_layer
// _step_slice, nats.py:336-372; kernel rows K3 in SURVEY §2.4): the three
// recurrent GEMMs h@U_r, h@U_u, h@Ux plus the gate nonlinearities and the
// mask blend are ONE kernel launch per timestep, tiled for MFMA
// (16x16x32 bf16, fp32 accumulate), with the per-step preactivations
// exchanged through LDS between the MFMA phase and the pointwise phase.
//
// Weight packing (python wrapper, ops/gru.py):
//   Upk  : [ngrp*3*16, Hpad] bf16, row = output slot. Workgroup `wg` owns
//          output columns j in [wg*16, wg*16+16); its rows are laid out
//          [r-cols | u-cols | cand-cols] so B-fragments are contiguous
//          16-byte loads (see common.h layout note).
//   Hpad : H rounded up to 32; padded K-regions of every operand are
//          zero-filled so MFMA accumulates exact zeros there.
//
// State: h_all (T,B,H) fp32 is the master hidden sequence; a ping-pong
// pair of [32][Hpad] bf16 buffers mirrors the current h for the next
// step's A-fragments (two buffers: every WG reads ALL columns while
// owning 16, so in-place update would race).
//
// The backward scan (reverse-time) mirrors the split: a pointwise kernel
// turns dh_t into gate-preactivation grads (stored to dpre_all for the
// big time-batched dW/dU GEMMs done by hipBLASLt from python), then an
// MFMA kernel computes the recurrent term dh_{t-1} = [dpr|dpu|dpxl] @
// [U|Ux]^T + passthrough. BPTT semantics = tensor.grad through the scan
// (nats.py:1340). These kernels are shared with the decoder's GRU_2
// (gru_kernels.h).

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "common.h"
#include "grid_barrier.h"
#include "gru_kernels.h"

// ---------------- forward step ----------------
// block: 384 threads = 6 waves; wave w -> (m = w/3, g = w%3) computes the
// 16x16 tile rows [16m,16m+16) of matrix g (0=r,1=u,2=cand).
__device__ __forceinline__ void gru_fwd_body(const GruFwdArgs& a,
                                             int ld_bfout, int B, int H,
                                             int Hpad, int wg) {
  __shared__ float pre[3][32][JB + 1];
  const int wave = threadIdx.x / NATS_WAVE;
  const int m = wave / 3;
  const int g = wave % 3;
  const int j0 = wg * JB;

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const bf16_t* brow = a.Upk + (long)(wg * 3 + g) * JB * Hpad;
  NATS_MFMA_KLOOP(acc, a.h_bf, 16 * m, Hpad, brow, 0, Hpad, 0, Hpad);
  store_cd_lds(pre[g], acc, 16 * m);
  __syncthreads();

  for (int idx = threadIdx.x; idx < B * JB; idx += blockDim.x) {
    const int b = idx / JB;
    const int c = idx % JB;
    const int j = j0 + c;
    if (j >= H) continue;
    gru_fwd_finish(a, ld_bfout, H, b, j, (long)b * H + j, pre[0][b][c],
                   pre[1][b][c], pre[2][b][c]);
  }
}

__global__ __launch_bounds__(384) void nats_gru_step_fwd(
    const bf16_t* __restrict__ h_bf,   // [32][Hpad] current h (bf16)
    const float* __restrict__ h_prev,  // [B][H] fp32 (= h_all[t-1] or h0)
    const bf16_t* __restrict__ Upk,    // [ngrp*3*16][Hpad]
    const bf16_t* __restrict__ xg_t,   // [B][2H] x@W+b at step t
    const bf16_t* __restrict__ xc_t,   // [B][H]  x@Wx+bx at step t
    const float* __restrict__ mask_t,  // [B] or nullptr
    float* __restrict__ h_out,         // [B][H] fp32 (h_all[t])
    bf16_t* __restrict__ h_bf_out,     // bf16 h out, row stride ld_bfout
    int ld_bfout,
    bf16_t* __restrict__ saved_t,      // [B][3H] (r,u,pxl) at step t
    int B, int H, int Hpad) {
  gru_fwd_body(GruFwdArgs{h_bf, h_prev, Upk, xg_t, xc_t, mask_t, h_out,
                          h_bf_out, saved_t},
               ld_bfout, B, H, Hpad, blockIdx.x);
}

// one launch per timestep covers both directions (blockIdx.y)
__global__ __launch_bounds__(384) void nats_gru_step_fwd_bidir(
    GruFwdArgs a0, GruFwdArgs a1, int ld_bfout, int B, int H, int Hpad) {
  gru_fwd_body(blockIdx.y == 0 ? a0 : a1, ld_bfout, B, H, Hpad, blockIdx.x);
}

// ---------------- forward step, split-K (decoder GRU_2) ----------------
// Same math as nats_gru_step_fwd but grid (ngrp, KS): each block computes
// a K-chunk of the three gate GEMMs and stores fp32 partials (no LDS
// exchange needed — one chunk per block); nats_gru2_step_pointwise sums
// the chunks and applies gates. Raises block count 4x for the decoder's
// per-step call (the fused variant ran ngrp=63 blocks, 25% of the chip).
__global__ __launch_bounds__(384) void nats_gru2_gemm_splitk(
    const bf16_t* __restrict__ h_bf,  // [32][Hpad]
    const bf16_t* __restrict__ Upk,   // [ngrp*3*16][Hpad]
    float* __restrict__ part,         // [KS][3][32][Hpad]
    int Hpad) {
  const int wg = blockIdx.x;
  const int ksb = blockIdx.y;
  const int KS = gridDim.y;
  const int wave = threadIdx.x / NATS_WAVE;
  const int m = wave / 3;
  const int g = wave % 3;
  const KRange k = k_part(KRange{0, Hpad}, KS, ksb);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const bf16_t* brow = Upk + (long)(wg * 3 + g) * JB * Hpad;
  NATS_MFMA_KLOOP(acc, h_bf, 16 * m, Hpad, brow, 0, Hpad, k.beg, k.end);
  store_cd_rowmajor(part + ((long)ksb * 3 + g) * 32 * Hpad, acc, 16 * m,
                    Hpad, wg * JB);
}

__global__ void nats_gru2_step_pointwise(
    const float* __restrict__ part,    // [KS][3][32][Hpad]
    int KS,
    const float* __restrict__ h_prev,  // [B][H]
    const bf16_t* __restrict__ xg_t,   // [B][2H]
    const bf16_t* __restrict__ xc_t,   // [B][H]
    const float* __restrict__ mask_t,  // [B] or null
    float* __restrict__ h_out,         // [B][H]
    bf16_t* __restrict__ h_bf_out,     // row stride ld_bfout
    int ld_bfout,
    bf16_t* __restrict__ saved_t,      // [B][3H] (r,u,pxl)
    int B, int H, int Hpad) {
  const long total = (long)B * H;
  for (long idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int b = idx / H;
    const int j = idx % H;
    float p0 = 0.f, p1 = 0.f, p2 = 0.f;
    const long bj = (long)b * Hpad + j;
    for (int k = 0; k < KS; ++k) {
      const float* pk = part + (long)k * 3 * 32 * Hpad;
      p0 += pk[bj];
      p1 += pk[(long)32 * Hpad + bj];
      p2 += pk[(long)2 * 32 * Hpad + bj];
    }
    gru_fwd_finish(GruFwdArgs{nullptr, h_prev, nullptr, xg_t, xc_t, mask_t,
                              h_out, h_bf_out, saved_t},
                   ld_bfout, H, b, j, idx, p0, p1, p2);
  }
}

// ---------------- backward pointwise ----------------
__global__ void nats_gru_step_bwd_pointwise(
    const float* __restrict__ dh_buf,   // [B][H] recurrent dh (from t+1)
    const float* __restrict__ dh_out_t, // [B][H] upstream grad (or null)
    const bf16_t* __restrict__ saved_t, // [B][3H] (r,u,pxl)
    const bf16_t* __restrict__ xc_t,    // [B][H]
    const float* __restrict__ h_prev,   // [B][H]
    const float* __restrict__ mask_t,   // [B] or nullptr
    bf16_t* __restrict__ dstep,         // [32][ld_dstep] [dpr|dpu|dpxl]
    int ld_dstep,
    float* __restrict__ ddirect,        // [B][H]
    bf16_t* __restrict__ dpre_t,        // [B][4H] [dpr|dpu|dpx|dpxl]
    int B, int H) {
  const long total = (long)B * H;
  for (long idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int b = idx / H;
    const int j = idx % H;
    gru_bwd_finish(GruBwdArgs{nullptr, nullptr, dh_out_t, saved_t, xc_t,
                              h_prev, mask_t, dstep, ddirect, dpre_t},
                   ld_dstep, H, b, j, idx, dh_buf[idx]);
  }
}

// ---------------- fused backward step (gemm of t+1's dstep + pointwise)
__device__ __forceinline__ void gru_bwd_fused_body(const GruBwdArgs& a,
                                                   const bf16_t* Ubwd, int B,
                                                   int H, int Kpad, int wg) {
  row_gemm(a.dstep_in, Ubwd, wg * JB, Kpad, KRange{0, Kpad}, B, H,
           [&](int b, int j, float sum) {
             // dh at step t for column j: recurrent + passthrough
             const long bj = (long)b * H + j;
             gru_bwd_finish(a, Kpad, H, b, j, bj, a.ddirect_in[bj] + sum);
           });
}

__global__ __launch_bounds__(384) void nats_gru_step_bwd_fused_bidir(
    GruBwdArgs a0, GruBwdArgs a1, const bf16_t* Ubwd0, const bf16_t* Ubwd1,
    int B, int H, int Kpad) {
  if (blockIdx.y == 0)
    gru_bwd_fused_body(a0, Ubwd0, B, H, Kpad, blockIdx.x);
  else
    gru_bwd_fused_body(a1, Ubwd1, B, H, Kpad, blockIdx.x);
}

// ---------------- persistent bidirectional scans ----------------
// The per-step launches re-read the packed weights from L2 every step
// (~14us/step, latency-bound). The persistent variant stages each
// workgroup's weight slice into LDS ONCE (XOR-swizzled against the
// 16-way ds_read_b128 bank conflict of 2KB row strides, §6 G4) and walks
// all T steps inside one launch, exchanging h through global memory with
// an agent-scope release/acquire grid barrier per step (guide §6 G16:
// placement-independent, bounded spin with a give-up flag the host
// checks — a barrier bug aborts instead of hanging the box).

// stage a [rows][Kpad] bf16 slice into LDS with the (row&15)<<4 byte-XOR
// swizzle; read back with the same XOR (write+read swizzled together).
__device__ __forceinline__ void stage_weights_lds(bf16_t* lds,
                                                  const bf16_t* src,
                                                  int rows, int Kpad) {
  const long total16 = (long)rows * Kpad * 2 / 16;  // 16B chunks
  for (long idx = threadIdx.x; idx < total16; idx += blockDim.x) {
    long byte = idx * 16;
    const int row = (int)(byte / ((long)Kpad * 2));
    const long dst = byte ^ (long)((row & 15) << 4);
    *(uint4*)((char*)lds + dst) = *(const uint4*)((const char*)src + byte);
  }
}

__device__ __forceinline__ bf16x8 frag_bt_lds_swz(const bf16_t* lds, int row,
                                                  int Kpad, int k) {
  const int lane = threadIdx.x & (NATS_WAVE - 1);
  const int r = row + (lane & 15);
  long byte = ((long)r * Kpad + k + (lane >> 4) * 8) * 2;
  byte ^= (long)((r & 15) << 4);
  return *(const bf16x8*)((const char*)lds + byte);
}

// swizzled-LDS MFMA K-loop (B operand from LDS, A from global), 4-deep on
// the A side: four global fragments stay in flight ahead of each MFMA so
// the post-acquire (L1-cold) L2 latency amortises over 4 iterations.
#define NATS_MFMA_KLOOP_LDSB(ACC, APTR, AROW, ALD, LDSB, BROW, BLD, KBEG,    \
                             KEND)                                           \
  do {                                                                       \
    const int _ke = (KEND);                                                  \
    int _k = (KBEG);                                                         \
    if (_k + 128 <= _ke) {                                                   \
      bf16x8 _a0 = frag_a_rowmajor((APTR), (AROW), (ALD), _k);               \
      bf16x8 _a1 = frag_a_rowmajor((APTR), (AROW), (ALD), _k + 32);          \
      bf16x8 _a2 = frag_a_rowmajor((APTR), (AROW), (ALD), _k + 64);          \
      bf16x8 _a3 = frag_a_rowmajor((APTR), (AROW), (ALD), _k + 96);          \
      for (_k += 128; _k + 32 <= _ke; _k += 32) {                            \
        bf16x8 _an = frag_a_rowmajor((APTR), (AROW), (ALD), _k);             \
        bf16x8 _b = frag_bt_lds_swz((LDSB), (BROW), (BLD), _k - 128);        \
        ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(_a0, _b, ACC, 0, 0, 0);\
        _a0 = _a1; _a1 = _a2; _a2 = _a3; _a3 = _an;                          \
      }                                                                      \
      {                                                                      \
        bf16x8 _b = frag_bt_lds_swz((LDSB), (BROW), (BLD), _k - 128);        \
        ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(_a0, _b, ACC, 0, 0, 0);\
        _b = frag_bt_lds_swz((LDSB), (BROW), (BLD), _k - 96);                \
        ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(_a1, _b, ACC, 0, 0, 0);\
        _b = frag_bt_lds_swz((LDSB), (BROW), (BLD), _k - 64);                \
        ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(_a2, _b, ACC, 0, 0, 0);\
        _b = frag_bt_lds_swz((LDSB), (BROW), (BLD), _k - 32);                \
        ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(_a3, _b, ACC, 0, 0, 0);\
      }                                                                      \
    } else {                                                                 \
      for (; _k < _ke; _k += 32) {                                           \
        bf16x8 _a0 = frag_a_rowmajor((APTR), (AROW), (ALD), _k);             \
        bf16x8 _b0 = frag_bt_lds_swz((LDSB), (BROW), (BLD), _k);             \
        ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(_a0, _b0, ACC, 0, 0, 0);\
      }                                                                      \
    }                                                                        \
  } while (0)

// One persistent-scan job = one (direction, batch-chunk): pointers are
// pre-offset to the chunk's first row and strides skip the FULL batch
// per timestep, so jobs of a B>32 call share the (T, Btot, ...) output
// tensors without copies. Up to 4 jobs run concurrently in one launch
// (2 directions x 2 chunks of the 32-row MFMA tiling).
struct GruPersistFwd {
  const bf16_t* xg;    // -> [t][b][2H] rows of this chunk
  const bf16_t* xc;
  const float* mask;   // or null
  const bf16_t* Upk;   // [ngrp*3*16][Hpad]
  float* h_all;
  bf16_t* h_bf;        // [2][32][Hpad] ping-pong (per job)
  bf16_t* saved;
  const float* h0;     // [B][H] chunk rows (contiguous)
  int B;               // rows in this chunk (<= 32)
  long sxg, sxc, smask, sh, ssaved;  // per-t element strides
};

// XCD-preferred direction claim (profiles/barrier_xcd.json: a 63-WG
// barrier costs 5.97us with blocks spread over all 8 XCDs but 3.66us
// confined to 4 — and confinement also keeps each direction's h-exchange
// lines in fewer L2s). The grid is overprovisioned (gridDim.x = 256, all
// resident at <=150KB LDS); each block claims a (direction, column-tile)
// slot with direction 0 preferred on XCDs 0-3 and direction 1 on 4-7; a
// block whose preferred side is full backs off briefly, then steals from
// the other side (correct under any placement — the barrier census is
// placement-independent); unclaimed blocks exit. Greedy claiming has NO
// census spin, so there is no new hang mode.
__device__ __forceinline__ int nats_claim_job_slot(unsigned* claim,
                                                   int ngrp, int njobs,
                                                   int xpj) {
  __shared__ int sh_sel;
  if (threadIdx.x == 0) {
    const unsigned xcc = nats_xcc_id();
    // xpj = preferred XCDs per job; jobs partition the first njobs*xpj
    // XCDs, blocks elsewhere have no preference
    int job = (xcc < (unsigned)(njobs * xpj)) ? (int)(xcc / xpj) : -1;
    int slot = -1;
    if (job >= 0) {
      const unsigned s0 = __hip_atomic_fetch_add(
          claim + job, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (s0 < (unsigned)ngrp) slot = (int)s0;
    }
    if (slot < 0) {
      // unpreferred block (or preferred job full): let the preferred
      // blocks claim first, then fill leftovers round-robin
      for (int i = 0; i < 6; ++i) __builtin_amdgcn_s_sleep(127);
      const int first = (job >= 0) ? (job + 1) % njobs
                                   : (int)(xcc % (unsigned)njobs);
      for (int k = 0; k < njobs && slot < 0; ++k) {
        const int d2 = (first + k) % njobs;
        const unsigned s1 = __hip_atomic_fetch_add(
            claim + d2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (s1 < (unsigned)ngrp) {
          job = d2;
          slot = (int)s1;
        }
      }
    }
    sh_sel = (slot < 0) ? -1 : (job << 16 | slot);
  }
  __syncthreads();
  return sh_sel;
}

// Entry of both persistent kernels once a block holds claim `sel` (= job
// << 16 | tile): move `sync` to the job's own barrier slab (jobs are
// data-independent: each syncs only its own ngrp blocks), stage the tile's
// weight rows in LDS, run the barrier census. False if the census gave up.
// (The job pick stays a reference ternary in each kernel: through a helper
// the four by-value job structs are copied into registers and spill.)
__device__ __forceinline__ bool persist_enter(unsigned*& sync, int sel,
                                              int ngrp, bf16_t* w_lds,
                                              const bf16_t* w_tile, int rows,
                                              int K, NatsBarrierCtx& bctx) {
  sync += (long)(sel >> 16) * NATS_SYNC_WORDS;
  stage_weights_lds(w_lds, w_tile, rows, K);
  __syncthreads();
  return nats_barrier_init(sync, (unsigned)ngrp, bctx);
}

__global__ __launch_bounds__(384) void nats_gru_persistent_fwd(
    GruPersistFwd p0, GruPersistFwd p1, GruPersistFwd p2, GruPersistFwd p3,
    int T, int H, int Hpad, unsigned* sync, int ngrp, int njobs, int xpd) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* upk_lds = (bf16_t*)smem;                       // [3*16][Hpad] swz
  float(*pre)[32][JB + 1] =
      (float(*)[32][JB + 1])(smem + (long)3 * JB * Hpad * 2);

  const int sel = nats_claim_job_slot(sync + (long)njobs * NATS_SYNC_WORDS,
                                      ngrp, njobs, xpd);
  if (sel < 0) return;
  const int jobsel = sel >> 16;
  const GruPersistFwd& p = (jobsel == 0) ? p0
                           : (jobsel == 1) ? p1
                           : (jobsel == 2) ? p2 : p3;
  const int wg = sel & 0xffff;
  const int B = p.B;
  NatsBarrierCtx bctx;
  if (!persist_enter(sync, sel, ngrp, upk_lds,
                     p.Upk + (long)wg * 3 * JB * Hpad, 3 * JB, Hpad, bctx)) {
    if (threadIdx.x == 0) p.h_all[0] = __builtin_nanf("");
    return;
  }

  const int wave = threadIdx.x / NATS_WAVE;
  const int m = wave / 3;
  const int g = wave % 3;
  const int j0 = wg * JB;
  const long hb = (long)32 * Hpad;

  // register-carry of this thread's own h columns (column-local: the same
  // thread wrote them last step) — removes an L2 round trip per step
  float h_keep[2];
  int own_b[2], own_j[2];
  bool own[2];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int idx = threadIdx.x + it * blockDim.x;
    own_b[it] = idx / JB;
    own_j[it] = j0 + idx % JB;
    own[it] = (idx < B * JB) && (own_j[it] < H);
    h_keep[it] = own[it] ? p.h0[(long)own_b[it] * H + own_j[it]] : 0.f;
  }
  // deferred saved-writes (not read in-kernel: flushed during the NEXT
  // step so their store latency never sits inside the barrier drain)
  float pend_r[2], pend_u[2], pend_px[2];
  bool have_pend = false;
  bf16_t* pend_saved = nullptr;

  for (int t = 0; t < T; ++t) {
    // prefetch this step's inputs; latency hides under the MFMA phase
    const bf16_t* xg_t = p.xg + (long)t * p.sxg;
    const bf16_t* xc_t = p.xc + (long)t * p.sxc;
    float pf_xr[2], pf_xu[2], pf_xc[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      if (own[it]) {
        const long b2 = (long)own_b[it] * 2 * H;
        pf_xr[it] = (float)xg_t[b2 + own_j[it]];
        pf_xu[it] = (float)xg_t[b2 + H + own_j[it]];
        pf_xc[it] = (float)xc_t[(long)own_b[it] * H + own_j[it]];
      }
    }
    // flush the previous step's saved gates (plenty of slack before the
    // next barrier drain)
    if (have_pend) {
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        if (own[it]) {
          const long s3 = (long)own_b[it] * 3 * H + own_j[it];
          pend_saved[s3] = (bf16_t)pend_r[it];
          pend_saved[s3 + H] = (bf16_t)pend_u[it];
          pend_saved[s3 + 2 * H] = (bf16_t)pend_px[it];
        }
      }
    }

    const bf16_t* h_bf_in = p.h_bf + (t % 2) * hb;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    NATS_MFMA_KLOOP_LDSB(acc, h_bf_in, 16 * m, Hpad, upk_lds, g * JB, Hpad,
                         0, Hpad);
    store_cd_lds(pre[g], acc, 16 * m);
    __syncthreads();

    const float* mask_t = p.mask ? p.mask + (long)t * p.smask : nullptr;
    float* h_out = p.h_all + (long)t * p.sh;
    bf16_t* h_bf_out = p.h_bf + ((t + 1) % 2) * hb;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      if (!own[it]) continue;
      const int b = own_b[it];
      const int c = (threadIdx.x + it * blockDim.x) % JB;
      const int j = own_j[it];
      const float hp = h_keep[it];
      const float pr = pre[0][b][c] + pf_xr[it];
      const float pu = pre[1][b][c] + pf_xu[it];
      const float px = pre[2][b][c];
      const GruCellFwd o =
          gru_cell_fwd(pr, pu, px, pf_xc[it], hp, mask_t, b);
      h_keep[it] = o.hnew;
      h_out[(long)b * H + j] = o.hnew;
      h_bf_out[(long)b * Hpad + j] = (bf16_t)o.hnew;
      pend_r[it] = o.r;
      pend_u[it] = o.u;
      pend_px[it] = px;
    }
    pend_saved = p.saved + (long)t * p.ssaved;
    have_pend = true;
    if (!nats_grid_barrier(sync, (unsigned)(t + 1), bctx)) {
      // poison output so a barrier give-up surfaces as NaN, never a hang
      if (threadIdx.x == 0) p.h_all[0] = __builtin_nanf("");
      return;
    }
  }
  // flush the last step's saved gates
  if (have_pend) {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      if (own[it]) {
        const long s3 = (long)own_b[it] * 3 * H + own_j[it];
        pend_saved[s3] = (bf16_t)pend_r[it];
        pend_saved[s3 + H] = (bf16_t)pend_u[it];
        pend_saved[s3 + 2 * H] = (bf16_t)pend_px[it];
      }
    }
  }
}

struct GruPersistBwd {
  const float* dh_out;  // -> [t][b][H] rows of this chunk
  const float* h_all;
  const bf16_t* saved;
  const bf16_t* xc;
  const float* mask;    // or null
  const bf16_t* Ubwd;   // [ngrp*16][K3pad]
  bf16_t* dstep;        // [2][32][K3pad] ping-pong (zeroed, per job)
  float* ddirect;       // [B][H] (zeroed, per job)
  bf16_t* dpre;
  const float* h0;      // [B][H] chunk rows (contiguous)
  int B;
  long sdh, sh, ssaved, sxc, smask, sdpre;  // per-t element strides
};

__global__ __launch_bounds__(384) void nats_gru_persistent_bwd(
    GruPersistBwd p0, GruPersistBwd p1, GruPersistBwd p2, GruPersistBwd p3,
    int T, int H, int K3pad, unsigned* sync, int ngrp, int njobs, int xpd) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* ub_lds = (bf16_t*)smem;  // [16][K3pad] swizzled
  float(*part)[32][JB + 1] =
      (float(*)[32][JB + 1])(smem + (long)JB * K3pad * 2);

  const int sel = nats_claim_job_slot(sync + (long)njobs * NATS_SYNC_WORDS,
                                      ngrp, njobs, xpd);
  if (sel < 0) return;
  const int jobsel = sel >> 16;
  const GruPersistBwd& p = (jobsel == 0) ? p0
                           : (jobsel == 1) ? p1
                           : (jobsel == 2) ? p2 : p3;
  const int wg = sel & 0xffff;
  const int B = p.B;
  NatsBarrierCtx bctx;
  if (!persist_enter(sync, sel, ngrp, ub_lds, p.Ubwd + (long)wg * JB * K3pad,
                     JB, K3pad, bctx)) {
    if (threadIdx.x == 0) p.ddirect[0] = __builtin_nanf("");
    return;
  }

  const int wave = threadIdx.x / NATS_WAVE;
  const int m = wave / 3;
  const int ks = wave % 3;
  const int i0 = wg * JB;
  // k_part(KRange{0, K3pad}, 3, ks) with an unclamped kbeg: the clamp's
  // extra v_min moves this kernel's register allocation
  const int kchunk = ((K3pad / 3 + 31) / 32) * 32;
  const int kbeg = ks * kchunk;
  const int kend = min(K3pad, (ks + 1) * kchunk);
  const long ds = (long)32 * K3pad;

  // register-carry of this thread's ddirect columns (column-local; the
  // global copy is still written — the host's final dh0 GEMM reads it)
  float dd_keep[2] = {0.f, 0.f};
  int own_b[2], own_j[2];
  bool own[2];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int idx = threadIdx.x + it * blockDim.x;
    own_b[it] = idx / JB;
    own_j[it] = i0 + idx % JB;
    own[it] = (idx < B * JB) && (own_j[it] < H);
  }
  // deferred dpre writes (only consumed by the host's time-batched GEMMs)
  float pend[2][4];
  bool have_pend = false;
  bf16_t* pend_dpre = nullptr;

  for (int t = T - 1; t >= 0; --t) {
    // prefetch this step's pointwise inputs under the MFMA phase
    const bf16_t* saved_t = p.saved + (long)t * p.ssaved;
    const bf16_t* xc_t = p.xc + (long)t * p.sxc;
    const float* h_prev =
        (t == 0) ? p.h0 : (p.h_all + (long)(t - 1) * p.sh);
    const float* dh_out_t = p.dh_out + (long)t * p.sdh;
    float pf_r[2], pf_u[2], pf_px[2], pf_xc[2], pf_hp[2], pf_dho[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      if (own[it]) {
        const long bj = (long)own_b[it] * H + own_j[it];
        const long s3 = (long)own_b[it] * 3 * H + own_j[it];
        pf_r[it] = (float)saved_t[s3];
        pf_u[it] = (float)saved_t[s3 + H];
        pf_px[it] = (float)saved_t[s3 + 2 * H];
        pf_xc[it] = (float)xc_t[bj];
        pf_hp[it] = h_prev[bj];
        pf_dho[it] = dh_out_t[bj];
      }
    }
    if (have_pend) {
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        if (own[it]) {
          const long d4 = (long)own_b[it] * 4 * H + own_j[it];
          pend_dpre[d4] = (bf16_t)pend[it][0];
          pend_dpre[d4 + H] = (bf16_t)pend[it][1];
          pend_dpre[d4 + 2 * H] = (bf16_t)pend[it][2];
          pend_dpre[d4 + 3 * H] = (bf16_t)pend[it][3];
        }
      }
    }

    const bf16_t* dstep_in = p.dstep + ((t + 1) % 2) * ds;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    NATS_MFMA_KLOOP_LDSB(acc, dstep_in, 16 * m, K3pad, ub_lds, 0, K3pad,
                         kbeg, kend);
    store_cd_lds(part[ks], acc, 16 * m);
    __syncthreads();

    const float* mask_t = p.mask ? p.mask + (long)t * p.smask : nullptr;
    bf16_t* dstep_out = p.dstep + (t % 2) * ds;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      if (!own[it]) continue;
      const int b = own_b[it];
      const int c = (threadIdx.x + it * blockDim.x) % JB;
      const int j = own_j[it];
      const long bj = (long)b * H + j;
      float dh = dd_keep[it] + part[0][b][c] + part[1][b][c] +
                 part[2][b][c] + pf_dho[it];
      const float r = pf_r[it];
      const float u = pf_u[it];
      const float px = pf_px[it];
      const float hbar = tanhf(px * r + pf_xc[it]);
      const float hp = pf_hp[it];
      const float mm = (mask_t != nullptr) ? mask_t[b] : 1.f;
      const GruCellBwd o = gru_cell_bwd(dh, r, u, px, hbar, hp, mm);
      dd_keep[it] = o.ddirect;
      p.ddirect[bj] = o.ddirect;
      dstep_out[(long)b * K3pad + j] = (bf16_t)o.dpr;
      dstep_out[(long)b * K3pad + H + j] = (bf16_t)o.dpu;
      dstep_out[(long)b * K3pad + 2 * H + j] = (bf16_t)o.dpxl;
      pend[it][0] = o.dpr;
      pend[it][1] = o.dpu;
      pend[it][2] = o.dpx;
      pend[it][3] = o.dpxl;
    }
    pend_dpre = p.dpre + (long)t * p.sdpre;
    have_pend = true;
    if (!nats_grid_barrier(sync, (unsigned)(T - t), bctx)) {
      if (threadIdx.x == 0) p.ddirect[0] = __builtin_nanf("");
      return;
    }
  }
  if (have_pend) {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      if (own[it]) {
        const long d4 = (long)own_b[it] * 4 * H + own_j[it];
        pend_dpre[d4] = (bf16_t)pend[it][0];
        pend_dpre[d4 + H] = (bf16_t)pend[it][1];
        pend_dpre[d4 + 2 * H] = (bf16_t)pend[it][2];
        pend_dpre[d4 + 3 * H] = (bf16_t)pend[it][3];
      }
    }
  }
}

// ---------------- backward recurrent GEMM ----------------
// out[b, i] = ddirect[b, i] + sum_k dstep[b, k] * Wt[i, k]
// Generic over the output width (rows of Wt): the encoder/GRU_2 call has
// Wt = [U|Ux] (H x 3Hpad); the decoder reuses it with Wt = [W_1|Wx_1]
// (C rows) and Wt = W_att (K = Apad).
__global__ __launch_bounds__(384) void nats_gru_step_bwd_gemm(
    const bf16_t* __restrict__ dstep,  // [32][Kpad]
    const bf16_t* __restrict__ Wt,     // [ngrp*16][Kpad]
    const float* __restrict__ ddirect, // [B][H]
    float* __restrict__ out,           // [B][H] (may alias ddirect)
    int B, int H, int Kpad) {
  row_gemm(dstep, Wt, blockIdx.x * JB, Kpad, KRange{0, Kpad}, B, H,
           [&](int b, int i, float sum) {
             out[(long)b * H + i] = ddirect[(long)b * H + i] + sum;
           });
}

// ---------------- host drivers ----------------

// entry checks of the forward / backward scans (one direction's tensors)
static void check_scan_fwd_args(const torch::Tensor& xg,
                                const torch::Tensor& xc,
                                const torch::Tensor& Upk) {
  check_scan_input(xg, torch::kBFloat16, "gru_scan xg");
  check_scan_input(xc, torch::kBFloat16, "gru_scan xc");
  TORCH_CHECK(xg.size(2) == 2 * xc.size(2));
  check_packed_weight(Upk, xc.size(2), 3, "gru_scan Upk");
}

static void check_scan_bwd_args(const torch::Tensor& dh_out,
                                const torch::Tensor& saved,
                                const torch::Tensor& xc,
                                const torch::Tensor& Ubwd) {
  check_scan_input(dh_out, torch::kFloat32, "gru_scan dh_out");
  check_scan_input(saved, torch::kBFloat16, "gru_scan saved");
  check_scan_input(xc, torch::kBFloat16, "gru_scan xc");
  check_packed_weight(Ubwd, dh_out.size(2), 1, "gru_scan Ubwd");
}

std::vector<torch::Tensor> gru_scan_fwd(torch::Tensor xg, torch::Tensor xc,
                                        c10::optional<torch::Tensor> mask,
                                        torch::Tensor Upk,
                                        c10::optional<torch::Tensor> h0) {
  check_scan_fwd_args(xg, xc, Upk);
  const int T = xg.size(0), B = xg.size(1), H = xc.size(2);
  TORCH_CHECK(B <= 32, "gru_scan: batch per step must be <= 32 (got ", B,
              "); use more DP ranks or smaller micro-batches");
  const int Hpad = Upk.size(1);
  const int ngrp = cdiv(H, JB);

  auto optsF = xg.options().dtype(torch::kFloat32);
  auto optsB = xg.options();
  auto h_all = torch::empty({T, B, H}, optsF);
  auto saved = torch::empty({T, B, 3 * H}, optsB);
  auto h_bf = torch::zeros({2, 32, Hpad}, optsB);  // ping-pong
  torch::Tensor hprev0;
  if (h0.has_value()) {
    hprev0 = h0->contiguous().to(torch::kFloat32);
    h_bf[0].slice(0, 0, B).slice(1, 0, H).copy_(hprev0.to(torch::kBFloat16));
  } else {
    hprev0 = torch::zeros({B, H}, optsF);
  }
  const OptF32 mask_f(mask);

  auto stream = at::cuda::getCurrentCUDAStream().stream();
  const Steps<const bf16_t> xg_s(xg), xc_s(xc);
  const Steps<const float> mask_s(mask_f.t);
  const Steps<float> h_s(h_all);
  const Steps<bf16_t> saved_s(saved), hbf_s(h_bf);
  for (int t = 0; t < T; ++t) {
    hipLaunchKernelGGL(nats_gru_step_fwd, dim3(ngrp), dim3(384), 0, stream,
                       hbf_s.at(t % 2),
                       t == 0 ? hprev0.data_ptr<float>() : h_s.at(t - 1),
                       (const bf16_t*)Upk.data_ptr(), xg_s.at(t), xc_s.at(t),
                       mask_s.at(t), h_s.at(t), hbf_s.at((t + 1) % 2), Hpad,
                       saved_s.at(t), B, H, Hpad);
  }
  HIP_CHECK(hipGetLastError());
  return {h_all, saved};
}

// ---------------- persistent-scan plan ----------------
// Both persistent kernels launch this many blocks; every (job, column-tile)
// slot needs a block of its own, all resident at once.
constexpr int NATS_PERSIST_GRID = 256;
constexpr size_t NATS_PERSIST_SMEM_MAX = 150 * 1024;  // >= 1 block per CU
constexpr int NATS_PERSIST_MAX_JOBS = 4;
// per-job claim counters, after the jobs' barrier slabs in the sync tensor
constexpr int NATS_CLAIM_WORDS = 8;

// The one place that decides whether (H, B) runs on the persistent scans
// and with which geometry: jobs = directions x 32-row batch chunks
// (B <= 64), all concurrent in ONE launch with per-job barriers — a 64-row
// batch costs the same T barrier intervals as a 32-row one instead of 2x.
struct GruPersistPlan {
  bool ok;
  int ngrp, njobs;
  int xpd;  // preferred XCDs per job (nats_claim_job_slot)
  size_t smem_fwd, smem_bwd;
};

static GruPersistPlan gru_persist_plan(int H, int B) {
  GruPersistPlan p;
  const size_t Hpad = cdiv(H, 32) * 32, K3pad = cdiv(3 * H, 32) * 32;
  const size_t tiles = sizeof(float) * 3 * 32 * (JB + 1);
  p.ngrp = cdiv(H, JB);
  p.njobs = 2 * cdiv(B, 32);
  p.smem_fwd = 3 * JB * Hpad * 2 + tiles;  // [3*16][Hpad] bf16 + pre
  p.smem_bwd = JB * K3pad * 2 + tiles;     // [16][K3pad] bf16 + part
  // 2 XCDs (64 CUs) per job when its grid fits comfortably (LCSTS
  // ngrp=32: +2.5% measured); 4 when 63 WGs would sit 1/CU
  p.xpd = p.njobs == 4 ? 2 : (p.ngrp <= 48 ? 2 : 4);
  if (const char* xpd_env = getenv("NATS_XPD")) {
    // the claim divides an XCC id by it: 0 or garbage must not get there
    char* end = nullptr;
    const long v = strtol(xpd_env, &end, 10);
    TORCH_CHECK(end != xpd_env && *end == '\0' && v >= 1 && v <= 8,
                "NATS_XPD must be an integer in [1, 8], got '", xpd_env, "'");
    p.xpd = (int)v;
  }
  p.ok = p.njobs <= NATS_PERSIST_MAX_JOBS && 2 * p.ngrp <= 192 &&
         p.njobs * p.ngrp <= NATS_PERSIST_GRID &&
         p.smem_fwd <= NATS_PERSIST_SMEM_MAX &&
         p.smem_bwd <= NATS_PERSIST_SMEM_MAX &&
         getenv("NATS_NO_PERSISTENT") == nullptr;
  return p;
}

// Can the persistent bidirectional scans take this hidden size and batch?
bool gru_persistent_ok(long H, long B) {
  return gru_persist_plan((int)H, (int)B).ok;
}

// Job j of a bidirectional scan -> direction d, first batch row a, rows;
// directions interleave so one direction's chunk pairs sit on far XCD sets.
// The per-step path runs jobs 0 and 1 (one per direction, all rows).
struct GruJob { int d, a, rows; };
static GruJob gru_job(int j, int B) {
  const int a = (j >> 1) * 32;
  return GruJob{j & 1, a, std::min(32, B - a)};
}

// zeroed sync tensor of a launch: a barrier slab per job, then the claims
static torch::Tensor persist_sync(int njobs, const torch::Tensor& like) {
  return torch::zeros({njobs * NATS_SYNC_WORDS + NATS_CLAIM_WORDS},
                      like.options().dtype(torch::kInt32));
}

// Bidirectional encoder forward: the persistent launch when the plan
// allows it, else one launch per timestep covering both directions
// (grid.y = direction). h0 = 0 (nats.py:360).
std::vector<torch::Tensor> gru_scan_fwd_bidir(
    torch::Tensor xg0, torch::Tensor xc0, c10::optional<torch::Tensor> mask0,
    torch::Tensor Upk0, torch::Tensor xg1, torch::Tensor xc1,
    c10::optional<torch::Tensor> mask1, torch::Tensor Upk1) {
  check_scan_fwd_args(xg0, xc0, Upk0);
  check_scan_fwd_args(xg1, xc1, Upk1);
  const int T = xg0.size(0), B = xg0.size(1), H = xc0.size(2);
  TORCH_CHECK(B <= 64, "bidir gru_scan: batch must be <= 64");
  const int Hpad = Upk0.size(1);
  const GruPersistPlan plan = gru_persist_plan(H, B);
  const int ngrp = plan.ngrp;

  auto optsF = xg0.options().dtype(torch::kFloat32);
  auto optsB = xg0.options();
  const torch::Tensor xg[2] = {xg0, xg1}, xc[2] = {xc0, xc1};
  const bf16_t* Upk[2] = {(const bf16_t*)Upk0.data_ptr(),
                          (const bf16_t*)Upk1.data_ptr()};
  const OptF32 mask[2] = {OptF32(mask0), OptF32(mask1)};
  torch::Tensor h_all[2], saved[2];
  for (int d = 0; d < 2; ++d) {
    h_all[d] = torch::empty({T, B, H}, optsF);
    saved[d] = torch::empty({T, B, 3 * H}, optsB);
  }
  auto h00 = torch::zeros({B, H}, optsF);
  const Steps<float> h00_rows(h00);
  auto stream = at::cuda::getCurrentCUDAStream().stream();

  if (plan.ok) {  // weight slices LDS-resident across all T steps
    const int njobs = plan.njobs;
    auto sync = persist_sync(njobs, xg0);
    auto h_bfj = torch::zeros({njobs, 2, 32, Hpad}, optsB);
    const Steps<bf16_t> hbf_jobs(h_bfj);
    GruPersistFwd jobs[NATS_PERSIST_MAX_JOBS];
    for (int j = 0; j < njobs; ++j) {
      const GruJob jb = gru_job(j, B);
      const int d = jb.d;
      const Steps<const bf16_t> xg_s(xg[d], jb.a), xc_s(xc[d], jb.a);
      const Steps<const float> mask_s(mask[d].t, jb.a);
      const Steps<float> h_s(h_all[d], jb.a);
      const Steps<bf16_t> saved_s(saved[d], jb.a);
      jobs[j] = GruPersistFwd{
          xg_s.base, xc_s.base, mask_s.base, Upk[d], h_s.base,
          hbf_jobs.at(j), saved_s.base, h00_rows.at(jb.a), jb.rows,
          xg_s.stride, xc_s.stride, mask_s.stride, h_s.stride,
          saved_s.stride};
    }
    for (int j = njobs; j < NATS_PERSIST_MAX_JOBS; ++j) jobs[j] = jobs[0];
    // overprovisioned 1-D grid: blocks self-select a (job, tile) slot
    // with XCD preference (see nats_claim_job_slot)
    hipLaunchKernelGGL(nats_gru_persistent_fwd, dim3(NATS_PERSIST_GRID),
                       dim3(384), plan.smem_fwd, stream, jobs[0], jobs[1],
                       jobs[2], jobs[3], T, H, Hpad,
                       (unsigned*)sync.data_ptr<int>(), ngrp, njobs,
                       plan.xpd);
    HIP_CHECK(hipGetLastError());
    return {h_all[0], saved[0], h_all[1], saved[1]};
  }

  TORCH_CHECK(B <= 32,
              "bidir scan: B > 32 requires the persistent path "
              "(gru_persistent_ok)");
  auto h_bf = torch::zeros({2 * 2, 32, Hpad}, optsB);  // [dir][pingpong]
  const Steps<bf16_t> hbf_s(h_bf);
  for (int t = 0; t < T; ++t) {
    auto args = [&](int d) {
      const Steps<float> h_s(h_all[d]);
      return GruFwdArgs{
          hbf_s.at(2 * d + t % 2), t == 0 ? h00_rows.base : h_s.at(t - 1),
          Upk[d], Steps<const bf16_t>(xg[d]).at(t),
          Steps<const bf16_t>(xc[d]).at(t),
          Steps<const float>(mask[d].t).at(t), h_s.at(t),
          hbf_s.at(2 * d + (t + 1) % 2), Steps<bf16_t>(saved[d]).at(t)};
    };
    hipLaunchKernelGGL(nats_gru_step_fwd_bidir, dim3(ngrp, 2), dim3(384), 0,
                       stream, args(0), args(1), Hpad, B, H, Hpad);
  }
  HIP_CHECK(hipGetLastError());
  return {h_all[0], saved[0], h_all[1], saved[1]};
}

// Bidirectional backward: the persistent launch, else one fused launch per
// timestep (both directions, gemm-of-previous-dstep + pointwise, SURVEY
// §2.4 backward of K3); then dh0 = ddirect(0) + dstep(0) @ Ubwd^T.
std::vector<torch::Tensor> gru_scan_bwd_bidir(
    torch::Tensor dh_out0, torch::Tensor h_all0, torch::Tensor saved0,
    torch::Tensor xc0, c10::optional<torch::Tensor> mask0,
    torch::Tensor Ubwd0, torch::Tensor dh_out1, torch::Tensor h_all1,
    torch::Tensor saved1, torch::Tensor xc1,
    c10::optional<torch::Tensor> mask1, torch::Tensor Ubwd1) {
  check_scan_bwd_args(dh_out0, saved0, xc0, Ubwd0);
  check_scan_bwd_args(dh_out1, saved1, xc1, Ubwd1);
  const int T = dh_out0.size(0), B = dh_out0.size(1), H = dh_out0.size(2);
  const int K3pad = Ubwd0.size(1);
  const GruPersistPlan plan = gru_persist_plan(H, B);
  const int ngrp = plan.ngrp;

  auto optsF = dh_out0.options();
  auto optsB = dh_out0.options().dtype(torch::kBFloat16);
  const torch::Tensor dh_out[2] = {dh_out0, dh_out1};
  const torch::Tensor h_all[2] = {h_all0, h_all1}, saved[2] = {saved0, saved1};
  const torch::Tensor xc[2] = {xc0, xc1};
  const bf16_t* Ubwd[2] = {(const bf16_t*)Ubwd0.data_ptr(),
                           (const bf16_t*)Ubwd1.data_ptr()};
  const OptF32 mask[2] = {OptF32(mask0), OptF32(mask1)};
  torch::Tensor dpre[2], dh0[2];
  for (int d = 0; d < 2; ++d) {
    dpre[d] = torch::empty({T, B, 4 * H}, optsB);
    dh0[d] = torch::empty({B, H}, optsF);
  }
  auto h00 = torch::zeros({B, H}, optsF);
  const Steps<const float> h00_rows(h00);
  auto stream = at::cuda::getCurrentCUDAStream().stream();

  // one job per (direction, 32-row chunk) on the persistent path, one per
  // direction on the per-step path; each owns a dstep ping-pong pair and a
  // ddirect slab
  const int njobs = plan.ok ? plan.njobs : 2;
  auto dstep = torch::zeros({njobs * 2, 32, K3pad}, optsB);  // [job][pingpong]
  auto ddir = torch::zeros({njobs, (plan.ok ? 32 : B) * H}, optsF);
  const Steps<bf16_t> dstep_s(dstep);
  const Steps<float> ddir_s(ddir);

  if (plan.ok) {
    auto sync = persist_sync(njobs, dh_out0);
    GruPersistBwd jobs[NATS_PERSIST_MAX_JOBS];
    for (int j = 0; j < njobs; ++j) {
      const GruJob jb = gru_job(j, B);
      const int d = jb.d;
      const Steps<const float> dh_s(dh_out[d], jb.a), h_s(h_all[d], jb.a);
      const Steps<const bf16_t> saved_s(saved[d], jb.a), xc_s(xc[d], jb.a);
      const Steps<const float> mask_s(mask[d].t, jb.a);
      const Steps<bf16_t> dpre_s(dpre[d], jb.a);
      jobs[j] = GruPersistBwd{
          dh_s.base, h_s.base, saved_s.base, xc_s.base, mask_s.base, Ubwd[d],
          dstep_s.at(2 * j), ddir_s.at(j), dpre_s.base, h00_rows.at(jb.a),
          jb.rows, dh_s.stride, h_s.stride, saved_s.stride, xc_s.stride,
          mask_s.stride, dpre_s.stride};
    }
    for (int j = njobs; j < NATS_PERSIST_MAX_JOBS; ++j) jobs[j] = jobs[0];
    hipLaunchKernelGGL(nats_gru_persistent_bwd, dim3(NATS_PERSIST_GRID),
                       dim3(384), plan.smem_bwd, stream, jobs[0], jobs[1],
                       jobs[2], jobs[3], T, H, K3pad,
                       (unsigned*)sync.data_ptr<int>(), ngrp, njobs,
                       plan.xpd);
  } else {
    TORCH_CHECK(B <= 32,
                "bidir scan: B > 32 requires the persistent path "
                "(gru_persistent_ok)");
    for (int t = T - 1; t >= 0; --t) {
      // parity: step t reads dstep[(t+1)%2], writes dstep[t%2]
      auto args = [&](int d) {
        return GruBwdArgs{
            dstep_s.at(2 * d + (t + 1) % 2), ddir_s.at(d),
            Steps<const float>(dh_out[d]).at(t),
            Steps<const bf16_t>(saved[d]).at(t),
            Steps<const bf16_t>(xc[d]).at(t),
            t == 0 ? h00_rows.base : Steps<const float>(h_all[d]).at(t - 1),
            Steps<const float>(mask[d].t).at(t), dstep_s.at(2 * d + t % 2),
            ddir_s.at(d), Steps<bf16_t>(dpre[d]).at(t)};
      };
      hipLaunchKernelGGL(nats_gru_step_bwd_fused_bidir, dim3(ngrp, 2),
                         dim3(384), 0, stream, args(0), args(1), Ubwd[0],
                         Ubwd[1], B, H, K3pad);
    }
  }
  // final dh0 per job (dstep(0) lives in ping-pong slot 0); each job
  // writes its chunk's rows of the (B,H) dh0 output
  for (int j = 0; j < njobs; ++j) {
    const GruJob jb = gru_job(j, B);
    hipLaunchKernelGGL(nats_gru_step_bwd_gemm, dim3(ngrp), dim3(384), 0,
                       stream, dstep_s.at(2 * j), Ubwd[jb.d], ddir_s.at(j),
                       Steps<float>(dh0[jb.d]).at(jb.a), jb.rows, H, K3pad);
  }
  HIP_CHECK(hipGetLastError());
  return {dpre[0], dh0[0], dpre[1], dh0[1]};
}

std::vector<torch::Tensor> gru_scan_bwd(torch::Tensor dh_out,
                                        torch::Tensor h_all,
                                        torch::Tensor saved, torch::Tensor xc,
                                        c10::optional<torch::Tensor> mask,
                                        torch::Tensor Ubwd,
                                        c10::optional<torch::Tensor> h0) {
  check_scan_bwd_args(dh_out, saved, xc, Ubwd);
  const int T = dh_out.size(0), B = dh_out.size(1), H = dh_out.size(2);
  const int K3pad = Ubwd.size(1);
  const int ngrp = cdiv(H, JB);

  auto optsF = dh_out.options();
  auto optsB = dh_out.options().dtype(torch::kBFloat16);
  auto dpre_all = torch::empty({T, B, 4 * H}, optsB);
  auto dh_buf = torch::zeros({B, H}, optsF);
  auto ddirect = torch::empty({B, H}, optsF);
  auto dstep = torch::zeros({32, K3pad}, optsB);
  torch::Tensor hprev0 = h0.has_value()
                             ? h0->contiguous().to(torch::kFloat32)
                             : torch::zeros({B, H}, optsF);
  const OptF32 mask_f(mask);

  auto stream = at::cuda::getCurrentCUDAStream().stream();
  const Steps<const float> dh_s(dh_out), h_s(h_all), mask_s(mask_f.t);
  const Steps<const bf16_t> saved_s(saved), xc_s(xc);
  const Steps<bf16_t> dpre_s(dpre_all);
  float* dh_buf_p = dh_buf.data_ptr<float>();
  float* ddirect_p = ddirect.data_ptr<float>();
  bf16_t* dstep_p = (bf16_t*)dstep.data_ptr();

  const int pw_blocks = (int)std::min<long>(1024, (((long)B * H) + 255) / 256);
  for (int t = T - 1; t >= 0; --t) {
    hipLaunchKernelGGL(nats_gru_step_bwd_pointwise, dim3(pw_blocks), dim3(256),
                       0, stream, dh_buf_p, dh_s.at(t), saved_s.at(t),
                       xc_s.at(t),
                       t == 0 ? hprev0.data_ptr<float>() : h_s.at(t - 1),
                       mask_s.at(t), dstep_p, K3pad, ddirect_p, dpre_s.at(t),
                       B, H);
    hipLaunchKernelGGL(nats_gru_step_bwd_gemm, dim3(ngrp), dim3(384), 0,
                       stream, dstep_p, (const bf16_t*)Ubwd.data_ptr(),
                       ddirect_p, dh_buf_p, B, H, K3pad);
  }
  HIP_CHECK(hipGetLastError());
  return {dpre_all, dh_buf};
}

