// Shared GRU kernel declarations (defined in gru_scan.hip, reused by the
// conditional-GRU decoder in cond_gru.hip — GRU_2's per-step math is
// identical to the encoder cell, nats.py:503-519 vs 336-356).
#pragma once

#include "common.h"

// The GRU cell (nats.py:336-356), shared by every forward/backward site of
// the encoder scans and both decoder GRUs. pr/pu/px are the recurrent
// preactivations (pr, pu with their input projections already added), xc
// the candidate's input projection, hp the previous state, mask_t the
// step's [B] mask or null and b this element's row. GRU_1 calls it with
// px = pxa + bx1 and xc = pxb.
struct GruCellFwd {
  float r, u, hbar, hnew;
};

__device__ __forceinline__ GruCellFwd gru_cell_fwd(float pr, float pu,
                                                   float px, float xc,
                                                   float hp,
                                                   const float* mask_t,
                                                   int b) {
  const float r = nats_sigmoid(pr);
  const float u = nats_sigmoid(pu);
  const float hbar = tanhf(px * r + xc);
  float hnew = u * hp + (1.f - u) * hbar;
  if (mask_t != nullptr) {
    const float mm = mask_t[b];
    hnew = mm * hnew + (1.f - mm) * hp;
  }
  return GruCellFwd{r, u, hbar, hnew};
}

// dh -> gate-preactivation grads; mm = 1 without a mask. dpx is the grad of
// the candidate preactivation (= dxc), dpxl = dpx * r the part that flows
// into h@Ux, ddirect the passthrough into dh_{t-1}.
struct GruCellBwd {
  float dpr, dpu, dpx, dpxl, ddirect;
};

__device__ __forceinline__ GruCellBwd gru_cell_bwd(float dh, float r, float u,
                                                   float px, float hbar,
                                                   float hp, float mm) {
  GruCellBwd o;
  const float du = dh * mm * (hp - hbar);
  const float dhbar = dh * mm * (1.f - u);
  o.dpx = dhbar * (1.f - hbar * hbar);
  o.dpxl = o.dpx * r;
  const float dr = o.dpx * px;
  o.dpr = dr * r * (1.f - r);
  o.dpu = du * u * (1.f - u);
  o.ddirect = dh * (mm * u + (1.f - mm));
  return o;
}

// host: optional tensor -> contiguous fp32 copy + raw pointer (null if absent)
struct OptF32 {
  torch::Tensor t;
  const float* p = nullptr;
  explicit OptF32(const c10::optional<torch::Tensor>& o) {
    if (o.has_value()) {
      t = o->contiguous().to(torch::kFloat32);
      p = t.data_ptr<float>();
    }
  }
};

// host: per-timestep view of a (T, ...) tensor: at(t) is step t's slab, the
// stride taken from the tensor itself; `row` starts every slab at that
// index of dim 1 (a batch chunk); an undefined tensor gives null throughout.
template <class T>
struct Steps {
  T* base = nullptr;
  long stride = 0;
  Steps() = default;
  explicit Steps(const torch::Tensor& x, int row = 0) {
    if (!x.defined()) return;
    base = (T*)x.data_ptr() + (row ? row * x.stride(1) : 0);
    stride = x.stride(0);
  }
  T* at(int t) const { return base ? base + (long)t * stride : nullptr; }
};

// host: the entry checks shared by the scan drivers
static inline void check_scan_input(const torch::Tensor& x,
                                    torch::ScalarType dtype,
                                    const char* name) {
  TORCH_CHECK(x.is_cuda() && x.dtype() == dtype && x.is_contiguous(), name,
              ": expected a contiguous device tensor of ", dtype);
}
// packed weight: one 16-row slot per (column tile, gate) of an H-wide output
static inline void check_packed_weight(const torch::Tensor& W, int H,
                                       int gates, const char* name) {
  TORCH_CHECK(W.size(0) == cdiv(H, JB) * gates * JB && W.is_contiguous(),
              name, ": packed weight rows do not match the hidden size");
}

// forward step: fused [h@U_r | h@U_u | h@Ux] MFMA + gates/mask pointwise.
// ld_bfout = row stride of the bf16 h output (lets the decoder write h1
// into the [h1|ctx] packed GRU_1 operand buffer).
__global__ __launch_bounds__(384) void nats_gru_step_fwd(
    const bf16_t* __restrict__ h_bf, const float* __restrict__ h_prev,
    const bf16_t* __restrict__ Upk, const bf16_t* __restrict__ xg_t,
    const bf16_t* __restrict__ xc_t, const float* __restrict__ mask_t,
    float* __restrict__ h_out, bf16_t* __restrict__ h_bf_out, int ld_bfout,
    bf16_t* __restrict__ saved_t, int B, int H, int Hpad);

__global__ __launch_bounds__(384) void nats_gru2_gemm_splitk(const bf16_t* h_bf, const bf16_t* Upk,
                                      float* part, int Hpad);

__global__ void nats_gru2_step_pointwise(
    const float* part, int KS, const float* h_prev, const bf16_t* xg_t,
    const bf16_t* xc_t, const float* mask_t, float* h_out, bf16_t* h_bf_out,
    int ld_bfout, bf16_t* saved_t, int B, int H, int Hpad);

// backward pointwise: dh -> gate preactivation grads. dh_out_t may be null.
__global__ void nats_gru_step_bwd_pointwise(
    const float* __restrict__ dh_buf, const float* __restrict__ dh_out_t,
    const bf16_t* __restrict__ saved_t, const bf16_t* __restrict__ xc_t,
    const float* __restrict__ h_prev, const float* __restrict__ mask_t,
    bf16_t* __restrict__ dstep, int ld_dstep, float* __restrict__ ddirect,
    bf16_t* __restrict__ dpre_t, int B, int H);

// backward recurrent GEMM: out[b,i] = ddirect[b,i] + dstep[b,:] @ Wt[i,:]
// (generic over output width "H" = rows of Wt; K = Kpad).
__global__ __launch_bounds__(384) void nats_gru_step_bwd_gemm(
    const bf16_t* __restrict__ dstep, const bf16_t* __restrict__ Wt,
    const float* __restrict__ ddirect, float* __restrict__ out, int B, int H,
    int Kpad);

// Per-direction argument sets for the bidirectional encoder kernels
// (both directions are independent — one launch covers both via
// blockIdx.y, halving launch count and overlapping the work).
struct GruFwdArgs {
  const bf16_t* h_bf;
  const float* h_prev;
  const bf16_t* Upk;
  const bf16_t* xg_t;
  const bf16_t* xc_t;
  const float* mask_t;
  float* h_out;
  bf16_t* h_bf_out;
  bf16_t* saved_t;
};

struct GruBwdArgs {
  const bf16_t* dstep_in;   // dstep written at step t+1 (zeros at t=T-1)
  const float* ddirect_in;  // passthrough written at step t+1
  const float* dh_out_t;    // upstream grad at t
  const bf16_t* saved_t;
  const bf16_t* xc_t;
  const float* h_prev;
  const float* mask_t;
  bf16_t* dstep_out;
  float* ddirect_out;
  bf16_t* dpre_t;
};

__global__ __launch_bounds__(384) void nats_gru_step_fwd_bidir(
    GruFwdArgs a0, GruFwdArgs a1, int ld_bfout, int B, int H, int Hpad);

// fused backward step: phase 1 recomputes dh for this WG's columns from
// the PREVIOUS (t+1) step's dstep/ddirect via the recurrent GEMM, phase 2
// does the pointwise gate backward on the same columns (column-local).
__global__ __launch_bounds__(384) void nats_gru_step_bwd_fused_bidir(
    GruBwdArgs a0, GruBwdArgs a1, const bf16_t* Ubwd0, const bf16_t* Ubwd1,
    int B, int H, int Kpad);

// ---------------- K ranges ----------------
// How every split-K site cuts its reduction range: [beg, end) into n
// 32-aligned parts, part i clamped to the range (a part past the end is
// empty and runs zero K-loop iterations).
struct KRange { int beg, end; };

__device__ __forceinline__ KRange k_part(KRange r, int n, int i) {
  const int chunk = (((r.end - r.beg) / n + 31) / 32) * 32;
  return KRange{min(r.end, r.beg + i * chunk),
                min(r.end, r.beg + (i + 1) * chunk)};
}

// ---------------- backward row GEMM ----------------
// sum[b, i] = A[b, kr) @ Wt[i, kr)^T for the 16 output columns from i0, in
// a 384-thread block: wave w -> rows [16*(w/3), +16), K third w%3; the
// three partials meet in LDS and epi(b, i, sum) runs once per valid
// (b < B, i < N).
template <class Epi>
__device__ __forceinline__ void row_gemm(const bf16_t* A, const bf16_t* Wt,
                                         int i0, int ld, KRange kr, int B,
                                         int N, Epi epi) {
  __shared__ float part[3][32][JB + 1];
  const int wave = threadIdx.x / NATS_WAVE;
  const int m = wave / 3;
  const int ks = wave % 3;
  const KRange k = k_part(kr, 3, ks);

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  NATS_MFMA_KLOOP(acc, A, 16 * m, ld, Wt, i0, ld, k.beg, k.end);
  store_cd_lds(part[ks], acc, 16 * m);
  __syncthreads();

  for (int idx = threadIdx.x; idx < B * JB; idx += blockDim.x) {
    const int b = idx / JB;
    const int c = idx % JB;
    const int i = i0 + c;
    if (i >= N) continue;
    epi(b, i, part[0][b][c] + part[1][b][c] + part[2][b][c]);
  }
}

// ---------------- encoder / GRU_2 epilogues ----------------
// Forward finish of element (b, j), bj = b * H + j: p0/p1/px are the recurrent
// preactivations h@U_r, h@U_u, h@Ux (a.h_bf and a.Upk are not read here).
__device__ __forceinline__ void gru_fwd_finish(const GruFwdArgs& a,
                                               int ld_bfout, int H, int b,
                                               int j, long bj, float p0,
                                               float p1, float px) {
  const float hp = a.h_prev[bj];
  const float pr = p0 + (float)a.xg_t[(long)b * 2 * H + j];
  const float pu = p1 + (float)a.xg_t[(long)b * 2 * H + H + j];
  const GruCellFwd o =
      gru_cell_fwd(pr, pu, px, (float)a.xc_t[bj], hp, a.mask_t, b);
  a.h_out[bj] = o.hnew;
  a.h_bf_out[(long)b * ld_bfout + j] = (bf16_t)o.hnew;
  a.saved_t[(long)b * 3 * H + j] = (bf16_t)o.r;
  a.saved_t[(long)b * 3 * H + H + j] = (bf16_t)o.u;
  a.saved_t[(long)b * 3 * H + 2 * H + j] = (bf16_t)px;
}

// Backward finish of element (b, j), bj = b * H + j: dh is the recurrent + passthrough
// grad, the upstream a.dh_out_t (if any) is added here (a.dstep_in and
// a.ddirect_in are not read).
__device__ __forceinline__ void gru_bwd_finish(const GruBwdArgs& a,
                                               int ld_dstep, int H, int b,
                                               int j, long bj, float dh) {
  if (a.dh_out_t != nullptr) dh += a.dh_out_t[bj];
  const float r = (float)a.saved_t[(long)b * 3 * H + j];
  const float u = (float)a.saved_t[(long)b * 3 * H + H + j];
  const float px = (float)a.saved_t[(long)b * 3 * H + 2 * H + j];
  const float hbar = tanhf(px * r + (float)a.xc_t[bj]);
  const float hp = a.h_prev[bj];
  const float mm = (a.mask_t != nullptr) ? a.mask_t[b] : 1.f;
  const GruCellBwd o = gru_cell_bwd(dh, r, u, px, hbar, hp, mm);
  a.ddirect_out[bj] = o.ddirect;
  a.dstep_out[(long)b * ld_dstep + j] = (bf16_t)o.dpr;
  a.dstep_out[(long)b * ld_dstep + H + j] = (bf16_t)o.dpu;
  a.dstep_out[(long)b * ld_dstep + 2 * H + j] = (bf16_t)o.dpxl;
  a.dpre_t[(long)b * 4 * H + j] = (bf16_t)o.dpr;
  a.dpre_t[(long)b * 4 * H + H + j] = (bf16_t)o.dpu;
  a.dpre_t[(long)b * 4 * H + 2 * H + j] = (bf16_t)o.dpx;
  a.dpre_t[(long)b * 4 * H + 3 * H + j] = (bf16_t)o.dpxl;
}

