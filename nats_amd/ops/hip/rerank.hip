// Fused decode-time distraction rerank (north star: "the distraction
// terms — KL divergence over the attention-weight history and cosine
// distance over the context/state history — ... are fused HIP
// reductions"). For every live hypothesis, the three penalties of
// nats.py:981-999 in a single pass over its history:
//   -kl * min_t KL(alpha_t || alpha_cur)        (scipy entropy conv.)
//   +cf * max_t (1 - cos(ctx_t, ctx_cur))
//   +sf * max_t (1 - cos(state_t, state_cur))
//
// Both penalty entry points share the per-(step, row) arithmetic (hist_kl,
// hist_cosine_dist, rerank_total below; one wave per history step,
// lane-strided loops, shuffle-down sums):
//
//   rerank_penalties        dense histories (n, k, dim) of ONE sentence.
//     grid (k); each wave owns the steps t = wave, wave+NW, ...; block-level
//     min/max combine in LDS.
//
//   rerank_penalties_paged  histories of ALL rows of a batched decode, kept
//     as slabs hist_*[t][slot] (Tmax, Rmax, dim) that are written once per
//     step and never moved, plus an int32 ancestor table anc[t][r] (row
//     stride Rmax) naming the slot that holds row r's entry for step t.
//     Partial pass: grid (R, G = ceil(n / STEPS_PER_BLOCK)), block (r, g)
//     walks steps [g*SPB, min(n, (g+1)*SPB)) of row r through the table and
//     writes (kl_min, cd_max, sd_max) to part[r][g]. Combine pass: one
//     thread per row folds its G partials in order and applies
//     rerank_total. min and max are exact, so regrouping the steps of a row
//     cannot change a bit: the result equals rerank_penalties on the same
//     history content bit for bit. No atomics, nothing to zero, no sync.
//     A table slot outside [0, Rmax) is never dereferenced: the row's
//     penalty becomes NaN (poison, not fault). A NaN partial can only be
//     that poison, since fminf/fmaxf against the +-FLT_MAX seeds drop a
//     NaN term exactly as the dense kernel does.
//
//   rerank_advance          the table reshuffle of a decode step, elementwise
//     over n x R entries: anc_new[t][r] = anc_old[t][parent[r]] for
//     t < n-1 and anc_new[n-1][r] = parent[r] (a parent outside [0, Rmax)
//     stores the poison slot -1).
//
// Resources (hipcc -O3 --offload-arch=gfx950, kernel-resource-usage):
//   rerank_penalties_kernel  42 VGPRs, 51 SGPRs, LDS 48 B, scratch 0
//   rerank_partial_kernel    52 VGPRs, 58 SGPRs, LDS 64 B, scratch 0
//   rerank_combine_kernel    11 VGPRs, 20 SGPRs, LDS 0,    scratch 0
//   rerank_advance_kernel     8 VGPRs, 18 SGPRs, LDS 0,    scratch 0

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <cfloat>

#include "common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int NW = BLOCK / NATS_WAVE;
// history steps one block of the paged partial pass walks (NW waves x 2
// trips); tests/test_rerank_paged.py mirrors it
constexpr int STEPS_PER_BLOCK = 8;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = NATS_WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

// The per-(step, row) terms. Called by a whole wave; the result is valid in
// lane 0.

// KL(p || q): scipy normalises both distributions first
__device__ __forceinline__ float hist_kl(const float* __restrict__ p,
                                         const float* __restrict__ q, int Ts,
                                         int lane) {
  float psum = 0.f, qsum = 0.f;
  for (int s = lane; s < Ts; s += NATS_WAVE) {
    psum += p[s];
    qsum += q[s];
  }
  psum = wave_sum(psum);
  qsum = wave_sum(qsum);
  psum = __shfl(psum, 0);
  qsum = __shfl(qsum, 0);
  float kl = 0.f;
  for (int s = lane; s < Ts; s += NATS_WAVE) {
    const float pv = p[s] / psum;
    const float qv = q[s] / qsum;
    if (pv > 0.f) kl += pv * (__logf(pv) - __logf(qv));
  }
  return wave_sum(kl);
}

// 1 - cos(h, c), 0 when either norm is 0 (context and state histories)
__device__ __forceinline__ float hist_cosine_dist(const float* __restrict__ h,
                                                  const float* __restrict__ c,
                                                  int D, int lane) {
  float dot = 0.f, n1 = 0.f, n2 = 0.f;
  for (int s = lane; s < D; s += NATS_WAVE) {
    dot += h[s] * c[s];
    n1 += h[s] * h[s];
    n2 += c[s] * c[s];
  }
  dot = wave_sum(dot);
  n1 = wave_sum(n1);
  n2 = wave_sum(n2);
  const float den = sqrtf(n1) * sqrtf(n2);
  return (den == 0.f) ? 0.f : (1.f - dot / den);
}

__device__ __forceinline__ float rerank_total(float kl_f, float ctx_f,
                                              float state_f, float kl_min,
                                              float cd_max, float sd_max) {
  return -kl_f * kl_min + ctx_f * cd_max + state_f * sd_max;
}

__global__ __launch_bounds__(BLOCK) void rerank_penalties_kernel(
    const float* __restrict__ hist_a,  // [n][k][Ts]
    const float* __restrict__ hist_c,  // [n][k][C]
    const float* __restrict__ hist_s,  // [n][k][H]
    const float* __restrict__ cur_a,   // [k][Ts]
    const float* __restrict__ cur_c,   // [k][C]
    const float* __restrict__ cur_s,   // [k][H]
    float* __restrict__ pen,           // [k]
    float kl_f, float ctx_f, float state_f, int n, int k, int Ts, int C,
    int H) {
  __shared__ float red_kl[NW], red_cd[NW], red_sd[NW];
  const int hyp = blockIdx.x;
  const int wave = threadIdx.x / NATS_WAVE;
  const int lane = threadIdx.x & (NATS_WAVE - 1);

  float kl_min = FLT_MAX, cd_max = -FLT_MAX, sd_max = -FLT_MAX;
  for (int t = wave; t < n; t += NW) {
    const long row = (long)t * k + hyp;
    const float kl = hist_kl(hist_a + row * Ts, cur_a + (long)hyp * Ts, Ts,
                             lane);
    const float cd = hist_cosine_dist(hist_c + row * C, cur_c + (long)hyp * C,
                                      C, lane);
    const float sd = hist_cosine_dist(hist_s + row * H, cur_s + (long)hyp * H,
                                      H, lane);
    if (lane == 0) {
      kl_min = fminf(kl_min, kl);
      cd_max = fmaxf(cd_max, cd);
      sd_max = fmaxf(sd_max, sd);
    }
  }
  if (lane == 0) {
    red_kl[wave] = kl_min;
    red_cd[wave] = cd_max;
    red_sd[wave] = sd_max;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = FLT_MAX, b = -FLT_MAX, c = -FLT_MAX;
    for (int w = 0; w < NW; ++w) {
      a = fminf(a, red_kl[w]);
      b = fmaxf(b, red_cd[w]);
      c = fmaxf(c, red_sd[w]);
    }
    pen[hyp] = (n > 0) ? rerank_total(kl_f, ctx_f, state_f, a, b, c) : 0.f;
  }
}

__global__ __launch_bounds__(BLOCK) void rerank_advance_kernel(
    const int* __restrict__ anc_old,  // [Tmax][Rmax]
    int* __restrict__ anc_new,        // [Tmax][Rmax]
    const int64_t* __restrict__ parent,  // [R]
    int n, int R, int Rmax) {
  const int idx = blockIdx.x * BLOCK + threadIdx.x;
  if (idx >= n * R) return;
  const int t = idx / R, r = idx - t * R;
  const int64_t p = parent[r];
  int slot = -1;
  if (p >= 0 && p < Rmax)
    slot = (t == n - 1) ? (int)p : anc_old[(long)t * Rmax + p];
  anc_new[(long)t * Rmax + r] = slot;
}

__global__ __launch_bounds__(BLOCK) void rerank_partial_kernel(
    const float* __restrict__ hist_a,  // [Tmax][Rmax][Ts]
    const float* __restrict__ hist_c,  // [Tmax][Rmax][C]
    const float* __restrict__ hist_s,  // [Tmax][Rmax][H]
    const int* __restrict__ anc,       // [Tmax][Rmax]
    const float* __restrict__ cur_a,   // [R][Ts]
    const float* __restrict__ cur_c,   // [R][C]
    const float* __restrict__ cur_s,   // [R][H]
    float* __restrict__ part,          // [R][G][3]
    int n, int Rmax, int Ts, int C, int H) {
  __shared__ float red_kl[NW], red_cd[NW], red_sd[NW];
  __shared__ int red_bad[NW];
  const int r = blockIdx.x, g = blockIdx.y;
  const int wave = threadIdx.x / NATS_WAVE;
  const int lane = threadIdx.x & (NATS_WAVE - 1);
  const int t_end = min(n, (g + 1) * STEPS_PER_BLOCK);

  float kl_min = FLT_MAX, cd_max = -FLT_MAX, sd_max = -FLT_MAX;
  int bad = 0;
  for (int t = g * STEPS_PER_BLOCK + wave; t < t_end; t += NW) {
    const int slot = anc[(long)t * Rmax + r];  // wave-uniform
    if (slot < 0 || slot >= Rmax) {
      bad = 1;
      continue;
    }
    const long row = (long)t * Rmax + slot;
    const float kl = hist_kl(hist_a + row * Ts, cur_a + (long)r * Ts, Ts,
                             lane);
    const float cd = hist_cosine_dist(hist_c + row * C, cur_c + (long)r * C,
                                      C, lane);
    const float sd = hist_cosine_dist(hist_s + row * H, cur_s + (long)r * H,
                                      H, lane);
    if (lane == 0) {
      kl_min = fminf(kl_min, kl);
      cd_max = fmaxf(cd_max, cd);
      sd_max = fmaxf(sd_max, sd);
    }
  }
  if (lane == 0) {
    red_kl[wave] = kl_min;
    red_cd[wave] = cd_max;
    red_sd[wave] = sd_max;
    red_bad[wave] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = FLT_MAX, b = -FLT_MAX, c = -FLT_MAX;
    int any_bad = 0;
    for (int w = 0; w < NW; ++w) {
      a = fminf(a, red_kl[w]);
      b = fmaxf(b, red_cd[w]);
      c = fmaxf(c, red_sd[w]);
      any_bad |= red_bad[w];
    }
    if (any_bad) a = b = c = NAN;
    float* out = part + ((long)r * gridDim.y + g) * 3;
    out[0] = a;
    out[1] = b;
    out[2] = c;
  }
}

__global__ __launch_bounds__(BLOCK) void rerank_combine_kernel(
    const float* __restrict__ part,  // [R][G][3]
    float* __restrict__ pen,         // [R]
    float kl_f, float ctx_f, float state_f, int n, int R, int G) {
  const int r = blockIdx.x * BLOCK + threadIdx.x;
  if (r >= R) return;
  float a = FLT_MAX, b = -FLT_MAX, c = -FLT_MAX;
  bool bad = false;
  for (int g = 0; g < G; ++g) {
    const float* p = part + ((long)r * G + g) * 3;
    bad |= (p[0] != p[0]);
    a = fminf(a, p[0]);
    b = fmaxf(b, p[1]);
    c = fmaxf(c, p[2]);
  }
  const float total =
      (n > 0) ? rerank_total(kl_f, ctx_f, state_f, a, b, c) : 0.f;
  pen[r] = bad ? NAN : total;
}

bool slab_ok(const torch::Tensor& t, const torch::Tensor& like) {
  return t.is_cuda() && t.dtype() == torch::kFloat32 && t.dim() == 3 &&
         t.is_contiguous() && t.size(0) == like.size(0) &&
         t.size(1) == like.size(1);
}

bool cur_ok(const torch::Tensor& t, long R, long dim) {
  return t.is_cuda() && t.dtype() == torch::kFloat32 && t.dim() == 2 &&
         t.is_contiguous() && t.size(0) == R && t.size(1) == dim;
}

bool table_ok(const torch::Tensor& t) {
  return t.is_cuda() && t.dtype() == torch::kInt32 && t.dim() == 2 &&
         t.is_contiguous();
}

}  // namespace

torch::Tensor rerank_penalties(torch::Tensor hist_a, torch::Tensor hist_c,
                               torch::Tensor hist_s, torch::Tensor cur_a,
                               torch::Tensor cur_c, torch::Tensor cur_s,
                               double kl_f, double ctx_f, double state_f) {
  TORCH_CHECK(hist_a.is_cuda() && hist_a.dtype() == torch::kFloat32);
  const int n = hist_a.size(0), k = hist_a.size(1), Ts = hist_a.size(2);
  const int C = hist_c.size(2), H = hist_s.size(2);
  auto pen = torch::empty({k}, hist_a.options());
  hipLaunchKernelGGL(rerank_penalties_kernel, dim3(k), dim3(256), 0,
                     at::cuda::getCurrentCUDAStream().stream(),
                     hist_a.contiguous().data_ptr<float>(),
                     hist_c.contiguous().data_ptr<float>(),
                     hist_s.contiguous().data_ptr<float>(),
                     cur_a.contiguous().data_ptr<float>(),
                     cur_c.contiguous().data_ptr<float>(),
                     cur_s.contiguous().data_ptr<float>(),
                     pen.data_ptr<float>(), (float)kl_f, (float)ctx_f,
                     (float)state_f, n, k, Ts, C, H);
  HIP_CHECK(hipGetLastError());
  return pen;
}

void rerank_advance(torch::Tensor anc_old, torch::Tensor anc_new,
                    torch::Tensor parent, long n) {
  TORCH_CHECK(table_ok(anc_old) && table_ok(anc_new) &&
                  anc_old.sizes() == anc_new.sizes() &&
                  anc_old.data_ptr() != anc_new.data_ptr(),
              "rerank_advance: anc_old and anc_new must be two contiguous "
              "(Tmax, Rmax) int32 GPU tensors of one shape");
  TORCH_CHECK(parent.is_cuda() && parent.dtype() == torch::kInt64 &&
                  parent.dim() == 1 && parent.is_contiguous(),
              "rerank_advance: parent must be a contiguous (R,) int64 GPU "
              "tensor");
  const long Tmax = anc_old.size(0), Rmax = anc_old.size(1);
  const long R = parent.size(0);
  TORCH_CHECK(n >= 1 && n <= Tmax && R >= 1 && R <= Rmax,
              "rerank_advance: need 1 <= n <= Tmax and 1 <= R <= Rmax, got "
              "n = ", n, ", R = ", R, " for a (", Tmax, ", ", Rmax,
              ") table");
  TORCH_CHECK(n * R < (1L << 31), "rerank_advance: n * R too large");
  hipLaunchKernelGGL(rerank_advance_kernel, dim3(cdiv((int)(n * R), BLOCK)),
                     dim3(BLOCK), 0, at::cuda::getCurrentCUDAStream().stream(),
                     anc_old.data_ptr<int>(), anc_new.data_ptr<int>(),
                     parent.data_ptr<int64_t>(), (int)n, (int)R,
                     (int)Rmax);
  HIP_CHECK(hipGetLastError());
}

torch::Tensor rerank_penalties_paged(torch::Tensor hist_a,
                                     torch::Tensor hist_c,
                                     torch::Tensor hist_s, torch::Tensor anc,
                                     long n, torch::Tensor cur_a,
                                     torch::Tensor cur_c, torch::Tensor cur_s,
                                     double kl_f, double ctx_f,
                                     double state_f) {
  TORCH_CHECK(slab_ok(hist_a, hist_a) && slab_ok(hist_c, hist_a) &&
                  slab_ok(hist_s, hist_a),
              "rerank_penalties_paged: hist_a/c/s must be contiguous (Tmax, "
              "Rmax, dim) fp32 GPU tensors");
  const long Tmax = hist_a.size(0), Rmax = hist_a.size(1);
  const long Ts = hist_a.size(2), C = hist_c.size(2), H = hist_s.size(2);
  TORCH_CHECK(table_ok(anc) && anc.size(0) == Tmax && anc.size(1) == Rmax,
              "rerank_penalties_paged: anc must be a contiguous (Tmax, Rmax) "
              "int32 GPU tensor");
  const long R = cur_a.dim() == 2 ? cur_a.size(0) : -1;
  TORCH_CHECK(R >= 1 && R <= Rmax && cur_ok(cur_a, R, Ts) &&
                  cur_ok(cur_c, R, C) && cur_ok(cur_s, R, H),
              "rerank_penalties_paged: cur_a/c/s must be contiguous (R <= "
              "Rmax, dim) fp32 GPU tensors matching the slabs");
  TORCH_CHECK(n >= 0 && n <= Tmax,
              "rerank_penalties_paged: n = ", n, " outside [0, Tmax = ", Tmax,
              "]");
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  const int G = cdiv((int)n, STEPS_PER_BLOCK);
  auto pen = torch::empty({R}, hist_a.options());
  auto part = torch::empty({R, G, 3}, hist_a.options());
  if (G > 0) {
    hipLaunchKernelGGL(rerank_partial_kernel, dim3((unsigned)R, (unsigned)G),
                       dim3(BLOCK), 0, stream, hist_a.data_ptr<float>(),
                       hist_c.data_ptr<float>(), hist_s.data_ptr<float>(),
                       anc.data_ptr<int>(), cur_a.data_ptr<float>(),
                       cur_c.data_ptr<float>(), cur_s.data_ptr<float>(),
                       part.data_ptr<float>(), (int)n, (int)Rmax, (int)Ts,
                       (int)C, (int)H);
    HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(rerank_combine_kernel, dim3(cdiv((int)R, BLOCK)),
                     dim3(BLOCK), 0, stream, part.data_ptr<float>(),
                     pen.data_ptr<float>(), (float)kl_f, (float)ctx_f,
                     (float)state_f, (int)n, (int)R, G);
  HIP_CHECK(hipGetLastError());
  return pen;
}
