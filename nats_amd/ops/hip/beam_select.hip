// Segmented beam candidate selection for the batched decoder: for every
// sentence s, the want[s] smallest keys
//   key[r][w] = (prev_cost[r] - log(probs[r][w])) + penalty[r]
// over that sentence's live rows r in [seg_off[s], seg_off[s+1]), ascending,
// ties to the lower flat index (r - seg_off[s])*V + w, NaN after +inf
// (nats.py:1001-1004: cand_scores, argsort, cand_flat[ranks]).
//
// Two launches, no atomics, no host sync, nothing that needs zeroing:
//   tile pass  grid (ceil(V/TILE), R): one block forms the keys of one
//     2048-word tile of one row and writes its own smallest want[seg(r)]
//     as partials[r][tile][0..K) (slots past want hold the sentinel);
//   merge pass grid (S): one block picks the final want[s] out of the
//     sentence's live*tiles*K partials in order, writes ranks, recomputes
//     the UN-reranked cost of each winner from prev_cost and probs, and
//     writes the -1 / +inf padding.
// A candidate travels as one 64-bit word: the fp32 key through the usual
// order-preserving bit transform (NaN -> all ones) in the high half, the
// flat index in the low half, so an unsigned min is both the order and the
// tie rule. Every word of a sentence is distinct (the index is), so round
// j of a selection is "the smallest word above round j-1's winner": no
// element is ever retired, the candidates stay in registers.
//
// Both kernels are safe for any seg_off / want contents (rows and counts
// are clamped), so callers that keep the tables device-resident and cannot
// validate them without a sync cannot make the kernels write out of range.
//
// Resource use (hipcc -O3 --offload-arch=gfx950
// -Rpass-analysis=kernel-resource-usage):
//   beam_select_tile_kernel   46 VGPRs, 40 SGPRs, LDS 512 B, scratch 0
//   beam_select_merge_kernel  50 VGPRs, 48 SGPRs, LDS 512 B, scratch 0
// (8 waves/SIMD each; no spill).

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <cstdint>

#include "common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int PER_THREAD = 8;             // candidates a thread keeps
constexpr int TILE = BLOCK * PER_THREAD;  // words per tile-pass block
constexpr int MAX_K = 32;
constexpr unsigned long long SENTINEL = ~0ull;  // "no candidate"

// fp32 -> uint32 whose unsigned order is the float order with every NaN
// last; -0 counts as +0 (they compare equal, the index breaks the tie)
__device__ __forceinline__ unsigned int order_bits(float key) {
  if (key != key) return 0xffffffffu;
  if (key == 0.f) key = 0.f;
  const unsigned int u = __float_as_uint(key);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float cand_cost(float prev, float p, int w,
                                           int use_unk, float neg_unk) {
  const float lp = (!use_unk && w == 1) ? neg_unk : logf(p);
  return prev - lp;
}

// ``want`` rounds of block-wide min over the candidates each thread holds
// in ``mine`` plus, for a merge longer than the registers, the strided
// remainder tail[BLOCK*PER_THREAD + tid + i*BLOCK] re-read every round.
// win[j] receives round j's winner; slots [want, K) get the sentinel.
__device__ __forceinline__ void select_rounds(
    const unsigned long long (&mine)[PER_THREAD],
    const unsigned long long* __restrict__ tail, long n_tail, int want, int K,
    unsigned long long* win) {
  unsigned long long last = 0;  // below every real word: order_bits >= 2^23
  for (int j = 0; j < want; ++j) {
    unsigned long long best = SENTINEL;
#pragma unroll
    for (int e = 0; e < PER_THREAD; ++e)
      if (mine[e] > last && mine[e] < best) best = mine[e];
    for (long q = TILE + threadIdx.x; q < n_tail; q += BLOCK) {
      const unsigned long long c = tail[q];
      if (c > last && c < best) best = c;
    }
    last = block_min_u64(best, j & 1);
    if (threadIdx.x == 0) win[j] = last;
    if (last == SENTINEL) {  // fewer candidates than want (block-uniform)
      for (int jj = j + 1 + threadIdx.x; jj < want; jj += BLOCK)
        win[jj] = SENTINEL;
      break;
    }
  }
  for (int j = want + threadIdx.x; j < K; j += BLOCK) win[j] = SENTINEL;
  __syncthreads();
}

__global__ __launch_bounds__(BLOCK) void beam_select_tile_kernel(
    const float* __restrict__ probs,      // [R][V]
    const float* __restrict__ prev_cost,  // [R]
    const float* __restrict__ penalty,    // [R] or null
    const int* __restrict__ seg_off,      // [S+1]
    const int* __restrict__ want,         // [S]
    unsigned long long* __restrict__ partials,  // [R][tiles][K]
    int S, int V, int K, int use_unk, float neg_unk) {
  __shared__ unsigned long long win[MAX_K];
  const int r = blockIdx.y;
  const int tile = blockIdx.x;
  const int tiles = gridDim.x;
  const int tid = threadIdx.x;

  // row -> segment (S is a handful; block-uniform scalar loads)
  int s = 0;
  while (s + 1 < S && r >= seg_off[s + 1]) ++s;
  const int local_row = r - seg_off[s];
  const bool in_seg = local_row >= 0 && r < seg_off[s + 1];
  const int w_s = in_seg ? min(max(want[s], 0), K) : 0;

  const float prev = prev_cost[r];
  const float pen = penalty ? penalty[r] : 0.f;
  const int w0 = tile * TILE;
  const float* src = probs + (long)r * V + w0;
  const unsigned int flat0 = (unsigned int)local_row * (unsigned int)V;

  unsigned long long mine[PER_THREAD];
  auto pack = [&](float p, int w) {
    const float c = cand_cost(prev, p, w, use_unk, neg_unk);
    const float key = penalty ? c + pen : c;
    return ((unsigned long long)order_bits(key) << 32) |
           (unsigned long long)(flat0 + (unsigned int)w);
  };
  // 16-byte loads only on a full tile whose first word is 16-byte aligned
  // (V % 4 != 0 leaves most row bases unaligned): otherwise coalesced
  // scalar loads with the tail of the row masked out
  const bool vec = (w0 + TILE <= V) && (((uintptr_t)src & 15) == 0);
  if (vec) {
#pragma unroll
    for (int h = 0; h < PER_THREAD / 4; ++h) {
      const int o = h * BLOCK * 4 + tid * 4;
      const f32x4 p4 = *(const f32x4*)(src + o);
#pragma unroll
      for (int i = 0; i < 4; ++i) mine[h * 4 + i] = pack(p4[i], w0 + o + i);
    }
  } else {
#pragma unroll
    for (int e = 0; e < PER_THREAD; ++e) {
      const int o = e * BLOCK + tid;
      mine[e] = (w0 + o < V) ? pack(src[o], w0 + o) : SENTINEL;
    }
  }

  select_rounds(mine, nullptr, 0, w_s, K, win);
  unsigned long long* dst = partials + ((long)r * tiles + tile) * K;
  for (int j = tid; j < K; j += BLOCK) dst[j] = win[j];
}

__global__ __launch_bounds__(BLOCK) void beam_select_merge_kernel(
    const float* __restrict__ probs, const float* __restrict__ prev_cost,
    const int* __restrict__ seg_off, const int* __restrict__ want,
    const unsigned long long* __restrict__ partials,  // [R][tiles][K]
    long* __restrict__ ranks,                         // [S][K]
    float* __restrict__ costs,                        // [S][K]
    int R, int V, int K, int tiles, int use_unk, float neg_unk) {
  __shared__ unsigned long long win[MAX_K];
  const int s = blockIdx.x;
  const int tid = threadIdx.x;
  const int r0 = min(max(seg_off[s], 0), R);
  const int r1 = min(max(seg_off[s + 1], r0), R);
  const int w_s = min(max(want[s], 0), K);

  // the sentence's partials are one contiguous run (its rows are)
  const unsigned long long* part = partials + (long)r0 * tiles * K;
  const long n = (long)(r1 - r0) * tiles * K;
  unsigned long long mine[PER_THREAD];
#pragma unroll
  for (int e = 0; e < PER_THREAD; ++e) {
    const long q = (long)e * BLOCK + tid;
    mine[e] = q < n ? part[q] : SENTINEL;
  }
  select_rounds(mine, part, n, w_s, K, win);

  for (int j = tid; j < K; j += BLOCK) {
    const unsigned long long wj = win[j];
    const unsigned int flat = (unsigned int)wj;
    long rank = -1;
    float cost = INFINITY;
    if (wj != SENTINEL) {
      const int row = r0 + (int)(flat / (unsigned int)V);
      const int w = (int)(flat % (unsigned int)V);
      if (row < r1) {
        rank = (long)flat;
        cost = cand_cost(prev_cost[row], probs[(long)row * V + w], w, use_unk,
                         neg_unk);
      }
    }
    ranks[(long)s * K + j] = rank;
    costs[(long)s * K + j] = cost;
  }
}

}  // namespace

std::vector<torch::Tensor> beam_select(torch::Tensor probs,
                                       torch::Tensor prev_cost,
                                       torch::Tensor seg_off,
                                       torch::Tensor want,
                                       c10::optional<torch::Tensor> penalty,
                                       long K, bool use_unk, double neg_unk) {
  TORCH_CHECK(probs.is_cuda() && probs.dim() == 2 &&
                  probs.dtype() == torch::kFloat32 && probs.is_contiguous(),
              "beam_select: probs must be a contiguous (R, V) fp32 GPU tensor");
  const long R = probs.size(0), V = probs.size(1);
  const long S = want.numel();
  TORCH_CHECK(prev_cost.is_cuda() && prev_cost.dtype() == torch::kFloat32 &&
                  prev_cost.is_contiguous() && prev_cost.numel() == R,
              "beam_select: prev_cost must be (R,) fp32");
  TORCH_CHECK(seg_off.is_cuda() && seg_off.dtype() == torch::kInt32 &&
                  seg_off.is_contiguous() && seg_off.numel() == S + 1 &&
                  want.is_cuda() && want.dtype() == torch::kInt32 &&
                  want.is_contiguous(),
              "beam_select: seg_off (S+1,) and want (S,) must be int32");
  TORCH_CHECK(K >= 1 && K <= MAX_K, "beam_select: K must be in [1, 32]");
  // (per-segment live*V < 2^31 is the caller's check: it knows seg_off)
  TORCH_CHECK(R >= 1 && S >= 1 && V >= 1 && R <= 65535 &&
                  V < (1L << 31) - 2 * TILE,
              "beam_select: bad shape (R, V) = (", R, ", ", V, ")");
  const float* pen = nullptr;
  if (penalty.has_value()) {
    TORCH_CHECK(penalty->is_cuda() && penalty->dtype() == torch::kFloat32 &&
                    penalty->is_contiguous() && penalty->numel() == R,
                "beam_select: penalty must be (R,) fp32");
    pen = penalty->data_ptr<float>();
  }
  const int tiles = (int)((V + TILE - 1) / TILE);
  auto partials = torch::empty({R, (long)tiles, K},
                               probs.options().dtype(torch::kInt64));
  auto ranks = torch::empty({S, K}, probs.options().dtype(torch::kInt64));
  auto costs = torch::empty({S, K}, probs.options());
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  auto* part = (unsigned long long*)partials.data_ptr<int64_t>();
  hipLaunchKernelGGL(beam_select_tile_kernel, dim3(tiles, (unsigned)R),
                     dim3(BLOCK), 0, stream, probs.data_ptr<float>(),
                     prev_cost.data_ptr<float>(), pen,
                     seg_off.data_ptr<int>(), want.data_ptr<int>(), part,
                     (int)S, (int)V, (int)K, (int)use_unk, (float)neg_unk);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(beam_select_merge_kernel, dim3((unsigned)S), dim3(BLOCK),
                     0, stream, probs.data_ptr<float>(),
                     prev_cost.data_ptr<float>(), seg_off.data_ptr<int>(),
                     want.data_ptr<int>(), part,
                     (long*)ranks.data_ptr<int64_t>(), costs.data_ptr<float>(),
                     (int)R, (int)V, (int)K, tiles, (int)use_unk,
                     (float)neg_unk);
  HIP_CHECK(hipGetLastError());
  return {ranks, costs};
}
