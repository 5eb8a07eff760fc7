// Beam-row reshuffle of a batched decode step, in one launch: the rows the
// host selected move from the step's output buffers into the step's static
// input buffers, together with the next words, the row -> sentence routing
// and the padding tail (decode/batched.py, resident_state).
//
//   table (3, L) int64 = [parent | word | sentence], L live rows of the next
//   step. For r < L:
//     dst_j[r] = src_j[parent[r]]   j < nbuf (h2, acc_ctx, acc_alpha)
//     y_out[r] = word[r], route_out[r] = sentence[r]
//   and every row L <= r < Rmax gets a copy of the new row 0, the padding
//   rule of _GraphStepper.step.
//
// Nothing here is arithmetic and the rows are 2 to 8 KB, a few hundred at
// most, so the launch is latency-bound: grid (Rmax, segments), one block
// per (destination row, 4 KB segment of one buffer), one 16-byte load and
// store per thread. The 16-byte path is taken where both row bases are
// 16-byte aligned (every row when D % 4 == 0; acc_alpha has D = Ts, any
// value) and covers the row's multiple-of-4 part; the rest goes by dwords.
// Pointers and widths travel by value in ReorderArgs: no pointer table, no
// upload, no atomics, nothing to zero.
//
// A parent outside [0, n_prev) is never dereferenced: that row's dst_j
// become NaN and its y_out / route_out 0 (poison, not fault), as the other
// tables taken on trust do (rerank.hip).
//
// Resources (hipcc -O3 --offload-arch=gfx950, kernel-resource-usage):
//   beam_reorder_kernel  8 VGPRs, 30 SGPRs, LDS 0, scratch 0

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <cstdint>
#include <vector>

#include "common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int SEG = BLOCK * 4;  // floats one block moves: 16 bytes a thread
constexpr int MAX_BUF = 4;

struct ReorderArgs {
  const float* src[MAX_BUF];  // [n_prev][D_j]
  float* dst[MAX_BUF];        // [Rmax][D_j]
  int D[MAX_BUF];
  int seg_end[MAX_BUF];  // buffer j owns blockIdx.y in [seg_end[j-1], seg_end[j])
  const int64_t* table;  // [3][L]
  int64_t* y_out;        // [Rmax]
  void* route_out;       // [Rmax] int64 or int32
  int route64;
  int nbuf;
  int L;
  int n_prev;
};

__global__ __launch_bounds__(BLOCK) void beam_reorder_kernel(ReorderArgs a) {
  const int r = blockIdx.x;
  const int col = r < a.L ? r : 0;  // padding rows copy the new row 0
  const int64_t parent = a.table[col];
  const bool ok = parent >= 0 && parent < a.n_prev;

  // static indices only: the struct stays in the kernel-argument segment
  const float* sp = a.src[0];
  float* dp = a.dst[0];
  int D = a.D[0], seg0 = 0;
#pragma unroll
  for (int j = 1; j < MAX_BUF; ++j) {
    if (j < a.nbuf && (int)blockIdx.y >= a.seg_end[j - 1]) {
      sp = a.src[j];
      dp = a.dst[j];
      D = a.D[j];
      seg0 = a.seg_end[j - 1];
    }
  }

  const int e0 = ((int)blockIdx.y - seg0) * SEG;
  const int e1 = min(D, e0 + SEG);
  const float* srow = ok ? sp + parent * D : nullptr;
  float* drow = dp + (long)r * D;
  const bool vec =
      (((uintptr_t)srow | (uintptr_t)drow) & 15) == 0;  // block-uniform
  const int v1 = vec ? min(e1, D & ~3) : e0;  // end of the 16-byte part

  const int e = e0 + (int)threadIdx.x * 4;
  if (e < v1) {
    f32x4 v = {NAN, NAN, NAN, NAN};
    if (ok) v = *(const f32x4*)(srow + e);
    *(f32x4*)(drow + e) = v;
  }
  for (int t = v1 + (int)threadIdx.x; t < e1; t += BLOCK)
    drow[t] = ok ? srow[t] : NAN;

  if (blockIdx.y == 0 && threadIdx.x == 0) {
    const int64_t word = ok ? a.table[(long)a.L + col] : 0;
    const int64_t sent = ok ? a.table[(long)a.L * 2 + col] : 0;
    a.y_out[r] = word;
    if (a.route64)
      ((int64_t*)a.route_out)[r] = sent;
    else
      ((int*)a.route_out)[r] = (int)sent;
  }
}

}  // namespace

void beam_reorder(torch::Tensor table, std::vector<torch::Tensor> src,
                  std::vector<torch::Tensor> dst, torch::Tensor y_out,
                  torch::Tensor route_out, long n_prev) {
  const long nbuf = (long)src.size();
  TORCH_CHECK(nbuf >= 1 && nbuf <= MAX_BUF && (long)dst.size() == nbuf,
              "beam_reorder: need 1 to ", MAX_BUF,
              " src buffers and as many dst buffers");
  TORCH_CHECK(table.is_cuda() && table.dtype() == torch::kInt64 &&
                  table.dim() == 2 && table.size(0) == 3 &&
                  table.is_contiguous(),
              "beam_reorder: table must be a contiguous (3, L) int64 GPU "
              "tensor");
  TORCH_CHECK(y_out.is_cuda() && y_out.dtype() == torch::kInt64 &&
                  y_out.dim() == 1 && y_out.is_contiguous(),
              "beam_reorder: y_out must be a contiguous (Rmax,) int64 GPU "
              "tensor");
  const long L = table.size(1), Rmax = y_out.size(0);
  TORCH_CHECK(route_out.is_cuda() && route_out.dim() == 1 &&
                  route_out.is_contiguous() && route_out.size(0) == Rmax &&
                  (route_out.dtype() == torch::kInt64 ||
                   route_out.dtype() == torch::kInt32),
              "beam_reorder: route_out must be a contiguous (Rmax,) int64 or "
              "int32 GPU tensor");
  TORCH_CHECK(L >= 1 && L <= Rmax, "beam_reorder: L = ", L,
              " outside [1, Rmax = ", Rmax, "]");
  TORCH_CHECK(n_prev >= 1, "beam_reorder: n_prev = ", n_prev);

  ReorderArgs a;
  int segs = 0;
  for (long j = 0; j < MAX_BUF; ++j) {
    a.src[j] = nullptr;
    a.dst[j] = nullptr;
    a.D[j] = 0;
    a.seg_end[j] = segs;
    if (j >= nbuf) continue;
    const auto& s = src[j];
    const auto& d = dst[j];
    TORCH_CHECK(s.is_cuda() && d.is_cuda() && s.dtype() == torch::kFloat32 &&
                    d.dtype() == torch::kFloat32 && s.dim() == 2 &&
                    d.dim() == 2 && s.is_contiguous() && d.is_contiguous(),
                "beam_reorder: src and dst must be contiguous 2-d fp32 GPU "
                "tensors");
    const long D = s.size(1);
    TORCH_CHECK(D >= 1 && D < (1L << 30) && d.size(1) == D &&
                    d.size(0) == Rmax && s.size(0) >= n_prev,
                "beam_reorder: buffer ", j, ": src (", s.size(0), ", ", D,
                ") / dst (", d.size(0), ", ", d.size(1),
                ") do not fit n_prev = ", n_prev, ", Rmax = ", Rmax);
    a.src[j] = s.data_ptr<float>();
    a.dst[j] = d.data_ptr<float>();
    a.D[j] = (int)D;
    segs += cdiv((int)D, SEG);
    a.seg_end[j] = segs;
  }
  TORCH_CHECK(Rmax < (1L << 31) && segs <= 65535,
              "beam_reorder: grid too large");
  a.table = table.data_ptr<int64_t>();
  a.y_out = y_out.data_ptr<int64_t>();
  a.route_out = route_out.data_ptr();
  a.route64 = route_out.dtype() == torch::kInt64;
  a.nbuf = (int)nbuf;
  a.L = (int)L;
  a.n_prev = (int)std::min<long>(n_prev, 1L << 30);
  hipLaunchKernelGGL(beam_reorder_kernel, dim3((unsigned)Rmax, (unsigned)segs),
                     dim3(BLOCK), 0, at::cuda::getCurrentCUDAStream().stream(),
                     a);
  HIP_CHECK(hipGetLastError());
}
