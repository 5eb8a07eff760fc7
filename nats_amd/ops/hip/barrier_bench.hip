// Grid-barrier micro-benchmark: isolates the per-step sync cost of the
// persistent GRU scans (timing evidence in profiles/README.md; driven by
// tools/barrier_xcd_bench.py).

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "common.h"
#include "grid_barrier.h"

__global__ __launch_bounds__(384) void nats_barrier_bench_kernel(
    unsigned* sync, unsigned nwg, int iters, float* out) {
  NatsBarrierCtx bctx;
  if (!nats_barrier_init(sync, nwg, bctx)) return;
  for (int t = 0; t < iters; ++t) {
    if (!nats_grid_barrier(sync, (unsigned)(t + 1), bctx)) return;
  }
  if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0) out[0] = 1.f;
}

// Extra sync words of the XCD-constrained variant, after the barrier's own
constexpr int BENCH_CENSUS = NATS_SYNC_WORDS;           // [8] blocks per XCD
constexpr int BENCH_CENSUS_TOTAL = NATS_SYNC_WORDS + 8;
constexpr int BENCH_SLOT = NATS_SYNC_WORDS + 9;         // participant counter
constexpr int BENCH_DONE = NATS_SYNC_WORDS + 10;        // participants found
constexpr int BENCH_SYNC_WORDS = NATS_SYNC_WORDS + 12;

// XCD-constrained variant: measures whether co-locating all
// participants on few XCDs cuts the barrier floor (candidate fix for
// the encoder persistent-scan sync floor — VERDICT r1 weak #1). Launch
// overprovisions blocks; a census picks exactly `nwg` participants that
// sit on XCDs with id < nxcd; everyone else exits.
__global__ __launch_bounds__(384) void nats_barrier_bench_xcd_kernel(
    unsigned* sync, unsigned nwg, unsigned nxcd, unsigned launched,
    int iters, float* out) {
  __shared__ int role;  // 0 = exit, 1 = participate
  if (threadIdx.x == 0) {
    const unsigned xcc = nats_xcc_id();
    __hip_atomic_fetch_add(sync + BENCH_CENSUS + xcc, 1u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(sync + BENCH_CENSUS_TOTAL, 1u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    unsigned spins = 0;
    while (__hip_atomic_load(sync + BENCH_CENSUS_TOTAL, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT) < launched &&
           ++spins < 200000000u)
      __builtin_amdgcn_s_sleep(2);
    int take = 0;
    if (xcc < nxcd) {
      const unsigned slot = __hip_atomic_fetch_add(
          sync + BENCH_SLOT, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      take = (slot < nwg);
    }
    role = take;
  }
  __syncthreads();
  if (!role) return;

  NatsBarrierCtx bctx;
  if (!nats_barrier_init(sync, nwg, bctx)) return;
  for (int t = 0; t < iters; ++t) {
    if (!nats_grid_barrier(sync, (unsigned)(t + 1), bctx)) return;
  }
  if (threadIdx.x == 0)
    __hip_atomic_store(sync + BENCH_DONE, 1u, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = 1.f;
}

double barrier_bench_xcd(int nwg, int nxcd, int iters) {
  auto opts = torch::TensorOptions().dtype(torch::kInt32).device(torch::kCUDA);
  auto sync = torch::zeros({BENCH_SYNC_WORDS}, opts);
  auto out = torch::zeros(
      {1}, torch::TensorOptions().dtype(torch::kFloat32).device(torch::kCUDA));
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  // overprovision so the target XCDs hold >= nwg blocks after round-robin
  // dispatch (256 CUs / 8 XCDs; 2 blocks per CU fit at 384 threads)
  const unsigned launched =
      (unsigned)std::min(512, std::max(8 * ((nwg + nxcd - 1) / nxcd), 64));
  hipEvent_t e0, e1;
  HIP_CHECK(hipEventCreate(&e0));
  HIP_CHECK(hipEventCreate(&e1));
  HIP_CHECK(hipEventRecord(e0, stream));
  hipLaunchKernelGGL(nats_barrier_bench_xcd_kernel, dim3(launched), dim3(384),
                     0, stream, (unsigned*)sync.data_ptr<int>(),
                     (unsigned)nwg, (unsigned)nxcd, launched, iters,
                     out.data_ptr<float>());
  HIP_CHECK(hipEventRecord(e1, stream));
  HIP_CHECK(hipEventSynchronize(e1));
  float ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  TORCH_CHECK(sync[BENCH_DONE].item<int>() == 1,
              "xcd barrier bench gave up");
  return (double)ms * 1000.0 / iters;  // us per barrier (incl. census)
}

double barrier_bench(int nwg_x, int nwg_y, int iters) {
  auto opts = torch::TensorOptions().dtype(torch::kInt32).device(torch::kCUDA);
  auto sync = torch::zeros({NATS_SYNC_WORDS}, opts);
  auto out = torch::zeros(
      {1}, torch::TensorOptions().dtype(torch::kFloat32).device(torch::kCUDA));
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  hipEvent_t e0, e1;
  HIP_CHECK(hipEventCreate(&e0));
  HIP_CHECK(hipEventCreate(&e1));
  HIP_CHECK(hipEventRecord(e0, stream));
  hipLaunchKernelGGL(nats_barrier_bench_kernel, dim3(nwg_x, nwg_y), dim3(384),
                     0, stream, (unsigned*)sync.data_ptr<int>(),
                     (unsigned)(nwg_x * nwg_y), iters, out.data_ptr<float>());
  HIP_CHECK(hipEventRecord(e1, stream));
  HIP_CHECK(hipEventSynchronize(e1));
  float ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  TORCH_CHECK(out.item<float>() == 1.f, "barrier bench gave up");
  return (double)ms * 1000.0 / iters;  // us per barrier
}
