// Grid barrier of the persistent GRU scans (gru_scan.hip), also driven on
// its own by the micro-benchmark in barrier_bench.hip.
//
// XCD-hierarchical grid barrier (microarch 'barrier-xcd' scheme). Blocks
// are bucketed by their REAL XCC id (s_getreg XCC_ID, gfx942/950 —
// amd_device_functions.h:754-793), established once by a census at kernel
// start (nats_barrier_init). Per barrier, only the LAST ARRIVER of each
// XCD executes the agent-release fence (ONE buffer_wbl2 L2 writeback per
// XCD instead of one per block — the per-block variant measured 7.8us at
// 126 WGs / 12.1us at 256; see profiles/barrier_bench.json); it then
// arrives at the top counter, acquire-fences, and publishes the XCD's
// generation word. Non-leaders poll their XCD's generation word and
// acquire-fence (buffer_inv) before returning. Correctness relies only on
// bucket == physical XCD (true by construction from XCC_ID): the leader's
// wbl2 flushes exactly the L2 holding its co-located blocks' drained
// (vmcnt(0)) stores.
#pragma once

#include "common.h"

// Sync layout (zeroed per launch), as word offsets into one barrier's slab:
constexpr int NATS_SYNC_ARRIVE = 0;    // [8] per-XCD arrive (nper*epoch)
constexpr int NATS_SYNC_TOP = 8;       // top counter (nxcd*epoch)
constexpr int NATS_SYNC_GEN = 9;       // [8] per-XCD generation words
constexpr int NATS_SYNC_GIVE_UP = 17;  // give-up flag (host sees NaN poison)
constexpr int NATS_SYNC_CENSUS = 18;   // [8] resident blocks per XCD
constexpr int NATS_SYNC_CENSUS_ARRIVE = 26;
constexpr int NATS_SYNC_WORDS = 27;

struct NatsBarrierCtx {  // valid on thread 0 only
  unsigned bucket;  // this block's physical XCD (0..7)
  unsigned nper;    // blocks resident on this XCD
  unsigned ntop;    // number of XCDs with >=1 block
};

__device__ __forceinline__ unsigned nats_xcc_id() {
  // s_getreg_b32 XCC_ID[3:0] (hwreg 20), gfx942/950
  return __builtin_amdgcn_s_getreg((3u << 11) | (0u << 6) | 20u) & 7u;
}

__device__ __forceinline__ bool nats_barrier_init(unsigned* sync,
                                                  unsigned nwg,
                                                  NatsBarrierCtx& ctx) {
  __shared__ unsigned sh[4];
  if (threadIdx.x == 0) {
    const unsigned xcc = nats_xcc_id();
    unsigned* census = sync + NATS_SYNC_CENSUS;
    unsigned* census_arrive = sync + NATS_SYNC_CENSUS_ARRIVE;
    unsigned* give_up = sync + NATS_SYNC_GIVE_UP;
    __hip_atomic_fetch_add(census + xcc, 1u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(census_arrive, 1u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    unsigned ok = 1u, spins = 0u;
    while (__hip_atomic_load(census_arrive, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT) < nwg) {
      if (__hip_atomic_load(give_up, __ATOMIC_RELAXED,
                            __HIP_MEMORY_SCOPE_AGENT) != 0u ||
          ++spins > 200000000u) {
        __hip_atomic_store(give_up, 1u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        ok = 0u;
        break;
      }
      __builtin_amdgcn_s_sleep(2);
    }
    unsigned ntop = 0u;
    for (int i = 0; i < 8; ++i)
      ntop += (__hip_atomic_load(census + i, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT) != 0u);
    sh[0] = xcc;
    sh[1] = __hip_atomic_load(census + xcc, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT);
    sh[2] = ntop;
    sh[3] = ok;
  }
  __syncthreads();
  ctx.bucket = sh[0];
  ctx.nper = sh[1];
  ctx.ntop = sh[2];
  return sh[3] != 0u;
}

__device__ __forceinline__ bool nats_grid_barrier(unsigned* sync,
                                                  unsigned epoch,
                                                  const NatsBarrierCtx& ctx) {
  __shared__ unsigned ok_sh;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // stores drained to L2
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned* arrive = sync + NATS_SYNC_ARRIVE + ctx.bucket;
    unsigned* top = sync + NATS_SYNC_TOP;
    unsigned* gen = sync + NATS_SYNC_GEN + ctx.bucket;
    unsigned* give_up = sync + NATS_SYNC_GIVE_UP;
    unsigned ok = 1u, spins = 0u;

    const unsigned prev = __hip_atomic_fetch_add(
        arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev + 1u == ctx.nper * epoch) {
      // last arriver on this XCD: one L2 writeback covers every
      // co-located block's (already vmcnt-drained) stores
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      __hip_atomic_fetch_add(top, 1u, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
      for (;;) {
        if (__hip_atomic_load(top, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT) >= ctx.ntop * epoch)
          break;
        if (__hip_atomic_load(give_up, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT) != 0u ||
            ++spins > 200000000u) {
          __hip_atomic_store(give_up, 1u, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
          ok = 0u;
          break;
        }
        __builtin_amdgcn_s_sleep(2);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      __hip_atomic_store(gen, epoch, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    } else {
      for (;;) {
        if (__hip_atomic_load(gen, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT) >= epoch)
          break;
        if (__hip_atomic_load(give_up, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT) != 0u ||
            ++spins > 200000000u) {
          __hip_atomic_store(give_up, 1u, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
          ok = 0u;
          break;
        }
        __builtin_amdgcn_s_sleep(2);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    ok_sh = ok;
  }
  __syncthreads();
  return ok_sh != 0u;
}
