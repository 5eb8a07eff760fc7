// Common device helpers for the nats_amd CDNA4 (gfx950) kernels.
//
// Conventions:
//  * wavefront = 64 lanes; blocks are multiples of 64 threads,
//  * bf16 storage / fp32 accumulate via MFMA f32_16x16x32_bf16,
//  * fragment lane maps (verified on-device by mfma_selftest):
//      A (M16xK32): row = lane&15, k = (lane>>4)*8 + i   (i = 0..7)
//      B (K32xN16): col = lane&15, k = (lane>>4)*8 + i
//      C/D (16x16): col = lane&15, row = (lane>>4)*4 + i (i = 0..3)
//    With B stored TRANSPOSED (row-major N x K, "Bt"), both A and B
//    fragments are 16-byte contiguous loads — the layout every packed
//    weight buffer in this extension uses.
#pragma once

#include <hip/hip_runtime.h>

#define NATS_WAVE 64

typedef __bf16 bf16_t;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float nats_sigmoid(float x) {
  return 1.0f / (1.0f + __expf(-x));
}

// Load an 8-element bf16 fragment (16B) from a row-major [rows][ld] matrix:
// element (r, k0..k0+7). Caller guarantees 16B alignment of (base + r*ld + k).
__device__ __forceinline__ bf16x8 load_frag8(const bf16_t* base, int r,
                                             long ld, int k) {
  return *(const bf16x8*)(base + (long)r * ld + k);
}

// A-fragment for mfma_f32_16x16x32_bf16 from row-major [M][ld] (M>=16 rows
// starting at row0): lane-determined (row, k).
__device__ __forceinline__ bf16x8 frag_a_rowmajor(const bf16_t* base,
                                                  int row0, long ld, int k0) {
  const int lane = threadIdx.x & (NATS_WAVE - 1);
  return load_frag8(base, row0 + (lane & 15), ld, k0 + (lane >> 4) * 8);
}

// B-fragment from a TRANSPOSED row-major [N][ld] buffer (row = output col).
__device__ __forceinline__ bf16x8 frag_bt_rowmajor(const bf16_t* base,
                                                   int col0, long ld, int k0) {
  const int lane = threadIdx.x & (NATS_WAVE - 1);
  return load_frag8(base, col0 + (lane & 15), ld, k0 + (lane >> 4) * 8);
}

// Scatter a C/D fragment into a row-major [M][ld] float buffer at (row0, col0).
__device__ __forceinline__ void store_cd_rowmajor(float* base, const f32x4& d,
                                                  int row0, long ld,
                                                  int col0) {
  const int lane = threadIdx.x & (NATS_WAVE - 1);
  const int col = col0 + (lane & 15);
  const int rbase = row0 + (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) base[(long)(rbase + i) * ld + col] = d[i];
}

constexpr int JB = 16;  // output columns per workgroup (one MFMA N-tile)

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// Scatter a C/D fragment into one [32][JB+1] LDS tile (rows row0..row0+15):
// the MFMA -> pointwise exchange after every gate/recurrent K-loop.
__device__ __forceinline__ void store_cd_lds(float (*dst)[JB + 1],
                                             const f32x4& acc, int row0) {
  const int lane = threadIdx.x & (NATS_WAVE - 1);
  const int col = lane & 15;
  const int rbase = row0 + (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) dst[rbase + i][col] = acc[i];
}

// Block reductions: wave shuffle-down, one LDS slot per wave, thread 0
// combines the slots in wave order and broadcasts through a separate word.
// The scratch holds the largest legal block (1024 threads = 16 waves)
// whatever the launch width, and the trailing barrier keeps a following
// call from overwriting it while the result is still being read.
constexpr int NATS_MAX_WAVES = 1024 / NATS_WAVE;

// one scratch per kernel, shared by every reduction in it
__device__ __forceinline__ float* block_reduce_scratch() {
  __shared__ float red[NATS_MAX_WAVES + 1];  // per-wave slots | broadcast
  return red;
}

template <bool MAX>
__device__ __forceinline__ float block_reduce(float v) {
  auto op = [](float a, float b) { return MAX ? fmaxf(a, b) : a + b; };
  float* red = block_reduce_scratch();
#pragma unroll
  for (int off = NATS_WAVE / 2; off > 0; off >>= 1)
    v = op(v, __shfl_down(v, off));
  if ((threadIdx.x & (NATS_WAVE - 1)) == 0) red[threadIdx.x / NATS_WAVE] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    float r = MAX ? -INFINITY : 0.f;
    for (int w = 0; w < (int)blockDim.x / NATS_WAVE; ++w) r = op(r, red[w]);
    red[NATS_MAX_WAVES] = r;
  }
  __syncthreads();
  const float r = red[NATS_MAX_WAVES];
  __syncthreads();
  return r;
}

__device__ __forceinline__ float block_reduce_sum(float v) {
  return block_reduce<false>(v);
}
__device__ __forceinline__ float block_reduce_max(float v) {
  return block_reduce<true>(v);
}

// Block-wide unsigned 64-bit min, result in every thread, ONE barrier per
// call: a wave butterfly, one LDS slot per wave, then every thread combines
// the slots itself. Consecutive calls must alternate ``parity`` (0/1): the
// slots are double-buffered, so a call's writes cannot land in the buffer
// the previous call is still reading, and its own barrier orders the call
// before that one.
__device__ __forceinline__ unsigned long long block_min_u64(
    unsigned long long v, int parity) {
  __shared__ unsigned long long red64[2][NATS_MAX_WAVES];
#pragma unroll
  for (int off = NATS_WAVE / 2; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off);
    v = o < v ? o : v;
  }
  if ((threadIdx.x & (NATS_WAVE - 1)) == 0)
    red64[parity][threadIdx.x / NATS_WAVE] = v;
  __syncthreads();
  unsigned long long r = red64[parity][0];
  for (int w = 1; w < (int)blockDim.x / NATS_WAVE; ++w) {
    const unsigned long long o = red64[parity][w];
    r = o < r ? o : r;
  }
  return r;
}

// 4-deep software-pipelined MFMA K-loop: four iterations' fragment loads
// (both operands) stay in flight ahead of each MFMA so the L2 latency of
// the 16 scattered 16B lines per fragment amortises over 4 iterations.
// (The plain loop measured ~13.9us/step on gfx950 — latency-bound; the
// 2-deep variant was still ~30us on the K=3k decoder GEMMs.)
#define NATS_MFMA_KLOOP(ACC, APTR, AROW, ALD, BPTR, BROW, BLD, KBEG, KEND)   \
  do {                                                                       \
    const int _ke = (KEND);                                                  \
    int _k = (KBEG);                                                         \
    if (_k + 128 <= _ke) {                                                   \
      bf16x8 _a0 = frag_a_rowmajor((APTR), (AROW), (ALD), _k);               \
      bf16x8 _b0 = frag_bt_rowmajor((BPTR), (BROW), (BLD), _k);              \
      bf16x8 _a1 = frag_a_rowmajor((APTR), (AROW), (ALD), _k + 32);          \
      bf16x8 _b1 = frag_bt_rowmajor((BPTR), (BROW), (BLD), _k + 32);         \
      bf16x8 _a2 = frag_a_rowmajor((APTR), (AROW), (ALD), _k + 64);          \
      bf16x8 _b2 = frag_bt_rowmajor((BPTR), (BROW), (BLD), _k + 64);         \
      bf16x8 _a3 = frag_a_rowmajor((APTR), (AROW), (ALD), _k + 96);          \
      bf16x8 _b3 = frag_bt_rowmajor((BPTR), (BROW), (BLD), _k + 96);         \
      for (_k += 128; _k + 32 <= _ke; _k += 32) {                            \
        bf16x8 _an = frag_a_rowmajor((APTR), (AROW), (ALD), _k);             \
        bf16x8 _bn = frag_bt_rowmajor((BPTR), (BROW), (BLD), _k);            \
        ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(_a0, _b0, ACC, 0, 0, 0);\
        _a0 = _a1; _b0 = _b1; _a1 = _a2; _b1 = _b2;                          \
        _a2 = _a3; _b2 = _b3; _a3 = _an; _b3 = _bn;                          \
      }                                                                      \
      ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(_a0, _b0, ACC, 0, 0, 0); \
      ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(_a1, _b1, ACC, 0, 0, 0); \
      ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(_a2, _b2, ACC, 0, 0, 0); \
      ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(_a3, _b3, ACC, 0, 0, 0); \
    } else {                                                                 \
      for (; _k < _ke; _k += 32) {                                           \
        bf16x8 _a0 = frag_a_rowmajor((APTR), (AROW), (ALD), _k);             \
        bf16x8 _b0 = frag_bt_rowmajor((BPTR), (BROW), (BLD), _k);            \
        ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(_a0, _b0, ACC, 0, 0, 0);\
      }                                                                      \
    }                                                                        \
  } while (0)

#define HIP_CHECK(expr)                                              \
  do {                                                               \
    hipError_t _e = (expr);                                          \
    if (_e != hipSuccess) {                                          \
      TORCH_CHECK(false, "HIP error: ", hipGetErrorString(_e), " at ",\
                  __FILE__, ":", __LINE__);                          \
    }                                                                \
  } while (0)
