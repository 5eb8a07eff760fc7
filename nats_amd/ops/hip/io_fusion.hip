// Glue kernels around the training scans: the passes torch makes between
// the hipBLASLt GEMMs and the scan / softmax kernels (bias add with an
// fp32 round trip, bf16<->fp32 copies, column sums over fp32 copies, the
// casts of the encoder context and the cast / add / slice / flip chain of
// its gradient) done in one pass each over the bf16 or fp32 data as it
// already lies. The masked mean of the context is not computed here: it
// stays torch's reduction (ops/io_fusion.py says why).
//
//   bias_cast_      y = bf16(float(g) + b), in place on the GEMM result
//   colsum_bf16     out[n] = sum_r g[r][n] over a strided bf16 matrix
//   ctx_head_fwd    ctx_bf = bf16([h_f | flip(h_r)])
//   ctx_head_bwd    the three gradient terms of ctx summed into the two
//                   fp32 [T,B,H] tensors the scan backward reads
//
// The column sum is two-stage with a fixed summation order (no float
// atomics): results are reproducible run to run.

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "common.h"

namespace {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int IO_BLOCK = 256;
constexpr int IO_WAVES = IO_BLOCK / NATS_WAVE;

// rows one colsum block reduces (IO_WAVES waves x 32 rows each)
constexpr int COLSUM_ROWS = 128;
// timesteps one ctx_head block walks
constexpr int CTX_TCHUNK = 16;

inline bool aligned_to(const void* p, size_t a) {
  return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0;
}

inline int grid_for(long work, int per_block, int cap) {
  long g = (work + per_block - 1) / per_block;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// ---- bias_cast ---------------------------------------------------------

// 8 bf16 per thread per iteration; requires N % 8 == 0 and 16B-aligned g,
// 16B-aligned b
__global__ void bias_cast_vec_kernel(bf16_t* __restrict__ g,
                                     const float* __restrict__ b, long n8,
                                     int N) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8;
       i += stride) {
    const int n = (int)((i * 8) % N);
    bf16x8 v = *(const bf16x8*)(g + i * 8);
    const f32x4 b0 = *(const f32x4*)(b + n);
    const f32x4 b1 = *(const f32x4*)(b + n + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = (bf16_t)((float)v[j] + b0[j]);
      v[4 + j] = (bf16_t)((float)v[4 + j] + b1[j]);
    }
    *(bf16x8*)(g + i * 8) = v;
  }
}

__global__ void bias_cast_scalar_kernel(bf16_t* __restrict__ g,
                                        const float* __restrict__ b,
                                        long total, int N) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride)
    g[i] = (bf16_t)((float)g[i] + b[i % N]);
}

// ---- colsum_bf16 -------------------------------------------------------

// block = IO_WAVES waves; every wave covers the same 64*VEC columns and
// rows (w, w+IO_WAVES, ...) of the block's COLSUM_ROWS chunk; the waves'
// sums are combined through LDS in wave order. part[chunk][n].
template <int VEC>
__global__ void colsum_partial_kernel(const bf16_t* __restrict__ g, long ld,
                                      int R, int N,
                                      float* __restrict__ part) {
  __shared__ float red[IO_WAVES][NATS_WAVE * VEC];
  const int lane = threadIdx.x & (NATS_WAVE - 1);
  const int w = threadIdx.x / NATS_WAVE;
  const int n0 = (blockIdx.x * NATS_WAVE + lane) * VEC;
  const int r0 = blockIdx.y * COLSUM_ROWS;
  const int r1 = min(r0 + COLSUM_ROWS, R);
  float acc[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
  if (n0 < N) {  // N % VEC == 0: a vector is inside or outside as a whole
#pragma unroll 4
    for (int r = r0 + w; r < r1; r += IO_WAVES) {
      const bf16_t* p = g + (long)r * ld + n0;
      if (VEC == 4) {
        const bf16x4 v = *(const bf16x4*)p;
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[j] += (float)v[j];
      } else {
        acc[0] += (float)p[0];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) red[w][lane * VEC + j] = acc[j];
  __syncthreads();
  if (w == 0 && n0 < N) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float s = red[0][lane * VEC + j];
      for (int k = 1; k < IO_WAVES; ++k) s += red[k][lane * VEC + j];
      part[(long)blockIdx.y * N + n0 + j] = s;
    }
  }
}

// out[n] = sum_c part[c][n] in a fixed order: four interleaved chains
// (chunk c goes to chain c % 4) combined as (s0 + s1) + (s2 + s3), so the
// dependent adds per thread are a quarter of nchunk
__global__ void colsum_final_kernel(const float* __restrict__ part,
                                    int nchunk, int N,
                                    float* __restrict__ out) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int c = 0;
#pragma unroll 2
  for (; c + 4 <= nchunk; c += 4) {
    s0 += part[(long)c * N + n];
    s1 += part[(long)(c + 1) * N + n];
    s2 += part[(long)(c + 2) * N + n];
    s3 += part[(long)(c + 3) * N + n];
  }
  if (c < nchunk) s0 += part[(long)c * N + n];
  if (c + 1 < nchunk) s1 += part[(long)(c + 1) * N + n];
  if (c + 2 < nchunk) s2 += part[(long)(c + 2) * N + n];
  out[n] = (s0 + s1) + (s2 + s3);
}

// ---- context head ------------------------------------------------------

// flat column j = b*2H + c over BC = B*2H; thread owns VEC consecutive
// columns (H % VEC == 0, so they lie in one half) and walks CTX_TCHUNK
// timesteps of ctx_bf[t][j..]
template <int VEC>
__global__ void ctx_head_fwd_kernel(const float* __restrict__ hf,
                                    const float* __restrict__ hr,
                                    bf16_t* __restrict__ ctx, int T, int B,
                                    int H) {
  const long BC = (long)B * 2 * H;
  const long j = ((long)blockIdx.x * blockDim.x + threadIdx.x) * VEC;
  if (j >= BC) return;
  const int b = (int)(j / (2 * H));
  const int c = (int)(j % (2 * H));
  const bool rev = c >= H;
  const long BH = (long)B * H;
  const long src_off = (long)b * H + (rev ? c - H : c);
  const float* src = rev ? hr : hf;
  const int t0 = blockIdx.y * CTX_TCHUNK;
  const int t1 = min(t0 + CTX_TCHUNK, T);
#pragma unroll 4
  for (int t = t0; t < t1; ++t) {
    const int ts = rev ? T - 1 - t : t;
    const float* p = src + (long)ts * BH + src_off;
    bf16_t* o = ctx + (long)t * BC + j;
    if (VEC == 4) {
      const f32x4 v = *(const f32x4*)p;
      bf16x4 q;
#pragma unroll
      for (int k = 0; k < VEC; ++k) q[k] = (bf16_t)v[k];
      *(bf16x4*)o = q;
    } else {
      o[0] = (bf16_t)p[0];
    }
  }
}

// dh_f[t][b][c]       = d(t, b, c)        c <  H
// dh_r[T-1-t][b][c-H] = d(t, b, c)        c >= H
// d = float(denc[t][b][c]) + float(dproj[t][b][c])
//     + mask[t][b] * (dmean[b][c] / cnt[b])
// denc has element strides (es_t, es_b, 1); dproj is contiguous.
template <int VEC>
__global__ void ctx_head_bwd_kernel(const bf16_t* __restrict__ denc,
                                    long es_t, long es_b,
                                    const bf16_t* __restrict__ dproj,
                                    const float* __restrict__ dmean,
                                    const float* __restrict__ mask,  // or null
                                    const float* __restrict__ cnt,
                                    float* __restrict__ dhf,
                                    float* __restrict__ dhr, int T, int B,
                                    int H) {
  const long BC = (long)B * 2 * H;
  const long j = ((long)blockIdx.x * blockDim.x + threadIdx.x) * VEC;
  if (j >= BC) return;
  const int b = (int)(j / (2 * H));
  const int c = (int)(j % (2 * H));
  const bool rev = c >= H;
  const long BH = (long)B * H;
  const long dst_off = (long)b * H + (rev ? c - H : c);
  float* dst = rev ? dhr : dhf;
  const float n = cnt[b];
  float dm[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) dm[k] = dmean[(long)b * 2 * H + c + k] / n;
  const int t0 = blockIdx.y * CTX_TCHUNK;
  const int t1 = min(t0 + CTX_TCHUNK, T);
#pragma unroll 4
  for (int t = t0; t < t1; ++t) {
    const int td = rev ? T - 1 - t : t;
    const float m = mask ? mask[(long)t * B + b] : 1.f;
    const bf16_t* pe = denc + (long)t * es_t + (long)b * es_b + c;
    const bf16_t* pp = dproj + (long)t * BC + j;
    float* o = dst + (long)td * BH + dst_off;
    if (VEC == 4) {
      const bf16x4 e = *(const bf16x4*)pe;
      const bf16x4 p = *(const bf16x4*)pp;
      f32x4 r;
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        r[k] = ((float)e[k] + (float)p[k]) + m * dm[k];
      *(f32x4*)o = r;
    } else {
      o[0] = ((float)pe[0] + (float)pp[0]) + m * dm[0];
    }
  }
}

}  // namespace

long colsum_rows_per_block() { return COLSUM_ROWS; }

torch::Tensor bias_cast_(torch::Tensor g, torch::Tensor b) {
  TORCH_CHECK(g.is_cuda() && g.dtype() == torch::kBFloat16 &&
              g.is_contiguous() && g.dim() >= 1, "bias_cast_: g must be a "
              "contiguous bf16 CUDA tensor");
  const long N = g.size(-1);
  TORCH_CHECK(b.is_cuda() && b.dtype() == torch::kFloat32 &&
              b.is_contiguous() && b.dim() == 1 && b.size(0) == N,
              "bias_cast_: b must be contiguous fp32 of g's last size");
  const long total = g.numel();
  if (total == 0) return g;
  TORCH_CHECK(N < (1L << 31));
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  bf16_t* gp = (bf16_t*)g.data_ptr();
  const float* bp = b.data_ptr<float>();
  if (N % 8 == 0 && aligned_to(gp, 16) && aligned_to(bp, 16)) {
    const long n8 = total / 8;
    hipLaunchKernelGGL(bias_cast_vec_kernel,
                       dim3(grid_for(n8, IO_BLOCK, 256 * 16)), dim3(IO_BLOCK),
                       0, stream, gp, bp, n8, (int)N);
  } else {
    hipLaunchKernelGGL(bias_cast_scalar_kernel,
                       dim3(grid_for(total, IO_BLOCK, 256 * 16)),
                       dim3(IO_BLOCK), 0, stream, gp, bp, total, (int)N);
  }
  HIP_CHECK(hipGetLastError());
  return g;
}

torch::Tensor colsum_bf16(torch::Tensor g) {
  TORCH_CHECK(g.is_cuda() && g.dtype() == torch::kBFloat16 && g.dim() == 2,
              "colsum_bf16: g must be a 2-d bf16 CUDA tensor");
  const long R = g.size(0), N = g.size(1);
  TORCH_CHECK(N == 1 || g.stride(1) == 1,
              "colsum_bf16: columns must be unit-stride");
  const long ld = R > 1 ? g.stride(0) : N;
  TORCH_CHECK(ld >= N && R < (1L << 31) && N < (1L << 31));
  auto optsF = g.options().dtype(torch::kFloat32);
  auto out = torch::empty({N}, optsF);
  if (N == 0) return out;
  if (R == 0) return out.zero_();
  const int nchunk = cdiv((int)R, COLSUM_ROWS);
  TORCH_CHECK(nchunk <= 65535, "colsum_bf16: too many rows");
  auto part = torch::empty({nchunk, N}, optsF);
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  const bf16_t* gp = (const bf16_t*)g.data_ptr();
  if (N % 4 == 0 && ld % 4 == 0 && aligned_to(gp, 8)) {
    hipLaunchKernelGGL(colsum_partial_kernel<4>,
                       dim3(cdiv((int)N, NATS_WAVE * 4), nchunk),
                       dim3(IO_BLOCK), 0, stream, gp, ld, (int)R, (int)N,
                       part.data_ptr<float>());
  } else {
    hipLaunchKernelGGL(colsum_partial_kernel<1>,
                       dim3(cdiv((int)N, NATS_WAVE), nchunk), dim3(IO_BLOCK),
                       0, stream, gp, ld, (int)R, (int)N,
                       part.data_ptr<float>());
  }
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(colsum_final_kernel, dim3(cdiv((int)N, IO_BLOCK)),
                     dim3(IO_BLOCK), 0, stream, part.data_ptr<float>(),
                     nchunk, (int)N, out.data_ptr<float>());
  HIP_CHECK(hipGetLastError());
  return out;
}

// (h_f, h_r [T,B,H] fp32) -> ctx_bf [T,B,2H] bf16, row t = [h_f[t] |
// h_r[T-1-t]]
torch::Tensor ctx_head_fwd(torch::Tensor hf, torch::Tensor hr) {
  TORCH_CHECK(hf.is_cuda() && hf.dtype() == torch::kFloat32 &&
              hf.dim() == 3 && hf.is_contiguous(),
              "ctx_head_fwd: h_f must be contiguous fp32 [T,B,H]");
  TORCH_CHECK(hr.is_cuda() && hr.dtype() == torch::kFloat32 &&
              hr.is_contiguous() && hr.sizes() == hf.sizes(),
              "ctx_head_fwd: h_r must match h_f");
  const long T = hf.size(0), B = hf.size(1), H = hf.size(2);
  TORCH_CHECK(T >= 1 && B >= 1 && H >= 1);
  const long C = 2 * H, BC = B * C;
  const int nchunk = cdiv((int)T, CTX_TCHUNK);
  TORCH_CHECK(nchunk <= 65535 && BC < (1L << 31));
  auto ctx = torch::empty({T, B, C}, hf.options().dtype(torch::kBFloat16));
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  if (H % 4 == 0) {  // torch allocations are >= 16B aligned
    hipLaunchKernelGGL(ctx_head_fwd_kernel<4>,
                       dim3(cdiv((int)(BC / 4), IO_BLOCK), nchunk),
                       dim3(IO_BLOCK), 0, stream, hf.data_ptr<float>(),
                       hr.data_ptr<float>(), (bf16_t*)ctx.data_ptr(), (int)T,
                       (int)B, (int)H);
  } else {
    hipLaunchKernelGGL(ctx_head_fwd_kernel<1>,
                       dim3(cdiv((int)BC, IO_BLOCK), nchunk), dim3(IO_BLOCK),
                       0, stream, hf.data_ptr<float>(), hr.data_ptr<float>(),
                       (bf16_t*)ctx.data_ptr(), (int)T, (int)B, (int)H);
  }
  HIP_CHECK(hipGetLastError());
  return ctx;
}

// (denc [T,B,2H] bf16 any strides with unit last, dproj [T,B,2H] bf16
// contiguous, dmean [B,2H] fp32, mask, cnt [B]) -> (dh_f, dh_r) fp32
// [T,B,H], dh_r in the reverse scan's own (flipped) time order
std::vector<torch::Tensor> ctx_head_bwd(torch::Tensor denc,
                                        torch::Tensor dproj,
                                        torch::Tensor dmean,
                                        c10::optional<torch::Tensor> mask,
                                        torch::Tensor cnt) {
  TORCH_CHECK(denc.is_cuda() && denc.dtype() == torch::kBFloat16 &&
              denc.dim() == 3, "ctx_head_bwd: denc must be bf16 [T,B,2H]");
  const long T = denc.size(0), B = denc.size(1), C = denc.size(2);
  TORCH_CHECK(C % 2 == 0 && T >= 1 && B >= 1 && C >= 2);
  const long H = C / 2;
  if (denc.stride(2) != 1) denc = denc.contiguous();
  TORCH_CHECK(dproj.is_cuda() && dproj.dtype() == torch::kBFloat16 &&
              dproj.is_contiguous() && dproj.sizes() == denc.sizes(),
              "ctx_head_bwd: dproj must be contiguous bf16 like denc");
  TORCH_CHECK(dmean.is_cuda() && dmean.dtype() == torch::kFloat32 &&
              dmean.is_contiguous() && dmean.dim() == 2 &&
              dmean.size(0) == B && dmean.size(1) == C,
              "ctx_head_bwd: dmean must be contiguous fp32 [B,2H]");
  TORCH_CHECK(cnt.is_cuda() && cnt.dtype() == torch::kFloat32 &&
              cnt.is_contiguous() && cnt.numel() == B);
  const float* mp = nullptr;
  if (mask.has_value()) {
    TORCH_CHECK(mask->is_cuda() && mask->dtype() == torch::kFloat32 &&
                mask->is_contiguous() && mask->dim() == 2 &&
                mask->size(0) == T && mask->size(1) == B,
                "ctx_head_bwd: mask must be contiguous fp32 [T,B]");
    mp = mask->data_ptr<float>();
  }
  const long BC = B * C;
  const int nchunk = cdiv((int)T, CTX_TCHUNK);
  TORCH_CHECK(nchunk <= 65535 && BC < (1L << 31));
  auto optsF = dmean.options();
  auto dhf = torch::empty({T, B, H}, optsF);
  auto dhr = torch::empty({T, B, H}, optsF);
  const long es_t = T > 1 ? denc.stride(0) : 0;
  const long es_b = B > 1 ? denc.stride(1) : 0;
  const bf16_t* ep = (const bf16_t*)denc.data_ptr();
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  if (H % 4 == 0 && es_t % 4 == 0 && es_b % 4 == 0 && aligned_to(ep, 8)) {
    hipLaunchKernelGGL(ctx_head_bwd_kernel<4>,
                       dim3(cdiv((int)(BC / 4), IO_BLOCK), nchunk),
                       dim3(IO_BLOCK), 0, stream, ep, es_t, es_b,
                       (const bf16_t*)dproj.data_ptr(),
                       dmean.data_ptr<float>(), mp, cnt.data_ptr<float>(),
                       dhf.data_ptr<float>(), dhr.data_ptr<float>(), (int)T,
                       (int)B, (int)H);
  } else {
    hipLaunchKernelGGL(ctx_head_bwd_kernel<1>,
                       dim3(cdiv((int)BC, IO_BLOCK), nchunk), dim3(IO_BLOCK),
                       0, stream, ep, es_t, es_b,
                       (const bf16_t*)dproj.data_ptr(),
                       dmean.data_ptr<float>(), mp, cnt.data_ptr<float>(),
                       dhf.data_ptr<float>(), dhr.data_ptr<float>(), (int)T,
                       (int)B, (int)H);
  }
  HIP_CHECK(hipGetLastError());
  return {dhf, dhr};
}
