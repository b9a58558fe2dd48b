// Global-norm gradient clipping for the dense clock (gradclip.h states the rule): one read pass over the
// gradient leaves fp64 partial sums of squares per workgroup (grad_sumsq), and the Adam that applies the
// shard folds those partials itself at its launch boundary (adam_clip_apply) -- no host sync, no atomics,
// no cross-workgroup communication, the same bits on every launch and every HIP-graph replay.
#include <stdexcept>
#include <string>

#include "common.h"
#include "dense_update.h"
#include "gradclip.h"

namespace minips_k {

namespace {

constexpr int kBlock = 256;

// a float squared is exact in fp64 (48 significant bits), so the sum differs from any other order of
// the same terms by rounding of the additions only
__device__ __forceinline__ double sq_acc(double acc, float4 G) {
  acc = fma((double)G.x, (double)G.x, acc);
  acc = fma((double)G.y, (double)G.y, acc);
  acc = fma((double)G.z, (double)G.z, acc);
  return fma((double)G.w, (double)G.w, acc);
}

// the workgroup's sum in one fixed order (xor butterfly inside each wave, then the four waves' sums
// added left to right by every thread): all 256 threads return the same bits
__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

}  // namespace

__global__ __launch_bounds__(kBlock) void grad_sumsq_kernel(const float* __restrict__ g, int64_t n4, AdamSlabs sl,
                                                            double* __restrict__ part) {
  __shared__ double sh[kBlock / 64];
  const float4* g4 = reinterpret_cast<const float4*>(g);
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (sl.n == 0) {  // the plain stream: four 16-byte loads in flight per lane
    for (; i + 3 * stride < n4; i += 4 * stride) {
      const float4 G0 = g4[i], G1 = g4[i + stride], G2 = g4[i + 2 * stride], G3 = g4[i + 3 * stride];
      a0 = sq_acc(a0, G0);
      a1 = sq_acc(a1, G1);
      a2 = sq_acc(a2, G2);
      a3 = sq_acc(a3, G3);
    }
  }
  for (; i < n4; i += stride) a0 = sq_acc(a0, slab_fold<true>(g4[i], i, sl));
  const double t = block_sum((a0 + a1) + (a2 + a3), sh);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

__global__ __launch_bounds__(kBlock) void adam_clip_kernel(float* __restrict__ w, float* __restrict__ m,
                                                           float* __restrict__ v, float* __restrict__ g, int64_t n4,
                                                           float lr, float b1, float b2, float eps, float wd,
                                                           float bc1, float bc2, bf16_t* __restrict__ wb,
                                                           const int* __restrict__ step_dev, bool zero_g,
                                                           AdamSlabs sl, const double* __restrict__ part, int np,
                                                           double max_norm, double* __restrict__ stats,
                                                           bool write_stats) {
  __shared__ double sh[kBlock / 64];
  // launch-boundary combine of the partial sums: the same order in every workgroup of every launch
  double a = 0.0;
  for (int k = threadIdx.x; k < np; k += kBlock) a += part[k];
  const double total = block_sum(a, sh);
  const bool skip = !isfinite(total);
  const double norm = sqrt(total);
  float gscale = 1.f;
  if (!skip) {
    const double scale_d = max_norm / (norm + 1e-6);
    if (scale_d < 1.0) gscale = (float)scale_d;
  }
  if (write_stats && blockIdx.x == 0 && threadIdx.x == 0) {
    stats[0] = norm;
    stats[1] = skip ? 0.0 : (double)gscale;
    if (skip)
      stats[3] += 1.0;
    else if (gscale < 1.f)
      stats[2] += 1.0;
  }
  if (skip) {  // a non-finite gradient: nothing applied, the accumulator still cleared
    if (zero_g)
      for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x)
        reinterpret_cast<float4*>(g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  if (step_dev) {  // device-side step (graph-replayable clocks): bias corrections from *step_dev
    const float t = (float)*step_dev;
    bc1 = 1.f - powf(b1, t);
    bc2 = 1.f - powf(b2, t);
  }
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x)
    adam_update4(w, m, v, g, i, sl, lr, b1, b2, eps, wd, bc1, bc2, gscale, wb, zero_g);
}

static void check_vec(const void* p, int64_t n, const char* what) {
  if (n % 4 || (reinterpret_cast<uintptr_t>(p) & 15))
    throw std::runtime_error(std::string(what) + " must be 16-byte aligned and hold a multiple of 4 floats");
}

void grad_sumsq(const float* g, int64_t n, const AdamSlabs* slabs, double* part, int L, hipStream_t s) {
  if (L < 1 || L > kSumsqMaxBlocks) throw std::runtime_error("grad_sumsq: L must be in [1, 1024]");
  if (n < 0) throw std::runtime_error("grad_sumsq: g holds a negative count");
  check_vec(g, n, "grad_sumsq: g");
  const AdamSlabs sl = checked_slabs(slabs, n, "grad_sumsq");
  hipLaunchKernelGGL(grad_sumsq_kernel, L, kBlock, 0, s, g, n / 4, sl, part);
  MINIPS_HIP_CHECK(hipGetLastError());
}

void adam_clip_apply(float* w, float* m, float* v, float* g, int64_t n, const AdamSlabs* slabs, float lr,
                     float beta1, float beta2, float eps, float weight_decay, int step, const int* step_dev,
                     bf16_t* w_bf16, bool zero_g, const double* part, int np, double max_norm, double* stats,
                     bool write_stats, hipStream_t s) {
  if (np < 1 || np > kClipMaxParts) throw std::runtime_error("adam_clip_apply: np must be in [1, 4096]");
  const AdamSlabs sl = checked_slabs(slabs, n, "adam_clip_apply");
  if (n <= 0) return;
  check_vec(w, n, "adam_clip_apply: w");
  check_vec(m, n, "adam_clip_apply: m");
  check_vec(v, n, "adam_clip_apply: v");
  check_vec(g, n, "adam_clip_apply: g");
  if (w_bf16 && (reinterpret_cast<uintptr_t>(w_bf16) & 7))
    throw std::runtime_error("adam_clip_apply: w_bf16 must be 8-byte aligned");
  const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
  hipLaunchKernelGGL(adam_clip_kernel, grid_for(n / 4, kBlock), kBlock, 0, s, w, m, v, g, n / 4, lr, beta1, beta2,
                     eps, weight_decay, bc1, bc2, w_bf16, step_dev, zero_g, sl, part, np, max_norm, stats,
                     write_stats);
  MINIPS_HIP_CHECK(hipGetLastError());
}

}  // namespace minips_k
