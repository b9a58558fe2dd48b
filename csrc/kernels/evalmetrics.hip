// Held-out evaluation metrics on gfx950: binned-score histograms (exact AUC on the host) and a
// fixed-point log-loss sum, standalone (binary_hist) or fused behind the last layer's dot product
// (eval_head_hist). The per-sample rule is stated in evalmetrics.h; eval_sample below is its one
// device implementation, shared by both kernels.
//
// Accumulation: one pair of uint32 histograms per workgroup in LDS (LDS integer atomics), flushed
// once at the end with 64-bit global integer atomics, zero bins skipped; the loss sum and the NaN
// count are reduced per workgroup first. Integer sums only: no float atomics, no fences (nothing
// is read back inside the kernel), results independent of the launch shape.
#include <algorithm>
#include <stdexcept>
#include <string>

#include "common.h"
#include "evalmetrics.h"

namespace minips_k {

namespace {

constexpr int kEvalBlock = 256;
constexpr int kEvalWaves = kEvalBlock / kWave;
constexpr int kEvalHeadUnroll = 4;  // row groups a wave of eval_head_kernel keeps in flight

typedef unsigned long long u64;

struct EvalLocal {
  long long loss;  // sum of llrintf(l * 2^24) over this thread's samples
  unsigned nan;
};

__device__ __forceinline__ void eval_sample(float z, float label, int NB, unsigned* hneg, unsigned* hpos,
                                            EvalLocal& loc) {
  if (z != z) {
    loc.nan += 1;
    return;
  }
  const bool y = label > 0.5f;
  const float zc = fminf(fmaxf(z, -16.f), 16.f);
  // NB/32 is a power of two: the multiply is exact, only the add rounds
  int bin = (int)floorf((zc + 16.f) * (float)(NB >> 5));
  bin = bin < NB - 1 ? bin : NB - 1;
  atomicAdd((y ? hpos : hneg) + bin, 1u);
  const float zl = fminf(fmaxf(z, -64.f), 64.f);
  const float l = fmaxf(zl, 0.f) - zl * (y ? 1.f : 0.f) + log1pf(expf(-fabsf(zl)));
  loc.loss += llrintf(l * 16777216.f);
}

__device__ __forceinline__ void eval_zero(unsigned* hist, int NB) {
  for (int i = threadIdx.x; i < 2 * NB; i += blockDim.x) hist[i] = 0u;
  __syncthreads();
}

// the workgroup's histograms, loss sum and NaN count into acc (every thread of the block calls it)
__device__ __forceinline__ void eval_flush(const unsigned* hist, int NB, EvalLocal loc, int64_t* acc) {
  __shared__ long long s_loss[kEvalWaves];
  __shared__ unsigned s_nan[kEvalWaves];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    loc.loss += __shfl_xor(loc.loss, o, 64);
    loc.nan += __shfl_xor(loc.nan, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_loss[threadIdx.x >> 6] = loc.loss;
    s_nan[threadIdx.x >> 6] = loc.nan;
  }
  __syncthreads();  // (also: every LDS histogram add of the block is done)
  u64* out = reinterpret_cast<u64*>(acc);
  for (int i = threadIdx.x; i < 2 * NB; i += blockDim.x) {
    const unsigned v = hist[i];
    if (v) atomicAdd(out + i, (u64)v);
  }
  if (threadIdx.x == 0) {
    long long l = 0;
    unsigned nn = 0;
#pragma unroll
    for (int w = 0; w < kEvalWaves; ++w) {
      l += s_loss[w];
      nn += s_nan[w];
    }
    if (l) atomicAdd(out + 2 * NB, (u64)l);
    if (nn) atomicAdd(out + 2 * NB + 1, (u64)nn);
  }
}

__global__ __launch_bounds__(kEvalBlock) void binary_hist_kernel(const float* __restrict__ logits,
                                                                 const float* __restrict__ labels, int64_t n, int NB,
                                                                 int64_t* acc) {
  extern __shared__ unsigned hist[];  // neg[NB] | pos[NB]
  eval_zero(hist, NB);
  EvalLocal loc{0, 0u};
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride)
    eval_sample(logits[i], labels[i], NB, hist, hist + NB, loc);
  eval_flush(hist, NB, loc, acc);
}

// LPR lanes share one row (each loads 16-byte chunks of it: chunk c, c + LPR, ...), 64 / LPR rows per
// wave and iteration; the partial dot products are summed inside the LPR-lane group.
template <int LPR>
__global__ __launch_bounds__(kEvalBlock) void eval_head_kernel(const bf16_t* __restrict__ H, int64_t B, int Hd,
                                                               int64_t ld, const bf16_t* __restrict__ w,
                                                               const bf16_t* __restrict__ b0,
                                                               const float* __restrict__ wide,
                                                               const float* __restrict__ labels, int NB, int64_t* acc,
                                                               float* __restrict__ logits_out) {
  extern __shared__ unsigned hist[];
  eval_zero(hist, NB);
  EvalLocal loc{0, 0u};
  constexpr int RPW = kWave / LPR;
  const int lane = threadIdx.x & 63;
  const int sub = lane % LPR, rsub = lane / LPR;
  const int nchunks = Hd >> 3;
  const float bias = bf2f(b0[0]);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  // S row groups per iteration: their loads and group reductions are independent (ILP), so a wave pays
  // one memory round trip per S * RPW rows
  constexpr int S = kEvalHeadUnroll;
  for (int64_t base = wave * (RPW * S); base < B; base += nwaves * (RPW * S)) {  // (uniform per wave: shuffles)
    float part[S], wd[S], yv[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const int64_t row = base + s * RPW + rsub;
      part[s] = wd[s] = yv[s] = 0.f;
      if (row < B) {
        if (sub == 0) {  // loaded with the row, not after the reduction: one round trip
          wd[s] = wide ? wide[row] : 0.f;
          yv[s] = labels[row];
        }
        const bf16_t* hp = H + row * ld;
        for (int c = sub; c < nchunks; c += LPR) {
          const uint4 hv = *reinterpret_cast<const uint4*>(hp + c * 8);
          const uint4 wv = *reinterpret_cast<const uint4*>(w + c * 8);
          const uint32_t hh[4] = {hv.x, hv.y, hv.z, hv.w}, ww[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            part[s] += __uint_as_float(hh[j] << 16) * __uint_as_float(ww[j] << 16);
            part[s] += __uint_as_float(hh[j] & 0xffff0000u) * __uint_as_float(ww[j] & 0xffff0000u);
          }
        }
      }
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
#pragma unroll
      for (int o = LPR >> 1; o > 0; o >>= 1) part[s] += __shfl_xor(part[s], o, 64);
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const int64_t row = base + s * RPW + rsub;
      if (row < B && sub == 0) {
        const float z = part[s] + bias + wd[s];
        if (logits_out) logits_out[row] = z;
        eval_sample(z, yv[s], NB, hist, hist + NB, loc);
      }
    }
  }
  eval_flush(hist, NB, loc, acc);
}

void check_bins(int NB, const char* op) {
  if (NB < kEvalMinBins || NB > kEvalMaxBins || (NB & (NB - 1)))
    throw std::runtime_error(std::string(op) + ": NB must be a power of two in [32, 8192], got " +
                             std::to_string(NB));
}

}  // namespace

void binary_hist(const float* logits, const float* labels, int64_t n, int NB, int64_t* acc, hipStream_t s) {
  check_bins(NB, "binary_hist");
  if (n <= 0) return;
  const size_t lds = 2 * (size_t)NB * sizeof(unsigned);
  hipLaunchKernelGGL(binary_hist_kernel, grid_for(n, kEvalBlock, 1024), kEvalBlock, lds, s, logits, labels, n, NB,
                     acc);
  MINIPS_HIP_CHECK(hipGetLastError());
}

void eval_head_hist(const bf16_t* H, int64_t B, int Hd, int64_t ld, const bf16_t* w, const bf16_t* b0,
                    const float* wide, const float* labels, int NB, int64_t* acc, float* logits_out,
                    hipStream_t s) {
  check_bins(NB, "eval_head_hist");
  if (Hd < 8 || Hd > 1024 || Hd % 8 || ld < Hd || ld % 8)
    throw std::runtime_error("eval_head_hist: Hd % 8 == 0, 8 <= Hd <= 1024, ld >= Hd, ld % 8 == 0; got Hd " +
                             std::to_string(Hd) + ", ld " + std::to_string(ld));
  if (B <= 0) return;
  const size_t lds = 2 * (size_t)NB * sizeof(unsigned);
  int lpr = 1;
  while (lpr < kWave && lpr * 8 < Hd) lpr <<= 1;
  const int64_t rows_per_block = (int64_t)kEvalWaves * (kWave / lpr) * kEvalHeadUnroll;
  // a few workgroups per CU at most: each pays for zeroing and scanning its LDS histograms
  const int grid = (int)std::min<int64_t>((B + rows_per_block - 1) / rows_per_block, 1024);
#define MINIPS_EVAL_HEAD(L)                                                                                    \
  case L:                                                                                                      \
    hipLaunchKernelGGL(eval_head_kernel<L>, grid, kEvalBlock, lds, s, H, B, Hd, ld, w, b0, wide, labels, NB, acc, \
                       logits_out);                                                                            \
    break;
  switch (lpr) {
    MINIPS_EVAL_HEAD(1)
    MINIPS_EVAL_HEAD(2)
    MINIPS_EVAL_HEAD(4)
    MINIPS_EVAL_HEAD(8)
    MINIPS_EVAL_HEAD(16)
    MINIPS_EVAL_HEAD(32)
    MINIPS_EVAL_HEAD(64)
  }
#undef MINIPS_EVAL_HEAD
  MINIPS_HIP_CHECK(hipGetLastError());
}

}  // namespace minips_k
