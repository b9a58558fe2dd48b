// Row-wise Adagrad on the deep columns and FTRL-Proximal on the wide columns of split table rows, in one
// pass (wideftrl.h states the rule and the state layout). The same latency-bound gather as the row-wise
// Adagrad apply of sparse.hip -- key -> row -> read-modify-write -- and its two mappings:
//   16 < W <= 64, W % 4 == 0, D1 % 4 == 0   8 lanes per row, 8 rows per wave: lane l owns the float4 at 4l and
//                                           the one at 32 + 4l when that is below W; a float4 is all deep or
//                                           all wide, and a wide one also moves its z and n float4 of the
//                                           row's zn segment (addresses known as soon as the row is)
//   any other shape or alignment            one wave per row, lanes striding the columns, scalar accesses
// The vector form needs 16-byte aligned table, grads and zn and ld % 4 == 0; the launcher picks.
#include <stdexcept>
#include <string>

#include "common.h"
#include "ftrl_rule.h"
#include "wideftrl.h"

namespace minips_k {

namespace {

constexpr int kBlock = 256;

struct WideHyper {
  float lr, eps, grad_scale;
  FtrlHyper f;
};

__device__ __forceinline__ int64_t count_of(int64_t n, const int64_t* n_dev) { return n_dev ? min(n, *n_dev) : n; }

// the gradient an FTRL column sees: its own rounded product, never fused into the rule's z update
__device__ __forceinline__ float scaled(float g, float s) {
#pragma clang fp contract(off)
  return g * s;
}

// a deep square, rounded before it is added: the sequence sparse_rowwise_adagrad_v4_kernel compiles to (its
// squares feed two sums and stay separate multiplies), so the deep columns of the two kernels agree bit for bit
__device__ __forceinline__ float square(float g) {
#pragma clang fp contract(off)
  return g * g;
}

__device__ __forceinline__ float4 scaled4(const float4 g, float s) {
  return make_float4(scaled(g.x, s), scaled(g.y, s), scaled(g.z, s), scaled(g.w, s));
}

__global__ __launch_bounds__(kBlock) void adagrad_ftrl_v4_kernel(float* table, int64_t ld, float* state, float* zn,
                                                                 int64_t rows, int D1, int W,
                                                                 const int64_t* __restrict__ keys, int64_t n,
                                                                 const int64_t* n_dev, int64_t base,
                                                                 const float* __restrict__ grads, WideHyper h,
                                                                 int64_t* oor) {
  n = count_of(n, n_dev);
  const int lane = threadIdx.x & 63, sub = lane >> 3, l = lane & 7;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int Wf = W - D1;
  const int c0 = 4 * l, c1 = 32 + 4 * l;
  const bool has0 = c0 < W, has1 = c1 < W;  // W % 4 == 0: a float4 is all in or all out
  const bool wide0 = has0 && c0 >= D1, wide1 = has1 && c1 >= D1;  // D1 % 4 == 0: all deep or all wide
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t i0 = wave * 8; i0 < n; i0 += nwaves * 8) {
    const int64_t i = i0 + sub;
    bool ok = i < n;
    int64_t row = 0;
    if (ok) {
      row = keys[i] - base;
      if ((uint64_t)row >= (uint64_t)rows) {  // skipped whole: its lanes join the shuffles with zeros
        if (oor && l == 0) atomicAdd(reinterpret_cast<unsigned long long*>(oor), 1ull);
        ok = false;
        row = 0;
      }
    }
    float4 g0 = zero4, g1 = zero4, t0 = zero4, t1 = zero4, z0 = zero4, z1 = zero4, n0 = zero4, n1 = zero4;
    float* tr = table + row * ld;
    float* zr = zn + row * 2 * Wf;  // z of wide column c at zr[c - D1], n at zr[Wf + c - D1]
    if (ok && has0) {
      g0 = *reinterpret_cast<const float4*>(grads + i * W + c0);
      t0 = *reinterpret_cast<const float4*>(tr + c0);
      if (wide0) {
        z0 = *reinterpret_cast<const float4*>(zr + (c0 - D1));
        n0 = *reinterpret_cast<const float4*>(zr + Wf + (c0 - D1));
      }
      if (has1) {
        g1 = *reinterpret_cast<const float4*>(grads + i * W + c1);
        t1 = *reinterpret_cast<const float4*>(tr + c1);
        if (wide1) {
          z1 = *reinterpret_cast<const float4*>(zr + (c1 - D1));
          n1 = *reinterpret_cast<const float4*>(zr + Wf + (c1 - D1));
        }
      }
    }
    const float st_old = ok ? state[row] : 0.f;
    float sq1 = 0.f;
    const float a[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int c = (q < 4 ? c0 : c1) + (q & 3);
      const float sq = square(a[q]);
      if (c < D1) sq1 += sq;
    }
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) sq1 += __shfl_xor(sq1, o, 64);
    if (!ok) continue;
    const float st = st_old + sq1 / (float)D1;
    if (l == 0) state[row] = st;
    const float s1 = h.lr / (sqrtf(st) + h.eps);
    float o[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int c = (q < 4 ? c0 : c1) + (q & 3);
      if (c < D1) o[q] -= s1 * a[q];
    }
    float4 w0 = make_float4(o[0], o[1], o[2], o[3]), w1 = make_float4(o[4], o[5], o[6], o[7]);
    if (wide0) {
      ftrl_coord4(w0, z0, n0, scaled4(g0, h.grad_scale), h.f);
      *reinterpret_cast<float4*>(zr + (c0 - D1)) = z0;
      *reinterpret_cast<float4*>(zr + Wf + (c0 - D1)) = n0;
    }
    if (wide1) {
      ftrl_coord4(w1, z1, n1, scaled4(g1, h.grad_scale), h.f);
      *reinterpret_cast<float4*>(zr + (c1 - D1)) = z1;
      *reinterpret_cast<float4*>(zr + Wf + (c1 - D1)) = n1;
    }
    if (has0) *reinterpret_cast<float4*>(tr + c0) = w0;
    if (has1) *reinterpret_cast<float4*>(tr + c1) = w1;
  }
}

__global__ __launch_bounds__(kBlock) void adagrad_ftrl_kernel(float* table, int64_t ld, float* state, float* zn,
                                                              int64_t rows, int D1, int W,
                                                              const int64_t* __restrict__ keys, int64_t n,
                                                              const int64_t* n_dev, int64_t base,
                                                              const float* __restrict__ grads, WideHyper h,
                                                              int64_t* oor) {
  n = count_of(n, n_dev);
  const int lane = threadIdx.x & 63;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int Wf = W - D1;
  for (int64_t i = wave; i < n; i += nwaves) {
    const int64_t row = keys[i] - base;  // the same for every lane of the wave
    if ((uint64_t)row >= (uint64_t)rows) {
      if (oor && lane == 0) atomicAdd(reinterpret_cast<unsigned long long*>(oor), 1ull);
      continue;
    }
    const float* gr = grads + i * W;
    float sq1 = 0.f;
    for (int d = lane; d < D1; d += 64) {
      const float g = gr[d];
      sq1 += g * g;
    }
    sq1 = warp_sum(sq1);
    const float st = state[row] + sq1 / (float)D1;
    if (lane == 0) state[row] = st;
    const float s1 = h.lr / (sqrtf(st) + h.eps);
    float* tr = table + row * ld;
    float* zr = zn + row * 2 * Wf;
    for (int d = lane; d < W; d += 64) {
      const float g = gr[d];
      if (d < D1) {
        tr[d] -= s1 * g;
      } else {
        float w = tr[d], z = zr[d - D1], nn = zr[Wf + d - D1];
        ftrl_coord(w, z, nn, scaled(g, h.grad_scale), h.f);
        tr[d] = w;
        zr[d - D1] = z;
        zr[Wf + d - D1] = nn;
      }
    }
  }
}

}  // namespace

void sparse_adagrad_ftrl(float* table, int64_t ld, float* state, float* zn, int64_t rows, int D1, int W,
                         const int64_t* keys, int64_t n, const int64_t* n_dev, int64_t base, const float* grads,
                         float lr, float eps, float alpha, float beta, float l1, float l2, float grad_scale,
                         int64_t* oor, int blocks, hipStream_t s) {
  if (D1 < 1 || D1 >= W || ld < W) throw std::runtime_error("sparse_adagrad_ftrl: 1 <= D1 < W <= ld");
  if (blocks < 0 || blocks > kWideFtrlMaxBlocks)
    throw std::runtime_error("sparse_adagrad_ftrl: blocks outside [0, 65535]");
  if (n <= 0 || rows <= 0) return;
  const WideHyper h{lr, eps, grad_scale, FtrlHyper{alpha, beta, l1, l2}};
  const bool vec4 = W > 16 && W <= 64 && W % 4 == 0 && D1 % 4 == 0 && ld % 4 == 0 && aligned16(table) &&
                    aligned16(grads) && aligned16(zn);
  if (vec4) {
    const int grid = blocks > 0 ? blocks : grid_for(n * 8, kBlock, 16384);
    hipLaunchKernelGGL(adagrad_ftrl_v4_kernel, grid, kBlock, 0, s, table, ld, state, zn, rows, D1, W, keys, n, n_dev,
                       base, grads, h, oor);
  } else {
    const int grid = blocks > 0 ? blocks : grid_for(n * 64, kBlock, 4096);
    hipLaunchKernelGGL(adagrad_ftrl_kernel, grid, kBlock, 0, s, table, ld, state, zn, rows, D1, W, keys, n, n_dev,
                       base, grads, h, oor);
  }
  MINIPS_HIP_CHECK(hipGetLastError());
}

}  // namespace minips_k
