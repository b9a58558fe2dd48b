// FTRL-Proximal apply on sparse table rows (ftrl.h states the rule and the state layout). A latency-bound
// gather: key -> row -> read-modify-write of w and of the row's (z, n) segment. The rule is per coordinate
// (no reduction across a row), so every mapping is a flat grid-stride loop over (key, lane-of-row) items
// and a wave keeps 64 / lanes-per-row independent rows in flight:
//   W == 1                    one lane per row (64 rows per wave), (z, n) as one float2
//   W % 4 == 0 && W <= 256    pow2(W / 4) lanes per row, one float4 each of w, z, n, g
//   any other W               one lane per (row, column), scalar accesses
// The vector forms need 16-byte (W == 1: 8-byte zn) aligned pointers and ld % 4 == 0; the launcher picks.
#include <stdexcept>
#include <string>

#include "common.h"
#include "ftrl.h"
#include "ftrl_rule.h"

namespace minips_k {

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ int64_t count_of(int64_t n, const int64_t* n_dev) { return n_dev ? min(n, *n_dev) : n; }

// row of key i inside [0, rows), or -1 (counted once per key by the item with first == true)
__device__ __forceinline__ int64_t checked_row(int64_t key, int64_t base, int64_t rows, int64_t* oor, bool first) {
  const int64_t row = key - base;
  if ((uint64_t)row < (uint64_t)rows) return row;
  if (oor && first) atomicAdd(reinterpret_cast<unsigned long long*>(oor), 1ull);
  return -1;
}

__global__ __launch_bounds__(kBlock) void ftrl_w1_kernel(float* table, int64_t ld, float* zn, int64_t rows,
                                                         const int64_t* __restrict__ keys, int64_t n,
                                                         const int64_t* n_dev, int64_t base,
                                                         const float* __restrict__ grads, FtrlHyper h,
                                                         int64_t* oor) {
  n = count_of(n, n_dev);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t row = checked_row(keys[i], base, rows, oor, true);
    if (row < 0) continue;
    float* wp = table + row * ld;
    float2* sp = reinterpret_cast<float2*>(zn) + row;
    float w = *wp;
    float2 s = *sp;
    ftrl_coord(w, s.x, s.y, grads[i], h);
    *wp = w;
    *sp = s;
  }
}

// lanes-per-row = 1 << sh >= W / 4; item = (key i, lane l of its row), lane l owns columns [4l, 4l + 4)
__global__ __launch_bounds__(kBlock) void ftrl_v4_kernel(float* table, int64_t ld, float* zn, int64_t rows,
                                                         const int64_t* __restrict__ keys, int64_t n,
                                                         const int64_t* n_dev, int64_t base, int W, int sh,
                                                         const float* __restrict__ grads, FtrlHyper h,
                                                         int64_t* oor) {
  const int64_t total = count_of(n, n_dev) << sh;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t i = t >> sh;
    const int c = 4 * (int)(t & ((1 << sh) - 1));
    if (c >= W) continue;  // W % 4 == 0: a float4 is all in or all out
    const int64_t row = checked_row(keys[i], base, rows, oor, c == 0);
    if (row < 0) continue;
    float4* wp = reinterpret_cast<float4*>(table + row * ld + c);
    float4* zp = reinterpret_cast<float4*>(zn + row * 2 * W + c);
    float4* np = reinterpret_cast<float4*>(zn + row * 2 * W + W + c);
    const float4 g = *reinterpret_cast<const float4*>(grads + i * W + c);
    float4 w = *wp, z = *zp, nn = *np;
    ftrl_coord4(w, z, nn, g, h);
    *wp = w;
    *zp = z;
    *np = nn;
  }
}

__global__ __launch_bounds__(kBlock) void ftrl_scalar_kernel(float* table, int64_t ld, float* zn, int64_t rows,
                                                             const int64_t* __restrict__ keys, int64_t n,
                                                             const int64_t* n_dev, int64_t base, int W,
                                                             const float* __restrict__ grads, FtrlHyper h,
                                                             int64_t* oor) {
  const int64_t total = count_of(n, n_dev) * W;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t i = t / W;
    const int c = (int)(t - i * W);
    const int64_t row = checked_row(keys[i], base, rows, oor, c == 0);
    if (row < 0) continue;
    float* wp = table + row * ld + c;
    float* zp = zn + row * 2 * W + c;
    float w = *wp, z = zp[0], nn = zp[W];
    ftrl_coord(w, z, nn, grads[t], h);
    *wp = w;
    zp[0] = z;
    zp[W] = nn;
  }
}

inline bool aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

}  // namespace

void sparse_ftrl(float* table, int64_t ld, float* zn, int64_t rows, const int64_t* keys, int64_t n,
                 const int64_t* n_dev, int64_t base, int W, const float* grads, float alpha, float beta, float l1,
                 float l2, int64_t* oor, int blocks, hipStream_t s) {
  if (W < 1 || ld < W) throw std::runtime_error("sparse_ftrl: W >= 1 and ld >= W");
  if (blocks < 0 || blocks > kFtrlMaxBlocks) throw std::runtime_error("sparse_ftrl: blocks outside [0, 65535]");
  if (n <= 0 || rows <= 0) return;
  const FtrlHyper h{alpha, beta, l1, l2};
  const bool vec4 =
      W % 4 == 0 && W <= 256 && ld % 4 == 0 && aligned(table, 16) && aligned(zn, 16) && aligned(grads, 16);
  if (W == 1 && aligned(zn, 8)) {
    const int grid = blocks > 0 ? blocks : grid_for(n, kBlock, 8192);
    hipLaunchKernelGGL(ftrl_w1_kernel, grid, kBlock, 0, s, table, ld, zn, rows, keys, n, n_dev, base, grads, h, oor);
  } else if (vec4) {
    int sh = 0;
    while ((4 << sh) < W) ++sh;
    const int grid = blocks > 0 ? blocks : grid_for(n << sh, kBlock, 16384);
    hipLaunchKernelGGL(ftrl_v4_kernel, grid, kBlock, 0, s, table, ld, zn, rows, keys, n, n_dev, base, W, sh, grads, h,
                       oor);
  } else {
    const int grid = blocks > 0 ? blocks : grid_for(n * W, kBlock, 16384);
    hipLaunchKernelGGL(ftrl_scalar_kernel, grid, kBlock, 0, s, table, ld, zn, rows, keys, n, n_dev, base, W, grads, h,
                       oor);
  }
  MINIPS_HIP_CHECK(hipGetLastError());
}

}  // namespace minips_k
