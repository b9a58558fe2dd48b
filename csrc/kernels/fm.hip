// Factorization-machine forward and backward over a CSR batch of pulled rows (fm.h states the rule, the
// mapping and which member counts take which backward path). Both kernels are latency-bound gathers of
// short rows: E floats per lane (4: one float4, or 1: the fallback for buffers that are not 16-byte
// friendly), L lanes per row, 64 / L lane groups per wave.
#include <stdexcept>
#include <string>

#include "common.h"
#include "fm.h"
#include "member_rows.h"

namespace minips_k {

namespace {

constexpr int kBlock = 256;

// One wave per sample. Lane group g (L lanes, lane l owns columns [E l, E l + E)) takes the lookups g, g + G,
// ... of the sample; the lane that owns column k carries the linear term in its first element.
template <int E, int L>
__global__ __launch_bounds__(kBlock) void fm_forward_kernel(const int64_t* __restrict__ rowptr,
                                                            const int64_t* __restrict__ inv,
                                                            const float* __restrict__ vals,
                                                            const float* __restrict__ labels,
                                                            const float* __restrict__ rows, int64_t ld, int64_t cap,
                                                            int k, const float* __restrict__ w0, float gscale,
                                                            int64_t B, int64_t n, float* __restrict__ S,
                                                            float* __restrict__ z, float* __restrict__ dz,
                                                            float* __restrict__ loss, int32_t* __restrict__ rowid) {
  constexpr int G = 64 / L;
  const int lane = threadIdx.x & 63, g = lane / L, l = lane % L;
  const int c0 = E * l;
  const bool fac = c0 < k, isl = c0 == k, act = c0 <= k;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const float w0v = w0 ? *w0 : 0.f;
  for (int64_t b = wave; b < B; b += nwaves) {
    int64_t st = rowptr[b], en = rowptr[b + 1];
    st = st < 0 ? 0 : st;
    en = en > n ? n : en;  // a rowptr outside [0, n] reads and writes nothing
    float s[E], q = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) s[e] = 0.f;
    for (int64_t c = st; c < en; c += 64) {
      const int64_t j = c + lane;
      int r = -1;
      float x = 0.f;
      if (j < en) {
        const int64_t rj = inv[j];
        x = vals[j];
        rowid[j] = (int32_t)b;
        if ((uint64_t)rj < (uint64_t)cap) r = (int)rj;
      }
      const int cnt = (int)((en - c) < 64 ? (en - c) : 64);
      const int its = (cnt + G - 1) / G;  // wave-uniform, <= L
      for (int it = 0; it < its; ++it) {
        const int src = it * G + g;
        const int rr = __shfl(r, src, 64);
        const float xx = __shfl(x, src, 64);
        if (rr >= 0 && act) {
          float a[E];
          load_e<E>(rows + (int64_t)rr * ld + c0, a);
#pragma unroll
          for (int e = 0; e < E; ++e) {
            const float p = a[e] * xx;
            s[e] += p;
            q += p * p;
          }
        }
      }
    }
    // the groups' partial sums, folded in a fixed order: afterwards every group holds the totals
#pragma unroll
    for (int o = L; o < 64; o <<= 1) {
#pragma unroll
      for (int e = 0; e < E; ++e) s[e] += __shfl_xor(s[e], o, 64);
      q += __shfl_xor(q, o, 64);
    }
    if (fac && g == 0) store_e<E>(S + b * k + c0, s);
    float ss = 0.f, qq = fac ? q : 0.f, lin = isl ? s[0] : 0.f;
    if (fac) {
#pragma unroll
      for (int e = 0; e < E; ++e) ss += s[e] * s[e];
    }
#pragma unroll
    for (int o = 1; o < L; o <<= 1) {
      ss += __shfl_xor(ss, o, 64);
      qq += __shfl_xor(qq, o, 64);
      lin += __shfl_xor(lin, o, 64);
    }
    if (lane == 0) {
      const float zz = (w0v + lin) + 0.5f * (ss - qq);
      float dzb, lossb;
      logistic_head(zz, labels[b] > 0.5f, gscale, &dzb, &lossb);
      z[b] = zz;
      dz[b] = dzb;
      loss[b] = lossb;
    }
  }
}

struct BwdArgs {
  const int32_t* members;
  const int32_t* memrow;
  const int32_t* rowid;
  const float* vals;
  const float* dz;
  const float* S;
  const float* rows;
  int64_t ld, cap, B;
  int k, n;
  float* grad;
  float* part;
};

// the term of member m of a row whose own values are v: acc += c (S[b] - v x) on the factor lanes; the
// linear lane sees S = (1, 0, 0, 0) and v = 0, so its first element sums c and the pad columns stay 0
template <int E>
__device__ __forceinline__ void fm_member(const BwdArgs& a, int m, int c0, bool fac, bool isl, const float (&v)[E],
                                          float (&acc)[E]) {
  const int j = a.members[m];
  if ((unsigned)j >= (unsigned)a.n) return;
  const int b = a.rowid[j];
  if ((uint64_t)b >= (uint64_t)a.B) return;
  const float x = a.vals[j];
  const float c = a.dz[b] * x;
  float sv[E];
#pragma unroll
  for (int e = 0; e < E; ++e) sv[e] = 0.f;
  if (fac) load_e<E>(a.S + (int64_t)b * a.k + c0, sv);
  else if (isl) sv[0] = 1.f;
#pragma unroll
  for (int e = 0; e < E; ++e) acc[e] += c * (sv[e] - v[e] * x);
}

template <int E>
__device__ __forceinline__ void fm_row_values(const BwdArgs& a, int u, int c0, bool fac, float (&v)[E]) {
#pragma unroll
  for (int e = 0; e < E; ++e) v[e] = 0.f;
  if (fac) load_e<E>(a.rows + (int64_t)u * a.ld + c0, v);
}

// Rows of up to kFmWaveMax members: a tile of G consecutive unique rows per wave and iteration, one lane group
// per row; the rows of a tile that have more than kFmGroupMax members are then walked by the whole wave.
template <int E, int L>
__global__ __launch_bounds__(kBlock) void fm_backward_kernel(BwdArgs a) {
  constexpr int G = 64 / L;
  const int lane = threadIdx.x & 63, g = lane / L, l = lane % L;
  const int c0 = E * l, W = a.k + 4;
  const bool fac = c0 < a.k, isl = c0 == a.k, wr = c0 < W;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int U = member_unique(a.memrow, a.n, a.cap);
  const int64_t ntiles = ((int64_t)U + G - 1) / G;
  for (int64_t tile = wave; tile < ntiles; tile += nwaves) {
    const int64_t u64 = tile * G + g;
    const bool valid = u64 < U;
    const int u = valid ? (int)u64 : 0;
    // one binary search per row; a row ends where the next group's row begins, and the tile's last row
    // gallops from its own start
    const int lo = valid ? lower_bound_i32(a.memrow, 0, a.n, u) : a.n;
    const int lo_next = __shfl_down(lo, L, 64);
    int hi = lo;
    if (valid) {
      if (g < G - 1 && u + 1 < U) hi = lo_next;  // the next group holds row u + 1
      else if (lo < a.n && a.memrow[lo] == u) hi = gallop_i32(a.memrow, lo, a.n, u + 1);
    }
    const int M = hi - lo;
    if (valid && M > 0 && M <= kFmGroupMax) {
      float v[E], acc[E];
      fm_row_values<E>(a, u, c0, fac, v);
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] = 0.f;
      for (int m = lo; m < hi; ++m) fm_member<E>(a, m, c0, fac, isl, v, acc);
      if (wr) store_e<E>(a.grad + (int64_t)u * W + c0, acc);
    }
    unsigned long long big = __ballot(valid && l == 0 && M > kFmGroupMax && M <= kFmWaveMax);
    while (big) {
      const int src = __ffsll(big) - 1;
      big &= big - 1;
      const int ru = __shfl(u, src, 64), rlo = __shfl(lo, src, 64), rhi = __shfl(hi, src, 64);
      float v[E], acc[E];
      fm_row_values<E>(a, ru, c0, fac, v);
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] = 0.f;
      for (int m = rlo + g; m < rhi; m += G) fm_member<E>(a, m, c0, fac, isl, v, acc);
#pragma unroll
      for (int o = L; o < 64; o <<= 1) {
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] += __shfl_xor(acc[e], o, 64);
      }
      if (g == 0 && wr) store_e<E>(a.grad + (int64_t)ru * W + c0, acc);
    }
  }
}

// block p sums the members of chunk p that belong to a heavy row into part[(2 p + s) * W ...] (member_rows.h)
template <int E, int L>
__global__ __launch_bounds__(kBlock) void fm_backward_heavy_kernel(BwdArgs a) {
  constexpr int G = 64 / L, NG = G * (kBlock / 64);
  __shared__ float red[kBlock / 64][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane / L, l = lane % L;
  const int c0 = E * l, W = a.k + 4;
  const bool fac = c0 < a.k, isl = c0 == a.k;
  const int64_t p = blockIdx.x;
  const int64_t c_lo = p * kFmChunk, c_hi = (c_lo + kFmChunk) < a.n ? (c_lo + kFmChunk) : a.n;
  for (int s = 0; s < 2; ++s) {
    int r, lo, hi;
    if (!member_heavy_row<kFmChunk, kFmWaveMax>(a.memrow, a.n, a.cap, p, s, r, lo, hi)) continue;  // block-uniform
    const int m0 = lo > c_lo ? lo : (int)c_lo, m1 = hi < c_hi ? hi : (int)c_hi;
    float v[E], acc[E];
    fm_row_values<E>(a, r, c0, fac, v);
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.f;
    for (int m = m0 + wv * G + g; m < m1; m += NG) fm_member<E>(a, m, c0, fac, isl, v, acc);
#pragma unroll
    for (int o = L; o < 64; o <<= 1) {
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] += __shfl_xor(acc[e], o, 64);
    }
    __syncthreads();  // (the previous candidate's reads of red)
    if (g == 0) {
#pragma unroll
      for (int e = 0; e < E; ++e) red[wv][c0 + e] = acc[e];
    }
    __syncthreads();
    if (threadIdx.x < W) {
      float t = red[0][threadIdx.x];
#pragma unroll
      for (int w = 1; w < kBlock / 64; ++w) t += red[w][threadIdx.x];
      a.part[(2 * p + s) * W + threadIdx.x] = t;
    }
  }
}

void check_shape(const char* op, int k, int64_t ld, int64_t cap, int64_t B, int64_t n, int blocks) {
  if (!fm_k_ok(k)) throw std::runtime_error(std::string(op) + ": k % 4 == 0 and 4 <= k <= 60");
  if (ld < k + 4) throw std::runtime_error(std::string(op) + ": ld < k + 4");
  if (blocks < 0 || blocks > kFmMaxBlocks) throw std::runtime_error(std::string(op) + ": blocks outside [0, 65535]");
  if (n >= (1ll << 31) || B >= (1ll << 31) || cap >= (1ll << 31))
    throw std::runtime_error(std::string(op) + ": n, B and cap must be below 2^31");
}

// f.run<E, L>() for the lane shape of (k, vec)
template <typename F>
void dispatch_shape(int k, bool vec, const F& f) {
  const int W = k + 4;
  if (vec) {
    switch (pow2ceil(W / 4)) {
      case 2: return f.template run<4, 2>();
      case 4: return f.template run<4, 4>();
      case 8: return f.template run<4, 8>();
      default: return f.template run<4, 16>();
    }
  }
  switch (pow2ceil(W)) {
    case 8: return f.template run<1, 8>();
    case 16: return f.template run<1, 16>();
    case 32: return f.template run<1, 32>();
    default: return f.template run<1, 64>();
  }
}

struct FwdLaunch {
  const int64_t* rowptr;
  const int64_t* inv;
  const float* vals;
  const float* labels;
  const float* rows;
  int64_t ld, cap;
  int k;
  const float* w0;
  float gscale;
  int64_t B, n;
  float *S, *z, *dz, *loss;
  int32_t* rowid;
  int blocks;
  hipStream_t s;
  template <int E, int L>
  void run() const {
    const int grid = blocks > 0 ? blocks : grid_for(B * 64, kBlock, 8192);
    hipLaunchKernelGGL((fm_forward_kernel<E, L>), grid, kBlock, 0, s, rowptr, inv, vals, labels, rows, ld, cap, k, w0,
                       gscale, B, n, S, z, dz, loss, rowid);
  }
};

struct BwdLaunch {
  BwdArgs a;
  int blocks;
  hipStream_t s;
  template <int E, int L>
  void run() const {
    const int64_t n = a.n, urows = a.cap < n ? a.cap : n;  // at most this many unique rows
    const int grid = blocks > 0 ? blocks : grid_for(urows * L, kBlock, 8192);
    hipLaunchKernelGGL((fm_backward_kernel<E, L>), grid, kBlock, 0, s, a);
    if (n > kFmWaveMax) {
      const int chunks = member_chunks(n, kFmChunk);
      hipLaunchKernelGGL((fm_backward_heavy_kernel<E, L>), chunks, kBlock, 0, s, a);
      hipLaunchKernelGGL((member_heavy_fold_kernel<float, float, kFmChunk, kFmWaveMax>), chunks, 64, 0, s, a.memrow,
                         a.n, a.cap, a.k + 4, a.part, a.grad);
    }
  }
};

}  // namespace

void fm_forward(const int64_t* rowptr, const int64_t* inv, const float* vals, const float* labels, const float* rows,
                int64_t ld, int64_t cap, int k, const float* w0, float gscale, int64_t B, int64_t n, float* S, float* z,
                float* dz, float* loss, int32_t* rowid, int blocks, hipStream_t s) {
  check_shape("fm_forward", k, ld, cap, B, n, blocks);
  if (B <= 0) return;
  const bool vec = ld % 4 == 0 && aligned16(rows) && aligned16(S);
  dispatch_shape(k, vec, FwdLaunch{rowptr, inv, vals, labels, rows, ld, cap, k, w0, gscale, B, n, S, z, dz, loss, rowid,
                                   blocks, s});
  MINIPS_HIP_CHECK(hipGetLastError());
}

int64_t fm_backward_part_floats(int64_t n, int W) {
  return member_part_elems(n, W, kFmChunk, kFmWaveMax);
}

void fm_backward(const int32_t* members, const int32_t* memrow, const int32_t* rowid, const float* vals,
                 const float* dz, const float* S, const float* rows, int64_t ld, int64_t cap, int k, int64_t B,
                 int64_t n, float* grad_rows, float* part, int blocks, hipStream_t s) {
  check_shape("fm_backward", k, ld, cap, B, n, blocks);
  if (n <= 0 || B <= 0 || cap <= 0) return;
  const int W = k + 4;
  const bool heavy = n > kFmWaveMax;
  if (heavy && part == nullptr) throw std::runtime_error("fm_backward: part workspace missing");
  const bool vec = ld % 4 == 0 && aligned16(rows) && aligned16(S) && aligned16(grad_rows);
  const BwdArgs a{members, memrow, rowid, vals, dz, S, rows, ld, cap, B, k, (int)n, grad_rows, part};
  dispatch_shape(k, vec, BwdLaunch{a, blocks, s});
  MINIPS_HIP_CHECK(hipGetLastError());
}

}  // namespace minips_k
