// Skip-gram with negative sampling over the pulled rows of a window of pairs (sgns.h states the rule, the mapping
// and which member counts take which backward path). The forward and the backward are latency-bound gathers of
// short rows: E floats per load (4: one float4, or 1: the fallback for buffers that are not 16-byte friendly), L
// lanes per pair or row, Q loads per lane (column E (l + q L)), 64 / L lane groups per wave.
#include <stdexcept>
#include <string>

#include "common.h"
#include "lda.h"
#include "member_rows.h"
#include "sgns.h"

namespace minips_k {

namespace {

constexpr int kBlock = 256;

struct LookupArgs {
  const int64_t* centres;
  const int64_t* contexts;
  const uint64_t* thr;
  const int32_t* alias;
  int64_t V;
  uint64_t T, base, pair_base;  // base = mix(seed + epoch * golden)
  int N;
  const int32_t* negatives;
  int64_t P;
  int64_t* keys;
};

__global__ __launch_bounds__(kBlock) void sgns_lookups_kernel(LookupArgs a) {
  const int K2 = a.N + 2;
  const int64_t total = a.P * K2, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t p = i / K2;
    const int col = (int)(i - p * K2);
    int64_t w;
    if (col == 0) {
      w = a.centres[p];
    } else if (col == 1) {
      w = a.contexts[p];
    } else if (a.negatives) {
      w = a.negatives[p * a.N + (col - 2)];
    } else {
      const uint64_t r = mix64(a.base ^ ((a.pair_base + (uint64_t)p) * 64ull + (uint64_t)(col - 2)));
      const uint64_t b = mulhi_u64(r, (uint64_t)a.V);  // < V
      const uint64_t x = mulhi_u64(mix64(r), a.T);
      w = x < a.thr[b] ? (int64_t)b : (int64_t)a.alias[b];
    }
    const bool ok = (uint64_t)w < (uint64_t)a.V;
    a.keys[i] = ok ? 2 * w + (col != 0) : -1;
  }
}

template <int E, int Q>
__device__ __forceinline__ void zero_q(float (&v)[Q][E]) {
#pragma unroll
  for (int q = 0; q < Q; ++q)
#pragma unroll
    for (int e = 0; e < E; ++e) v[q][e] = 0.f;
}

// the lane's Q pieces of one row of d floats: column E (l + q L); pieces at or beyond d read as 0
template <int E, int L, int Q>
__device__ __forceinline__ void load_q(const float* __restrict__ row, int l, int d, float (&v)[Q][E]) {
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int c = E * (l + q * L);
    if (c < d) load_e<E>(row + c, v[q]);
    else
#pragma unroll
      for (int e = 0; e < E; ++e) v[q][e] = 0.f;
  }
}

template <int E, int L, int Q>
__device__ __forceinline__ void store_q(float* __restrict__ row, int l, int d, const float (&v)[Q][E]) {
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int c = E * (l + q * L);
    if (c < d) store_e<E>(row + c, v[q]);
  }
}

struct FwdArgs {
  const int64_t* inv;
  const float* rows;
  int64_t ld, cap, P;
  int d, N;
  float gscale;
  float *e, *loss, *h;
};

// A tile of G = 64 / L consecutive pairs per wave and iteration, one lane group per pair. Every lane of a group
// reads the same inv entries (one broadcast load); the branches are uniform within a group and the shuffles stay
// inside it.
template <int E, int L, int Q>
__global__ __launch_bounds__(kBlock) void sgns_forward_kernel(FwdArgs a) {
  constexpr int G = 64 / L;
  const int lane = threadIdx.x & 63, g = lane / L, l = lane % L;
  const int K2 = a.N + 2, T1 = a.N + 1;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t ntiles = (a.P + G - 1) / G;
  for (int64_t tile = wave; tile < ntiles; tile += nwaves) {
    const int64_t p = tile * G + g;
    const bool live = p < a.P;
    const int64_t* ip = a.inv + (live ? p : 0) * K2;
    const int64_t ai = live ? ip[0] : -1, b0 = live ? ip[1] : -1;
    const bool cen = live && (uint64_t)ai < (uint64_t)a.cap;
    float va[Q][E], hh[Q][E], un[Q][E];
    zero_q<E, Q>(va);
    zero_q<E, Q>(hh);
    zero_q<E, Q>(un);
    if (cen) load_q<E, L, Q>(a.rows + ai * a.ld, l, a.d, va);
    bool vn = cen && (uint64_t)b0 < (uint64_t)a.cap;
    if (vn) load_q<E, L, Q>(a.rows + b0 * a.ld, l, a.d, un);
    float lsum = 0.f;
    for (int t = 0; t <= a.N; ++t) {
      float u[Q][E];
      const bool v = vn;
#pragma unroll
      for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int e = 0; e < E; ++e) u[q][e] = un[q][e];
      if (t < a.N) {  // the next target's row, in flight while this one is folded
        const int64_t bn = live ? ip[2 + t] : -1;
        vn = cen && (uint64_t)bn < (uint64_t)a.cap && bn != b0;
        if (vn) load_q<E, L, Q>(a.rows + bn * a.ld, l, a.d, un);
        else zero_q<E, Q>(un);
      }
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int e = 0; e < E; ++e) s += va[q][e] * u[q][e];
#pragma unroll
      for (int o = 1; o < L; o <<= 1) s += __shfl_xor(s, o, 64);
      float et = 0.f, lt = 0.f;
      if (v) logistic_head(s, t == 0, a.gscale, &et, &lt);
      lsum += lt;
#pragma unroll
      for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int e = 0; e < E; ++e) hh[q][e] += et * u[q][e];
      if (live && l == 0) a.e[p * T1 + t] = et;
    }
    if (live) {
      if (l == 0) a.loss[p] = lsum;
      store_q<E, L, Q>(a.h + p * a.d, l, a.d, hh);
    }
  }
}

struct BwdArgs {
  const int32_t* members;
  const int32_t* memrow;
  const int64_t* inv;
  const float* e;
  const float* h;
  const float* rows;
  int64_t ld, cap, P;
  int d, N, n;
  float* grad;
  float* part;
};

// members a wave or a workgroup fetches ahead (a lane group that walks a short row alone: 2)
template <int E, int Q>
constexpr int kAhead = E * Q <= 4 ? 8 : 4;

// the term of member m: src = h_p and c = 1 (the centre's lookup), or src = v_{a_p} and c = e[p, col - 1] (a
// target's); src stays null for a member that is skipped
__device__ __forceinline__ void sgns_term(const BwdArgs& a, int m, const float*& src, float& c) {
  src = nullptr;
  c = 1.f;
  const int j = a.members[m];
  if ((unsigned)j >= (unsigned)a.n) return;
  const int K2 = a.N + 2;
  const int p = j / K2, col = j - p * K2;
  if (col == 0) {
    src = a.h + (int64_t)p * a.d;
  } else {
    const int64_t ai = a.inv[(int64_t)p * K2];
    if ((uint64_t)ai >= (uint64_t)a.cap) return;
    src = a.rows + ai * a.ld;
    c = a.e[(int64_t)p * (a.N + 1) + (col - 1)];
  }
}

// acc += the terms of the members m0, m0 + step, ... below m1, in that order. A term is three dependent loads
// (member -> centre row index -> row), so UN members are fetched before the first is added: the order of the
// additions, and with it every bit, is that of the plain loop.
template <int E, int L, int Q, int UN>
__device__ __forceinline__ void sgns_walk(const BwdArgs& a, int m0, int m1, int step, int l, float (&acc)[Q][E]) {
  int m = m0;
  for (; (int64_t)m + (UN - 1) * step < m1; m += UN * step) {
    const float* src[UN];
    float c[UN], v[UN][Q][E];
#pragma unroll
    for (int i = 0; i < UN; ++i) sgns_term(a, m + i * step, src[i], c[i]);
#pragma unroll
    for (int i = 0; i < UN; ++i) {
      if (src[i]) load_q<E, L, Q>(src[i], l, a.d, v[i]);
      else zero_q<E, Q>(v[i]);
    }
#pragma unroll
    for (int i = 0; i < UN; ++i) {
      if (src[i]) {
#pragma unroll
        for (int q = 0; q < Q; ++q)
#pragma unroll
          for (int e = 0; e < E; ++e) acc[q][e] += c[i] * v[i][q][e];
      }
    }
  }
  for (; m < m1; m += step) {
    const float* src;
    float c, v[Q][E];
    sgns_term(a, m, src, c);
    if (src) {
      load_q<E, L, Q>(src, l, a.d, v);
#pragma unroll
      for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int e = 0; e < E; ++e) acc[q][e] += c * v[q][e];
    }
  }
}

// Rows of up to kSgnsWaveMax members: a tile of G consecutive unique rows per wave and iteration, one lane group
// per row; the rows of a tile that have more than kSgnsGroupMax members are then walked by the whole wave.
template <int E, int L, int Q>
__global__ __launch_bounds__(kBlock) void sgns_backward_kernel(BwdArgs a) {
  constexpr int G = 64 / L;
  const int lane = threadIdx.x & 63, g = lane / L, l = lane % L;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int U = member_unique(a.memrow, a.n, a.cap);
  const int64_t ntiles = ((int64_t)U + G - 1) / G;
  for (int64_t tile = wave; tile < ntiles; tile += nwaves) {
    const int64_t u64 = tile * G + g;
    const bool valid = u64 < U;
    const int u = valid ? (int)u64 : 0;
    const int lo = valid ? lower_bound_i32(a.memrow, 0, a.n, u) : a.n;
    const int lo_next = __shfl_down(lo, L % 64, 64);
    int hi = lo;
    if (valid) {
      if (g < G - 1 && u + 1 < U) hi = lo_next;  // the next group holds row u + 1
      else if (lo < a.n && a.memrow[lo] == u) hi = gallop_i32(a.memrow, lo, a.n, u + 1);
    }
    const int M = hi - lo;
    if (valid && M > 0 && M <= kSgnsGroupMax) {
      float acc[Q][E];
      zero_q<E, Q>(acc);
      sgns_walk<E, L, Q, 2>(a, lo, hi, 1, l, acc);
      store_q<E, L, Q>(a.grad + (int64_t)u * a.d, l, a.d, acc);
    }
    unsigned long long big = __ballot(valid && l == 0 && M > kSgnsGroupMax && M <= kSgnsWaveMax);
    while (big) {
      const int src = __ffsll(big) - 1;
      big &= big - 1;
      const int ru = __shfl(u, src, 64), rlo = __shfl(lo, src, 64), rhi = __shfl(hi, src, 64);
      float acc[Q][E];
      zero_q<E, Q>(acc);
      sgns_walk<E, L, Q, kAhead<E, Q>>(a, rlo + g, rhi, G, l, acc);
#pragma unroll
      for (int o = L; o < 64; o <<= 1) {
#pragma unroll
        for (int q = 0; q < Q; ++q)
#pragma unroll
          for (int e = 0; e < E; ++e) acc[q][e] += __shfl_xor(acc[q][e], o, 64);
      }
      if (g == 0) store_q<E, L, Q>(a.grad + (int64_t)ru * a.d, l, a.d, acc);
    }
  }
}

// block p sums the members of chunk p that belong to a heavy row into part[(2 p + s) * d ...] (member_rows.h)
template <int E, int L, int Q>
__global__ __launch_bounds__(kBlock) void sgns_backward_heavy_kernel(BwdArgs a) {
  constexpr int G = 64 / L, NG = G * (kBlock / 64);
  __shared__ __align__(16) float red[kBlock / 64][kSgnsMaxDim];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane / L, l = lane % L;
  const int64_t p = blockIdx.x;
  const int64_t c_lo = p * kSgnsChunk, c_hi = (c_lo + kSgnsChunk) < a.n ? (c_lo + kSgnsChunk) : a.n;
  for (int s = 0; s < 2; ++s) {
    int r, lo, hi;
    if (!member_heavy_row<kSgnsChunk, kSgnsWaveMax>(a.memrow, a.n, a.cap, p, s, r, lo, hi)) continue;  // block-uniform
    const int m0 = lo > c_lo ? lo : (int)c_lo, m1 = hi < c_hi ? hi : (int)c_hi;
    float acc[Q][E];
    zero_q<E, Q>(acc);
    sgns_walk<E, L, Q, kAhead<E, Q>>(a, m0 + wv * G + g, m1, NG, l, acc);
#pragma unroll
    for (int o = L; o < 64; o <<= 1) {
#pragma unroll
      for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int e = 0; e < E; ++e) acc[q][e] += __shfl_xor(acc[q][e], o, 64);
    }
    __syncthreads();  // (the previous candidate's reads of red)
    if (g == 0) store_q<E, L, Q>(red[wv], l, a.d, acc);
    __syncthreads();
    for (int col = threadIdx.x; col < a.d; col += kBlock) {
      float t = red[0][col];
#pragma unroll
      for (int w = 1; w < kBlock / 64; ++w) t += red[w][col];
      a.part[(2 * p + s) * a.d + col] = t;
    }
  }
}

void check_shape(const char* op, int d, int N, int64_t ld, int64_t cap, int64_t P, int blocks) {
  if (!sgns_dim_ok(d)) throw std::runtime_error(std::string(op) + ": d % 4 == 0 and 4 <= d <= 512");
  if (!sgns_neg_ok(N)) throw std::runtime_error(std::string(op) + ": 1 <= N <= 64");
  if (ld < d) throw std::runtime_error(std::string(op) + ": ld < d");
  if (blocks < 0 || blocks > kSgnsMaxBlocks)
    throw std::runtime_error(std::string(op) + ": blocks outside [0, 65535]");
  if (P < 0 || P * (N + 2) >= (1ll << 31) || cap >= (1ll << 31))
    throw std::runtime_error(std::string(op) + ": P (N + 2) and cap must be below 2^31");
}

// f.run<E, L, Q>() for the lane shape of (d, vec)
template <typename F>
void dispatch_shape(int d, bool vec, const F& f) {
  if (vec) {
    if (d > 256) return f.template run<4, 64, 2>();
    switch (pow2ceil(d / 4)) {
      case 1: return f.template run<4, 1, 1>();
      case 2: return f.template run<4, 2, 1>();
      case 4: return f.template run<4, 4, 1>();
      case 8: return f.template run<4, 8, 1>();
      case 16: return f.template run<4, 16, 1>();
      case 32: return f.template run<4, 32, 1>();
      default: return f.template run<4, 64, 1>();
    }
  }
  if (d > 256) return f.template run<1, 64, 8>();
  if (d > 128) return f.template run<1, 64, 4>();
  if (d > 64) return f.template run<1, 64, 2>();
  switch (pow2ceil(d)) {
    case 4: return f.template run<1, 4, 1>();
    case 8: return f.template run<1, 8, 1>();
    case 16: return f.template run<1, 16, 1>();
    case 32: return f.template run<1, 32, 1>();
    default: return f.template run<1, 64, 1>();
  }
}

struct FwdLaunch {
  FwdArgs a;
  int blocks;
  hipStream_t s;
  template <int E, int L, int Q>
  void run() const {
    const int grid = blocks > 0 ? blocks : grid_for(a.P * L, kBlock, 8192);
    hipLaunchKernelGGL((sgns_forward_kernel<E, L, Q>), grid, kBlock, 0, s, a);
  }
};

struct BwdLaunch {
  BwdArgs a;
  int blocks;
  hipStream_t s;
  template <int E, int L, int Q>
  void run() const {
    const int64_t n = a.n, urows = a.cap < n ? a.cap : n;  // at most this many unique rows
    const int grid = blocks > 0 ? blocks : grid_for(urows * L, kBlock, 8192);
    hipLaunchKernelGGL((sgns_backward_kernel<E, L, Q>), grid, kBlock, 0, s, a);
    if (n > kSgnsWaveMax) {
      const int chunks = member_chunks(n, kSgnsChunk);
      hipLaunchKernelGGL((sgns_backward_heavy_kernel<E, L, Q>), chunks, kBlock, 0, s, a);
      hipLaunchKernelGGL((member_heavy_fold_kernel<float, float, kSgnsChunk, kSgnsWaveMax>), chunks, kBlock, 0, s,
                         a.memrow, a.n, a.cap, a.d, a.part, a.grad);
    }
  }
};

}  // namespace

void sgns_lookups(const int64_t* centres, const int64_t* contexts, const uint64_t* thr, const int32_t* alias,
                  int64_t V, uint64_t T, uint64_t seed, uint64_t epoch, uint64_t pair_base, int N,
                  const int32_t* negatives, int64_t P, int64_t* keys, hipStream_t s) {
  if (!sgns_neg_ok(N)) throw std::runtime_error("sgns_lookups: 1 <= N <= 64");
  if (V < 1 || V >= (1ll << 31)) throw std::runtime_error("sgns_lookups: 1 <= V < 2^31");
  if (P < 0 || P * (N + 2) >= (1ll << 31)) throw std::runtime_error("sgns_lookups: P (N + 2) must be below 2^31");
  if (!negatives && (thr == nullptr || alias == nullptr || T < 1 || T >= (1ull << 59)))
    throw std::runtime_error("sgns_lookups: draws need thr, alias and 1 <= T < 2^59");
  if (P == 0) return;
  const uint64_t base = mix64(seed + epoch * 0x9E3779B97F4A7C15ull);
  const LookupArgs a{centres, contexts, thr, alias, V, T, base, pair_base, N, negatives, P, keys};
  hipLaunchKernelGGL(sgns_lookups_kernel, grid_for(P * (N + 2), kBlock, 8192), kBlock, 0, s, a);
  MINIPS_HIP_CHECK(hipGetLastError());
}

void sgns_forward(const int64_t* inv, const float* rows, int64_t ld, int64_t cap, int d, int N, float gscale,
                  int64_t P, float* e, float* loss, float* h, int blocks, hipStream_t s) {
  check_shape("sgns_forward", d, N, ld, cap, P, blocks);
  if (P <= 0) return;
  const bool vec = ld % 4 == 0 && aligned16(rows) && aligned16(h);
  dispatch_shape(d, vec, FwdLaunch{FwdArgs{inv, rows, ld, cap, P, d, N, gscale, e, loss, h}, blocks, s});
  MINIPS_HIP_CHECK(hipGetLastError());
}

int64_t sgns_backward_part_floats(int64_t n, int d) {
  return member_part_elems(n, d, kSgnsChunk, kSgnsWaveMax);
}

void sgns_backward(const int32_t* members, const int32_t* memrow, const int64_t* inv, const float* e, const float* h,
                   const float* rows, int64_t ld, int64_t cap, int d, int N, int64_t P, float* grad_rows, float* part,
                   int blocks, hipStream_t s) {
  check_shape("sgns_backward", d, N, ld, cap, P, blocks);
  const int64_t n = P * (N + 2);
  if (n <= 0 || cap <= 0) return;
  if (n > kSgnsWaveMax && part == nullptr) throw std::runtime_error("sgns_backward: part workspace missing");
  const bool vec = ld % 4 == 0 && aligned16(rows) && aligned16(h) && aligned16(grad_rows);
  const BwdArgs a{members, memrow, inv, e, h, rows, ld, cap, P, d, N, (int)n, grad_rows, part};
  dispatch_shape(d, vec, BwdLaunch{a, blocks, s});
  MINIPS_HIP_CHECK(hipGetLastError());
}

}  // namespace minips_k
