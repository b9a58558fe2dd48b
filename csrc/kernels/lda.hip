// LDA Gibbs kernels for gfx950 (the rule and the lane mapping: lda.h). Integer accumulation only -- LDS integer
// atomics per wave or workgroup, 64-bit global integer atomics with zero entries skipped, as gbdt.hip -- and fp64
// weights formed one correctly rounded operation at a time, so every result is a function of the inputs alone.
#include <stdexcept>
#include <string>

#include "common.h"
#include "lda.h"
#include "member_rows.h"

namespace minips_k {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;

typedef unsigned long long u64;
typedef long long i64;

__device__ __forceinline__ u64 sweep_base(u64 seed, u64 it) { return mix64(seed + it * 0x9E3779B97F4A7C15ull); }

__device__ __forceinline__ u64 draw(u64 base, i64 g, i64 j) { return mix64(base ^ ((u64)g * 4096ull + (u64)j)); }

// orders this wave's LDS traffic (one wave shares a slice of LDS among its lanes; the hardware keeps a wave's LDS
// operations in order, this keeps the compiler from moving them)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// the topics [k0, k0 + R) of one row; topics >= K read as 0. VEC: float4 loads (ld % 4 == 0, 16-byte aligned rows)
template <int R, bool VEC>
__device__ __forceinline__ void load_topics(const float* __restrict__ row, int k0, int K, float (&v)[R]) {
  if constexpr (VEC) {
#pragma unroll
    for (int q = 0; q < R / 4; ++q) {
      float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k0 + 4 * q < K) f = *reinterpret_cast<const float4*>(row + k0 + 4 * q);
      v[4 * q] = f.x;
      v[4 * q + 1] = k0 + 4 * q + 1 < K ? f.y : 0.f;
      v[4 * q + 2] = k0 + 4 * q + 2 < K ? f.z : 0.f;
      v[4 * q + 3] = k0 + 4 * q + 3 < K ? f.w : 0.f;
    }
  } else {
#pragma unroll
    for (int i = 0; i < R; ++i) v[i] = k0 + i < K ? row[k0 + i] : 0.f;
  }
}

struct DocArgs {
  const int64_t* rowptr;
  const int64_t* gid;
  const int64_t* inv;
  const int16_t* z_old;
  const float* rows;
  int64_t ld, cap;
  const int64_t* nk;
  int K;
  double alpha, beta, Vbeta;
  u64 seed, it;
  int64_t B, n;
  int16_t* z_new;
  int64_t* out;  // dk [K] of sample, acc [2] of loglik
};

// the token range of document d, clamped into [0, n]
__device__ __forceinline__ void doc_range(const DocArgs& a, i64 d, i64& lo, i64& hi) {
  lo = a.rowptr[d];
  hi = a.rowptr[d + 1];
  lo = lo < 0 ? 0 : (lo > a.n ? a.n : lo);
  hi = hi < lo ? lo : (hi > a.n ? a.n : hi);
}

// ndk of the live tokens of [lo, hi) into the wave's LDS slice; returns their number
__device__ __forceinline__ int doc_counts(const DocArgs& a, const int16_t* __restrict__ z, i64 lo, i64 hi, int lane,
                                          int* my) {
  for (int k = lane; k < a.K; k += 64) my[k] = 0;
  wave_lds_sync();
  int live = 0;
  for (i64 t = lo + lane; t < hi; t += 64) {
    const i64 u = a.inv[t];
    const int zo = z[t];
    if ((u64)u < (u64)a.cap && (unsigned)zo < (unsigned)a.K) {
      atomicAdd(&my[zo], 1);
      ++live;
    }
  }
  wave_lds_sync();
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) live += __shfl_xor(live, o, 64);
  return live;
}

__device__ __forceinline__ void flush_hist(const int* h, int K, int64_t* out) {
  for (int k = threadIdx.x; k < K; k += kBlock) {
    const int v = h[k];
    if (v) atomicAdd(reinterpret_cast<u64*>(out) + k, (u64)(i64)v);
  }
}

// ------------------------------------------------------------------------------------------- sample
__global__ __launch_bounds__(kBlock) void lda_init_kernel(DocArgs a) {
  __shared__ int dkh[kLdaMaxK];
  const int lane = threadIdx.x & 63;
  for (int k = threadIdx.x; k < a.K; k += kBlock) dkh[k] = 0;
  __syncthreads();
  const u64 base = sweep_base(a.seed, 0);
  const i64 wave0 = (blockIdx.x * (i64)kBlock + threadIdx.x) >> 6, nwaves = ((i64)gridDim.x * kBlock) >> 6;
  for (i64 d = wave0; d < a.B; d += nwaves) {
    i64 lo, hi;
    doc_range(a, d, lo, hi);
    const i64 g = a.gid[d];
    for (i64 t = lo + lane; t < hi; t += 64) {
      int kn = -1;
      if ((u64)a.inv[t] < (u64)a.cap) {
        kn = (int)__umul64hi(draw(base, g, t - lo), (u64)a.K);
        atomicAdd(&dkh[kn], 1);
      }
      a.z_new[t] = (int16_t)kn;
    }
  }
  __syncthreads();
  flush_hist(dkh, a.K, a.out);
}

template <int R, bool VEC>
__global__ __launch_bounds__(kBlock) void lda_sample_kernel(DocArgs a) {
#pragma clang fp contract(off)
  __shared__ int cnt[kWaves][64 * R];
  __shared__ int dkh[64 * R];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int K = a.K, k0 = lane * R;
  int* my = cnt[wv];
  for (int k = threadIdx.x; k < K; k += kBlock) dkh[k] = 0;
  __syncthreads();
  const u64 base = sweep_base(a.seed, a.it);
  const double alpha = a.alpha, beta = a.beta, Vbeta = a.Vbeta;
  double cinv[R];  // 1 / (max(nk, 0) + Vbeta) of this lane's topics: the clock's snapshot
#pragma unroll
  for (int i = 0; i < R; ++i) {
    i64 t = k0 + i < K ? a.nk[k0 + i] : 0;
    if (t < 0) t = 0;
    cinv[i] = 1.0 / ((double)t + Vbeta);
  }
  const i64 wave0 = (blockIdx.x * (i64)kBlock + threadIdx.x) >> 6, nwaves = ((i64)gridDim.x * kBlock) >> 6;
  for (i64 d = wave0; d < a.B; d += nwaves) {
    i64 lo, hi;
    doc_range(a, d, lo, hi);
    const i64 g = a.gid[d];
    doc_counts(a, a.z_old, lo, hi, lane, my);
    int ndk[R];
#pragma unroll
    for (int i = 0; i < R; ++i) ndk[i] = k0 + i < K ? my[k0 + i] : 0;
    wave_lds_sync();  // (the next document clears the slice)
    for (i64 c0 = lo; c0 < hi; c0 += 64) {
      const int cn = hi - c0 < 64 ? (int)(hi - c0) : 64;
      int u_l = -1, zo_l = -1;
      if (lane < cn) {
        const i64 u = a.inv[c0 + lane];
        zo_l = a.z_old[c0 + lane];
        if ((u64)u < (u64)a.cap && (unsigned)zo_l < (unsigned)K) u_l = (int)u;
      }
      int zn_l = zo_l;
      u64 todo = __ballot(u_l >= 0);
      float cur[R], nxt[R];
      if (todo) load_topics<R, VEC>(a.rows + (i64)__shfl(u_l, __ffsll(todo) - 1, 64) * a.ld, k0, K, cur);
      while (todo) {
        const int jj = __ffsll(todo) - 1;
        todo &= todo - 1;
        if (todo) load_topics<R, VEC>(a.rows + (i64)__shfl(u_l, __ffsll(todo) - 1, 64) * a.ld, k0, K, nxt);
        const int ko = __shfl(zo_l, jj, 64);
        const u64 r = draw(base, g, c0 - lo + jj);
        u64 wt[R], s = 0;
#pragma unroll
        for (int i = 0; i < R; ++i) {
          const int k = k0 + i;
          wt[i] = 0;
          if (k < K) {
            const bool e = k == ko;
            ndk[i] -= e;
            const double av = (double)ndk[i] + alpha;
            double bv = (double)cur[i];
            double cv = cinv[i];
            if (e) {
              bv = bv - 1.0;
              i64 t = a.nk[k] - 1;
              if (t < 0) t = 0;
              cv = 1.0 / ((double)t + Vbeta);
            }
            bv = fmax(bv, 0.0) + beta;
            const double x = (av * bv) * cv;
            wt[i] = (u64)(x * 1099511627776.0) + 1;
          }
          s += wt[i];
        }
        u64 incl = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const u64 t = __shfl_up(incl, o, 64);
          if (lane >= o) incl += t;
        }
        const u64 T = __shfl(incl, 63, 64);
        const u64 target = __umul64hi(r, T);
        const u64 win = __ballot(incl > target);
        int kn = ko;  // (only weights outside the rule's bounds can leave no winner)
        if (win) {
          int cand = K - 1;
          u64 p = incl - s;
          bool found = false;
#pragma unroll
          for (int i = 0; i < R; ++i) {
            p += wt[i];
            if (!found && k0 + i < K && p > target) {
              cand = k0 + i;
              found = true;
            }
          }
          kn = __shfl(cand, __ffsll(win) - 1, 64);
        }
#pragma unroll
        for (int i = 0; i < R; ++i) ndk[i] += k0 + i == kn;
        if (lane == jj) zn_l = kn;
        if (lane == 0 && kn != ko) {
          atomicAdd(&dkh[ko], -1);
          atomicAdd(&dkh[kn], 1);
        }
        if (todo) {
#pragma unroll
          for (int i = 0; i < R; ++i) cur[i] = nxt[i];
        }
      }
      if (lane < cn) a.z_new[c0 + lane] = (int16_t)zn_l;
    }
  }
  __syncthreads();
  flush_hist(dkh, K, a.out);
}

// ------------------------------------------------------------------------------------------- loglik
template <int R, bool VEC>
__global__ __launch_bounds__(kBlock) void lda_loglik_kernel(DocArgs a) {
#pragma clang fp contract(off)
  __shared__ int cnt[kWaves][64 * R];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int K = a.K, k0 = lane * R;
  int* my = cnt[wv];
  const double alpha = a.alpha, beta = a.beta, Vbeta = a.Vbeta;
  const double Ka = (double)K * alpha;
  double den[R];
#pragma unroll
  for (int i = 0; i < R; ++i) den[i] = (double)(k0 + i < K ? a.nk[k0 + i] : 0) + Vbeta;
  i64 sum = 0, tokens = 0;
  const i64 wave0 = (blockIdx.x * (i64)kBlock + threadIdx.x) >> 6, nwaves = ((i64)gridDim.x * kBlock) >> 6;
  for (i64 d = wave0; d < a.B; d += nwaves) {
    i64 lo, hi;
    doc_range(a, d, lo, hi);
    const int L = doc_counts(a, a.z_old, lo, hi, lane, my);
    const double dl = (double)L + Ka;
    double th[R];
#pragma unroll
    for (int i = 0; i < R; ++i) th[i] = k0 + i < K ? ((double)my[k0 + i] + alpha) / dl : 0.0;
    wave_lds_sync();
    tokens += L;
    for (i64 c0 = lo; c0 < hi; c0 += 64) {
      const int cn = hi - c0 < 64 ? (int)(hi - c0) : 64;
      int u_l = -1;
      if (lane < cn) {
        const i64 u = a.inv[c0 + lane];
        const int zo = a.z_old[c0 + lane];
        if ((u64)u < (u64)a.cap && (unsigned)zo < (unsigned)K) u_l = (int)u;
      }
      u64 todo = __ballot(u_l >= 0);
      while (todo) {
        const int jj = __ffsll(todo) - 1;
        todo &= todo - 1;
        float v[R];
        load_topics<R, VEC>(a.rows + (i64)__shfl(u_l, jj, 64) * a.ld, k0, K, v);
        double p = 0.0;
#pragma unroll
        for (int i = 0; i < R; ++i)
          if (k0 + i < K) p += th[i] * (((double)v[i] + beta) / den[i]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o, 64);
        sum += llrint(-log(p) * 16777216.0);
      }
    }
  }
  if (lane == 0) {
    if (sum) atomicAdd(reinterpret_cast<u64*>(a.out), (u64)sum);
    if (tokens) atomicAdd(reinterpret_cast<u64*>(a.out) + 1, (u64)tokens);
  }
}

// ------------------------------------------------------------------------------------------- delta
struct DeltaArgs {
  const int32_t* members;
  const int32_t* memrow;
  const int16_t* z_old;
  const int16_t* z_new;
  int n, K, W;
  int64_t cap;
  float* delta;
  int32_t* part;
};

__device__ __forceinline__ void delta_member(const DeltaArgs& a, int m, int* h) {
  const int j = a.members[m];
  if ((unsigned)j >= (unsigned)a.n) return;
  if (a.z_old != nullptr) {
    const int zo = a.z_old[j];
    if ((unsigned)zo < (unsigned)a.K) atomicAdd(&h[zo], -1);
  }
  const int zn = a.z_new[j];
  if ((unsigned)zn < (unsigned)a.K) atomicAdd(&h[zn], 1);
}

// rows of up to kLdaWaveMax members: a tile of kTile consecutive unique rows per wave and iteration (one binary
// search per lane), then the wave counts the tile's rows one after another
constexpr int kTile = 8;

__global__ __launch_bounds__(kBlock) void lda_delta_kernel(DeltaArgs a) {
  __shared__ int hist[kWaves][kLdaMaxK];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int* my = hist[wv];
  const int U = member_unique(a.memrow, a.n, a.cap), W = a.W;
  const i64 wave0 = (blockIdx.x * (i64)kBlock + threadIdx.x) >> 6, nwaves = ((i64)gridDim.x * kBlock) >> 6;
  const i64 ntiles = ((i64)U + kTile - 1) / kTile;
  for (i64 tile = wave0; tile < ntiles; tile += nwaves) {
    const i64 ul = tile * kTile + lane;
    const bool valid = lane < kTile && ul < U;
    const int lo_l = valid ? lower_bound_i32(a.memrow, 0, a.n, ul) : a.n;
    int hi_l = __shfl_down(lo_l, 1, 64);
    if (lane == kTile - 1 || ul + 1 >= U) hi_l = valid ? lower_bound_i32(a.memrow, lo_l, a.n, ul + 1) : a.n;
    const int rows_here = U - tile * kTile < kTile ? (int)(U - tile * kTile) : kTile;
    for (int r = 0; r < rows_here; ++r) {
      const int lo = __shfl(lo_l, r, 64), hi = __shfl(hi_l, r, 64);
      const int M = hi - lo;
      if (M <= 0 || M > kLdaWaveMax) continue;  // (uniform)
      for (int k = lane; k < W; k += 64) my[k] = 0;
      wave_lds_sync();
      for (int m = lo + lane; m < hi; m += 64) delta_member(a, m, my);
      wave_lds_sync();
      float* out = a.delta + (tile * kTile + r) * W;
      for (int k = lane; k < W; k += 64) out[k] = (float)my[k];
      wave_lds_sync();
    }
  }
}

// workgroup p counts the members of chunk p that belong to a heavy row into part[(2 p + s) * W ...] (member_rows.h)
__global__ __launch_bounds__(kBlock) void lda_delta_heavy_kernel(DeltaArgs a) {
  __shared__ int h[kLdaMaxK];
  const int W = a.W;
  const int64_t p = blockIdx.x;
  const int64_t c_lo = p * kLdaChunk, c_hi = (c_lo + kLdaChunk) < a.n ? (c_lo + kLdaChunk) : a.n;
  for (int s = 0; s < 2; ++s) {
    int r, lo, hi;
    if (!member_heavy_row<kLdaChunk, kLdaWaveMax>(a.memrow, a.n, a.cap, p, s, r, lo, hi)) continue;  // block-uniform
    const int m0 = lo > c_lo ? lo : (int)c_lo, m1 = hi < c_hi ? hi : (int)c_hi;
    for (int k = threadIdx.x; k < W; k += kBlock) h[k] = 0;
    __syncthreads();
    for (int m = m0 + threadIdx.x; m < m1; m += kBlock) delta_member(a, m, h);
    __syncthreads();
    for (int k = threadIdx.x; k < W; k += kBlock) a.part[(2 * p + s) * W + k] = h[k];
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------- launchers
void check_model(const char* op, int K, double alpha, double beta, double Vbeta, int64_t ld, int64_t cap, int64_t B,
                 int64_t n, int blocks) {
  const std::string o(op);
  if (K < kLdaMinK || K > kLdaMaxK) throw std::runtime_error(o + ": K outside [2, 1024]");
  if (!(alpha > 0.0 && alpha <= kLdaMaxPrior)) throw std::runtime_error(o + ": alpha outside (0, 64]");
  if (!(beta > 0.0 && beta <= kLdaMaxPrior)) throw std::runtime_error(o + ": beta outside (0, 64]");
  if (!(Vbeta > 0.0 && Vbeta < 1.0e300)) throw std::runtime_error(o + ": Vbeta must be positive and finite");
  if (ld < K) throw std::runtime_error(o + ": ld < K");
  if (blocks < 0 || blocks > kLdaMaxBlocks) throw std::runtime_error(o + ": blocks outside [0, 65535]");
  if (n < 0 || B < 0 || cap < 0 || n >= (1ll << 31) || B >= (1ll << 31) || cap >= (1ll << 31))
    throw std::runtime_error(o + ": n, B and cap must lie in [0, 2^31)");
}

// f.run<R, VEC>() for the lane shape of (K, vec)
template <typename F>
void dispatch_topics(int K, bool vec, const F& f) {
  const int per = (K + 63) >> 6;
  if (per <= 1) return f.template run<1, false>();
  if (per <= 2) return f.template run<2, false>();
  if (per <= 4) return vec ? f.template run<4, true>() : f.template run<4, false>();
  if (per <= 8) return vec ? f.template run<8, true>() : f.template run<8, false>();
  return vec ? f.template run<16, true>() : f.template run<16, false>();
}

struct SampleLaunch {
  DocArgs a;
  int grid;
  hipStream_t s;
  template <int R, bool VEC>
  void run() const {
    hipLaunchKernelGGL((lda_sample_kernel<R, VEC>), grid, kBlock, 0, s, a);
  }
};

struct LoglikLaunch {
  DocArgs a;
  int grid;
  hipStream_t s;
  template <int R, bool VEC>
  void run() const {
    hipLaunchKernelGGL((lda_loglik_kernel<R, VEC>), grid, kBlock, 0, s, a);
  }
};

}  // namespace

void lda_sample(const int64_t* rowptr, const int64_t* gid, const int64_t* inv, const int16_t* z_old,
                const float* rows, int64_t ld, int64_t width, int64_t cap, const int64_t* nk, int K, double alpha,
                double beta, double Vbeta, uint64_t seed, uint64_t it, int64_t B, int64_t n, int16_t* z_new,
                int64_t* dk, int blocks, hipStream_t stream) {
  check_model("lda_sample", K, alpha, beta, Vbeta, ld, cap, B, n, blocks);
  if (width < K || width > ld) throw std::runtime_error("lda_sample: width outside [K, ld]");
  if (B <= 0 || n <= 0) return;  // (an empty z_old has no address: checked after this)
  if ((z_old == nullptr) != (it == 0))
    throw std::runtime_error("lda_sample: it == 0 is the initialisation and takes no z_old; a sweep needs one");
  const DocArgs a{rowptr, gid, inv, z_old, rows, ld, cap, nk, K, alpha, beta, Vbeta, seed, it, B, n, z_new, dk};
  const int grid = blocks > 0 ? blocks : grid_for(B * 64, kBlock, 4096);
  if (z_old == nullptr) {
    hipLaunchKernelGGL(lda_init_kernel, grid, kBlock, 0, stream, a);
  } else {
    const bool vec = ld % 4 == 0 && aligned16(rows) && width >= ((K + 3) & ~3);
    dispatch_topics(K, vec, SampleLaunch{a, grid, stream});
  }
  MINIPS_HIP_CHECK(hipGetLastError());
}

void lda_loglik(const int64_t* rowptr, const int64_t* inv, const int16_t* z, const float* rows, int64_t ld,
                int64_t width, int64_t cap, const int64_t* nk, int K, double alpha, double beta, double Vbeta,
                int64_t B, int64_t n, int64_t* acc, int blocks, hipStream_t stream) {
  check_model("lda_loglik", K, alpha, beta, Vbeta, ld, cap, B, n, blocks);
  if (width < K || width > ld) throw std::runtime_error("lda_loglik: width outside [K, ld]");
  if (B <= 0 || n <= 0) return;
  const DocArgs a{rowptr, nullptr, inv, z, rows, ld, cap, nk, K, alpha, beta, Vbeta, 0, 0, B, n, nullptr, acc};
  const int grid = blocks > 0 ? blocks : grid_for(B * 64, kBlock, 4096);
  const bool vec = ld % 4 == 0 && aligned16(rows) && width >= ((K + 3) & ~3);
  dispatch_topics(K, vec, LoglikLaunch{a, grid, stream});
  MINIPS_HIP_CHECK(hipGetLastError());
}

int64_t lda_delta_part_ints(int64_t n, int W) {
  return member_part_elems(n, W, kLdaChunk, kLdaWaveMax);
}

void lda_delta(const int32_t* members, const int32_t* memrow, const int16_t* z_old, const int16_t* z_new, int64_t n,
               int K, int64_t cap, float* delta, int32_t* part, int blocks, hipStream_t stream) {
  if (K < kLdaMinK || K > kLdaMaxK) throw std::runtime_error("lda_delta: K outside [2, 1024]");
  if (blocks < 0 || blocks > kLdaMaxBlocks) throw std::runtime_error("lda_delta: blocks outside [0, 65535]");
  if (n < 0 || cap < 0 || n >= (1ll << 31) || cap >= (1ll << 31))
    throw std::runtime_error("lda_delta: n and cap must lie in [0, 2^31)");
  if (n <= 0 || cap <= 0) return;
  const int W = (K + 3) & ~3;
  const bool heavy = n > kLdaWaveMax;
  if (heavy && part == nullptr) throw std::runtime_error("lda_delta: part workspace missing");
  const DeltaArgs a{members, memrow, z_old, z_new, (int)n, K, W, cap, delta, part};
  const int64_t urows = cap < n ? cap : n;  // at most this many unique rows
  const int grid = blocks > 0 ? blocks : grid_for(urows * 8, kBlock, 4096);
  hipLaunchKernelGGL(lda_delta_kernel, grid, kBlock, 0, stream, a);
  if (heavy) {
    const int chunks = member_chunks(n, kLdaChunk);
    hipLaunchKernelGGL(lda_delta_heavy_kernel, chunks, kBlock, 0, stream, a);
    hipLaunchKernelGGL((member_heavy_fold_kernel<int32_t, int64_t, kLdaChunk, kLdaWaveMax>), chunks, kBlock, 0, stream,
                       a.memrow, a.n, a.cap, W, a.part, a.delta);
  }
  MINIPS_HIP_CHECK(hipGetLastError());
}

}  // namespace minips_k
