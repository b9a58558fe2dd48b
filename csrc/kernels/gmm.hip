// Gaussian-mixture EM-step kernels for gfx950: scores, row softmax and sufficient statistics of a tile of points in one
// workgroup, both products by v_mfma_f32_16x16x4_f32. The rule, the mapping and the launchers' contracts are in gmm.h.
#include <math.h>

#include <stdexcept>
#include <string>

#include "common.h"
#include "gmm.h"

namespace minips_k {
namespace {

constexpr int kBlock = 256;
constexpr int kTP = kGmmTile;

// LDS of one workgroup, in floats (every region a multiple of 4 floats: float4 stores stay aligned).
template <int KPB, int DPB, bool ACC>
struct Lds {
  static constexpr int kLdX = DPB + 4;
  static constexpr int kLdR = KPB + 4;
  static constexpr int kLdC = 2 * DPB + 4;
  static constexpr int kTile = kTP * kLdX;
  static constexpr int kR = 2 * kTile;                    // R [64][KPB + 4]; the chunk's s0 fold is laid over it
  static constexpr int kC = kR + (ACC ? kTP * kLdR : 0);  // coef [KPB][2 DPB + 4]
  static constexpr int kCst = kC + KPB * kLdC;
  static constexpr int kShift = kCst + KPB;
  static constexpr int kLse = kShift + DPB;               // the tile's lse [64] (0 where it does not count)
  static constexpr int kBad = kLse + kTP;                 // the tile's bad flags [64] (int)
  static constexpr int kLl = kBad + kTP;                  // the chunk's ll fold [64] (double)
  static constexpr int kTotal = kLl + 2 * kTP;
  static_assert(!ACC || kTP * kLdR >= 16 * KPB, "the s0 fold must fit the R tile");
  static_assert(kTotal * 4 <= 160 * 1024, "LDS budget of a CU");
};

// The accumulator tiles (kt, jt) of R^T [x | x^2]: NK x NJ tiles of 16 x 16, dealt to the four waves as WK row groups
// by WJ column groups. Wave (wk, wj) owns kt = wk + WK a, jt = wj + WJ b.
template <int KPB, int DPB>
struct Deal {
  static constexpr int NK = KPB / 16, NJX = DPB / 16, NJ = 2 * NJX;
  static constexpr int WJ = NJ >= 4 ? 4 : NJ, WK = 4 / WJ;
  static constexpr int AK = (NK + WK - 1) / WK, BJ = (NJ + WJ - 1) / WJ;
};

struct EArgs {
  const float* X;
  int64_t ld;
  int n, D, K, dp;
  bool vec;
  const float* shift;
  const float* coef;
  const float* cst;
  float* part;
  double* llpart;
  int32_t* assign;
  float* logp;
  int32_t* bad;
  int nchunks;
};

template <int DPB>
struct Prefetch {
  float4 v[DPB / 16];
};

// 64 points from j0 (below hi) minus shift -> registers; a thread holds DPB / 16 quads, the same columns every tile
template <int DPB>
__device__ __forceinline__ void tile_fetch(const EArgs& g, const float* shift_s, int j0, int hi, Prefetch<DPB>& pf) {
  constexpr int Q = DPB / 4;
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < DPB / 16; ++i) {
    const int idx = tid + kBlock * i, r = idx / Q, q = idx - r * Q, j = j0 + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < hi && 4 * q < g.D) {
      const float* p = g.X + (int64_t)j * g.ld + 4 * q;
      const float4 sh = *reinterpret_cast<const float4*>(shift_s + 4 * q);
      if (g.vec && 4 * q + 3 < g.D) {
        const float4 x = *reinterpret_cast<const float4*>(p);
        v = make_float4(x.x - sh.x, x.y - sh.y, x.z - sh.z, x.w - sh.w);
      } else {
        v.x = p[0] - sh.x;
        if (4 * q + 1 < g.D) v.y = p[1] - sh.y;
        if (4 * q + 2 < g.D) v.z = p[2] - sh.z;
        if (4 * q + 3 < g.D) v.w = p[3] - sh.w;
      }
    }
    pf.v[i] = v;
  }
}

template <int DPB>
__device__ __forceinline__ void tile_stash(float* tile, const Prefetch<DPB>& pf) {
  constexpr int Q = DPB / 4;
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < DPB / 16; ++i) {
    const int idx = tid + kBlock * i, r = idx / Q, q = idx - r * Q;
    *reinterpret_cast<float4*>(tile + r * (DPB + 4) + 4 * q) = pf.v[i];
  }
}

__device__ __forceinline__ float group_sum16(float v) {  // over the 16 lanes of a lane group, the same bits in each
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int KPB, int DPB, bool ACC>
__global__ __launch_bounds__(kBlock) void gmm_estep_kernel(EArgs g) {
  using L = Lds<KPB, DPB, ACC>;
  using T = Deal<KPB, DPB>;
  __shared__ __attribute__((aligned(16))) float sm[L::kTotal];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = lane >> 4, c16 = lane & 15;
  float* cs = sm + L::kC;
  float* cst_s = sm + L::kCst;
  float* shift_s = sm + L::kShift;
  float* lse_s = sm + L::kLse;
  int* bad_s = reinterpret_cast<int*>(sm + L::kBad);
  double* ll_s = reinterpret_cast<double*>(sm + L::kLl);

  // coef, cst and shift stay in LDS for the whole kernel; the pads are zero and the components past K dead
  for (int idx = tid; idx < KPB * L::kLdC; idx += kBlock) {
    const int k = idx / L::kLdC, c = idx - k * L::kLdC;
    const int half = c >= DPB ? 1 : 0, d = c - half * DPB;
    float v = 0.f;
    if (k < g.K && c < 2 * DPB && d < g.D) v = g.coef[(int64_t)k * 2 * g.dp + half * g.dp + d];
    cs[idx] = v;
  }
  for (int k = tid; k < KPB; k += kBlock) cst_s[k] = k < g.K ? g.cst[k] : -INFINITY;
  for (int d = tid; d < DPB; d += kBlock) shift_s[d] = d < g.D ? g.shift[d] : 0.f;
  __syncthreads();

  const int wk = wave / T::WJ, wj = wave - wk * T::WJ;
  const int dsteps = (g.D + 3) / 4;
  float cstv[T::NK];
#pragma unroll
  for (int ct = 0; ct < T::NK; ++ct) cstv[ct] = cst_s[16 * ct + c16];

  for (int c = blockIdx.x; c < g.nchunks; c += gridDim.x) {
    const int lo = c * kGmmChunk, hi = g.n - lo < kGmmChunk ? g.n : lo + kGmmChunk;
    const int ntile = (hi - lo + kTP - 1) / kTP;
    v4f acc[ACC ? T::AK * T::BJ : 1];
    float racc[T::NK];
    if (ACC) {
#pragma unroll
      for (int p = 0; p < T::AK * T::BJ; ++p) acc[p] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ct = 0; ct < T::NK; ++ct) racc[ct] = 0.f;
    }
    double llacc = 0.0;  // threads < 64: the point tid of every tile, in tile order
    int badacc = 0;
    Prefetch<DPB> pf;
    tile_fetch<DPB>(g, shift_s, lo, hi, pf);
    tile_stash<DPB>(sm, pf);
    __syncthreads();
    for (int t = 0; t < ntile; ++t) {
      const int buf = t & 1, j0 = lo + t * kTP;
      const bool more = t + 1 < ntile;
      if (more) tile_fetch<DPB>(g, shift_s, j0 + kTP, hi, pf);  // in flight during the math below
      float* xt = sm + buf * L::kTile;

      // ---- scores of this wave's 16 points against every component tile
      v4f tt[T::NK];
#pragma unroll
      for (int ct = 0; ct < T::NK; ++ct) tt[ct] = v4f{0.f, 0.f, 0.f, 0.f};
      {
        const float* xp = xt + (16 * wave + c16) * L::kLdX + grp;
        const float* cp = cs + c16 * L::kLdC + grp;
        for (int kk = 0; kk < dsteps; ++kk) {
          const float x = xp[4 * kk], xx = x * x;
#pragma unroll
          for (int ct = 0; ct < T::NK; ++ct) {
            if (16 * ct < g.K) {
              tt[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(xx, cp[16 * ct * L::kLdC + 4 * kk], tt[ct], 0, 0, 0);
              tt[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(x, cp[16 * ct * L::kLdC + DPB + 4 * kk], tt[ct], 0, 0, 0);
            }
          }
        }
      }

      // ---- row softmax: tt[ct][v] is the score of point 4 grp + v against component 16 ct + c16
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = 16 * wave + 4 * grp + v, j = j0 + row;
        const bool valid = j < hi;
        float m = -INFINITY;
        int arg = c16;
#pragma unroll
        for (int ct = 0; ct < T::NK; ++ct) {
          const float tv = tt[ct][v] + cstv[ct];
          tt[ct][v] = tv;
          if (tv > m) {
            m = tv;
            arg = 16 * ct + c16;
          }
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          const float om = __shfl_xor(m, o, 64);
          const int oa = __shfl_xor(arg, o, 64);
          if (om > m || (om == m && oa < arg)) {
            m = om;
            arg = oa;
          }
        }
        float s = 0.f;
#pragma unroll
        for (int ct = 0; ct < T::NK; ++ct) s += expf(tt[ct][v] - m);
        s = group_sum16(s);
        const float lse = m + logf(s);
        const bool fin = valid && lse - lse == 0.f;  // finite
        if (ACC) {
#pragma unroll
          for (int ct = 0; ct < T::NK; ++ct) {
            const float r = fin ? expf(tt[ct][v] - lse) : 0.f;
            sm[L::kR + row * L::kLdR + 16 * ct + c16] = r;
            racc[ct] += r;
          }
          if (valid && !fin) {  // 0 * NaN: the point leaves the x operand too
            for (int col = c16; col < DPB; col += 16) xt[row * L::kLdX + col] = 0.f;
          }
        }
        if (c16 == 0) {
          lse_s[row] = fin ? lse : 0.f;
          bad_s[row] = valid && !fin ? 1 : 0;
          if (valid) {
            if (g.assign) g.assign[j] = fin ? arg : -1;
            if (g.logp) g.logp[j] = fin ? lse : NAN;
          }
        }
      }
      __syncthreads();  // R, lse and the zeroed rows are complete
      if (tid < kTP) {
        llacc += (double)lse_s[tid];
        badacc += bad_s[tid];
      }

      // ---- S += R^T [x | x^2]
      if (ACC) {
        const int here = min(kTP, hi - j0), nst = (here + 3) / 4;
        const float* rp = sm + L::kR + grp * L::kLdR + c16;
        const float* xp = xt + grp * L::kLdX + c16;
        for (int s4 = 0; s4 < nst; ++s4) {
          float a[T::AK], b[T::BJ];
#pragma unroll
          for (int ia = 0; ia < T::AK; ++ia) {
            const int kt = wk + T::WK * ia;
            a[ia] = kt < T::NK ? rp[4 * s4 * L::kLdR + 16 * kt] : 0.f;
          }
#pragma unroll
          for (int ib = 0; ib < T::BJ; ++ib) {
            const int jt = wj + T::WJ * ib, sq = jt >= T::NJX ? 1 : 0, jx = jt - sq * T::NJX;
            const float x = jt < T::NJ ? xp[4 * s4 * L::kLdX + 16 * jx] : 0.f;
            b[ib] = sq ? x * x : x;
          }
#pragma unroll
          for (int ia = 0; ia < T::AK; ++ia) {
#pragma unroll
            for (int ib = 0; ib < T::BJ; ++ib) {
              const int kt = wk + T::WK * ia, jt = wj + T::WJ * ib, jx = jt >= T::NJX ? jt - T::NJX : jt;
              if (kt < T::NK && jt < T::NJ && 16 * kt < g.K && 16 * jx < g.D)
                acc[ia * T::BJ + ib] =
                    __builtin_amdgcn_mfma_f32_16x16x4f32(a[ia], b[ib], acc[ia * T::BJ + ib], 0, 0, 0);
            }
          }
        }
      }
      if (more) tile_stash<DPB>(sm + (buf ^ 1) * L::kTile, pf);
      __syncthreads();  // the next tile is staged; R, lse and this tile are free
    }

    // ---- the chunk's partial: accumulators straight to the workspace, s0 and ll folded through LDS in a fixed order
    if (ACC) {
      const int W = 2 * g.D + 1;
      float* out = g.part + (int64_t)c * g.K * W;
#pragma unroll
      for (int ia = 0; ia < T::AK; ++ia) {
#pragma unroll
        for (int ib = 0; ib < T::BJ; ++ib) {
          const int kt = wk + T::WK * ia, jt = wj + T::WJ * ib, sq = jt >= T::NJX ? 1 : 0, jx = jt - sq * T::NJX;
          const int d = 16 * jx + c16;
          if (kt < T::NK && jt < T::NJ && d < g.D) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              const int k = 16 * kt + 4 * grp + v;
              if (k < g.K) out[(int64_t)k * W + sq * g.D + d] = acc[ia * T::BJ + ib][v];
            }
          }
        }
      }
#pragma unroll
      for (int ct = 0; ct < T::NK; ++ct) sm[L::kR + (4 * wave + grp) * KPB + 16 * ct + c16] = racc[ct];
    }
    if (tid < kTP) {
      ll_s[tid] = llacc;
      bad_s[tid] = badacc;
    }
    __syncthreads();
    if (ACC && tid < g.K) {
      float s0 = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) s0 += sm[L::kR + i * KPB + tid];
      g.part[(int64_t)c * g.K * (2 * g.D + 1) + (int64_t)tid * (2 * g.D + 1) + 2 * g.D] = s0;
    }
    if (tid == 0) {
      double ll = 0.0;
      int nb = 0;
      for (int i = 0; i < kTP; ++i) {
        ll += ll_s[i];
        nb += bad_s[i];
      }
      g.llpart[c] = ll;
      if (nb > 0 && g.bad) atomicAdd(g.bad, nb);
    }
    __syncthreads();
  }
}

// S[j] = sum over chunks of part[c][j] in chunk order (blocks < gridDim.x - 1); the last workgroup adds llpart.
__global__ __launch_bounds__(kBlock) void gmm_fold_kernel(const float* part, const double* llpart, int nchunks, int m,
                                                          float* S, double* ll) {
  if (blockIdx.x + 1 == gridDim.x) {
    if (threadIdx.x >= 64) return;
    double s = 0.0;
    for (int c = threadIdx.x; c < nchunks; c += 64) s += llpart[c];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) *ll = s;
    return;
  }
  const int idx = blockIdx.x * kBlock + threadIdx.x;
  if (S == nullptr || idx >= m) return;
  // eight loads in flight at a time, added in chunk order all the same
  float s = 0.f;
  int c = 0;
  for (; c + 8 <= nchunks; c += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[(int64_t)(c + u) * m + idx];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; c < nchunks; ++c) s += part[(int64_t)c * m + idx];
  S[idx] = s;
}

__device__ __forceinline__ bool finite_(float v) { return v - v == 0.f; }

// a wave per component (gmm.h: Prepare)
__global__ __launch_bounds__(kBlock) void gmm_prepare_kernel(const float* s, int K, int D, int dp, float var_floor,
                                                             float* coef, float* cst) {
  const int lane = threadIdx.x & 63, k = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  const int W = 2 * D + 1;
  float tot = 0.f;
  for (int j = lane; j < K; j += 64) {
    const float v = s[(int64_t)j * W + 2 * D];
    if (finite_(v) && v > 0.f) tot += v;
  }
  tot = warp_sum(tot);
  if (k >= K) return;  // the whole wave
  const float s0 = s[(int64_t)k * W + 2 * D];
  bool dead = !(finite_(s0) && s0 > 0.f);
  float q = 0.f, ca[2] = {0.f, 0.f}, cb[2] = {0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int d = lane + 64 * i;
    if (d < D) {
      const float s1 = s[(int64_t)k * W + d], s2 = s[(int64_t)k * W + D + d];
      if (!finite_(s1) || !finite_(s2)) dead = true;
      const float mu = s1 / s0, v = s2 / s0 - mu * mu, var = v > var_floor ? v : var_floor;
      ca[i] = -0.5f / var;
      cb[i] = mu / var;
      q += mu * mu / var + logf(var);
    }
  }
  q = warp_sum(q);
  const float c = logf(s0 / tot) - 0.5f * q - 0.5f * (float)D * 1.8378770664093453f;
  dead = __any(dead) || !finite_(c);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int d = lane + 64 * i;
    if (d < dp) {
      coef[(int64_t)k * 2 * dp + d] = (dead || d >= D) ? 0.f : ca[i];
      coef[(int64_t)k * 2 * dp + dp + d] = (dead || d >= D) ? 0.f : cb[i];
    }
  }
  if (lane == 0) cst[k] = dead ? -INFINITY : c;
}

template <int KPB, int DPB>
void launch_estep(const EArgs& a, bool accumulate, int grid, hipStream_t s) {
  if (accumulate) {
    hipLaunchKernelGGL((gmm_estep_kernel<KPB, DPB, true>), grid, kBlock, 0, s, a);
  } else {
    hipLaunchKernelGGL((gmm_estep_kernel<KPB, DPB, false>), grid, kBlock, 0, s, a);
  }
}

}  // namespace

void gmm_prepare(const float* s, int K, int D, float var_floor, float* coef, float* cst, hipStream_t stream) {
  if (!gmm_shape_ok(K, D)) throw std::runtime_error("gmm_prepare: 1 <= K, D <= 128 and KP * DP <= 8192");
  if (!(var_floor > 0.f)) throw std::runtime_error("gmm_prepare: var_floor must be > 0");
  hipLaunchKernelGGL(gmm_prepare_kernel, (K + 3) / 4, kBlock, 0, stream, s, K, D, gmm_pad(D), var_floor, coef, cst);
  MINIPS_HIP_CHECK(hipGetLastError());
}

void gmm_estep(const float* X, int64_t ld, int64_t n, int D, int K, const float* shift, const float* coef,
               const float* cst, float* S, double* ll, int32_t* assign, float* logp, int32_t* bad, float* part,
               double* llpart, int blocks, hipStream_t stream) {
  if (!gmm_shape_ok(K, D)) throw std::runtime_error("gmm_estep: 1 <= K, D <= 128 and KP * DP <= 8192");
  if (n < 0 || n >= (1ll << 31) - kGmmChunk) throw std::runtime_error("gmm_estep: n must be below 2^31 - 2048");
  if (ld < D) throw std::runtime_error("gmm_estep: the points' leading dimension is below D");
  if (blocks < 0 || blocks > kGmmMaxBlocks) throw std::runtime_error("gmm_estep: 0 <= blocks <= 65535");
  const int nchunks = (int)gmm_chunks(n), m = K * (2 * D + 1);
  if (nchunks > 0) {
    if (llpart == nullptr || (S != nullptr && part == nullptr))
      throw std::runtime_error("gmm_estep: workspace missing");
    const EArgs a{X, ld, (int)n, D, K, gmm_pad(D), ld % 4 == 0 && aligned16(X), shift, coef, cst,
                  part, llpart, assign, logp, bad, nchunks};
    const int grid = blocks > 0 ? blocks : (nchunks < 1024 ? nchunks : 1024);
    const int kp = gmm_pad(K), dp = gmm_pad(D);
    const bool acc = S != nullptr;
    // the cheapest bucket that holds the shape; every shape of gmm_shape_ok fits one
    if (kp <= 16 && dp <= 16) launch_estep<16, 16>(a, acc, grid, stream);
    else if (kp <= 32 && dp <= 32) launch_estep<32, 32>(a, acc, grid, stream);
    else if (kp <= 64 && dp <= 64) launch_estep<64, 64>(a, acc, grid, stream);
    else if (kp <= 16) launch_estep<16, 128>(a, acc, grid, stream);
    else if (dp <= 16) launch_estep<128, 16>(a, acc, grid, stream);
    else if (kp <= 64) launch_estep<64, 128>(a, acc, grid, stream);
    else if (dp <= 64) launch_estep<128, 64>(a, acc, grid, stream);
    else launch_estep<96, 96>(a, acc, grid, stream);
  }
  hipLaunchKernelGGL(gmm_fold_kernel, (S ? (m + kBlock - 1) / kBlock : 0) + 1, kBlock, 0, stream, part, llpart, nchunks,
                     m, S, ll);
  MINIPS_HIP_CHECK(hipGetLastError());
}

}  // namespace minips_k
