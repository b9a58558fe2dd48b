// Full-covariance Gaussian-mixture EM-step kernels for gfx950: whitened scores with an online softmax, weighted
// second moments on lower-triangle tiles, both by v_mfma_f32_16x16x4_f32, and the Cholesky prepare. The rule, the
// mapping and the launchers' contracts are in gmm_full.h.
#include <math.h>

#include <stdexcept>
#include <string>

#include "common.h"
#include "gmm_full.h"

namespace minips_k {
namespace {

constexpr int kBlock = 256;
constexpr int kTS = 64;  // points per statistics tile

__device__ __forceinline__ bool finite_(float v) { return v - v == 0.f; }

// ------------------------------------------------------------------------------------------------ scores
struct SArgs {
  const float* X;
  int64_t ld;
  int n, D, K, kp;
  const float* shift;
  const float* Wh;
  const float* b;
  const float* cst;
  float* T;
  double* llpart;
  int32_t* assign;
  float* logp;
  int32_t* bad;
  int ntiles;
};

// Wh_k [DPB][DPB] and b_k [DPB] -> registers; a thread holds NF quads of Wh and one value of b
template <int DPB>
struct WFetch {
  static constexpr int kQuads = DPB * DPB / 4, NF = (kQuads + kBlock - 1) / kBlock;
  float4 v[NF];
  float b;
};

template <int DPB>
__device__ __forceinline__ void wh_fetch(const SArgs& g, int k, WFetch<DPB>& f) {
  using F = WFetch<DPB>;
  const int tid = threadIdx.x;
  const float4* src = reinterpret_cast<const float4*>(g.Wh + (int64_t)k * DPB * DPB);
#pragma unroll
  for (int i = 0; i < F::NF; ++i) {
    const int idx = tid + kBlock * i;
    f.v[i] = idx < F::kQuads ? src[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  f.b = tid < DPB ? g.b[(int64_t)k * DPB + tid] : 0.f;
}

template <int DPB>
__device__ __forceinline__ void wh_stash(float* buf, const WFetch<DPB>& f) {
  using F = WFetch<DPB>;
  constexpr int Q = DPB / 4;
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < F::NF; ++i) {
    const int idx = tid + kBlock * i, r = idx / Q, q = idx - r * Q;
    if (idx < F::kQuads) *reinterpret_cast<float4*>(buf + r * (DPB + 4) + 4 * q) = f.v[i];
  }
  if (tid < DPB) buf[DPB * (DPB + 4) + tid] = f.b;
}

// one halving step of the fold over a lane group: 2 O sums in, O sums out; the lanes with bit O set keep the upper half
template <int O>
__device__ __forceinline__ void fold_half(float* q, int c16) {
  const bool up = (c16 & O) != 0;
#pragma unroll
  for (int j = 0; j < O; ++j) {
    const float send = up ? q[j] : q[j + O], keep = up ? q[j + O] : q[j];
    q[j] = keep + __shfl_xor(send, O, 64);
  }
}

template <int DPB>
__global__ __launch_bounds__(kBlock) void gmmf_scores_kernel(SArgs g) {
  constexpr int NT = DPB / 16, KS = DPB / 4, LdW = DPB + 4, kBuf = DPB * LdW + DPB;
  __shared__ __attribute__((aligned(16))) float sm[2 * kBuf];
  __shared__ double ll_s[4];
  __shared__ int bad_s[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = lane >> 4, c16 = lane & 15;
  // after the fold this lane holds the score of one point of the wave's 64
  const int mine = 16 * (c16 >> 2) + 4 * grp + (c16 & 3);

  for (int tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
    const int64_t j0 = (int64_t)tile * kGmmFullTile + 64 * wave;
    // this wave's 64 points minus shift, as the MFMA A operand: xr[rt][kk] = x[16 rt + c16][4 kk + grp]
    float xr[4][KS];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
      const int64_t j = j0 + 16 * rt + c16;
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) {
        const int d = 4 * kk + grp;
        xr[rt][kk] = (j < g.n && d < g.D) ? g.X[j * g.ld + d] - g.shift[d] : 0.f;
      }
    }
    float m = -INFINITY, ssum = 0.f;
    int arg = 0;
    v4f tb = {0.f, 0.f, 0.f, 0.f};
    const int64_t jm = j0 + mine;
    const bool valid = jm < g.n;

    WFetch<DPB> pf;
    wh_fetch<DPB>(g, 0, pf);
    wh_stash<DPB>(sm, pf);
    __syncthreads();
    for (int k = 0; k < g.K; ++k) {
      const bool more = k + 1 < g.K;
      if (more) wh_fetch<DPB>(g, k + 1, pf);  // in flight during the math below
      const float* W = sm + (k & 1) * kBuf;
      const float* bs = W + DPB * LdW;
      float q[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) q[i] = 0.f;
#pragma unroll
      for (int jt = 0; jt < NT; ++jt) {
        v4f acc[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) acc[rt] = v4f{0.f, 0.f, 0.f, 0.f};
        const float* wp = W + (16 * jt + c16) * LdW + grp;
#pragma unroll
        for (int kk = 0; kk < 4 * (jt + 1); ++kk) {  // Wh is lower triangular: nothing right of the diagonal tile
          const float bv = wp[4 * kk];
#pragma unroll
          for (int rt = 0; rt < 4; ++rt)
            acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(xr[rt][kk], bv, acc[rt], 0, 0, 0);
        }
        const float bj = bs[16 * jt + c16];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const float y = acc[rt][v] - bj;
            q[4 * rt + v] += y * y;
          }
        }
      }
      fold_half<8>(q, c16);
      fold_half<4>(q, c16);
      fold_half<2>(q, c16);
      fold_half<1>(q, c16);
      const float t = g.cst[k] - 0.5f * q[0];
      if (t > m) {
        ssum = ssum * expf(m - t) + 1.f;
        m = t;
        arg = k;
      } else if (t != -INFINITY) {  // a NaN score lands here and poisons the sum
        ssum += expf(t - m);
      }
      tb[k & 3] = t;
      if (g.T != nullptr && valid && ((k & 3) == 3 || !more))
        *reinterpret_cast<v4f*>(g.T + jm * g.kp + (k & ~3)) = tb;
      if (more) wh_stash<DPB>(sm + ((k + 1) & 1) * kBuf, pf);
      __syncthreads();  // the next component is staged; this one's buffer is free
    }

    const float lse = m + logf(ssum);
    const bool fin = valid && finite_(lse);
    if (valid) {
      if (g.assign) g.assign[jm] = fin ? arg : -1;
      if (g.logp) g.logp[jm] = fin ? lse : NAN;
    }
    double ll = fin ? (double)lse : 0.0;
    int nb = valid && !fin ? 1 : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      ll += __shfl_xor(ll, o, 64);
      nb += __shfl_xor(nb, o, 64);
    }
    if (lane == 0) {
      ll_s[wave] = ll;
      bad_s[wave] = nb;
    }
    __syncthreads();
    if (tid == 0) {
      g.llpart[tile] = ((ll_s[0] + ll_s[1]) + ll_s[2]) + ll_s[3];
      const int tot = bad_s[0] + bad_s[1] + bad_s[2] + bad_s[3];
      if (tot > 0 && g.bad) atomicAdd(g.bad, tot);
    }
  }
}

// ------------------------------------------------------------------------------------------------ statistics
struct TArgs {
  const float* X;
  int64_t ld;
  int n, D, K, kp;
  bool vec;
  const float* shift;
  const float* T;
  const float* lse;
  float* part;
  int64_t chunk;
  int nchunks;
};

template <int DPB>
struct Stat {
  static constexpr int NT = DPB / 16, NTRI = NT * (NT + 1) / 2;
  static constexpr int G = DPB >= 48 ? 8 : 16, CW = G / 4;  // components a group, components a wave
  static constexpr int kLdX = DPB + 4, kLdR = 20;
  static constexpr int kX = kTS * kLdX, kBuf = kX + kTS * kLdR;
  static constexpr int kShift = 2 * kBuf, kTotal = kShift + DPB;
};

template <int DPB>
struct SFetch {
  float4 x[DPB / 16];
  float4 t;
  float lse;
};

// 64 points from j0 (below hi): x minus shift (zero for the rows of bad points), the group's scores and lse
template <int DPB>
__device__ __forceinline__ void stat_fetch(const TArgs& g, const float* shift_s, int64_t j0, int64_t hi, int kbase,
                                           SFetch<DPB>& f) {
  constexpr int Q = DPB / 4;
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < DPB / 16; ++i) {
    const int idx = tid + kBlock * i, r = idx / Q, q = idx - r * Q;
    const int64_t j = j0 + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < hi && 4 * q < g.D && finite_(g.lse[j])) {
      const float* p = g.X + j * g.ld + 4 * q;
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
    f.x[i] = v;
  }
  const int64_t j = j0 + (tid >> 2);
  const int c = 4 * (tid & 3);
  f.lse = NAN;
  f.t = make_float4(0.f, 0.f, 0.f, 0.f);
  if (j < hi && c < Stat<DPB>::G && kbase + c < g.K) {  // kbase + c + 3 < KP: both multiples of 4
    f.lse = g.lse[j];
    f.t = *reinterpret_cast<const float4*>(g.T + j * g.kp + kbase + c);
  }
}

template <int DPB>
__device__ __forceinline__ void stat_stash(const TArgs& g, float* buf, int kbase, const SFetch<DPB>& f) {
  using C = Stat<DPB>;
  constexpr int Q = DPB / 4;
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < DPB / 16; ++i) {
    const int idx = tid + kBlock * i, r = idx / Q, q = idx - r * Q;
    *reinterpret_cast<float4*>(buf + r * C::kLdX + 4 * q) = f.x[i];
  }
  const int c = 4 * (tid & 3), k = kbase + c;
  const bool fin = finite_(f.lse);  // NaN: a bad point, a point past the chunk or a column of another group
  float4 r;
  r.x = fin && k < g.K ? expf(f.t.x - f.lse) : 0.f;
  r.y = fin && k + 1 < g.K ? expf(f.t.y - f.lse) : 0.f;
  r.z = fin && k + 2 < g.K ? expf(f.t.z - f.lse) : 0.f;
  r.w = fin && k + 3 < g.K ? expf(f.t.w - f.lse) : 0.f;
  *reinterpret_cast<float4*>(buf + C::kX + (tid >> 2) * C::kLdR + c) = r;
}

template <int DPB>
__global__ __launch_bounds__(kBlock) void gmmf_stats_kernel(TArgs g) {
  using C = Stat<DPB>;
  __shared__ __attribute__((aligned(16))) float sm[C::kTotal];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = lane >> 4, c16 = lane & 15;
  const int kbase = blockIdx.y * C::G;
  float* shift_s = sm + C::kShift;
  for (int d = tid; d < DPB; d += kBlock) shift_s[d] = d < g.D ? g.shift[d] : 0.f;
  __syncthreads();
  const int W = g.D + g.D * g.D + 1;
  const bool ones_mine = wave == (C::NT & 3);  // the wave that owns the column of ones of R^T [X | 1]

  for (int c = blockIdx.x; c < g.nchunks; c += gridDim.x) {
    const int64_t lo = (int64_t)c * g.chunk, hi = g.n - lo < g.chunk ? g.n : lo + g.chunk;
    const int ntile = (int)((hi - lo + kTS - 1) / kTS);
    v4f acc[C::CW * C::NTRI], accx = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int p = 0; p < C::CW * C::NTRI; ++p) acc[p] = v4f{0.f, 0.f, 0.f, 0.f};
    SFetch<DPB> pf;
    stat_fetch<DPB>(g, shift_s, lo, hi, kbase, pf);
    stat_stash<DPB>(g, sm, kbase, pf);
    __syncthreads();
    for (int t = 0; t < ntile; ++t) {
      const int64_t j0 = lo + (int64_t)t * kTS;
      const bool more = t + 1 < ntile;
      if (more) stat_fetch<DPB>(g, shift_s, j0 + kTS, hi, kbase, pf);  // in flight during the math below
      const float* xt = sm + (t & 1) * C::kBuf;
      const float* rt = xt + C::kX;
      const int here = hi - j0 < kTS ? (int)(hi - j0) : kTS, nst = (here + 3) / 4;
      for (int s4 = 0; s4 < nst; ++s4) {
        const int row = 4 * s4 + grp;
        float xv[C::NT];
#pragma unroll
        for (int i = 0; i < C::NT; ++i) xv[i] = xt[row * C::kLdX + 16 * i + c16];
#pragma unroll
        for (int cw = 0; cw < C::CW; ++cw) {
          if (kbase + wave * C::CW + cw < g.K) {
            const float r = rt[row * C::kLdR + wave * C::CW + cw];
#pragma unroll
            for (int it = 0; it < C::NT; ++it) {
              const float a = r * xv[it];
#pragma unroll
              for (int jt = 0; jt <= it; ++jt) {
                const int p = cw * C::NTRI + it * (it + 1) / 2 + jt;
                acc[p] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xv[jt], acc[p], 0, 0, 0);
              }
            }
          }
        }
        // R^T [X | 1]: wave w takes the column tile w of X; one wave takes the column of ones as well
        const float ra = rt[row * C::kLdR + c16];
        if (wave < C::NT) {
          float bx = xv[0];
#pragma unroll
          for (int i = 1; i < C::NT; ++i) bx = wave == i ? xv[i] : bx;
          accx = __builtin_amdgcn_mfma_f32_16x16x4f32(ra, bx, accx, 0, 0, 0);
        }
        if (ones_mine) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ra, 1.f, acc1, 0, 0, 0);
      }
      if (more) stat_stash<DPB>(g, sm + ((t + 1) & 1) * C::kBuf, kbase, pf);
      __syncthreads();  // the next tile is staged; this one's buffer is free
    }

    // ---- the chunk's partial, straight from the accumulators: C[4 grp + v][c16]
    float* out = g.part + (int64_t)c * g.K * W;
#pragma unroll
    for (int cw = 0; cw < C::CW; ++cw) {
      const int k = kbase + wave * C::CW + cw;
      if (k < g.K) {
#pragma unroll
        for (int it = 0; it < C::NT; ++it) {
#pragma unroll
          for (int jt = 0; jt <= it; ++jt) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              const int d1 = 16 * it + 4 * grp + v, d2 = 16 * jt + c16;
              if (d1 < g.D && d2 <= d1)
                out[(int64_t)k * W + g.D + d1 * g.D + d2] = acc[cw * C::NTRI + it * (it + 1) / 2 + jt][v];
            }
          }
        }
      }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int kl = 4 * grp + v, k = kbase + kl, d = 16 * wave + c16;
      if (kl < C::G && k < g.K) {
        if (wave < C::NT && d < g.D) out[(int64_t)k * W + d] = accx[v];
        if (ones_mine && c16 == 0) out[(int64_t)k * W + W - 1] = acc1[v];
      }
    }
  }
}

// S[j] = sum over chunks of part[c][j] in chunk order, a thread per entry of the lower triangle (and of the other two
// blocks), which writes its mirror image too; the last workgroup adds llpart.
__global__ __launch_bounds__(kBlock) void gmmf_fold_kernel(const float* part, const double* llpart, int nchunks,
                                                           int ntiles, int K, int D, float* S, double* ll) {
  if (blockIdx.x + 1 == gridDim.x) {
    if (threadIdx.x >= 64) return;
    double s = 0.0;
    for (int c = threadIdx.x; c < ntiles; c += 64) s += llpart[c];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) *ll = s;
    return;
  }
  const int W = D + D * D + 1, m = K * W;
  const int idx = blockIdx.x * kBlock + threadIdx.x;
  if (S == nullptr || idx >= m) return;
  const int k = idx / W, e = idx - k * W;
  int d1 = 0, d2 = 0;
  if (e >= D && e < W - 1) {
    d1 = (e - D) / D;
    d2 = (e - D) - d1 * D;
    if (d2 > d1) return;  // written by its mirror image
  }
  float s = 0.f;
  int c = 0;
  for (; c + 8 <= nchunks; c += 8) {  // eight loads in flight at a time, added in chunk order all the same
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[(int64_t)(c + u) * m + idx];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; c < nchunks; ++c) s += part[(int64_t)c * m + idx];
  S[idx] = s;
  if (d1 > d2) S[k * W + D + d2 * D + d1] = s;
}

// ------------------------------------------------------------------------------------------------ prepare
// a workgroup per component (gmm_full.h: Prepare)
template <int DPB>
__global__ __launch_bounds__(kBlock) void gmmf_prepare_kernel(const float* s, int K, int D, float reg, float* Wh,
                                                              float* b, float* cst) {
  constexpr int Ld = DPB + 1;
  __shared__ float A[DPB * Ld];   // Sigma's lower triangle, then L in place
  __shared__ float Wi[DPB * Ld];  // L^-1
  __shared__ float mu_s[DPB];
  __shared__ float piv_s, tot_s, cst_s;
  const int tid = threadIdx.x, k = blockIdx.x;
  const int W = D + D * D + 1;
  const float* sk = s + (int64_t)k * W;
  if (tid < 64) {
    float tot = 0.f;
    for (int j = tid; j < K; j += 64) {
      const float v = s[(int64_t)j * W + W - 1];
      if (finite_(v) && v > 0.f) tot += v;
    }
    tot = warp_sum(tot);
    if (tid == 0) tot_s = tot;
  }
  const float s0 = sk[W - 1];
  int nonfin = 0;
  for (int e = tid; e < W; e += kBlock) nonfin |= finite_(sk[e]) ? 0 : 1;
  bool dead = __syncthreads_or(nonfin) != 0 || !(s0 > 0.f);
  if (tid < DPB) mu_s[tid] = tid < D ? __fdiv_rn(sk[tid], s0) : 0.f;
  __syncthreads();
  for (int e = tid; e < D * D; e += kBlock) {
    const int i = e / D, j = e - i * D;
    if (j <= i) A[i * Ld + j] = __fdiv_rn(sk[D + e], s0) - mu_s[i] * mu_s[j] + (i == j ? reg : 0.f);
  }
  __syncthreads();
  // left-looking Cholesky, thread i owns row i; every dot product serial in ascending order
  for (int j = 0; j < D; ++j) {
    float v = 0.f;
    if (tid >= j && tid < D) {
      v = A[tid * Ld + j];
      for (int p = 0; p < j; ++p) v -= A[tid * Ld + p] * A[j * Ld + p];
      if (tid == j) piv_s = v;
    }
    __syncthreads();
    const float piv = piv_s;
    if (!(piv > 0.f) || !finite_(piv)) dead = true;
    const float ljj = __fsqrt_rn(piv);
    if (tid >= j && tid < D) A[tid * Ld + j] = tid == j ? ljj : __fdiv_rn(v, ljj);
    __syncthreads();
  }
  // Wi = L^-1 by forward substitution, thread c owns column c
  if (tid < D) {
    const int c = tid;
    Wi[c * Ld + c] = __fdiv_rn(1.f, A[c * Ld + c]);
    for (int i = c + 1; i < D; ++i) {
      float sum = 0.f;
      for (int p = c; p < i; ++p) sum += A[i * Ld + p] * Wi[p * Ld + c];
      Wi[i * Ld + c] = __fdiv_rn(-sum, A[i * Ld + i]);
    }
  }
  __syncthreads();
  float bi = 0.f;
  if (tid < D) {
    for (int c = 0; c <= tid; ++c) bi += Wi[tid * Ld + c] * mu_s[c];
  }
  if (tid == 0) {
    float ld = 0.f;
    for (int d = 0; d < D; ++d) ld += logf(A[d * Ld + d]);
    cst_s = logf(__fdiv_rn(s0, tot_s)) - ld - 0.5f * (float)D * 1.8378770664093453f;
  }
  __syncthreads();
  const float c0 = cst_s;
  dead = dead || !finite_(c0);
  for (int e = tid; e < DPB * DPB; e += kBlock) {
    const int i = e / DPB, c = e - i * DPB;
    Wh[(int64_t)k * DPB * DPB + e] = (dead || i >= D || c > i) ? 0.f : Wi[i * Ld + c];
  }
  if (tid < DPB) b[(int64_t)k * DPB + tid] = (dead || tid >= D) ? 0.f : bi;
  if (tid == 0) cst[k] = dead ? -INFINITY : c0;
}

template <int DPB>
void launch_estep(const SArgs& sa, const TArgs& ta, bool acc, int sgrid, dim3 tgrid, hipStream_t s) {
  hipLaunchKernelGGL((gmmf_scores_kernel<DPB>), sgrid, kBlock, 0, s, sa);
  if (acc) hipLaunchKernelGGL((gmmf_stats_kernel<DPB>), tgrid, kBlock, 0, s, ta);
}

}  // namespace

void gmm_full_prepare(const float* s, int K, int D, float reg_covar, float* Wh, float* b, float* cst,
                      hipStream_t stream) {
  if (!gmm_full_shape_ok(K, D)) throw std::runtime_error("gmm_full_prepare: 1 <= K <= 128 and 1 <= D <= 64");
  if (!(reg_covar >= 0.f) || !std::isfinite(reg_covar))
    throw std::runtime_error("gmm_full_prepare: reg_covar must be finite and >= 0");
  switch (gmm_full_pad(D)) {
    case 16: hipLaunchKernelGGL(gmmf_prepare_kernel<16>, K, kBlock, 0, stream, s, K, D, reg_covar, Wh, b, cst); break;
    case 32: hipLaunchKernelGGL(gmmf_prepare_kernel<32>, K, kBlock, 0, stream, s, K, D, reg_covar, Wh, b, cst); break;
    case 48: hipLaunchKernelGGL(gmmf_prepare_kernel<48>, K, kBlock, 0, stream, s, K, D, reg_covar, Wh, b, cst); break;
    default: hipLaunchKernelGGL(gmmf_prepare_kernel<64>, K, kBlock, 0, stream, s, K, D, reg_covar, Wh, b, cst); break;
  }
  MINIPS_HIP_CHECK(hipGetLastError());
}

void gmm_full_estep(const float* X, int64_t ld, int64_t n, int D, int K, const float* shift, const float* Wh,
                    const float* b, const float* cst, float* S, double* ll, int32_t* assign, float* logp,
                    int32_t* bad, float* T, float* part, double* llpart, int blocks, hipStream_t stream) {
  if (!gmm_full_shape_ok(K, D)) throw std::runtime_error("gmm_full_estep: 1 <= K <= 128 and 1 <= D <= 64");
  if (n < 0 || n >= (1ll << 31) - kGmmFullChunk)
    throw std::runtime_error("gmm_full_estep: n must be below 2^31 - 2048");
  if (ld < D) throw std::runtime_error("gmm_full_estep: the points' leading dimension is below D");
  if (blocks < 0 || blocks > kGmmFullMaxBlocks) throw std::runtime_error("gmm_full_estep: 0 <= blocks <= 65535");
  const bool acc = S != nullptr;
  const int ntiles = (int)gmm_full_tiles(n), nchunks = (int)gmm_full_chunks(n, K, D);
  const int kp = gmm_full_pad(K), dp = gmm_full_pad(D);
  if (ntiles > 0) {
    if (llpart == nullptr || (acc && (part == nullptr || T == nullptr || logp == nullptr)))
      throw std::runtime_error("gmm_full_estep: workspace missing");
    const SArgs sa{X, ld, (int)n, D, K, kp, shift, Wh, b, cst, acc ? T : nullptr, llpart, assign, logp, bad, ntiles};
    const TArgs ta{X, ld, (int)n, D, K, kp, ld % 4 == 0 && aligned16(X), shift, T, logp, part,
                   gmm_full_chunk(n, K, D), nchunks};
    const int sgrid = blocks > 0 ? blocks : (ntiles < 1024 ? ntiles : 1024);
    const int group = dp >= 48 ? 8 : 16;
    const dim3 tgrid(blocks > 0 ? blocks : nchunks, (K + group - 1) / group);
    switch (dp) {
      case 16: launch_estep<16>(sa, ta, acc, sgrid, tgrid, stream); break;
      case 32: launch_estep<32>(sa, ta, acc, sgrid, tgrid, stream); break;
      case 48: launch_estep<48>(sa, ta, acc, sgrid, tgrid, stream); break;
      default: launch_estep<64>(sa, ta, acc, sgrid, tgrid, stream); break;
    }
  }
  const int m = K * (int)gmm_full_width(D);
  hipLaunchKernelGGL(gmmf_fold_kernel, (acc ? (m + kBlock - 1) / kBlock : 0) + 1, kBlock, 0, stream, part, llpart,
                     nchunks, ntiles, K, D, S, ll);
  MINIPS_HIP_CHECK(hipGetLastError());
}

}  // namespace minips_k
