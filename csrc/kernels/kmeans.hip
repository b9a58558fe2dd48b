// K-Means' fused step for gfx950: the nearest centre by a flash-shaped fp32 MFMA sweep (the points resident in
// registers, the centres streamed through two LDS buffers, a running argmin in place of a softmax), a stable integer
// group-by and the per-centre row sums on member_rows.h. The rule, the mapping and the launchers' contracts are stated
// in kmeans.h.
#include <stdexcept>
#include <string>

#include "common.h"
#include "kmeans.h"
#include "member_rows.h"

namespace minips_k {
namespace {

constexpr int kBlock = 256;
constexpr int kT = kKmTile;
static_assert(kKmTile == 64 && kKmStrip == 64 && kKmChunk == kKmTile, "four waves of 16 points, a partial a tile");
static_assert(kKmWaveMax >= 2 * kKmRowChunk && kKmGroup == kBlock, "member_rows.h's chunk rule; a point a thread");

// ------------------------------------------------------------------------------------------------ centre norms
__global__ __launch_bounds__(kBlock) void km_norms_kernel(const float* __restrict__ C, int K, int D,
                                                          float* __restrict__ cn) {
  const int lane = threadIdx.x & 63;
  const int k = (int)((blockIdx.x * (int64_t)kBlock + threadIdx.x) >> 6);
  if (k >= K) return;
  const float* c = C + (int64_t)k * D;
  float s = 0.f;
  for (int d = lane; d < D; d += 64) s += c[d] * c[d];
  s = warp_sum(s);
  if (lane == 0) cn[k] = s;
}

// ------------------------------------------------------------------------------------------------ nearest
template <int DPB>
struct Lds {
  static constexpr int kLd = DPB + 4;
  static constexpr int kTile = kT * kLd;
  static constexpr int kCn = 2 * kTile;
  static constexpr int kTotal = kCn + 2 * kT;
};

struct NearArgs {
  const float* X;
  int64_t ld, n;
  int D, K;
  bool xvec, cvec;
  const float* C;
  const float* cn;
  int32_t* assign;
  float* dist;
  double* ssepart;
  int32_t* badpart;
};

// What one thread holds of a tile of 64 rows between its global loads and its LDS stores.
template <int DPB>
struct Prefetch {
  float4 v[DPB / 16];
  float cn;
};

// rows [row0, row0 + 64) of the matrix M [nrows, ld], columns [0, D): a row beyond nrows and a column beyond D are 0.
// Nothing beyond column D of a row is read, whatever ld.
template <int DPB>
__device__ __forceinline__ void tile_fetch(const float* __restrict__ M, int64_t ld, int64_t row0, int64_t nrows,
                                           int D, bool vec, Prefetch<DPB>& pf) {
  constexpr int Q = DPB / 4;
  const int tid = threadIdx.x;
#pragma unroll
  for (int t = 0; t < DPB / 16; ++t) {
    const int idx = tid + kBlock * t, r = idx / Q, q = idx - r * Q;
    const int64_t row = row0 + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < nrows && 4 * q < D) {
      const float* p = M + row * ld + 4 * q;
      if (vec && 4 * q + 4 <= D) {
        v = *reinterpret_cast<const float4*>(p);
      } else {
        v.x = p[0];
        if (4 * q + 1 < D) v.y = p[1];
        if (4 * q + 2 < D) v.z = p[2];
        if (4 * q + 3 < D) v.w = p[3];
      }
    }
    pf.v[t] = v;
  }
}

// the strip's norms: +inf for a dead centre and beyond K
template <int DPB>
__device__ __forceinline__ void norms_fetch(const NearArgs& a, int k0, Prefetch<DPB>& pf) {
  pf.cn = INFINITY;
  const int k = k0 + (int)threadIdx.x;
  if (threadIdx.x < kKmStrip && k < a.K) {
    const float c = a.cn[k];
    pf.cn = c < INFINITY ? c : INFINITY;  // (a NaN compares false)
  }
}

template <int DPB>
__device__ __forceinline__ void tile_stash(float* sm, int slot, bool norms, const Prefetch<DPB>& pf) {
  using L = Lds<DPB>;
  constexpr int Q = DPB / 4;
  const int tid = threadIdx.x;
  float* tile = sm + slot * L::kTile;
#pragma unroll
  for (int t = 0; t < DPB / 16; ++t) {
    const int idx = tid + kBlock * t, r = idx / Q, q = idx - r * Q;
    *reinterpret_cast<float4*>(tile + r * L::kLd + 4 * q) = pf.v[t];
  }
  if (norms && tid < kKmStrip) sm[L::kCn + slot * kKmStrip + tid] = pf.cn;
}

__device__ __forceinline__ float f4(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

// JN 16-centre tiles of one strip against the wave's 16 points, then the running argmin. Lane (g, i): aq[m] holds
// point 16 w + i's columns 16 m + 4 g .. + 3, S points at the strip's row i, column 4 g; MFMA e of quad m reduces the
// columns 16 m + 4 g' + e (g' = 0 .. 3): the same order for every centre. acc[j][v] = point 16 w + 4 g + v against
// centre 16 j + i.
template <int DPB, int JN>
__device__ __forceinline__ void strip_scores(const float4 (&aq)[DPB / 16], const float* S, const float* cns, int k0,
                                             int i, float (&bv)[4], int (&bi)[4]) {
  constexpr int kLd = Lds<DPB>::kLd;
  v4f acc[JN];
#pragma unroll
  for (int j = 0; j < JN; ++j) acc[j] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int m = 0; m < DPB / 16; ++m) {
    float4 b[JN];
#pragma unroll
    for (int j = 0; j < JN; ++j) b[j] = *reinterpret_cast<const float4*>(S + 16 * j * kLd + 16 * m);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int j = 0; j < JN; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4(aq[m], e), f4(b[j], e), acc[j], 0, 0, 0);
  }
#pragma unroll
  for (int j = 0; j < JN; ++j) {
    const float cnv = cns[16 * j + i];
    const int k = k0 + 16 * j + i;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const float t = cnv < INFINITY ? cnv - 2.f * acc[j][v] : INFINITY;
      if (t < bv[v]) bv[v] = t, bi[v] = k;
    }
  }
}

template <int DPB>
__global__ __launch_bounds__(kBlock) void km_nearest_kernel(NearArgs a) {
  using L = Lds<DPB>;
  __shared__ __attribute__((aligned(16))) float sm[L::kTotal];
  __shared__ double red_sse[4];
  __shared__ int red_bad[4];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, i = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t ntiles = (a.n + kT - 1) / kT;
  const int ns = (a.K + kKmStrip - 1) / kKmStrip;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    Prefetch<DPB> pf;
    tile_fetch<DPB>(a.X, a.ld, tile * kT, a.n, a.D, a.xvec, pf);
    tile_stash<DPB>(sm, 1, false, pf);
    tile_fetch<DPB>(a.C, a.D, 0, a.K, a.D, a.cvec, pf);
    norms_fetch<DPB>(a, 0, pf);
    tile_stash<DPB>(sm, 0, true, pf);
    __syncthreads();
    float4 aq[DPB / 16];
    float xx = 0.f;
    {
      const float* R = sm + L::kTile + (16 * w + i) * L::kLd + 4 * g;
#pragma unroll
      for (int m = 0; m < DPB / 16; ++m) {
        aq[m] = *reinterpret_cast<const float4*>(R + 16 * m);
        xx += aq[m].x * aq[m].x;
        xx += aq[m].y * aq[m].y;
        xx += aq[m].z * aq[m].z;
        xx += aq[m].w * aq[m].w;
      }
    }
    xx += __shfl_xor(xx, 16, 64);
    xx += __shfl_xor(xx, 32, 64);  // point 16 w + i's sum of squares, in its four lanes
    __syncthreads();               // the point tile is in registers: buffer 1 is free for strip 1
    float bv[4];
    int bi[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) bv[v] = INFINITY, bi[v] = -1;
    for (int s = 0; s < ns; ++s) {
      const int buf = s & 1, k0 = s * kKmStrip;
      const bool more = s + 1 < ns;
      if (more) {  // in flight during the MFMAs below
        tile_fetch<DPB>(a.C, a.D, k0 + kKmStrip, a.K, a.D, a.cvec, pf);
        norms_fetch<DPB>(a, k0 + kKmStrip, pf);
      }
      const float* S = sm + buf * L::kTile + i * L::kLd + 4 * g;
      const float* cns = sm + L::kCn + buf * kKmStrip;
      const int left = a.K - k0;  // block-uniform
      if (left > 48) strip_scores<DPB, 4>(aq, S, cns, k0, i, bv, bi);
      else if (left > 32) strip_scores<DPB, 3>(aq, S, cns, k0, i, bv, bi);
      else if (left > 16) strip_scores<DPB, 2>(aq, S, cns, k0, i, bv, bi);
      else strip_scores<DPB, 1>(aq, S, cns, k0, i, bv, bi);
      if (more) tile_stash<DPB>(sm, buf ^ 1, true, pf);
      __syncthreads();
    }
    // the 16 lanes of group g hold point 16 w + 4 g + v's candidates: lowest value, then lowest index
#pragma unroll
    for (int v = 0; v < 4; ++v) {
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const float ov = __shfl_xor(bv[v], o, 64);
        const int oi = __shfl_xor(bi[v], o, 64);
        if (ov < bv[v] || (ov == bv[v] && oi < bi[v])) bv[v] = ov, bi[v] = oi;
      }
    }
    // point 16 w + i's winner, to the four lanes that hold its columns
    const int src = 16 * (i >> 2);
    const int w0 = __shfl(bi[0], src, 64), w1 = __shfl(bi[1], src, 64);
    const int w2 = __shfl(bi[2], src, 64), w3 = __shfl(bi[3], src, 64);
    const int win = (i & 3) == 0 ? w0 : (i & 3) == 1 ? w1 : (i & 3) == 2 ? w2 : w3;
    float dd = 0.f;
    if (win >= 0 && win < a.K) {
      const float* c = a.C + (int64_t)win * a.D + 4 * g;
#pragma unroll
      for (int m = 0; m < DPB / 16; ++m) {
        const int d = 16 * m + 4 * g;
        float4 cv = make_float4(0.f, 0.f, 0.f, 0.f);  // (the point's pad columns are 0 too)
        if (d >= a.D) {
        } else if (a.cvec) {  // D % 4 == 0: the quad lies inside the row
          cv = *reinterpret_cast<const float4*>(c + 16 * m);
        } else {
          cv.x = c[16 * m];
          if (d + 1 < a.D) cv.y = c[16 * m + 1];
          if (d + 2 < a.D) cv.z = c[16 * m + 2];
          if (d + 3 < a.D) cv.w = c[16 * m + 3];
        }
        const float ex = aq[m].x - cv.x, ey = aq[m].y - cv.y, ez = aq[m].z - cv.z, ew = aq[m].w - cv.w;
        dd += ex * ex;
        dd += ey * ey;
        dd += ez * ez;
        dd += ew * ew;
      }
    }
    dd += __shfl_xor(dd, 16, 64);
    dd += __shfl_xor(dd, 32, 64);
    const int64_t p = tile * kT + 16 * w + i;
    const bool mine = g == 0 && p < a.n;
    const bool isbad = !(xx < INFINITY) || win < 0;
    if (mine) {
      a.assign[p] = isbad ? -1 : win;
      a.dist[p] = isbad ? __builtin_nanf("") : dd;
    }
    double sd = mine && !isbad ? (double)dd : 0.0;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) sd += __shfl_xor(sd, o, 64);
    const int nb = __popcll(__ballot(mine && isbad));
    if (lane == 0) red_sse[w] = sd, red_bad[w] = nb;
    __syncthreads();
    if (tid == 0) {
      a.ssepart[tile] = ((red_sse[0] + red_sse[1]) + red_sse[2]) + red_sse[3];
      a.badpart[tile] = red_bad[0] + red_bad[1] + red_bad[2] + red_bad[3];
    }
    // the next tile writes red_* only behind several more barriers
  }
}

// one workgroup: sse = the partials in chunk order (thread-strided ascending, then a fixed tree); bad += the counts
__global__ __launch_bounds__(kBlock) void km_fold_kernel(const double* __restrict__ ssepart,
                                                         const int32_t* __restrict__ badpart, int64_t nt,
                                                         double* __restrict__ sse, int32_t* __restrict__ bad) {
  __shared__ double rs[kBlock];
  __shared__ int rb[kBlock];
  const int tid = threadIdx.x;
  double s = 0.0;
  int b = 0;
  for (int64_t t = tid; t < nt; t += kBlock) s += ssepart[t], b += badpart[t];
  rs[tid] = s, rb[tid] = b;
  __syncthreads();
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if (tid < o) rs[tid] += rs[tid + o], rb[tid] += rb[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    sse[0] = rs[0];
    if (bad != nullptr && rb[0] != 0) bad[0] += rb[0];
  }
}

template <int DPB>
void launch_nearest(const NearArgs& a, int grid, hipStream_t s) {
  hipLaunchKernelGGL((km_nearest_kernel<DPB>), grid, kBlock, 0, s, a);
}

// ------------------------------------------------------------------------------------------------ group-by
// bin of a point: its centre, or K for a point without one
__device__ __forceinline__ int km_bin(int a, int K) { return (unsigned)a < (unsigned)K ? a : K; }

__global__ __launch_bounds__(kBlock) void km_hist_kernel(const int32_t* __restrict__ assign, int64_t n, int K,
                                                         int64_t gp, int64_t ngroups, int32_t* __restrict__ hist) {
  __shared__ int h[kKmMaxK + 1];
  const int KB = K + 1, tid = threadIdx.x;
  for (int64_t c = blockIdx.x; c < ngroups; c += gridDim.x) {
    for (int k = tid; k < KB; k += kBlock) h[k] = 0;
    __syncthreads();
    const int64_t i1 = (c + 1) * gp < n ? (c + 1) * gp : n;
    for (int64_t i = c * gp + tid; i < i1; i += kBlock) atomicAdd(&h[km_bin(assign[i], K)], 1);
    __syncthreads();
    for (int k = tid; k < KB; k += kBlock) hist[c * KB + k] = h[k];
    __syncthreads();
  }
}

// a thread per bin: hist[c][k] becomes the count of the earlier blocks, tot[k] the count of all
__global__ __launch_bounds__(kBlock) void km_colscan_kernel(int32_t* __restrict__ hist, int64_t ngroups, int KB,
                                                            int32_t* __restrict__ tot) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= KB) return;
  int run = 0;
#pragma unroll 8
  for (int64_t c = 0; c < ngroups; ++c) {
    const int v = hist[c * KB + k];
    hist[c * KB + k] = run;
    run += v;
  }
  tot[k] = run;
}

// one workgroup: start [K + 2] = the exclusive scan of tot [K + 1]; counts [K]
__global__ __launch_bounds__(kBlock) void km_start_kernel(const int32_t* __restrict__ tot, int K,
                                                          int32_t* __restrict__ start, int32_t* __restrict__ counts) {
  __shared__ int part[kBlock];
  const int KB = K + 1, tid = threadIdx.x, per = (KB + kBlock - 1) / kBlock;
  const int k0 = tid * per < KB ? tid * per : KB, k1 = k0 + per < KB ? k0 + per : KB;
  int s = 0;
  for (int k = k0; k < k1; ++k) s += tot[k];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int t = 0; t < kBlock; ++t) {
      const int v = part[t];
      part[t] = run;
      run += v;
    }
  }
  __syncthreads();
  int run = part[tid];
  for (int k = k0; k < k1; ++k) {
    start[k] = run;
    run += tot[k];
    if (k < K) counts[k] = tot[k];
  }
  if (k0 < k1 && k1 == KB) start[KB] = run;
}

// members / memrow sorted by (bin, point index): a point's slot is its bin's start, plus the bin's count in the
// earlier blocks, plus the earlier rounds of this block, plus its rank among the round's earlier points of the bin
__global__ __launch_bounds__(kBlock) void km_place_kernel(const int32_t* __restrict__ assign, int64_t n, int K,
                                                          int64_t gp, int64_t ngroups,
                                                          const int32_t* __restrict__ hist,
                                                          const int32_t* __restrict__ start,
                                                          int32_t* __restrict__ members, int32_t* __restrict__ memrow) {
  __shared__ int run[kKmMaxK + 1];
  __shared__ int keys[kBlock];
  const int KB = K + 1, tid = threadIdx.x;
  for (int64_t c = blockIdx.x; c < ngroups; c += gridDim.x) {
    for (int k = tid; k < KB; k += kBlock) run[k] = start[k] + hist[c * KB + k];
    const int64_t i0 = c * gp, i1 = i0 + gp < n ? i0 + gp : n;
    for (int64_t b = i0; b < i1; b += kBlock) {
      const int64_t i = b + tid;
      const int key = i < i1 ? km_bin(assign[i], K) : -1;
      keys[tid] = key;
      __syncthreads();
      int64_t pos = -1;
      if (key >= 0) {
        int rank = 0;
        for (int u = 0; u < tid; ++u) rank += keys[u] == key ? 1 : 0;
        pos = (int64_t)run[key] + rank;
      }
      __syncthreads();  // every read of run and keys is done
      if (pos >= 0 && pos < n) {
        members[pos] = (int)i;
        memrow[pos] = key;
        atomicAdd(&run[key], 1);
      }
      __syncthreads();
    }
  }
}

// ------------------------------------------------------------------------------------------------ row sums
struct SumArgs {
  const float* X;
  int64_t ld;
  int n, D, K, lg;  // lane groups of 1 << lg lanes
  bool vec, svec;
  const int32_t* members;
  const int32_t* memrow;
  const int32_t* start;
  float* sums;
  float* part;
};

__device__ __forceinline__ void add4(float4& s, const float4& v) {
  s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
}

// lane l's column e: a float4 of consecutive columns, or four columns a lane group apart
__device__ __forceinline__ int km_col(const SumArgs& a, int l, int e) { return a.vec ? 4 * l + e : l + (e << a.lg); }

__device__ __forceinline__ float4 km_row(const SumArgs& a, int64_t row, int l) {
  const float* p = a.X + row * a.ld;
  if (a.vec && 4 * l + 4 <= a.D) return *reinterpret_cast<const float4*>(p + 4 * l);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  const int c0 = km_col(a, l, 0), c1 = km_col(a, l, 1), c2 = km_col(a, l, 2), c3 = km_col(a, l, 3);
  if (c0 < a.D) v.x = p[c0];
  if (c1 < a.D) v.y = p[c1];
  if (c2 < a.D) v.z = p[c2];
  if (c3 < a.D) v.w = p[c3];
  return v;
}

// the members [m0, m1) with the given stride, in that order
__device__ __forceinline__ float4 km_walk(const SumArgs& a, int m0, int m1, int stride, int l) {
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
  for (int m = m0; m < m1; m += stride) {
    const int j = a.members[m];
    if ((unsigned)j < (unsigned)a.n) add4(s, km_row(a, j, l));
  }
  return s;
}

__device__ __forceinline__ void km_store(const SumArgs& a, float* dst, const float4& s, int l) {
  if (a.svec && 4 * l + 4 <= a.D) {
    *reinterpret_cast<float4*>(dst + 4 * l) = s;
    return;
  }
  const int c0 = km_col(a, l, 0), c1 = km_col(a, l, 1), c2 = km_col(a, l, 2), c3 = km_col(a, l, 3);
  if (c0 < a.D) dst[c0] = s.x;
  if (c1 < a.D) dst[c1] = s.y;
  if (c2 < a.D) dst[c2] = s.z;
  if (c3 < a.D) dst[c3] = s.w;
}

// Centres of up to kKmWaveMax members (the empty ones too): 64 >> lg consecutive centres per wave and iteration
__global__ __launch_bounds__(kBlock) void km_sums_kernel(SumArgs a) {
  const int G = 64 >> a.lg, lane = threadIdx.x & 63, g = lane >> a.lg, l = lane & ((1 << a.lg) - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t ntiles = ((int64_t)a.K + G - 1) / G;
  for (int64_t tile = wave; tile < ntiles; tile += nwaves) {
    const int64_t k = tile * G + g;
    if (k >= a.K) continue;
    const int lo = a.start[k], hi = a.start[k + 1];
    if (lo < 0 || hi > a.n || hi - lo > kKmWaveMax) continue;
    km_store(a, a.sums + k * a.D, km_walk(a, lo, hi, 1, l), l);
  }
}

// block p sums the members of chunk p that belong to a heavy centre into part[(2 p + s) * D ...] (member_rows.h):
// 256 >> lg lane groups take the members in turn and are folded through LDS in group order
__global__ __launch_bounds__(kBlock) void km_sums_heavy_kernel(SumArgs a) {
  __shared__ float4 red[kBlock];
  const int L = 1 << a.lg, NG = kBlock >> a.lg;
  const int gi = threadIdx.x >> a.lg, l = threadIdx.x & (L - 1);
  const int64_t p = blockIdx.x;
  const int64_t c_lo = p * kKmRowChunk, c_hi = (c_lo + kKmRowChunk) < a.n ? (c_lo + kKmRowChunk) : a.n;
  for (int s = 0; s < 2; ++s) {
    int r, lo, hi;
    if (!member_heavy_row<kKmRowChunk, kKmWaveMax>(a.memrow, a.n, a.K, p, s, r, lo, hi)) continue;  // block-uniform
    const int m0 = lo > c_lo ? lo : (int)c_lo, m1 = hi < c_hi ? hi : (int)c_hi;
    __syncthreads();  // (the previous candidate's reads of red)
    red[threadIdx.x] = km_walk(a, m0 + gi, m1, NG, l);
    __syncthreads();
    if (threadIdx.x < L) {
      float4 t = red[l];
      for (int q = 1; q < NG; ++q) add4(t, red[q * L + l]);
      km_store(a, a.part + (2 * p + s) * a.D, t, l);
    }
  }
}

void check(const char* op, int64_t n, int D, int K, int64_t ld, int blocks) {
  if (!km_shape_ok(K, D)) throw std::runtime_error(std::string(op) + ": 1 <= K <= 4096 and 1 <= D <= 256");
  if (n < 0 || n >= (1ll << 31) - kKmGroup) throw std::runtime_error(std::string(op) + ": n must be below 2^31 - 256");
  if (ld < D) throw std::runtime_error(std::string(op) + ": ld < D");
  if (blocks < 0 || blocks > kKmMaxBlocks) throw std::runtime_error(std::string(op) + ": blocks outside [0, 65535]");
}

}  // namespace

void km_nearest(const float* X, int64_t ld, int64_t n, int D, const float* C, int K, int32_t* assign, float* dist,
                double* sse, int32_t* bad, float* cn, double* ssepart, int32_t* badpart, int blocks, hipStream_t s) {
  check("km_nearest", n, D, K, ld, blocks);
  const int64_t nt = km_chunks(n);
  if (nt > 0) {
    hipLaunchKernelGGL(km_norms_kernel, (K + 3) / 4, kBlock, 0, s, C, K, D, cn);
    const NearArgs a{X, ld, n, D, K, ld % 4 == 0 && aligned16(X), D % 4 == 0 && aligned16(C), C, cn, assign, dist,
                     ssepart, badpart};
    const int grid = blocks > 0 ? blocks : (int)(nt < 4096 ? nt : 4096);
    switch (km_bucket(D)) {
      case 16: launch_nearest<16>(a, grid, s); break;
      case 32: launch_nearest<32>(a, grid, s); break;
      case 64: launch_nearest<64>(a, grid, s); break;
      case 96: launch_nearest<96>(a, grid, s); break;
      case 128: launch_nearest<128>(a, grid, s); break;
      case 192: launch_nearest<192>(a, grid, s); break;
      default: launch_nearest<256>(a, grid, s); break;
    }
  }
  hipLaunchKernelGGL(km_fold_kernel, 1, kBlock, 0, s, ssepart, badpart, nt, sse, bad);
  MINIPS_HIP_CHECK(hipGetLastError());
}

int64_t km_sums_ws_ints(int64_t n, int K) { return km_groups(n) * (K + 1) + (K + 1) + (K + 2) + 2 * n; }

int64_t km_sums_part_floats(int64_t n, int D) { return member_part_elems(n, D, kKmRowChunk, kKmWaveMax); }

void km_sums(const float* X, int64_t ld, int64_t n, int D, const int32_t* assign, int K, float* sums, int32_t* counts,
             int32_t* ws, float* part, int blocks, hipStream_t s) {
  check("km_sums", n, D, K, ld, blocks);
  if (ws == nullptr) throw std::runtime_error("km_sums: ws workspace missing");
  if (n > kKmWaveMax && part == nullptr) throw std::runtime_error("km_sums: part workspace missing");
  const int KB = K + 1;
  const int64_t gp = km_group_points(n), ng = km_groups(n);
  int32_t* hist = ws;
  int32_t* tot = hist + ng * KB;
  int32_t* start = tot + KB;
  int32_t* members = start + KB + 1;
  int32_t* memrow = members + n;
  const int ggrid = blocks > 0 ? blocks : (int)ng;
  if (n > 0) hipLaunchKernelGGL(km_hist_kernel, ggrid, kBlock, 0, s, assign, n, K, gp, ng, hist);
  hipLaunchKernelGGL(km_colscan_kernel, (KB + kBlock - 1) / kBlock, kBlock, 0, s, hist, ng, KB, tot);
  hipLaunchKernelGGL(km_start_kernel, 1, kBlock, 0, s, tot, K, start, counts);
  if (n > 0)
    hipLaunchKernelGGL(km_place_kernel, ggrid, kBlock, 0, s, assign, n, K, gp, ng, hist, start, members, memrow);
  int lg = 0;
  while ((4 << lg) < D) ++lg;
  const bool vec = ld % 4 == 0 && aligned16(X);
  const SumArgs a{X, ld, (int)n, D, K, lg, vec, vec && D % 4 == 0 && aligned16(sums) && aligned16(part), members,
                  memrow, start, sums, part};
  const int grid = blocks > 0 ? blocks : grid_for((int64_t)K << lg, kBlock, 8192);
  hipLaunchKernelGGL(km_sums_kernel, grid, kBlock, 0, s, a);
  if (n > kKmWaveMax) {
    const int chunks = member_chunks(n, kKmRowChunk);
    hipLaunchKernelGGL(km_sums_heavy_kernel, chunks, kBlock, 0, s, a);
    hipLaunchKernelGGL((member_heavy_fold_kernel<float, float, kKmRowChunk, kKmWaveMax>), chunks, kBlock, 0, s, memrow,
                       (int)n, (int64_t)K, D, part, sums);
  }
  MINIPS_HIP_CHECK(hipGetLastError());
}

}  // namespace minips_k
