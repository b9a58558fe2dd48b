// Histogram GBDT kernels for gfx950 (the rule and the lane mapping: gbdt.h). Integer accumulation only -- LDS
// integer atomics per workgroup, 64-bit global integer atomics with zero entries skipped, as evalmetrics.hip --
// so every result is a function of the inputs alone.
#include <algorithm>
#include <stdexcept>
#include <string>

#include "common.h"
#include "gbdt.h"

namespace minips_k {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kS = 1 << kGbdtScaleBits;

typedef unsigned long long u64;
typedef long long i64;

// ---------------------------------------------------------------------------------------------- bin
__device__ __forceinline__ unsigned bin_of(float x, const float* __restrict__ c, int ncut) {
  int lo = 0, hi = ncut;  // #{j : x > c[j]} over ascending c: the first j with !(x > c[j])
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (x > c[mid]) lo = mid + 1;
    else hi = mid;
  }
  return (unsigned)lo;
}

// WORD: a thread takes four features and stores one word (bins and ldb 4-byte friendly); else a byte per thread
template <bool WORD>
__global__ __launch_bounds__(kBlock) void gbdt_bin_kernel(const float* __restrict__ X, int64_t ldx,
                                                          const float* __restrict__ cuts, int64_t N, int F, int NB,
                                                          uint8_t* __restrict__ bins, int64_t ldb) {
  const int ncut = NB - 1;
  const int per = WORD ? (F + 3) >> 2 : F;
  const int64_t total = N * per, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += stride) {
    const int64_t i = idx / per;
    const int c = (int)(idx - i * per);
    if (WORD) {
      const int f = c * 4;
      unsigned b[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (f + j < F) b[j] = bin_of(X[i * ldx + f + j], cuts + (int64_t)(f + j) * ncut, ncut);
      if (f + 4 <= F) {
        *reinterpret_cast<uint32_t*>(bins + i * ldb + f) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
      } else {
        for (int j = 0; f + j < F; ++j) bins[i * ldb + f + j] = (uint8_t)b[j];
      }
    } else {
      bins[i * ldb + c] = (uint8_t)bin_of(X[i * ldx + c], cuts + (int64_t)c * ncut, ncut);
    }
  }
}

// ---------------------------------------------------------------------------------------------- grad
__global__ __launch_bounds__(kBlock) void gbdt_grad_kernel(const float* __restrict__ z,
                                                           const float* __restrict__ labels, int64_t N,
                                                           int32_t* __restrict__ gh, int64_t* loss_acc) {
  __shared__ i64 s_loss[kWaves];
  i64 loss = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N; i += stride) {
    const float zi = z[i];
    const float y = labels[i] > 0.5f ? 1.f : 0.f;
    const float zc = fminf(fmaxf(zi, -30.f), 30.f);
    const float p = 1.f / (1.f + expf(-zc));
    const float h = fmaxf(p * (1.f - p), 1.f / (float)kS);
    gh[2 * i] = (int32_t)llrintf((p - y) * (float)kS);
    gh[2 * i + 1] = (int32_t)llrintf(h * (float)kS);
    const float zl = fminf(fmaxf(zi, -64.f), 64.f);
    const float l = fmaxf(zl, 0.f) - zl * y + log1pf(expf(-fabsf(zl)));
    loss += llrintf(l * 16777216.f);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) loss += __shfl_xor(loss, o, 64);
  if ((threadIdx.x & 63) == 0) s_loss[threadIdx.x >> 6] = loss;
  __syncthreads();
  if (threadIdx.x == 0) {
    i64 l = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) l += s_loss[w];
    if (l) atomicAdd(reinterpret_cast<u64*>(loss_acc), (u64)l);
  }
}

// ---------------------------------------------------------------------------------------------- hist
__device__ __forceinline__ void hist_global_add(int64_t* hist, int64_t e, int qg, int qh) {
  u64* h = reinterpret_cast<u64*>(hist) + e;
  if (qg) atomicAdd(h, (u64)(i64)qg);
  if (qh) atomicAdd(h + 1, (u64)(i64)qh);
  atomicAdd(h + 2, (u64)1);
}

// acc int32 [nodes][tf][NB][3] in LDS; a block owns features [blockIdx.y tf, + tf) and takes the sample chunks
// blockIdx.x, + gridDim.x, ...; flushed and cleared after every chunk (the bound of gbdt.h)
template <bool VEC>
__global__ __launch_bounds__(kBlock) void gbdt_hist_lds_kernel(const uint8_t* __restrict__ bins, int64_t ldb,
                                                               const int32_t* __restrict__ node,
                                                               const int32_t* __restrict__ gh, int64_t N, int F,
                                                               int NB, int nodes, int tf, int64_t* hist) {
  extern __shared__ int acc[];
  const int f0 = blockIdx.y * tf, f1 = min(F, f0 + tf), nf = f1 - f0;
  const int per = NB * 3, entries = nodes * tf * per;
  for (int e = threadIdx.x; e < entries; e += kBlock) acc[e] = 0;
  __syncthreads();
  const int64_t nchunks = (N + kGbdtFlushRows - 1) / kGbdtFlushRows;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t lo = c * kGbdtFlushRows, hi = min(N, lo + (int64_t)kGbdtFlushRows);
    for (int64_t i = lo + threadIdx.x; i < hi; i += kBlock) {
      const int nd = node[i];
      if ((unsigned)nd >= (unsigned)nodes) continue;
      const int qg = gh[2 * i], qh = gh[2 * i + 1];
      // outside the rule's range (a caller's own gh): exact through the global atomics
      const bool big = qg > kS || qg < -kS || qh > kS || qh < -kS;
      const uint8_t* row = bins + i * ldb;
      auto add = [&](int f, int b) {
        if (b >= NB) return;
        if (big) {
          hist_global_add(hist, (((int64_t)nd * F + f) * NB + b) * 3, qg, qh);
        } else {
          int* a = acc + ((nd * tf + (f - f0)) * NB + b) * 3;
          if (qg) atomicAdd(a, qg);
          if (qh) atomicAdd(a + 1, qh);
          atomicAdd(a + 2, 1);
        }
      };
      if (VEC) {
        for (int g = f0 >> 4; g <= (f1 - 1) >> 4; ++g) {
          const uint4 v = *reinterpret_cast<const uint4*>(row + g * 16);
          const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const int f = g * 16 + j;
            if (f >= f0 && f < f1) add(f, (int)((w[j >> 2] >> ((j & 3) * 8)) & 0xffu));
          }
        }
      } else {
        for (int f = f0; f < f1; ++f) add(f, (int)row[f]);
      }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < entries; e += kBlock) {
      const int v = acc[e];
      if (v) {
        acc[e] = 0;
        const int q = e / per, rem = e - q * per;
        const int nd = q / tf, t = q - nd * tf;
        if (t < nf)
          atomicAdd(reinterpret_cast<u64*>(hist) + ((int64_t)nd * F + f0 + t) * per + rem, (u64)(i64)v);
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void gbdt_hist_global_kernel(const uint8_t* __restrict__ bins, int64_t ldb,
                                                                  const int32_t* __restrict__ node,
                                                                  const int32_t* __restrict__ gh, int64_t N, int F,
                                                                  int NB, int nodes, int64_t* hist) {
  const int64_t total = N * F, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += stride) {
    const int64_t i = idx / F;
    const int f = (int)(idx - i * F);
    const int nd = node[i];
    if ((unsigned)nd >= (unsigned)nodes) continue;
    const int b = bins[i * ldb + f];
    if (b >= NB) continue;
    hist_global_add(hist, (((int64_t)nd * F + f) * NB + b) * 3, gh[2 * i], gh[2 * i + 1]);
  }
}

// ---------------------------------------------------------------------------------------------- split
struct Best {
  double gain;
  int f, t;  // f < 0: no valid candidate
};

// a before b in (gain descending, f ascending, t ascending); "none" after everything
__device__ __forceinline__ bool before(const Best& a, const Best& b) {
  if (a.f < 0) return false;
  if (b.f < 0) return true;
  if (a.gain != b.gain) return a.gain > b.gain;
  if (a.f != b.f) return a.f < b.f;
  return a.t < b.t;
}

__device__ __forceinline__ Best wave_best(Best m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Best x;
    x.gain = __shfl_xor(m.gain, o, 64);
    x.f = __shfl_xor(m.f, o, 64);
    x.t = __shfl_xor(m.t, o, 64);
    if (before(x, m)) m = x;
  }
  return m;
}

__device__ __forceinline__ double split_gain(i64 gl, i64 hl, i64 g, i64 h, double lambda) {
#pragma clang fp contract(off)
  const double sc = 1.0 / (double)kS;
  const double GL = (double)gl * sc, HL = (double)hl * sc, G = (double)g * sc, H = (double)h * sc;
  const double GR = (double)(g - gl) * sc, HR = (double)(h - hl) * sc;
  const double a = GL * GL / (HL + lambda);
  const double b = GR * GR / (HR + lambda);
  const double c = G * G / (H + lambda);
  return (a + b) - c;
}

// one wave per (node, feature): the best threshold of the feature into wgain / wthr (wthr -1: none)
__global__ __launch_bounds__(kBlock) void gbdt_split_feature_kernel(const int64_t* __restrict__ hist, int64_t pairs,
                                                                    int F, int NB, double lambda, int64_t min_child,
                                                                    double min_gain, double* __restrict__ wgain,
                                                                    int32_t* __restrict__ wthr) {
  const int64_t w = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  if (w >= pairs) return;  // (uniform per wave)
  const int lane = threadIdx.x & 63;
  const int R = (NB + 63) >> 6, b0 = lane * R;
  const int64_t* h = hist + w * NB * 3;
  i64 vg[4], vh[4], vc[4], sg = 0, sh = 0, sc = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const bool in = r < R && b0 + r < NB;
    vg[r] = in ? h[(b0 + r) * 3] : 0;
    vh[r] = in ? h[(b0 + r) * 3 + 1] : 0;
    vc[r] = in ? h[(b0 + r) * 3 + 2] : 0;
    sg += vg[r];
    sh += vh[r];
    sc += vc[r];
  }
  i64 pg = sg, ph = sh, pc = sc;  // inclusive prefix over the lanes
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const i64 xg = __shfl_up(pg, o, 64), xh = __shfl_up(ph, o, 64), xc = __shfl_up(pc, o, 64);
    if (lane >= o) {
      pg += xg;
      ph += xh;
      pc += xc;
    }
  }
  const i64 G = __shfl(pg, 63, 64), H = __shfl(ph, 63, 64), C = __shfl(pc, 63, 64);
  pg -= sg;
  ph -= sh;
  pc -= sc;
  Best m{0.0, -1, 0};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int t = b0 + r;
    if (r < R && t <= NB - 2) {
      pg += vg[r];
      ph += vh[r];
      pc += vc[r];
      if (pc >= min_child && C - pc >= min_child) {
        const double gain = split_gain(pg, ph, G, H, lambda);
        if (gain > min_gain && (m.f < 0 || gain > m.gain)) m = Best{gain, 0, t};
      }
    }
  }
  m = wave_best(m);
  if (lane == 0) {
    wgain[w] = m.f < 0 ? 0.0 : m.gain;
    wthr[w] = m.f < 0 ? -1 : m.t;
  }
}

// one wave per node: folds the features, writes feat / thr / gain / child
__global__ __launch_bounds__(kBlock) void gbdt_split_node_kernel(const int64_t* __restrict__ hist, int nodes, int F,
                                                                 int NB, const double* __restrict__ wgain,
                                                                 const int32_t* __restrict__ wthr,
                                                                 int32_t* __restrict__ feat, int32_t* __restrict__ thr,
                                                                 double* __restrict__ gain,
                                                                 int64_t* __restrict__ child) {
  const int n = (int)((blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6);
  if (n >= nodes) return;
  const int lane = threadIdx.x & 63;
  Best m{0.0, -1, 0};
  for (int f = lane; f < F; f += 64) {
    const int t = wthr[(int64_t)n * F + f];
    if (t >= 0 && t <= NB - 2) {
      const Best x{wgain[(int64_t)n * F + f], f, t};
      if (before(x, m)) m = x;
    }
  }
  m = wave_best(m);
  const int fc = m.f < 0 ? 0 : m.f, tl = m.f < 0 ? NB - 1 : m.t;
  const int64_t* h = hist + ((int64_t)n * F + fc) * NB * 3;
  i64 s[6] = {0, 0, 0, 0, 0, 0};  // left | total
  for (int b = lane; b < NB; b += 64) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const i64 v = h[b * 3 + c];
      s[3 + c] += v;
      if (b <= tl) s[c] += v;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int c = 0; c < 6; ++c) s[c] += __shfl_xor(s[c], o, 64);
  }
  if (lane == 0) {
    feat[n] = m.f;
    thr[n] = m.f < 0 ? 0 : m.t;
    gain[n] = m.f < 0 ? 0.0 : m.gain;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      child[n * 6 + c] = s[c];
      child[n * 6 + 3 + c] = s[3 + c] - s[c];
    }
  }
}

__global__ __launch_bounds__(kBlock) void gbdt_leaf_kernel(const int64_t* __restrict__ child, int n2, double lambda,
                                                           double lr, float* __restrict__ leaf) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n2) return;
  const double sc = 1.0 / (double)kS;
  const double G = (double)child[i * 3] * sc, H = (double)child[i * 3 + 1] * sc;
  const double num = -G;
  const double den = H + lambda;
  const double q = num / den;
  const double v = q * lr;
  leaf[i] = child[i * 3 + 2] == 0 ? 0.f : (float)v;
}

// ---------------------------------------------------------------------------------------------- advance / predict
__global__ __launch_bounds__(kBlock) void gbdt_advance_kernel(const uint8_t* __restrict__ bins, int64_t ldb,
                                                              int32_t* __restrict__ node,
                                                              const int32_t* __restrict__ feat,
                                                              const int32_t* __restrict__ thr, int64_t N, int F,
                                                              int nodes, const float* __restrict__ leaf,
                                                              float* __restrict__ z) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N; i += stride) {
    const int nd = node[i];
    int out = -1;
    if ((unsigned)nd < (unsigned)nodes) {
      const int f = feat[nd];
      if (f < 0) out = 2 * nd;
      else if (f < F) out = 2 * nd + ((int)bins[i * ldb + f] > thr[nd] ? 1 : 0);
    }
    node[i] = out;
    if (leaf && out >= 0) z[i] += leaf[out];
  }
}

__global__ __launch_bounds__(kBlock) void gbdt_predict_kernel(const uint8_t* __restrict__ bins, int64_t ldb,
                                                              int64_t N, int F, const int32_t* __restrict__ feat,
                                                              const uint8_t* __restrict__ thr,
                                                              const float* __restrict__ leaf, int T, int depth,
                                                              float base, float* __restrict__ z,
                                                              int32_t* __restrict__ leaf_index) {
  const int nn = (1 << depth) - 1, nl = 1 << depth;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N; i += stride) {
    const uint8_t* row = bins + i * ldb;
    float s = base;
    for (int t = 0; t < T; ++t) {
      const int32_t* ft = feat + (int64_t)t * nn;
      const uint8_t* tt = thr + (int64_t)t * nn;
      int n = 0;
      for (int d = 0; d < depth; ++d) {
        const int at = (1 << d) - 1 + n;
        const int f = ft[at];
        const bool right = f >= 0 && f < F && row[f] > tt[at];
        n = 2 * n + (right ? 1 : 0);
      }
      s += leaf[(int64_t)t * nl + n];
      if (leaf_index) leaf_index[i * T + t] = n;
    }
    z[i] = s;
  }
}

void bad(const char* op, const std::string& what) { throw std::runtime_error(std::string(op) + ": " + what); }

void check_shape(const char* op, int F, int NB, int nodes, int blocks) {
  if (F < 1 || F > kGbdtMaxF) bad(op, "F is " + std::to_string(F) + ", expected 1 <= F <= 4096");
  if (NB < 2 || NB > kGbdtMaxBins) bad(op, "NB is " + std::to_string(NB) + ", expected 2 <= NB <= 256");
  if (nodes < 1 || nodes > kGbdtMaxNodes || (nodes & (nodes - 1)))
    bad(op, "nodes is " + std::to_string(nodes) + ", expected a power of two in [1, 128]");
  if (blocks < 0 || blocks > kGbdtMaxBlocks)
    bad(op, "blocks is " + std::to_string(blocks) + ", expected 0 <= blocks <= 65535");
}

inline bool friendly(const void* p, int64_t ld, int a) {
  return reinterpret_cast<uintptr_t>(p) % a == 0 && ld % a == 0;
}

}  // namespace

void gbdt_bin(const float* X, int64_t ldx, const float* cuts, int64_t N, int F, int NB, uint8_t* bins, int64_t ldb,
              int blocks, hipStream_t s) {
  check_shape("gbdt_bin", F, NB, 1, blocks);
  if (ldx < F || ldb < F) bad("gbdt_bin", "ldx / ldb below F");
  if (N <= 0) return;
  if (friendly(bins, ldb, 4)) {
    const int grid = blocks > 0 ? blocks : grid_for(N * ((F + 3) >> 2), kBlock);
    hipLaunchKernelGGL(gbdt_bin_kernel<true>, grid, kBlock, 0, s, X, ldx, cuts, N, F, NB, bins, ldb);
  } else {
    const int grid = blocks > 0 ? blocks : grid_for(N * F, kBlock);
    hipLaunchKernelGGL(gbdt_bin_kernel<false>, grid, kBlock, 0, s, X, ldx, cuts, N, F, NB, bins, ldb);
  }
  MINIPS_HIP_CHECK(hipGetLastError());
}

void gbdt_grad(const float* z, const float* labels, int64_t N, int32_t* gh, int64_t* loss_acc, int blocks,
               hipStream_t s) {
  check_shape("gbdt_grad", 1, 2, 1, blocks);
  if (N <= 0) return;
  const int grid = blocks > 0 ? blocks : grid_for(N, kBlock, 1024);
  hipLaunchKernelGGL(gbdt_grad_kernel, grid, kBlock, 0, s, z, labels, N, gh, loss_acc);
  MINIPS_HIP_CHECK(hipGetLastError());
}

void gbdt_hist(const uint8_t* bins, int64_t ldb, int64_t width, const int32_t* node, const int32_t* gh, int64_t N,
               int F, int NB, int nodes, int64_t* hist, int path, int blocks, hipStream_t s) {
  check_shape("gbdt_hist", F, NB, nodes, blocks);
  if (path < 0 || path > 2)
    bad("gbdt_hist", "path is " + std::to_string(path) + ", expected 0 auto, 1 LDS, 2 global");
  if (ldb < F || width < F || width > ldb) bad("gbdt_hist", "ldb / width below F");
  const int tf = gbdt_hist_tile(nodes, F, NB);
  if (path == 1 && tf < 1)
    bad("gbdt_hist", "path 1: one feature of " + std::to_string(nodes) + " nodes x " + std::to_string(NB) +
                         " bins does not fit the LDS accumulators");
  if (N <= 0) return;
  if (path == 2 || tf < 1) {
    const int grid = blocks > 0 ? blocks : grid_for(N * F, kBlock, 4096);
    hipLaunchKernelGGL(gbdt_hist_global_kernel, grid, kBlock, 0, s, bins, ldb, node, gh, N, F, NB, nodes, hist);
  } else {
    const int tiles = (F + tf - 1) / tf;
    const int64_t nchunks = (N + kGbdtFlushRows - 1) / kGbdtFlushRows;
    const int gx = blocks > 0 ? blocks : (int)std::min<int64_t>(nchunks, std::max(1, 2048 / tiles));
    const size_t lds = (size_t)nodes * tf * NB * 3 * sizeof(int);
    const dim3 grid(gx, tiles);
    const int64_t f16 = ((int64_t)F + 15) & ~15ll;
    if (friendly(bins, ldb, 16) && width >= f16)
      hipLaunchKernelGGL(gbdt_hist_lds_kernel<true>, grid, kBlock, lds, s, bins, ldb, node, gh, N, F, NB, nodes, tf,
                         hist);
    else
      hipLaunchKernelGGL(gbdt_hist_lds_kernel<false>, grid, kBlock, lds, s, bins, ldb, node, gh, N, F, NB, nodes, tf,
                         hist);
  }
  MINIPS_HIP_CHECK(hipGetLastError());
}

void gbdt_split(const int64_t* hist, int nodes, int F, int NB, double lambda, int64_t min_child_count,
                double min_gain, int32_t* feat, int32_t* thr, double* gain, int64_t* child, double* wgain,
                int32_t* wthr, hipStream_t s) {
  check_shape("gbdt_split", F, NB, nodes, 0);
  if (!(lambda > 0.0) || !(lambda < 1e300)) bad("gbdt_split", "reg_lambda must be positive and finite");
  if (min_child_count < 1) bad("gbdt_split", "min_child_count must be >= 1");
  if (!(min_gain >= 0.0) || !(min_gain < 1e300)) bad("gbdt_split", "min_gain must be >= 0 and finite");
  const int64_t pairs = (int64_t)nodes * F;
  hipLaunchKernelGGL(gbdt_split_feature_kernel, (int)((pairs + kWaves - 1) / kWaves), kBlock, 0, s, hist, pairs, F, NB,
                     lambda, min_child_count, min_gain, wgain, wthr);
  hipLaunchKernelGGL(gbdt_split_node_kernel, (nodes + kWaves - 1) / kWaves, kBlock, 0, s, hist, nodes, F, NB, wgain,
                     wthr, feat, thr, gain, child);
  MINIPS_HIP_CHECK(hipGetLastError());
}

void gbdt_leaf(const int64_t* child, int nodes, double lambda, double lr, float* leaf, hipStream_t s) {
  check_shape("gbdt_leaf", 1, 2, nodes, 0);
  if (!(lambda > 0.0) || !(lambda < 1e300)) bad("gbdt_leaf", "reg_lambda must be positive and finite");
  if (!(lr > 0.0) || !(lr < 1e300)) bad("gbdt_leaf", "lr must be positive and finite");
  hipLaunchKernelGGL(gbdt_leaf_kernel, (2 * nodes + kBlock - 1) / kBlock, kBlock, 0, s, child, 2 * nodes, lambda, lr,
                     leaf);
  MINIPS_HIP_CHECK(hipGetLastError());
}

void gbdt_advance(const uint8_t* bins, int64_t ldb, int32_t* node, const int32_t* feat, const int32_t* thr,
                  int64_t N, int F, int nodes, const float* leaf, float* z, int blocks, hipStream_t s) {
  check_shape("gbdt_advance", F, 2, nodes, blocks);
  if (ldb < F) bad("gbdt_advance", "ldb below F");
  if (N <= 0) return;  // (an empty z has no address: checked after this)
  if ((leaf == nullptr) != (z == nullptr)) bad("gbdt_advance", "leaf and z come together");
  const int grid = blocks > 0 ? blocks : grid_for(N, kBlock);
  hipLaunchKernelGGL(gbdt_advance_kernel, grid, kBlock, 0, s, bins, ldb, node, feat, thr, N, F, nodes, leaf, z);
  MINIPS_HIP_CHECK(hipGetLastError());
}

void gbdt_predict(const uint8_t* bins, int64_t ldb, int64_t N, int F, const int32_t* feat, const uint8_t* thr,
                  const float* leaf, int T, int depth, float base, float* z, int32_t* leaf_index, int blocks,
                  hipStream_t s) {
  check_shape("gbdt_predict", F, 2, 1, blocks);
  if (depth < 1 || depth > kGbdtMaxDepth) bad("gbdt_predict", "depth is " + std::to_string(depth) + ", expected 1..8");
  if (T < 0 || T > kGbdtMaxTrees) bad("gbdt_predict", "T is " + std::to_string(T) + ", expected 0 <= T <= 65536");
  if (ldb < F) bad("gbdt_predict", "ldb below F");
  if (N <= 0) return;
  const int grid = blocks > 0 ? blocks : grid_for(N, kBlock);
  hipLaunchKernelGGL(gbdt_predict_kernel, grid, kBlock, 0, s, bins, ldb, N, F, feat, thr, leaf, T, depth, base, z,
                     leaf_index);
  MINIPS_HIP_CHECK(hipGetLastError());
}

}  // namespace minips_k
