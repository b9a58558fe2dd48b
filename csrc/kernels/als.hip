// ALS normal-equation kernels for gfx950: gathered SYRK by v_mfma_f32_16x16x4_f32 and a fused blocked Cholesky solve.
// The rule, the mapping and the launchers' contracts are stated in als.h.
#include <stdexcept>
#include <string>

#include "als.h"
#include "common.h"

namespace minips_k {
namespace {

constexpr int kBlock = 256;

// LDS of one workgroup, in floats. The two staging tiles [64][KP + 4] come first; the solve's lower triangle
// L [KP][KP + 1] is laid over them once the last stage has been multiplied.
template <int KP>
struct Lds {
  static constexpr int kLd = KP + 4;
  static constexpr int kTile = kAlsStage * kLd;
  static constexpr int kWa = 2 * kTile;            // a_t of the two stages [2][64]
  static constexpr int kWc = kWa + 2 * kAlsStage;  // c_t [2][64]
  static constexpr int kB = kWc + 2 * kAlsStage;   // b [KP]
  static constexpr int kCnt = kB + KP;             // contributing lookups of the 64 staging threads (int)
  static constexpr int kTotal = kCnt + kAlsStage;
  static constexpr int kLdL = KP + 1;
  static_assert(KP * kLdL <= 2 * kTile, "the solve's triangle must fit the staging tiles");
};

template <int KP>
struct Tri {
  static constexpr int T = KP / 16;
  static constexpr int NT = T * (T + 1) / 2;   // lower-triangle tiles
  static constexpr int MT = (NT + 3) / 4;      // a wave's share
  static constexpr int NP = KP * (KP + 1) / 2; // packed lower-triangle entries
};

// tile idx of the row-major lower triangle -> (ti, tj), tj <= ti
__device__ __forceinline__ void tile_of(int idx, int& ti, int& tj) {
  ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= idx) ++ti;
  tj = idx - ti * (ti + 1) / 2;
}

// packed entry idx -> (r, c), c <= r
__device__ __forceinline__ void entry_of(int idx, int& r, int& c) {
  r = (int)((sqrtf(8.f * (float)idx + 1.f) - 1.f) * 0.5f);
  while (r * (r + 1) / 2 > idx) --r;
  while ((r + 1) * (r + 2) / 2 <= idx) ++r;
  c = idx - r * (r + 1) / 2;
}

struct Src {
  const float* rows;
  int64_t ld, cap;
  int k;
  bool vec;
  const int64_t* inv;  // GATHER only
  const float* a;
  const float* c;
};

// The tiles of this wave: idx = wave + 4 p, ti < 0 when the wave has no p-th tile. Wave-uniform.
template <int KP>
struct WaveTiles {
  int ti[Tri<KP>::MT], tj[Tri<KP>::MT];
  __device__ __forceinline__ explicit WaveTiles(int wave) {
#pragma unroll
    for (int p = 0; p < Tri<KP>::MT; ++p) {
      const int idx = wave + 4 * p;
      if (idx < Tri<KP>::NT) {
        tile_of(idx, ti[p], tj[p]);
      } else {
        ti[p] = tj[p] = -1;
      }
    }
  }
};

// What one thread holds of the next stage while the current one is multiplied.
template <int KP>
struct Prefetch {
  float4 v[KP / 16];
  float a, c;
  int live;
};

template <int KP, bool GATHER>
__device__ __forceinline__ void stage_fetch(const Src& s, int base, int hi, Prefetch<KP>& pf) {
  constexpr int Q = KP / 4;
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < KP / 16; ++i) {
    const int idx = tid + kBlock * i, r = idx / Q, q = idx - r * Q, j = base + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < hi && 4 * q < s.k) {
      const int64_t row = GATHER ? s.inv[j] : (int64_t)j;
      if (row >= 0 && row < s.cap) {
        const float* p = s.rows + row * s.ld + 4 * q;
        if (s.vec) {
          v = *reinterpret_cast<const float4*>(p);
        } else {
          v = make_float4(p[0], p[1], p[2], p[3]);
        }
      }
    }
    pf.v[i] = v;
  }
  pf.a = pf.c = 0.f;
  pf.live = 0;
  if (tid < kAlsStage) {
    const int j = base + tid;
    if (j < hi) {
      const int64_t row = GATHER ? s.inv[j] : (int64_t)j;
      if (row >= 0 && row < s.cap) {
        pf.live = 1;
        pf.a = GATHER ? s.a[j] : 1.f;
        pf.c = GATHER ? s.c[j] : 0.f;
      }
    }
  }
}

template <int KP>
__device__ __forceinline__ void stage_stash(float* sm, int buf, const Prefetch<KP>& pf, int& cnt) {
  constexpr int Q = KP / 4;
  const int tid = threadIdx.x;
  float* tile = sm + buf * Lds<KP>::kTile;
#pragma unroll
  for (int i = 0; i < KP / 16; ++i) {
    const int idx = tid + kBlock * i, r = idx / Q, q = idx - r * Q;
    *reinterpret_cast<float4*>(tile + r * Lds<KP>::kLd + 4 * q) = pf.v[i];
  }
  if (tid < kAlsStage) {
    sm[Lds<KP>::kWa + buf * kAlsStage + tid] = pf.a;
    sm[Lds<KP>::kWc + buf * kAlsStage + tid] = pf.c;
    cnt += pf.live;
  }
}

// Gram tiles and b of the members [lo, hi): acc (this wave's tiles), bacc (thread c < k) and cnt (threads < 64: the
// contributing lookups they staged). Ends behind a barrier: the tiles are free.
template <int KP, bool GATHER>
__device__ __forceinline__ void als_accumulate(const Src& s, int lo, int hi, float* sm, const WaveTiles<KP>& wt,
                                               v4f (&acc)[Tri<KP>::MT], float& bacc, int& cnt) {
  using L = Lds<KP>;
  const int tid = threadIdx.x, lane = tid & 63;
  const int len = hi - lo, nst = (len + kAlsStage - 1) / kAlsStage;
  Prefetch<KP> pf;
  if (nst > 0) {
    stage_fetch<KP, GATHER>(s, lo, hi, pf);
    stage_stash<KP>(sm, 0, pf, cnt);
  }
  __syncthreads();
  for (int st = 0; st < nst; ++st) {
    const int buf = st & 1;
    const bool more = st + 1 < nst;
    if (more) stage_fetch<KP, GATHER>(s, lo + (st + 1) * kAlsStage, hi, pf);  // in flight during the MFMAs below
    const int here = min(kAlsStage, len - st * kAlsStage), nkk = (here + 3) / 4;
    const float* tile = sm + buf * L::kTile;
    const float* wa = sm + L::kWa + buf * kAlsStage;
    for (int kk = 0; kk < nkk; ++kk) {
      const int t = 4 * kk + (lane >> 4);
      const float w = wa[t];
      const float* rp = tile + t * L::kLd + (lane & 15);
#pragma unroll
      for (int p = 0; p < Tri<KP>::MT; ++p) {
        if (wt.ti[p] >= 0) {
          const float av = rp[16 * wt.ti[p]] * w, bv = rp[16 * wt.tj[p]];
          acc[p] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[p], 0, 0, 0);
        }
      }
    }
    if (GATHER && tid < s.k) {
      const float* wc = sm + L::kWc + buf * kAlsStage;
      for (int t = 0; t < here; ++t) bacc = fmaf(wc[t], tile[t * L::kLd + tid], bacc);
    }
    if (more) stage_stash<KP>(sm, buf ^ 1, pf, cnt);
    __syncthreads();
  }
}

// this wave's accumulators -> the triangle L [KP][KP + 1] (the diagonal tiles whole)
template <int KP>
__device__ __forceinline__ void store_tiles(float* Lm, const WaveTiles<KP>& wt, const v4f (&acc)[Tri<KP>::MT]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int p = 0; p < Tri<KP>::MT; ++p) {
    if (wt.ti[p] >= 0) {
#pragma unroll
      for (int v = 0; v < 4; ++v)
        Lm[(16 * wt.ti[p] + 4 * (lane >> 4) + v) * Lds<KP>::kLdL + 16 * wt.tj[p] + (lane & 15)] = acc[p][v];
    }
  }
}

__device__ __forceinline__ float lane_value(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

struct Out {
  const float* reg;
  const int64_t* slot;
  const float* x_old;
  float* x_out;
  float* delta;
  int64_t m;
  const float* gram0;
  int32_t* bad;
};

// Solves entity e from the Gram triangle in L (sm), b in sm[kB] and `total` contributing lookups; every thread of
// the workgroup calls it. Starts behind a barrier (L and b are complete).
template <int KP>
__device__ void als_solve_lds(float* sm, int k, int e, int total, const Out& o) {
  constexpr int LD = Lds<KP>::kLdL;
  float* Lm = sm;
  const float* sb = sm + Lds<KP>::kB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float reg = o.reg[e];
  for (int idx = tid; idx < k * k; idx += kBlock) {
    const int r = idx / k, c = idx - r * k;
    if (c <= r) {
      float v = Lm[r * LD + c];
      if (o.gram0) v += o.gram0[idx];
      if (r == c) v += reg;
      Lm[r * LD + c] = v;
    }
  }
  __syncthreads();
  const int Tk = (k + 15) / 16;
  int bad = 0;  // wave 0's
  for (int p = 0; p < Tk; ++p) {
    const int p0 = 16 * p, nb = min(16, k - p0);
    // Only the lower triangle of L is data. The upper halves of the diagonal tiles (no G0, no reg; zero after a fold)
    // are loaded and updated below as don't-care values: every entry c <= i depends on lower entries alone, and only
    // those are stored or read by the solves.
    if (wave == 0) {  // the diagonal block, a row a lane, in registers
      const int i = lane & 15;
      float r[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) r[c] = Lm[(p0 + i) * LD + p0 + c];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (j < nb) {
          const float d = lane_value(r[j], j);
          if (!(d > 0.f && d < INFINITY)) bad = 1;
          const float s = sqrtf(d);
          r[j] = i == j ? s : r[j] / s;
#pragma unroll
          for (int c = j + 1; c < 16; ++c) r[c] = fmaf(-r[j], lane_value(r[j], c), r[c]);
        }
      }
      if (lane < 16) {
#pragma unroll
        for (int c = 0; c < 16; ++c)
          if (c <= i) Lm[(p0 + i) * LD + p0 + c] = r[c];
      }
    }
    __syncthreads();
    {  // every row below solves its 16 entries against the block (rows below exist only under a full panel)
      const int i = p0 + 16 + tid;
      if (i < k) {
        float x[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) x[c] = Lm[i * LD + p0 + c];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          float s = x[j];
#pragma unroll
          for (int c = 0; c < j; ++c) s = fmaf(-x[c], Lm[(p0 + j) * LD + p0 + c], s);
          x[j] = s / Lm[(p0 + j) * LD + p0 + j];
        }
#pragma unroll
        for (int c = 0; c < 16; ++c) Lm[i * LD + p0 + c] = x[c];
      }
    }
    __syncthreads();
    const int mt = Tk - 1 - p, ntr = mt * (mt + 1) / 2;  // trailing tiles: C -= P_ti P_tj^T, 4 MFMA steps
    for (int idx = wave; idx < ntr; idx += 4) {
      int ta, tb;
      tile_of(idx, ta, tb);
      const int ri = 16 * (p + 1 + ta), rj = 16 * (p + 1 + tb);
      v4f cc;
#pragma unroll
      for (int v = 0; v < 4; ++v) cc[v] = Lm[(ri + 4 * (lane >> 4) + v) * LD + rj + (lane & 15)];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float av = -Lm[(ri + (lane & 15)) * LD + p0 + 4 * s + (lane >> 4)];
        const float bv = Lm[(rj + (lane & 15)) * LD + p0 + 4 * s + (lane >> 4)];
        cc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, cc, 0, 0, 0);
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) Lm[(ri + 4 * (lane >> 4) + v) * LD + rj + (lane & 15)] = cc[v];
    }
    __syncthreads();
  }
  if (wave != 0) return;
  // L z = b then L^T x = z in one wave, column-oriented: lane l owns the elements l and l + 64
  const int i1 = lane + 64;
  float z0 = lane < k ? sb[lane] : 0.f, z1 = (KP > 64 && i1 < k) ? sb[i1] : 0.f;
  for (int j = 0; j < k; ++j) {
    const float zj = __shfl(j < 64 ? z0 : z1, j & 63, 64) / Lm[j * LD + j];
    if (lane == (j & 63)) {
      if (j < 64) z0 = zj; else z1 = zj;
    }
    if (lane > j && lane < k) z0 = fmaf(-Lm[lane * LD + j], zj, z0);
    if (KP > 64 && i1 > j && i1 < k) z1 = fmaf(-Lm[i1 * LD + j], zj, z1);
  }
  for (int j = k - 1; j >= 0; --j) {
    const float xj = __shfl(j < 64 ? z0 : z1, j & 63, 64) / Lm[j * LD + j];
    if (lane == (j & 63)) {
      if (j < 64) z0 = xj; else z1 = xj;
    }
    if (lane < j) z0 = fmaf(-Lm[j * LD + lane], xj, z0);
    if (KP > 64 && i1 < j) z1 = fmaf(-Lm[j * LD + i1], xj, z1);
  }
  const int64_t sl = o.slot[e];
  if (sl < 0 || sl >= o.m) return;
  const bool solved = total > 0 && !bad;
  if (total > 0 && bad && lane == 0 && o.bad) atomicAdd(o.bad, 1);
  if (lane < k) {
    const float xo = o.x_old[sl * k + lane];
    o.x_out[sl * k + lane] = solved ? z0 : xo;
    o.delta[sl * k + lane] = solved ? z0 - xo : 0.f;
  }
  if (KP > 64 && i1 < k) {
    const float xo = o.x_old[sl * k + i1];
    o.x_out[sl * k + i1] = solved ? z1 : xo;
    o.delta[sl * k + i1] = solved ? z1 - xo : 0.f;
  }
}

struct SolveArgs {
  Src s;
  Out o;
  const int64_t* rowptr;
  int n, B;
  const int32_t* desc;
  int n_desc, n_multi_desc;
  const int32_t* multi;
  int n_multi;
  float* ws;
};

__device__ __forceinline__ int clamp_ptr(int64_t v, int n) { return (int)(v < 0 ? 0 : (v > n ? n : v)); }

template <int KP>
__global__ __launch_bounds__(kBlock) void als_solve_kernel(SolveArgs g) {
  using L = Lds<KP>;
  __shared__ __attribute__((aligned(16))) float sm[L::kTotal];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const WaveTiles<KP> wt(wave);
  int* scnt = reinterpret_cast<int*>(sm + L::kCnt);
  for (int d = blockIdx.x; d < g.n_desc; d += gridDim.x) {
    const int e = g.desc[3 * d];
    if (e < 0 || e >= g.B) {  // skipped; a multi-chunk slot is zeroed, so the fold adds nothing from it
      if (d < g.n_multi_desc)
        for (int idx = tid; idx < Tri<KP>::NP + KP + 4; idx += kBlock)
          g.ws[(int64_t)d * (Tri<KP>::NP + KP + 4) + idx] = 0.f;
      continue;
    }
    const int r0 = clamp_ptr(g.rowptr[e], g.n), r1 = max(r0, clamp_ptr(g.rowptr[e + 1], g.n));
    const int lo = min(max(g.desc[3 * d + 1], r0), r1), hi = max(lo, min(g.desc[3 * d + 2], r1));
    v4f acc[Tri<KP>::MT];
#pragma unroll
    for (int p = 0; p < Tri<KP>::MT; ++p) acc[p] = v4f{0.f, 0.f, 0.f, 0.f};
    float bacc = 0.f;
    int cnt = 0;
    als_accumulate<KP, true>(g.s, lo, hi, sm, wt, acc, bacc, cnt);
    store_tiles<KP>(sm, wt, acc);
    if (tid < KP) sm[L::kB + tid] = bacc;
    if (tid < kAlsStage) scnt[tid] = cnt;
    __syncthreads();
    int total = 0;
    for (int i = 0; i < kAlsStage; ++i) total += scnt[i];
    if (d < g.n_multi_desc) {  // a chunk of a multi-chunk entity: its partial, folded by als_fold_solve_kernel
      float* w = g.ws + (int64_t)d * (Tri<KP>::NP + KP + 4);
      for (int idx = tid; idx < Tri<KP>::NP; idx += kBlock) {
        int r, c;
        entry_of(idx, r, c);
        w[idx] = sm[r * L::kLdL + c];
      }
      if (tid < KP) w[Tri<KP>::NP + tid] = sm[L::kB + tid];
      if (tid == 0) w[Tri<KP>::NP + KP] = (float)total;
    } else {
      als_solve_lds<KP>(sm, g.s.k, e, total, g.o);
    }
    __syncthreads();
  }
}

template <int KP>
__global__ __launch_bounds__(kBlock) void als_fold_solve_kernel(SolveArgs g) {
  using L = Lds<KP>;
  __shared__ __attribute__((aligned(16))) float sm[L::kTotal];
  constexpr int NP = Tri<KP>::NP, SLOT = NP + KP + 4;
  const int tid = threadIdx.x;
  for (int q = blockIdx.x; q < g.n_multi; q += gridDim.x) {
    const int e = g.multi[3 * q], first = g.multi[3 * q + 1], nd = g.multi[3 * q + 2];
    if (e < 0 || e >= g.B || first < 0 || nd < 1 || nd > g.n_multi_desc || first > g.n_multi_desc - nd) continue;
    for (int idx = tid; idx < KP * L::kLdL; idx += kBlock) sm[idx] = 0.f;
    __syncthreads();
    const float* w = g.ws + (int64_t)first * SLOT;
    for (int idx = tid; idx < NP; idx += kBlock) {
      float s = w[idx];
      for (int c = 1; c < nd; ++c) s += w[(int64_t)c * SLOT + idx];
      int r, cc;
      entry_of(idx, r, cc);
      sm[r * L::kLdL + cc] = s;
    }
    if (tid < KP) {
      float s = w[NP + tid];
      for (int c = 1; c < nd; ++c) s += w[(int64_t)c * SLOT + NP + tid];
      sm[L::kB + tid] = s;
    }
    int total = 0;
    for (int c = 0; c < nd; ++c) total += (int)w[(int64_t)c * SLOT + NP + KP];
    __syncthreads();
    als_solve_lds<KP>(sm, g.s.k, e, total, g.o);
    __syncthreads();
  }
}

template <int KP>
__global__ __launch_bounds__(kBlock) void als_gram_kernel(Src s, float* part) {
  using L = Lds<KP>;
  __shared__ __attribute__((aligned(16))) float sm[L::kTotal];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const WaveTiles<KP> wt(wave);
  const int64_t lo64 = (int64_t)blockIdx.x * kAlsGramStrip;
  const int lo = (int)lo64, hi = (int)(s.cap - lo64 < kAlsGramStrip ? s.cap : lo64 + kAlsGramStrip);
  v4f acc[Tri<KP>::MT];
#pragma unroll
  for (int p = 0; p < Tri<KP>::MT; ++p) acc[p] = v4f{0.f, 0.f, 0.f, 0.f};
  float bacc = 0.f;
  int cnt = 0;
  als_accumulate<KP, false>(s, lo, hi, sm, wt, acc, bacc, cnt);
  store_tiles<KP>(sm, wt, acc);
  __syncthreads();
  float* w = part + (int64_t)blockIdx.x * Tri<KP>::NP;
  for (int idx = tid; idx < Tri<KP>::NP; idx += kBlock) {
    int r, c;
    entry_of(idx, r, c);
    w[idx] = sm[r * L::kLdL + c];
  }
}

// out [k, k] = the partials added in index order, mirrored
__global__ __launch_bounds__(kBlock) void als_gram_fold_kernel(const float* part, int64_t nstrips, int np, int k,
                                                               float* out) {
  const int idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx >= np) return;
  int r, c;
  entry_of(idx, r, c);
  if (r >= k) return;
  float s = 0.f;
  for (int64_t i = 0; i < nstrips; ++i) s += part[i * np + idx];
  out[r * k + c] = s;
  out[c * k + r] = s;
}

template <typename F>
void dispatch_kp(int k, const F& f) {
  switch (als_kp(k)) {
    case 16: return f.template run<16>();
    case 32: return f.template run<32>();
    case 48: return f.template run<48>();
    case 64: return f.template run<64>();
    case 80: return f.template run<80>();
    case 96: return f.template run<96>();
    case 112: return f.template run<112>();
    default: return f.template run<128>();
  }
}

struct SolveLaunch {
  SolveArgs a;
  int blocks;
  hipStream_t s;
  template <int KP>
  void run() const {
    const int grid = blocks > 0 ? blocks : (a.n_desc < (1 << 20) ? a.n_desc : (1 << 20));
    hipLaunchKernelGGL((als_solve_kernel<KP>), grid, kBlock, 0, s, a);
    if (a.n_multi > 0) {
      const int fgrid = blocks > 0 ? blocks : (a.n_multi < (1 << 20) ? a.n_multi : (1 << 20));
      hipLaunchKernelGGL((als_fold_solve_kernel<KP>), fgrid, kBlock, 0, s, a);
    }
  }
};

struct GramLaunch {
  Src src;
  float* part;
  int strips;
  hipStream_t s;
  template <int KP>
  void run() const {
    hipLaunchKernelGGL((als_gram_kernel<KP>), strips, kBlock, 0, s, src, part);
  }
};

void check_rows(const char* op, int k, int64_t ld, int64_t cap) {
  if (!als_k_ok(k)) throw std::runtime_error(std::string(op) + ": k % 4 == 0 and 4 <= k <= 128");
  if (ld < k) throw std::runtime_error(std::string(op) + ": rows' leading dimension is below k");
  if (cap < 0 || cap >= (1ll << 31))
    throw std::runtime_error(std::string(op) + ": rows must hold fewer than 2^31 rows");
}

}  // namespace

void als_solve(const int64_t* rowptr, const int64_t* inv, const float* a, const float* c, int64_t n, const float* rows,
               int64_t ld, int64_t cap, int k, const float* reg, const int64_t* slot, int64_t B, const float* x_old,
               float* x_out, float* delta, int64_t m, const int32_t* desc, int64_t n_desc, int64_t n_multi_desc,
               const int32_t* multi, int64_t n_multi, float* ws, const float* gram0, int32_t* bad, int blocks,
               hipStream_t s) {
  check_rows("als_solve", k, ld, cap);
  if (n < 0 || n >= (1ll << 31) || B < 0 || B >= (1ll << 31) || m < 0)
    throw std::runtime_error("als_solve: n and B must be below 2^31");
  if (n_desc < 0 || n_desc >= (1ll << 31) || n_multi_desc < 0 || n_multi_desc > n_desc || n_multi < 0 ||
      n_multi > n_multi_desc)
    throw std::runtime_error("als_solve: 0 <= n_multi <= n_multi_desc <= n_desc < 2^31");
  if (n_multi_desc > 0 && ws == nullptr) throw std::runtime_error("als_solve: ws workspace missing");
  if (blocks < 0 || blocks > kAlsMaxBlocks) throw std::runtime_error("als_solve: 0 <= blocks <= 65535");
  if (n_desc == 0) return;
  const bool vec = ld % 4 == 0 && aligned16(rows);
  const SolveArgs g{Src{rows, ld, cap, k, vec, inv, a, c},
                    Out{reg, slot, x_old, x_out, delta, m, gram0, bad},
                    rowptr, (int)n, (int)B, desc, (int)n_desc, (int)n_multi_desc, multi, (int)n_multi, ws};
  dispatch_kp(k, SolveLaunch{g, blocks, s});
  MINIPS_HIP_CHECK(hipGetLastError());
}

void als_gram(const float* rows, int64_t ld, int64_t R, int k, float* part, float* out, hipStream_t s) {
  check_rows("als_gram", k, ld, R);
  const int64_t strips = (R + kAlsGramStrip - 1) / kAlsGramStrip;
  const int kp = als_kp(k), np = kp * (kp + 1) / 2;
  if (strips > 0) {
    if (part == nullptr) throw std::runtime_error("als_gram: part workspace missing");
    const bool vec = ld % 4 == 0 && aligned16(rows);
    dispatch_kp(k, GramLaunch{Src{rows, ld, R, k, vec, nullptr, nullptr, nullptr}, part, (int)strips, s});
  }
  hipLaunchKernelGGL(als_gram_fold_kernel, (np + kBlock - 1) / kBlock, kBlock, 0, s, part, strips, np, k, out);
  MINIPS_HIP_CHECK(hipGetLastError());
}

}  // namespace minips_k
