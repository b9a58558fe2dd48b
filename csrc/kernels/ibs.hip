// In-batch sampled softmax kernels for gfx950: a flash-attention-shaped fp32 MFMA tile routine (resident side against
// streamed side) as the forward and the two gradient sweeps, and the row reduce on member_rows.h.
// The rule, the mapping and the launchers' contracts are stated in ibs.h.
#include <stdexcept>
#include <string>

#include "common.h"
#include "ibs.h"
#include "member_rows.h"

namespace minips_k {
namespace {

constexpr int kBlock = 256;
constexpr int kT = kIbsTile;
constexpr int kLdG = kT + 4;

enum Mode { kFwd = 0, kGradUser = 1, kGradItem = 2 };

// LDS of one workgroup, in floats: the resident tile and the two streamed buffers [64][KP + 4], the G tile [64][68]
// of the gradient sweeps, and per tile the 64 item rows (int, -1: not a valid pair) and 64 floats (logq on the item
// side, the query's lse on the user side).
template <int KP, bool GRAD>
struct Lds {
  static constexpr int kLd = KP + 4;
  static constexpr int kTile = kT * kLd;
  static constexpr int kG = 3 * kTile;
  static constexpr int kItem = kG + (GRAD ? kT * kLdG : 0);
  static constexpr int kF = kItem + 3 * kT;
  static constexpr int kTotal = kF + 3 * kT;
};

struct Args {
  const int64_t* inv;
  const float* rows;
  int64_t ld, cap;
  int P, d;
  bool vec;
  float rtau, gs;
  const float* logq;
  const float* lse_in;
  float* lse;
  float* loss;
  float* ws;
};

// What one thread holds of a tile between its global loads and its LDS stores.
template <int KP>
struct Prefetch {
  float4 v[KP / 16];
  int item;
  float f;
};

__device__ __forceinline__ bool pair_rows(const Args& a, int j, int64_t& ru, int64_t& ri) {
  ru = a.inv[2 * (int64_t)j];
  ri = a.inv[2 * (int64_t)j + 1];
  return ru >= 0 && ru < a.cap && ri >= 0 && ri < a.cap;
}

// the pairs [base, base + 64): the item rows (ITEM) or the user rows; a pair beyond P or not valid is a zero row
template <int KP, bool ITEM>
__device__ __forceinline__ void tile_fetch(const Args& a, int base, Prefetch<KP>& pf) {
  constexpr int Q = KP / 4;
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < KP / 16; ++i) {
    const int idx = tid + kBlock * i, r = idx / Q, q = idx - r * Q, j = base + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    int64_t ru, ri;
    if (j < a.P && 4 * q < a.d && pair_rows(a, j, ru, ri)) {
      const float* p = a.rows + (ITEM ? ri : ru) * a.ld + 4 * q;
      if (a.vec) {
        v = *reinterpret_cast<const float4*>(p);
      } else {
        v = make_float4(p[0], p[1], p[2], p[3]);
      }
    }
    pf.v[i] = v;
  }
  pf.item = -1;
  pf.f = 0.f;
  if (tid < kT) {
    const int j = base + tid;
    int64_t ru, ri;
    if (j < a.P && pair_rows(a, j, ru, ri)) {
      pf.item = (int)ri;
      const float* f = ITEM ? a.logq : a.lse_in;
      if (f) pf.f = f[j];
    }
  }
}

template <int KP, bool GRAD>
__device__ __forceinline__ void tile_stash(float* sm, int slot, const Prefetch<KP>& pf) {
  using L = Lds<KP, GRAD>;
  constexpr int Q = KP / 4;
  const int tid = threadIdx.x;
  float* tile = sm + slot * L::kTile;
#pragma unroll
  for (int i = 0; i < KP / 16; ++i) {
    const int idx = tid + kBlock * i, r = idx / Q, q = idx - r * Q;
    *reinterpret_cast<float4*>(tile + r * L::kLd + 4 * q) = pf.v[i];
  }
  if (tid < kT) {
    reinterpret_cast<int*>(sm + L::kItem)[slot * kT + tid] = pf.item;
    sm[L::kF + slot * kT + tid] = pf.f;
  }
}

// the sum / maximum over the 16 lanes that hold one row of a 16 x 16 accumulator; every lane gets the same bits
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float row_max(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Resident tile rt against every streamed tile. The logit tile's rows are the resident pairs, its columns the
// streamed ones; lane (g = lane >> 4, i = lane & 15) of wave w holds acc[j][v] = row 16 w + 4 g + v, column 16 j + i.
template <int KP, int MODE>
__global__ __launch_bounds__(kBlock) void ibs_tile_kernel(Args a) {
  constexpr bool GRAD = MODE != kFwd, RES_ITEM = MODE == kGradItem;
  using L = Lds<KP, GRAD>;
  __shared__ __attribute__((aligned(16))) float sm[L::kTotal];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, i = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int* items = reinterpret_cast<const int*>(sm + L::kItem);
  const float* fs = sm + L::kF;
  const int nt = (a.P + kT - 1) / kT;
  for (int rt = blockIdx.x; rt < nt; rt += gridDim.x) {
    Prefetch<KP> pf;
    tile_fetch<KP, RES_ITEM>(a, rt * kT, pf);
    tile_stash<KP, GRAD>(sm, 0, pf);
    tile_fetch<KP, !RES_ITEM>(a, 0, pf);
    tile_stash<KP, GRAD>(sm, 1, pf);
    __syncthreads();
    int ritem[4];
    float rf[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      ritem[v] = items[16 * w + 4 * g + v];
      rf[v] = fs[16 * w + 4 * g + v];
    }
    float mx[4], sum[4], spp[4];
    v4f dacc[KP / 16];
#pragma unroll
    for (int v = 0; v < 4; ++v) mx[v] = -INFINITY, sum[v] = 0.f, spp[v] = 0.f;
#pragma unroll
    for (int n = 0; n < KP / 16; ++n) dacc[n] = v4f{0.f, 0.f, 0.f, 0.f};
    for (int st = 0; st < nt; ++st) {
      const int buf = st & 1;
      const bool more = st + 1 < nt;
      if (more) tile_fetch<KP, !RES_ITEM>(a, (st + 1) * kT, pf);  // in flight during the MFMAs below
      const float* R = sm + (16 * w + i) * L::kLd + g;
      const float* S = sm + (1 + buf) * L::kTile;
      const int* sitem = items + (1 + buf) * kT;
      const float* sf = fs + (1 + buf) * kT;
      v4f acc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int kk = 0; kk < KP / 4; ++kk) {
        const float av = R[4 * kk];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, S[(16 * j + i) * L::kLd + 4 * kk + g], acc[j], 0, 0, 0);
      }
      // logits and the live mask
      bool live[4][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int citem = sitem[16 * j + i], c = st * kT + 16 * j + i;
        const float cf = sf[16 * j + i];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int r = rt * kT + 16 * w + 4 * g + v;
          live[j][v] = citem >= 0 && ritem[v] >= 0 && (c == r || citem != ritem[v]);
          acc[j][v] = acc[j][v] * a.rtau - (RES_ITEM ? rf[v] : cf);
        }
      }
      if constexpr (!GRAD) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          float tm = -INFINITY;
#pragma unroll
          for (int j = 0; j < 4; ++j) tm = fmaxf(tm, live[j][v] ? acc[j][v] : -INFINITY);
          const float mnew = fmaxf(mx[v], row_max(tm));
          const float ms = mnew == -INFINITY ? 0.f : mnew;
          float ps = 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            ps += live[j][v] ? expf(acc[j][v] - ms) : 0.f;
            // the diagonal: column 16 j + i == row 16 w + 4 g + v
            if (st == rt && j == w && i == 4 * g + v) spp[v] = acc[j][v];
          }
          sum[v] = sum[v] * expf(mx[v] - ms) + row_sum(ps);
          mx[v] = mnew;
        }
      } else {
        float* Gt = sm + L::kG;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c = st * kT + 16 * j + i;
          const float ql = RES_ITEM ? sf[16 * j + i] : 0.f;
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int r = rt * kT + 16 * w + 4 * g + v;
            const float pi = expf(acc[j][v] - (RES_ITEM ? ql : rf[v]));
            Gt[(16 * w + 4 * g + v) * kLdG + 16 * j + i] = live[j][v] ? (pi - (c == r ? 1.f : 0.f)) * a.gs : 0.f;
          }
        }
        __syncthreads();
        const float* Ga = Gt + (16 * w + i) * kLdG + g;
#pragma unroll 4
        for (int kk = 0; kk < kT / 4; ++kk) {
          const float gv = Ga[4 * kk];
          const float* Sb = S + (4 * kk + g) * L::kLd + i;
#pragma unroll
          for (int n = 0; n < KP / 16; ++n)
            dacc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(gv, Sb[16 * n], dacc[n], 0, 0, 0);
        }
      }
      if (more) tile_stash<KP, GRAD>(sm, 1 + (buf ^ 1), pf);
      __syncthreads();
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int r = rt * kT + 16 * w + 4 * g + v;
      if (r >= a.P) continue;
      if constexpr (!GRAD) {
        if (i == 4 * g + v) {
          const float lse = ritem[v] >= 0 ? mx[v] + logf(sum[v]) : 0.f;
          a.lse[r] = lse;
          a.loss[r] = ritem[v] >= 0 ? lse - spp[v] : 0.f;
        }
      } else {
        float* out = a.ws + (2 * (int64_t)r + (RES_ITEM ? 1 : 0)) * KP + i;
#pragma unroll
        for (int n = 0; n < KP / 16; ++n) out[16 * n] = dacc[n][v];
      }
    }
    // the last sweep iteration ended behind a barrier: the tiles are free for the next resident tile
  }
}

struct RedArgs {
  const int32_t* members;
  const int32_t* memrow;
  int n;
  int64_t cap;
  const float* ws;
  int kp, d;
  bool vec;
  float* grad;
  float* part;
};

__device__ __forceinline__ void add4(float4& s, const float4& v) {
  s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
}

// the members [m0, m1) with the given stride, in that order: column float4 l of their workspace rows
__device__ __forceinline__ float4 walk(const RedArgs& a, int m0, int m1, int stride, int l) {
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
  for (int m = m0; m < m1; m += stride) {
    const int j = a.members[m];
    if ((unsigned)j < (unsigned)a.n) add4(s, *reinterpret_cast<const float4*>(a.ws + (int64_t)j * a.kp + 4 * l));
  }
  return s;
}

__device__ __forceinline__ void store4(float* p, const float4& s, bool vec) {
  if (vec) {
    *reinterpret_cast<float4*>(p) = s;
  } else {
    p[0] = s.x, p[1] = s.y, p[2] = s.z, p[3] = s.w;
  }
}

// Rows of up to kIbsWaveMax members: G = 64 / L consecutive unique rows per wave and iteration, a lane group a row.
template <int L>
__global__ __launch_bounds__(kBlock) void ibs_reduce_kernel(RedArgs a) {
  constexpr int G = 64 / L;
  const int lane = threadIdx.x & 63, g = lane / L, l = lane % L;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int U = member_unique(a.memrow, a.n, a.cap);
  const int64_t ntiles = ((int64_t)U + G - 1) / G;
  for (int64_t tile = wave; tile < ntiles; tile += nwaves) {
    const int64_t u = tile * G + g;
    if (u >= U || 4 * l >= a.d) continue;
    const int lo = lower_bound_i32(a.memrow, 0, a.n, u);
    if (lo >= a.n || a.memrow[lo] != u) continue;
    const int hi = gallop_i32(a.memrow, lo, a.n, u + 1);
    if (hi - lo > kIbsWaveMax) continue;
    store4(a.grad + u * a.d + 4 * l, walk(a, lo, hi, 1, l), a.vec);
  }
}

// block p sums the members of chunk p that belong to a heavy row into part[(2 p + s) * d ...] (member_rows.h):
// 256 / L lane groups take the members in turn and are folded through LDS in group order
template <int L>
__global__ __launch_bounds__(kBlock) void ibs_reduce_heavy_kernel(RedArgs a) {
  constexpr int NG = kBlock / L;
  __shared__ float4 red[kBlock];
  const int gi = threadIdx.x / L, l = threadIdx.x % L;
  const int64_t p = blockIdx.x;
  const int64_t c_lo = p * kIbsChunk, c_hi = (c_lo + kIbsChunk) < a.n ? (c_lo + kIbsChunk) : a.n;
  for (int s = 0; s < 2; ++s) {
    int r, lo, hi;
    if (!member_heavy_row<kIbsChunk, kIbsWaveMax>(a.memrow, a.n, a.cap, p, s, r, lo, hi)) continue;  // block-uniform
    const int m0 = lo > c_lo ? lo : (int)c_lo, m1 = hi < c_hi ? hi : (int)c_hi;
    __syncthreads();  // (the previous candidate's reads of red)
    red[gi * L + l] = 4 * l < a.d ? walk(a, m0 + gi, m1, NG, l) : make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    if (threadIdx.x < L && 4 * l < a.d) {
      float4 t = red[l];
      for (int q = 1; q < NG; ++q) add4(t, red[q * L + l]);
      store4(a.part + (2 * p + s) * a.d + 4 * l, t, true);
    }
  }
}

void check_shape(const char* op, int d, float tau, int64_t ld, int64_t cap, int64_t P, int blocks) {
  if (!ibs_d_ok(d)) throw std::runtime_error(std::string(op) + ": d % 4 == 0 and 8 <= d <= 128");
  if (!(tau > 0.f && tau < INFINITY)) throw std::runtime_error(std::string(op) + ": tau must be positive and finite");
  if (ld < d) throw std::runtime_error(std::string(op) + ": ld < d");
  if (blocks < 0 || blocks > kIbsMaxBlocks) throw std::runtime_error(std::string(op) + ": blocks outside [0, 65535]");
  if (P < 0 || P >= (1ll << 30) || cap < 0 || cap >= (1ll << 31))
    throw std::runtime_error(std::string(op) + ": P must be below 2^30 and cap below 2^31");
}

template <typename F>
void dispatch_kp(int d, const F& f) {
  switch (ibs_kp(d)) {
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

struct TileLaunch {
  Args a;
  bool grad;
  int blocks;
  hipStream_t s;
  template <int KP>
  void run() const {
    const int nt = (a.P + kT - 1) / kT, grid = blocks > 0 ? blocks : nt;
    if (!grad) {
      hipLaunchKernelGGL((ibs_tile_kernel<KP, kFwd>), grid, kBlock, 0, s, a);
    } else {
      hipLaunchKernelGGL((ibs_tile_kernel<KP, kGradUser>), grid, kBlock, 0, s, a);
      hipLaunchKernelGGL((ibs_tile_kernel<KP, kGradItem>), grid, kBlock, 0, s, a);
    }
  }
};

template <int L>
void launch_reduce(const RedArgs& a, int blocks, hipStream_t s) {
  const int64_t urows = a.cap < a.n ? a.cap : a.n;  // at most this many unique rows
  const int grid = blocks > 0 ? blocks : grid_for(urows * L, kBlock, 8192);
  hipLaunchKernelGGL((ibs_reduce_kernel<L>), grid, kBlock, 0, s, a);
  if (a.n > kIbsWaveMax) {
    const int chunks = member_chunks(a.n, kIbsChunk);
    hipLaunchKernelGGL((ibs_reduce_heavy_kernel<L>), chunks, kBlock, 0, s, a);
    hipLaunchKernelGGL((member_heavy_fold_kernel<float, float, kIbsChunk, kIbsWaveMax>), chunks, kBlock, 0, s,
                       a.memrow, a.n, a.cap, a.d, a.part, a.grad);
  }
}

}  // namespace

void ibs_forward(const int64_t* inv, const float* rows, int64_t ld, int64_t cap, int d, float tau, const float* logq,
                 int64_t P, float* lse, float* loss, int blocks, hipStream_t s) {
  check_shape("ibs_forward", d, tau, ld, cap, P, blocks);
  if (P <= 0) return;
  const bool vec = ld % 4 == 0 && aligned16(rows);
  const Args a{inv, rows, ld, cap, (int)P, d, vec, 1.f / tau, 0.f, logq, nullptr, lse, loss, nullptr};
  dispatch_kp(d, TileLaunch{a, false, blocks, s});
  MINIPS_HIP_CHECK(hipGetLastError());
}

int64_t ibs_backward_ws_floats(int64_t P, int d) { return 2 * P * ibs_kp(d); }

int64_t ibs_backward_part_floats(int64_t P, int d) { return member_part_elems(2 * P, d, kIbsChunk, kIbsWaveMax); }

void ibs_backward(const int32_t* members, const int32_t* memrow, const int64_t* inv, const float* rows, int64_t ld,
                  int64_t cap, int d, float tau, const float* logq, const float* lse, float gscale, int64_t P,
                  float* grad_rows, float* ws, float* part, int blocks, hipStream_t s) {
  check_shape("ibs_backward", d, tau, ld, cap, P, blocks);
  if (P <= 0 || cap <= 0) return;
  const int64_t n = 2 * P;
  if (ws == nullptr || !aligned16(ws)) throw std::runtime_error("ibs_backward: ws workspace missing or unaligned");
  if (n > kIbsWaveMax && (part == nullptr || !aligned16(part)))
    throw std::runtime_error("ibs_backward: part workspace missing or unaligned");
  const bool vec = ld % 4 == 0 && aligned16(rows);
  const Args a{inv, rows, ld, cap, (int)P, d, vec, 1.f / tau, (float)((double)gscale / (double)tau), logq, lse,
               nullptr, nullptr, ws};
  dispatch_kp(d, TileLaunch{a, true, blocks, s});
  const RedArgs r{members, memrow, (int)n, cap, ws, ibs_kp(d), d, aligned16(grad_rows), grad_rows, part};
  switch (pow2ceil(d / 4)) {
    case 2: launch_reduce<2>(r, blocks, s); break;
    case 4: launch_reduce<4>(r, blocks, s); break;
    case 8: launch_reduce<8>(r, blocks, s); break;
    case 16: launch_reduce<16>(r, blocks, s); break;
    default: launch_reduce<32>(r, blocks, s); break;
  }
  MINIPS_HIP_CHECK(hipGetLastError());
}

}  // namespace minips_k
