// Compressed Interaction Network layers over the assembled Wide & Deep input (cin.h states the rule and the design):
// bf16 MFMA sweeps whose right operand -- the outer products z = X^{k-1}[i, c] X^0[j, c] -- is formed in registers.
#include <stdexcept>
#include <string>

#include "cin.h"
#include "common.h"

namespace minips_k {

namespace {

typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
constexpr int kBlock = 256;
constexpr int kWPitch = 40;          // bf16 per row of a forward W slice (32 + 8: 80-byte rows, 16-byte aligned)
constexpr int kLdsBudget = 64 * 1024;  // dynamic LDS a launch may ask for

__device__ __forceinline__ v4f mfma(v8s a, v8s b, v4f c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, b), c, 0, 0, 0);
}

__device__ __forceinline__ void unpack8(const uint4& w, float (&a)[8]) {
  const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    a[2 * i] = __uint_as_float(u[i] << 16);
    a[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
  }
}

__device__ __forceinline__ v8s pack8(const float (&a)[8]) {
  const uint4 u = make_uint4(pack_bf2(a[0], a[1]), pack_bf2(a[2], a[3]), pack_bf2(a[4], a[5]), pack_bf2(a[6], a[7]));
  return __builtin_bit_cast(v8s, u);
}

// 8 consecutive bf16 at p: one 16-byte load, or element by element
__device__ __forceinline__ uint4 load8(const bf16_t* p, bool vec) {
  if (vec) return *reinterpret_cast<const uint4*>(p);
  uint32_t u[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int e = 0; e < 8; ++e) u[e >> 1] |= (uint32_t)p[e] << (16 * (e & 1));
  return make_uint4(u[0], u[1], u[2], u[3]);
}

// z of 8 consecutive columns: bf16_rne(x0 * xp) element-wise
__device__ __forceinline__ v8s z8(const uint4& x0, const uint4& xp) {
  float a[8], b[8];
  unpack8(x0, a);
  unpack8(xp, b);
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] *= b[e];
  return pack8(a);
}

// ---------------------------------------------------------------------------------------------- forward
// NT 16-column tiles per wave (NC = 64 NT columns per workgroup), HT >= H / 16 row tiles
template <int HT, int NT>
__global__ __launch_bounds__(kBlock) void cin_fwd(const bf16_t* __restrict__ X, int64_t ldx, int64_t B, CinLayer L,
                                                  const bf16_t* __restrict__ W, bool wvec, bf16_t* XK,
                                                  int64_t ntiles) {
  extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
  constexpr int NC = 64 * NT;
  const int m = L.m, mp = (m + 7) / 8 * 8, D = L.D, Hp = L.Hp, H = L.H, xp_pitch = mp + 8;
  const int K = Hp * mp, nsteps = (K + 31) / 32, spt = NC / D;
  const int64_t sstride = (int64_t)L.Hs * D;
  bf16_t* Ws = lds;                         // [2][H][kWPitch]
  bf16_t* X0t = Ws + 2 * H * kWPitch;        // [NC][mp + 8]
  bf16_t* Xps = X0t + NC * xp_pitch;         // [Hp][NC]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;

  auto wload = [&](int ks, uint4 (&r)[2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int idx = tid + kBlock * s, row = idx >> 2, k = 32 * ks + 8 * (idx & 3);
      r[s] = (row < H && k < K) ? load8(W + (int64_t)row * K + k, wvec) : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  auto wstore = [&](int buf, const uint4 (&r)[2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int idx = tid + kBlock * s, row = idx >> 2;
      if (row < H) *reinterpret_cast<uint4*>(Ws + (buf * H + row) * kWPitch + 8 * (idx & 3)) = r[s];
    }
  };

  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t b0 = tile * spt;
    for (int idx = tid; idx < NC * xp_pitch + Hp * NC; idx += kBlock) X0t[idx] = 0;  // (X0t and Xps are adjacent)
    __syncthreads();
    for (int idx = tid; idx < spt * m * D; idx += kBlock) {
      const int s = idx / (m * D), e = idx - s * (m * D), j = e / D, c = e - j * D;
      if (b0 + s < B) {
        const bf16_t v = X[(b0 + s) * ldx + e];
        X0t[(s * D + c) * xp_pitch + j] = v;
        if (L.first) Xps[j * NC + s * D + c] = v;
      }
    }
    if (!L.first) {
      const bf16_t* xp = XK + (int64_t)L.off_prev * D;
      for (int idx = tid; idx < spt * Hp * D; idx += kBlock) {
        const int s = idx / (Hp * D), e = idx - s * (Hp * D), i = e / D, c = e - i * D;
        if (b0 + s < B) Xps[i * NC + s * D + c] = xp[(b0 + s) * sstride + e];
      }
    }
    uint4 wr[2];
    wload(0, wr);
    wstore(0, wr);
    __syncthreads();

    v4f acc[HT][NT];
#pragma unroll
    for (int t = 0; t < HT; ++t)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[t][nt] = v4f{0.f, 0.f, 0.f, 0.f};
    int cur = 0;
    for (int ks = 0; ks < nsteps; ++ks) {
      const bool has_next = ks + 1 < nsteps;
      if (has_next) wload(ks + 1, wr);
      const int kk = 32 * ks + 8 * g;
      const int i = kk / mp, j0 = kk - i * mp;
      v8s bz[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int n = wave * (16 * NT) + 16 * nt + l15;
        if (kk < K) {
          float a[8];
          unpack8(*reinterpret_cast<const uint4*>(X0t + n * xp_pitch + j0), a);
          const float xv = bf2f(Xps[i * NC + n]);
#pragma unroll
          for (int e = 0; e < 8; ++e) a[e] *= xv;
          bz[nt] = pack8(a);
        } else {
          bz[nt] = v8s{0, 0, 0, 0, 0, 0, 0, 0};
        }
      }
#pragma unroll
      for (int t = 0; t < HT; ++t) {
        if (16 * t < H) {  // (uniform)
          const v8s a = *reinterpret_cast<const v8s*>(Ws + (cur * H + 16 * t + l15) * kWPitch + 8 * g);
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) acc[t][nt] = mfma(a, bz[nt], acc[t][nt]);
        }
      }
      if (has_next) wstore(cur ^ 1, wr);
      __syncthreads();
      cur ^= 1;
    }
    bf16_t* xk = XK + (int64_t)L.off * D;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int n = wave * (16 * NT) + 16 * nt + l15, s = n / D, c = n - s * D;
      if (s >= spt || b0 + s >= B) continue;
#pragma unroll
      for (int t = 0; t < HT; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int h = 16 * t + 4 * g + q;
          if (h < H) xk[(b0 + s) * sstride + (int64_t)h * D + c] = f2bf(acc[t][nt][q]);
        }
    }
    // (the sweep's last barrier lies behind every LDS read: the next tile may restage)
  }
}

// ---------------------------------------------------------------------------------------------- output
__global__ __launch_bounds__(kBlock) void cin_out(const bf16_t* __restrict__ XK, int64_t B, int Hs, int D,
                                                  const bf16_t* __restrict__ w_out, float* __restrict__ wide,
                                                  float* __restrict__ p) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t b = wave; b < B; b += nwaves) {
    float tot = 0.f;
    for (int o = lane; o < Hs; o += 64) {
      const bf16_t* row = XK + (b * Hs + o) * D;
      float s = 0.f;
      for (int c = 0; c < D; c += 8) {
        float a[8];
        unpack8(*reinterpret_cast<const uint4*>(row + c), a);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += a[e];
      }
      p[b * Hs + o] = s;
      tot += bf2f(w_out[o]) * s;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off, 64);
    if (lane == 0) wide[b] = wide[b] + tot;
  }
}

// ---------------------------------------------------------------------------------------------- backward (data)
template <int MQ, int NT>
__global__ __launch_bounds__(kBlock) void cin_bwd(const bf16_t* __restrict__ X, int64_t ldx, int64_t B, CinLayer L,
                                                  const bf16_t* __restrict__ W, bool wvec,
                                                  const bf16_t* __restrict__ XK, bf16_t* dXK,
                                                  const bf16_t* __restrict__ w_out, const float* __restrict__ dwide,
                                                  float* g0, const int32_t* __restrict__ perm, bf16_t* dX,
                                                  int64_t ntiles) {
  extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
  constexpr int NC = 64 * NT, HS = 4, SP = MQ >= 32 ? MQ / 32 : 1;
  const int m = L.m, mp = (m + 7) / 8 * 8, D = L.D, Hp = L.Hp, H = L.H;
  const int K = Hp * mp, hpad = (H + 31) / 32 * 32, wt_pitch = hpad + 8, spt = NC / D;
  const int nper = (Hp * MQ + 32 * SP - 1) / (32 * SP);
  const int64_t sstride = (int64_t)L.Hs * D, nrows = B * m;
  bf16_t* WsT = lds;                          // [2][32][hpad + 8]
  bf16_t* Xps = WsT + 2 * 32 * wt_pitch;       // [Hp][NC]
  float* g0a = reinterpret_cast<float*>(Xps + Hp * NC);  // [m][NC], first layer only: dX^0's share of g0
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;

  auto wload = [&](int s, uint4 (&r)[2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = tid + kBlock * u, h = idx >> 2, flat = 32 * s + 8 * (idx & 3);
      const int i = flat / MQ, jj = flat & (MQ - 1);
      r[u] = (h < H && i < Hp && jj < mp) ? load8(W + (int64_t)h * K + i * mp + jj, wvec) : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  auto wstore = [&](int buf, const uint4 (&r)[2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = tid + kBlock * u, h = idx >> 2, r0 = 8 * (idx & 3);
      if (h < H) {
        const uint32_t w[4] = {r[u].x, r[u].y, r[u].z, r[u].w};
#pragma unroll
        for (int e = 0; e < 8; ++e)
          WsT[(buf * 32 + r0 + e) * wt_pitch + h] = (bf16_t)(w[e >> 1] >> (16 * (e & 1)));
      }
    }
  };

  for (int idx = tid; idx < 2 * 32 * wt_pitch; idx += kBlock) WsT[idx] = 0;  // the columns h >= H stay zero
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t b0 = tile * spt;
    __syncthreads();
    for (int idx = tid; idx < Hp * NC; idx += kBlock) Xps[idx] = 0;
    __syncthreads();
    {
      const bf16_t* xp = L.first ? X : XK + (int64_t)L.off_prev * D;
      const int64_t ld = L.first ? ldx : sstride;
      for (int idx = tid; idx < spt * Hp * D; idx += kBlock) {
        const int s = idx / (Hp * D), e = idx - s * (Hp * D), i = e / D, c = e - i * D;
        if (b0 + s < B) Xps[i * NC + s * D + c] = xp[(b0 + s) * ld + e];
      }
    }
    // the lane's columns: dz, the B operands dX^k[h = 32 hs + 8 g .., n] and X^0[jj, n] of its accumulator rows
    float dz[NT], x0r[NT][SP][2][4], g0r[NT][SP][2][4], part[NT];
    v8s bop[NT][HS];
    int64_t bn[NT];
    int cn[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int n = wave * (16 * NT) + 16 * nt + l15, s = n / D;
      cn[nt] = n - s * D;
      bn[nt] = (s < spt && b0 + s < B) ? b0 + s : -1;
      dz[nt] = bn[nt] >= 0 ? dwide[bn[nt]] : 0.f;
      part[nt] = 0.f;
#pragma unroll
      for (int hs = 0; hs < HS; ++hs) {
        float a[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int h = 32 * hs + 8 * g + e;
          a[e] = 0.f;
          if (h < H && bn[nt] >= 0)
            a[e] = L.last ? dz[nt] * bf2f(w_out[L.off + h])
                          : bf2f(dXK[bn[nt] * sstride + (int64_t)(L.off + h) * D + cn[nt]]);
        }
        bop[nt][hs] = pack8(a);
      }
#pragma unroll
      for (int sp = 0; sp < SP; ++sp)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int jj = (32 * sp + 16 * mt + 4 * g + q) & (MQ - 1);
            g0r[nt][sp][mt][q] = 0.f;
            x0r[nt][sp][mt][q] = (jj < m && bn[nt] >= 0) ? bf2f(X[bn[nt] * ldx + jj * D + cn[nt]]) : 0.f;
          }
    }
    uint4 wr[2];
    wload(0, wr);
    wstore(0, wr);
    __syncthreads();
    int cur = 0;
    for (int per = 0; per < nper; ++per) {
#pragma unroll
      for (int sp = 0; sp < SP; ++sp) {
        const int s = per * SP + sp;
        const bool has_next = s + 1 < nper * SP;
        if (has_next) wload(s + 1, wr);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          v4f acc[NT];
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) acc[nt] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int hs = 0; hs < HS; ++hs) {
            if (32 * hs < H) {  // (uniform)
              const v8s a =
                  *reinterpret_cast<const v8s*>(WsT + (cur * 32 + 16 * mt + l15) * wt_pitch + 32 * hs + 8 * g);
#pragma unroll
              for (int nt = 0; nt < NT; ++nt) acc[nt] = mfma(a, bop[nt][hs], acc[nt]);
            }
          }
          const int i = (32 * s + 16 * mt + 4 * g) / MQ;  // the one i of the lane's four rows
          // the rows of one i end with this tile: always below MQ = 32, at mt = 1 for 32, at (sp, mt) = (1, 1) for 64
          const bool group_end = MQ <= 16 || (mt == 1 && sp == SP - 1);
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            const float xv = i < Hp ? bf2f(Xps[i * NC + wave * (16 * NT) + 16 * nt + l15]) : 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              part[nt] += acc[nt][q] * x0r[nt][sp][mt][q];
              g0r[nt][sp][mt][q] += acc[nt][q] * xv;
            }
            if (group_end) {
              float v = part[nt];
              v += __shfl_xor(v, 16, 64);
              if (MQ >= 16) v += __shfl_xor(v, 32, 64);
              const bool owner = MQ >= 16 ? g == 0 : (g & 1) == 0;
              if (owner && i < Hp && bn[nt] >= 0) {
                if (L.first)
                  g0a[i * NC + wave * (16 * NT) + 16 * nt + l15] = v;
                else
                  dXK[bn[nt] * sstride + (int64_t)(L.off_prev + i) * D + cn[nt]] =
                      f2bf(v + dz[nt] * bf2f(w_out[L.off_prev + i]));
              }
              part[nt] = 0.f;
            }
          }
        }
        if (has_next) wstore(cur ^ 1, wr);
        __syncthreads();
        cur ^= 1;
      }
    }
    // g0 of the lane's (jj, column) pairs
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int sp = 0; sp < SP; ++sp)
#pragma unroll
        for (int mt = 0; mt < (MQ <= 16 ? 1 : 2); ++mt)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int jj = (32 * sp + 16 * mt + 4 * g + q) & (MQ - 1);
            float v = g0r[nt][sp][mt][q];
            if (MQ <= 16) v += g0r[nt][sp][1][q];
            if (MQ == 8) v += __shfl_xor(v, 32, 64);
            if ((MQ == 8 && g >= 2) || jj >= m || bn[nt] < 0) continue;
            const int64_t gi = (bn[nt] * m + jj) * D + cn[nt];
            if (L.first) v += g0a[jj * NC + wave * (16 * NT) + 16 * nt + l15];
            if (!L.last) v += g0[gi];
            if (!L.first) {
              g0[gi] = v;
            } else {
              const int64_t lk = bn[nt] * m + jj;
              const int64_t r = perm ? (int64_t)perm[lk] : lk;
              if ((uint64_t)r < (uint64_t)nrows) {
                bf16_t* gp = dX + r * D + cn[nt];
                *gp = f2bf(bf2f(*gp) + v);
              }
            }
          }
  }
}

// ---------------------------------------------------------------------------------------------- weight gradient
template <int HT>
__global__ __launch_bounds__(kBlock) void cin_wgrad(const bf16_t* __restrict__ X, int64_t ldx, int64_t B, CinLayer L,
                                                    bool xvec, const bf16_t* __restrict__ XK,
                                                    const bf16_t* __restrict__ dXK, const bf16_t* __restrict__ w_out,
                                                    const float* __restrict__ dwide, int64_t chunk,
                                                    float* __restrict__ part) {
  constexpr int KT = 2;
  const int m = L.m, mp = (m + 7) / 8 * 8, D = L.D, Hp = L.Hp, H = L.H, K = Hp * mp;
  const int64_t sstride = (int64_t)L.Hs * D;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, l15 = lane & 15;
  const int64_t ch = blockIdx.y, b0 = ch * chunk, b1 = b0 + chunk < B ? b0 + chunk : B;
  const int64_t ncol = (b1 - b0) * D;  // the chunk's flattened (b, c) columns: the reduction
  int ki[KT], kj[KT];
  bool kv[KT];
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) {
    const int kidx = (blockIdx.x * 4 + wave) * (16 * KT) + 16 * kt + l15;
    ki[kt] = kidx / mp;
    kj[kt] = kidx - ki[kt] * mp;
    kv[kt] = kidx < K && kj[kt] < m;
  }
  v4f acc[HT][KT];
#pragma unroll
  for (int t = 0; t < HT; ++t)
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) acc[t][kt] = v4f{0.f, 0.f, 0.f, 0.f};
  for (int64_t col0 = 0; col0 < ncol; col0 += 32) {
    const int64_t col = col0 + 8 * g;
    const bool cv = col < ncol;  // (D % 8 == 0: an octet lies inside one sample)
    const int64_t b = b0 + (cv ? col / D : 0);
    const int c = cv ? (int)(col % D) : 0;
    v8s bz[KT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      bz[kt] = v8s{0, 0, 0, 0, 0, 0, 0, 0};
      if (cv && kv[kt]) {
        const uint4 x0 = load8(X + b * ldx + kj[kt] * D + c, xvec);
        const bf16_t* prev = XK + b * sstride + (int64_t)(L.off_prev + ki[kt]) * D + c;
        const uint4 xp =
            L.first ? load8(X + b * ldx + ki[kt] * D + c, xvec) : *reinterpret_cast<const uint4*>(prev);
        bz[kt] = z8(x0, xp);
      }
    }
    const float dzb = (cv && L.last) ? dwide[b] : 0.f;
#pragma unroll
    for (int t = 0; t < HT; ++t) {
      if (16 * t < H) {  // (uniform)
        const int h = 16 * t + l15;
        v8s a = v8s{0, 0, 0, 0, 0, 0, 0, 0};
        if (cv) {
          if (L.last) {
            const uint32_t v = pack_bf2(dzb * bf2f(w_out[L.off + h]), 0.f) & 0xffffu;
            const uint32_t vv = v | (v << 16);
            a = __builtin_bit_cast(v8s, make_uint4(vv, vv, vv, vv));
          } else {
            a = __builtin_bit_cast(
                v8s, *reinterpret_cast<const uint4*>(dXK + b * sstride + (int64_t)(L.off + h) * D + c));
          }
        }
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) acc[t][kt] = mfma(a, bz[kt], acc[t][kt]);
      }
    }
  }
  float* out = part + ch * (int64_t)H * K;
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) {
    const int kidx = (blockIdx.x * 4 + wave) * (16 * KT) + 16 * kt + l15;
    if (kidx >= K) continue;
#pragma unroll
    for (int t = 0; t < HT; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int h = 16 * t + 4 * g + q;
        if (h < H) out[(int64_t)h * K + kidx] = acc[t][kt][q];
      }
  }
}

__global__ __launch_bounds__(kBlock) void cin_wout(const float* __restrict__ dwide, const float* __restrict__ p,
                                                   int64_t B, int Hs, int64_t chunk, float* __restrict__ part) {
  const int64_t ch = blockIdx.x, b0 = ch * chunk, b1 = b0 + chunk < B ? b0 + chunk : B;
  for (int o = threadIdx.x; o < Hs; o += kBlock) {
    float s = 0.f;
    for (int64_t b = b0; b < b1; ++b) s += dwide[b] * p[b * Hs + o];
    part[ch * Hs + o] = s;
  }
}

__global__ __launch_bounds__(kBlock) void cin_fold(const float* __restrict__ part, int64_t nchunks, int64_t n,
                                                   float* __restrict__ G) {
  const int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int64_t ch = 0; ch < nchunks; ++ch) s += part[ch * n + i];
  G[i] = G[i] + s;
}

// ---------------------------------------------------------------------------------------------- launchers
void check_layer(const char* op, int64_t ldx, int64_t B, const CinLayer& L, int blocks) {
  const std::string o(op);
  if (L.m < 1 || L.m > kCinMaxM) throw std::runtime_error(o + ": F outside [1, 64]");
  if (L.D < 8 || L.D > kCinMaxD || L.D % 8) throw std::runtime_error(o + ": D must be a multiple of 8 in [8, 64]");
  if (L.H < 16 || L.H > kCinMaxH || L.H % 16) throw std::runtime_error(o + ": layers outside the rule (H)");
  if (L.first ? L.Hp != L.m : (L.Hp < 16 || L.Hp > kCinMaxH || L.Hp % 16))
    throw std::runtime_error(o + ": layers outside the rule (H of the layer below)");
  if (L.Hs > kCinMaxT * kCinMaxH || L.off < 0 || L.off + L.H > L.Hs ||
      (!L.first && (L.off_prev < 0 || L.off_prev + L.Hp > L.off)))
    throw std::runtime_error(o + ": layers: offsets outside the stacked buffer");
  if ((int64_t)L.m * L.D > ldx) throw std::runtime_error(o + ": X has fewer than F D columns");
  if (blocks < 0 || blocks > kCinMaxBlocks) throw std::runtime_error(o + ": blocks outside [0, 65535]");
  if (B < 0 || B >= (1ll << 31) / (L.Hs * L.D)) throw std::runtime_error(o + ": B Hs D must be below 2^31");
}

inline int fwd_lds(const CinLayer& L, int nc) {
  return 2 * (2 * L.H * kWPitch + nc * (cin_mp(L.m) + 8) + L.Hp * nc);  // (two W slices)
}
inline int bwd_lds(const CinLayer& L, int nc) {
  const int hpad = (L.H + 31) / 32 * 32;
  return 2 * (64 * (hpad + 8) + L.Hp * nc) + (L.first ? 4 * L.m * nc : 0);
}

template <int HT, int NT>
void launch_fwd(const bf16_t* X, int64_t ldx, int64_t B, const CinLayer& L, const bf16_t* W, bf16_t* XK, int blocks,
                hipStream_t s) {
  const int64_t ntiles = (B + (64 * NT) / L.D - 1) / ((64 * NT) / L.D);
  const int grid = blocks > 0 ? blocks : (int)(ntiles < 2048 ? ntiles : 2048);
  hipLaunchKernelGGL((cin_fwd<HT, NT>), grid, kBlock, fwd_lds(L, 64 * NT), s, X, ldx, B, L, W, aligned16(W), XK,
                     ntiles);
}

template <int HT>
void launch_fwd_nt(const bf16_t* X, int64_t ldx, int64_t B, const CinLayer& L, const bf16_t* W, bf16_t* XK, int blocks,
                   hipStream_t s) {
  if (fwd_lds(L, 256) <= kLdsBudget) return launch_fwd<HT, 4>(X, ldx, B, L, W, XK, blocks, s);
  if (fwd_lds(L, 128) <= kLdsBudget) return launch_fwd<HT, 2>(X, ldx, B, L, W, XK, blocks, s);
  launch_fwd<HT, 1>(X, ldx, B, L, W, XK, blocks, s);  // 46 KB at the largest shapes
}

struct BwdArgs {
  const bf16_t* X;
  int64_t ldx, B;
  const CinLayer& L;
  const bf16_t *W, *XK;
  bf16_t* dXK;
  const bf16_t* w_out;
  const float* dwide;
  float* g0;
  const int32_t* perm;
  bf16_t* dX;
  int blocks;
  hipStream_t s;
};

template <int MQ, int NT>
void launch_bwd(const BwdArgs& a) {
  const int64_t ntiles = (a.B + (64 * NT) / a.L.D - 1) / ((64 * NT) / a.L.D);
  const int grid = a.blocks > 0 ? a.blocks : (int)(ntiles < 2048 ? ntiles : 2048);
  hipLaunchKernelGGL((cin_bwd<MQ, NT>), grid, kBlock, bwd_lds(a.L, 64 * NT), a.s, a.X, a.ldx, a.B, a.L, a.W,
                     aligned16(a.W), a.XK, a.dXK, a.w_out, a.dwide, a.g0, a.perm, a.dX, ntiles);
}

template <int MQ>
void launch_bwd_nt(const BwdArgs& a) {
  if (bwd_lds(a.L, 128) <= kLdsBudget) return launch_bwd<MQ, 2>(a);
  launch_bwd<MQ, 1>(a);  // 50 KB at the largest shapes
}

}  // namespace

void wd_cin_layer_forward(const uint16_t* X, int64_t ldx, int64_t B, const CinLayer& L, const uint16_t* W,
                          uint16_t* XK, int blocks, hipStream_t s) {
  check_layer("wd_cin_layer_forward", ldx, B, L, blocks);
  if (!aligned16(XK)) throw std::runtime_error("wd_cin_layer_forward: XK must be 16-byte aligned");
  if (B <= 0) return;
  if (L.H <= 32)
    launch_fwd_nt<2>(X, ldx, B, L, W, XK, blocks, s);
  else if (L.H <= 64)
    launch_fwd_nt<4>(X, ldx, B, L, W, XK, blocks, s);
  else
    launch_fwd_nt<8>(X, ldx, B, L, W, XK, blocks, s);
  MINIPS_HIP_CHECK(hipGetLastError());
}

void wd_cin_output(const uint16_t* XK, int64_t B, int Hs, int D, const uint16_t* w_out, float* wide, float* p,
                   int blocks, hipStream_t s) {
  if (Hs < 16 || Hs > kCinMaxT * kCinMaxH || D < 8 || D > kCinMaxD || D % 8)
    throw std::runtime_error("wd_cin_output: layers or D outside the rule");
  if (blocks < 0 || blocks > kCinMaxBlocks) throw std::runtime_error("wd_cin_output: blocks outside [0, 65535]");
  if (!aligned16(XK)) throw std::runtime_error("wd_cin_output: XK must be 16-byte aligned");
  if (B <= 0) return;
  const int grid = blocks > 0 ? blocks : grid_for(B * 64, kBlock, 2048);
  hipLaunchKernelGGL(cin_out, grid, kBlock, 0, s, XK, B, Hs, D, w_out, wide, p);
  MINIPS_HIP_CHECK(hipGetLastError());
}

void wd_cin_layer_backward(const uint16_t* X, int64_t ldx, int64_t B, const CinLayer& L, const uint16_t* W,
                           const uint16_t* XK, uint16_t* dXK, const uint16_t* w_out, const float* dwide, float* g0,
                           const int32_t* perm, uint16_t* dX, int blocks, hipStream_t s) {
  check_layer("wd_cin_layer_backward", ldx, B, L, blocks);
  if (!(L.first && L.last) && g0 == nullptr) throw std::runtime_error("wd_cin_layer_backward: g0 is missing");
  if (B >= (1ll << 31) / L.m) throw std::runtime_error("wd_cin_layer_backward: B F must be below 2^31");
  if (B <= 0) return;
  const BwdArgs a{X, ldx, B, L, W, XK, dXK, w_out, dwide, g0, perm, dX, blocks, s};
  const int mp = cin_mp(L.m);
  if (mp <= 8)
    launch_bwd_nt<8>(a);
  else if (mp <= 16)
    launch_bwd_nt<16>(a);
  else if (mp <= 32)
    launch_bwd_nt<32>(a);
  else
    launch_bwd_nt<64>(a);
  MINIPS_HIP_CHECK(hipGetLastError());
}

void wd_cin_layer_wgrad(const uint16_t* X, int64_t ldx, int64_t B, const CinLayer& L, const uint16_t* XK,
                        const uint16_t* dXK, const uint16_t* w_out, const float* dwide, float* part, hipStream_t s) {
  check_layer("wd_cin_layer_wgrad", ldx, B, L, 0);
  if (!aligned16(XK) || !aligned16(dXK))
    throw std::runtime_error("wd_cin_layer_wgrad: XK and dXK must be 16-byte aligned");
  if (B <= 0) return;
  const int K = L.Hp * cin_mp(L.m);
  const dim3 grid((K + 127) / 128, (unsigned)cin_nchunks(B));
  const bool xvec = ldx % 8 == 0 && aligned16(X);
  const int64_t chunk = cin_chunk(B);
  if (L.H <= 32)
    hipLaunchKernelGGL(cin_wgrad<2>, grid, kBlock, 0, s, X, ldx, B, L, xvec, XK, dXK, w_out, dwide, chunk, part);
  else if (L.H <= 64)
    hipLaunchKernelGGL(cin_wgrad<4>, grid, kBlock, 0, s, X, ldx, B, L, xvec, XK, dXK, w_out, dwide, chunk, part);
  else
    hipLaunchKernelGGL(cin_wgrad<8>, grid, kBlock, 0, s, X, ldx, B, L, xvec, XK, dXK, w_out, dwide, chunk, part);
  MINIPS_HIP_CHECK(hipGetLastError());
}

void wd_cin_wout_partial(const float* dwide, const float* p, int64_t B, int Hs, float* part, hipStream_t s) {
  if (Hs < 16 || Hs > kCinMaxT * kCinMaxH) throw std::runtime_error("wd_cin_wout_partial: layers outside the rule");
  if (B <= 0) return;
  hipLaunchKernelGGL(cin_wout, (unsigned)cin_nchunks(B), kBlock, 0, s, dwide, p, B, Hs, cin_chunk(B), part);
  MINIPS_HIP_CHECK(hipGetLastError());
}

void wd_cin_fold(const float* part, int64_t nchunks, int64_t n, float* G, hipStream_t s) {
  if (nchunks < 0 || nchunks > kCinMaxChunks) throw std::runtime_error("wd_cin_fold: nchunks outside [0, 64]");
  if (n < 0 || n >= (1ll << 31)) throw std::runtime_error("wd_cin_fold: n outside [0, 2^31)");
  if (nchunks == 0 || n == 0) return;
  hipLaunchKernelGGL(cin_fold, (unsigned)((n + kBlock - 1) / kBlock), kBlock, 0, s, part, nchunks, n, G);
  MINIPS_HIP_CHECK(hipGetLastError());
}

}  // namespace minips_k
