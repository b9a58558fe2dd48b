// Deep & Cross layers over the assembled Wide & Deep input (dcn.h states the rule and the mapping). Three
// memory-bound kernels: the forward and the backward stream X once, one wave per sample, with the L+1 weight rows a
// lane needs held in registers as packed bf16 (vector form); the fold adds the per-chunk partial batch sums.
#include <stdexcept>
#include <string>

#include "common.h"
#include "dcn.h"

namespace minips_k {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

// row of w_j in Pc: w_0, b_0, ..., w_{L-1}, b_{L-1}, w_c -- j = L is w_c
__device__ __forceinline__ int wrow(int j) { return 2 * j; }

// 8 bf16 at p, of which the first n (> 0) exist: one 16-byte load, or element by element into zeros
__device__ __forceinline__ uint4 load_piece(const bf16_t* p, int n) {
  if (n >= 8) return *reinterpret_cast<const uint4*>(p);
  uint32_t u[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (e < n) u[e >> 1] |= (uint32_t)p[e] << (16 * (e & 1));
  return make_uint4(u[0], u[1], u[2], u[3]);
}

// a lane's pieces of one row of X (zeros where the lane owns no column)
template <int NP>
__device__ __forceinline__ void load_x(const bf16_t* __restrict__ xb, int lane, int d, uint4 (&q)[NP]) {
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int c0 = 8 * (lane + 64 * i);
    q[i] = c0 < d ? load_piece(xb + c0, d - c0) : make_uint4(0u, 0u, 0u, 0u);
  }
}

__device__ __forceinline__ void unpack(const uint4& w, float (&a)[8]) {
  const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    a[2 * i] = __uint_as_float(u[i] << 16);
    a[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
  }
}

__device__ __forceinline__ float fold64(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the forward's scalar rule: c of (p, k)
template <int L1>
__device__ __forceinline__ float fwd_rule(const float (&p)[L1], const float (&k)[L1]) {
#pragma clang fp contract(off)
  float a = 1.f;
#pragma unroll
  for (int l = 0; l < L1 - 1; ++l) {
    const float t = a * p[l];
    const float s = t + k[l];
    a = a + s;
  }
  const float t = a * p[L1 - 1];
  return t + k[L1 - 1];
}

// the backward's scalar rule: ds_j (ds_L = dz) and m_j = ds_j a_j
template <int L1>
__device__ __forceinline__ void bwd_rule(const float (&p)[L1], const float (&k)[L1], float dz, float (&m)[L1],
                                         float (&ds)[L1]) {
#pragma clang fp contract(off)
  constexpr int L = L1 - 1;
  float a[L1];
  a[0] = 1.f;
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const float t = a[l] * p[l];
    const float s = t + k[l];
    a[l + 1] = a[l] + s;
  }
  ds[L] = dz;
  float r = dz * p[L];
#pragma unroll
  for (int l = L - 1; l >= 0; --l) {
    ds[l] = r;
    const float t = ds[l] * p[l];
    r = r + t;
  }
#pragma unroll
  for (int j = 0; j < L1; ++j) m[j] = ds[j] * a[j];
}

// ---------------------------------------------------------------------------------------------- forward
template <int NP, int L1>
__global__ __launch_bounds__(kBlock) void cross_fwd_vec(const bf16_t* __restrict__ X, int64_t ldx, int64_t B, int d,
                                                        const bf16_t* __restrict__ Pc, int dp,
                                                        float* __restrict__ wide, float* __restrict__ p,
                                                        float* __restrict__ k) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  uint4 wq[L1][NP];
  float kk[L1];
#pragma unroll
  for (int j = 0; j < L1; ++j) kk[j] = 0.f;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int c0 = 8 * (lane + 64 * i);
    float bacc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bacc[e] = 0.f;
#pragma unroll
    for (int j = 0; j < L1; ++j) {
      wq[j][i] = c0 < d ? load_piece(Pc + (int64_t)wrow(j) * dp + c0, d - c0) : make_uint4(0u, 0u, 0u, 0u);
      if (c0 < d) {
        float w[8];
        unpack(wq[j][i], w);
#pragma unroll
        for (int e = 0; e < 8; ++e) kk[j] += bacc[e] * w[e];
        if (j < L1 - 1) {
          float bb[8];
          unpack(load_piece(Pc + (int64_t)(wrow(j) + 1) * dp + c0, d - c0), bb);
#pragma unroll
          for (int e = 0; e < 8; ++e) bacc[e] += bb[e];
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < L1; ++j) kk[j] = fold64(kk[j]);
  if (wave == 0 && lane == 0) {
#pragma unroll
    for (int j = 0; j < L1; ++j) k[j] = kk[j];
  }
  uint4 xq[NP], xn[NP];  // this sample's pieces and the next one's, loaded one sample ahead
  if (wave < B) load_x<NP>(X + wave * ldx, lane, d, xq);
  for (int64_t b = wave; b < B; b += nwaves) {
    if (b + nwaves < B) load_x<NP>(X + (b + nwaves) * ldx, lane, d, xn);
    float acc[L1];
#pragma unroll
    for (int j = 0; j < L1; ++j) acc[j] = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int c0 = 8 * (lane + 64 * i);
      if (c0 < d) {
        float x[8];
        unpack(xq[i], x);
#pragma unroll
        for (int j = 0; j < L1; ++j) {
          float w[8];
          unpack(wq[j][i], w);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[j] += x[e] * w[e];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < L1; ++j) acc[j] = fold64(acc[j]);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < L1; ++j) p[b * L1 + j] = acc[j];
      wide[b] = wide[b] + fwd_rule<L1>(acc, kk);
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) xq[i] = xn[i];
  }
}

template <int L1>
__global__ __launch_bounds__(kBlock) void cross_fwd_scalar(const bf16_t* __restrict__ X, int64_t ldx, int64_t B, int d,
                                                           const bf16_t* __restrict__ Pc, int dp,
                                                           float* __restrict__ wide, float* __restrict__ p,
                                                           float* __restrict__ k) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  float kk[L1];
#pragma unroll
  for (int j = 0; j < L1; ++j) kk[j] = 0.f;
  for (int c = lane; c < d; c += 64) {
    float bacc = 0.f;
#pragma unroll
    for (int j = 0; j < L1; ++j) {
      kk[j] += bacc * bf2f(Pc[(int64_t)wrow(j) * dp + c]);
      if (j < L1 - 1) bacc += bf2f(Pc[(int64_t)(wrow(j) + 1) * dp + c]);
    }
  }
#pragma unroll
  for (int j = 0; j < L1; ++j) kk[j] = fold64(kk[j]);
  if (wave == 0 && lane == 0) {
#pragma unroll
    for (int j = 0; j < L1; ++j) k[j] = kk[j];
  }
  for (int64_t b = wave; b < B; b += nwaves) {
    const bf16_t* xb = X + b * ldx;
    float acc[L1];
#pragma unroll
    for (int j = 0; j < L1; ++j) acc[j] = 0.f;
    for (int c = lane; c < d; c += 64) {
      const float x = bf2f(xb[c]);
#pragma unroll
      for (int j = 0; j < L1; ++j) acc[j] += x * bf2f(Pc[(int64_t)wrow(j) * dp + c]);
    }
#pragma unroll
    for (int j = 0; j < L1; ++j) acc[j] = fold64(acc[j]);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < L1; ++j) p[b * L1 + j] = acc[j];
      wide[b] = wide[b] + fwd_rule<L1>(acc, kk);
    }
  }
}

// ---------------------------------------------------------------------------------------------- backward
// the rule's inputs of sample b, read uniformly by every lane
template <int L1>
__device__ __forceinline__ void sample_rule(const float* __restrict__ p, const float (&kk)[L1],
                                            const float* __restrict__ dwide, int64_t b, float (&m)[L1],
                                            float (&ds)[L1]) {
  float pj[L1];
#pragma unroll
  for (int j = 0; j < L1; ++j) pj[j] = p[b * L1 + j];
  bwd_rule<L1>(pj, kk, dwide[b], m, ds);
}

// a lane's pieces of sample b's dX rows (vector form, D % 8 == 0: a piece lies inside one field's row): the element
// offset of each piece, -1 where the lane owns no embedding column or the lookup's perm entry is out of range
template <int NP>
__device__ __forceinline__ void load_dx(const bf16_t* dX, const int32_t* __restrict__ perm, int64_t b, int64_t n,
                                        int F, int D, int FD, int lane, int64_t (&go)[NP], uint4 (&gq)[NP]) {
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int c0 = 8 * (lane + 64 * i);
    go[i] = -1;
    gq[i] = make_uint4(0u, 0u, 0u, 0u);
    if (c0 < FD) {
      const int f = c0 / D;
      const int64_t q = b * F + f;
      const int64_t r = perm ? (int64_t)perm[q] : q;
      if ((uint64_t)r < (uint64_t)n) {
        go[i] = r * D + (c0 - f * D);
        gq[i] = *reinterpret_cast<const uint4*>(dX + go[i]);
      }
    }
  }
}

// the four waves' scalar sums -> the chunk's trailer (call between the two barriers of a fold)
template <int L1>
__device__ __forceinline__ void store_sd(const float (*sds)[8], float* __restrict__ prow, int dp) {
#pragma clang fp contract(off)
  if (threadIdx.x < L1) {
    const int j = threadIdx.x;
    prow[(int64_t)L1 * dp + j] = ((sds[0][j] + sds[1][j]) + sds[2][j]) + sds[3][j];
  }
}

template <int NP, int L1>
__global__ __launch_bounds__(kBlock) void cross_bwd_vec(const bf16_t* __restrict__ X, int64_t ldx, int64_t B, int d,
                                                        const float* __restrict__ p, const float* __restrict__ k,
                                                        const float* __restrict__ dwide,
                                                        const bf16_t* __restrict__ Pc, int dp,
                                                        const int32_t* __restrict__ perm, bf16_t* __restrict__ dX,
                                                        int F, int D, float* __restrict__ part, int64_t pcols,
                                                        int64_t nchunks) {
#pragma clang fp contract(off)
  __shared__ float lds[kWaves][kDcnMaxD];
  __shared__ float sds[kWaves][8];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int FD = F * D;
  const int64_t n = B * F;
  uint4 wq[L1][NP];
  float kk[L1];
#pragma unroll
  for (int j = 0; j < L1; ++j) kk[j] = k[j];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int c0 = 8 * (lane + 64 * i);
#pragma unroll
    for (int j = 0; j < L1; ++j)
      wq[j][i] = c0 < FD ? load_piece(Pc + (int64_t)wrow(j) * dp + c0, d - c0) : make_uint4(0u, 0u, 0u, 0u);
  }
  for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    float acc[L1][NP][8], sd[L1];
#pragma unroll
    for (int j = 0; j < L1; ++j) {
      sd[j] = 0.f;
#pragma unroll
      for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[j][i][e] = 0.f;
    }
    uint4 xq[NP], xn[NP];  // this sample's pieces and the next one's, loaded one sample ahead
    const int64_t b0 = ch * kDcnChunk + w;
    const int64_t bend = (ch + 1) * kDcnChunk < B ? (ch + 1) * kDcnChunk : B;
    int64_t go[NP], gon[NP];  // likewise the element offsets of its dX pieces (-1: skipped) and their values
    uint4 gq[NP], gqn[NP];
    if (b0 < bend) {
      load_x<NP>(X + b0 * ldx, lane, d, xq);
      load_dx<NP>(dX, perm, b0, n, F, D, FD, lane, go, gq);
    }
    for (int64_t b = b0; b < bend; b += kWaves) {  // (wave-uniform)
      if (b + kWaves < bend) {  // (a permutation sends the next sample's lookups to other rows than this one's)
        load_x<NP>(X + (b + kWaves) * ldx, lane, d, xn);
        load_dx<NP>(dX, perm, b + kWaves, n, F, D, FD, lane, gon, gqn);
      }
      float m[L1], ds[L1];
      sample_rule<L1>(p, kk, dwide, b, m, ds);
#pragma unroll
      for (int j = 0; j < L1; ++j) sd[j] = sd[j] + ds[j];
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int c0 = 8 * (lane + 64 * i);
        if (c0 >= d) continue;
        float x[8];
        unpack(xq[i], x);
#pragma unroll
        for (int j = 0; j < L1; ++j)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float t2 = m[j] * x[e];
            acc[j][i][e] = acc[j][i][e] + t2;
          }
        if (c0 < FD) {
          if (go[i] >= 0) {  // otherwise nothing of that row is touched
            float g[8], wv[8], gx[8];
            unpack(wq[0][i], wv);
#pragma unroll
            for (int e = 0; e < 8; ++e) g[e] = m[0] * wv[e];
#pragma unroll
            for (int j = 1; j < L1; ++j) {
              unpack(wq[j][i], wv);
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                const float t2 = m[j] * wv[e];
                g[e] = g[e] + t2;
              }
            }
            unpack(gq[i], gx);
#pragma unroll
            for (int e = 0; e < 8; ++e) gx[e] = gx[e] + g[e];
            *reinterpret_cast<uint4*>(dX + go[i]) = make_uint4(pack_bf2(gx[0], gx[1]), pack_bf2(gx[2], gx[3]),
                                                       pack_bf2(gx[4], gx[5]), pack_bf2(gx[6], gx[7]));
          }
        }
      }
#pragma unroll
      for (int i = 0; i < NP; ++i) xq[i] = xn[i], go[i] = gon[i], gq[i] = gqn[i];
    }
    // the four waves' accumulators, folded through LDS in wave order, one row j at a time
    float* prow = part + ch * pcols;
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < L1; ++j) sds[w][j] = sd[j];
    }
#pragma unroll
    for (int j = 0; j < L1; ++j) {
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int c0 = 8 * (lane + 64 * i);
        if (c0 < d) {
#pragma unroll
          for (int e = 0; e < 8; ++e) lds[w][c0 + e] = acc[j][i][e];
        }
      }
      __syncthreads();
      for (int c = threadIdx.x; c < dp; c += kBlock)
        prow[(int64_t)j * dp + c] = ((lds[0][c] + lds[1][c]) + lds[2][c]) + lds[3][c];
      if (j == 0) store_sd<L1>(sds, prow, dp);
      __syncthreads();
    }
  }
}

// one column per lane-step: per block of 64 columns the wave walks its samples again (p, dwide and the scalar rule are
// re-read per block), so the accumulators stay L+1 registers for any d
template <int L1>
__global__ __launch_bounds__(kBlock) void cross_bwd_scalar(const bf16_t* __restrict__ X, int64_t ldx, int64_t B, int d,
                                                           const float* __restrict__ p, const float* __restrict__ k,
                                                           const float* __restrict__ dwide,
                                                           const bf16_t* __restrict__ Pc, int dp,
                                                           const int32_t* __restrict__ perm, bf16_t* __restrict__ dX,
                                                           int F, int D, float* __restrict__ part, int64_t pcols,
                                                           int64_t nchunks) {
#pragma clang fp contract(off)
  __shared__ float lds[kWaves][8][64];
  __shared__ float sds[kWaves][8];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int FD = F * D;
  const int64_t n = B * F;
  float kk[L1];
#pragma unroll
  for (int j = 0; j < L1; ++j) kk[j] = k[j];
  for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    float* prow = part + ch * pcols;
    for (int cb = 0; cb < dp; cb += 64) {
      const int c = cb + lane;
      float acc[L1], sd[L1], wv[L1];
#pragma unroll
      for (int j = 0; j < L1; ++j) {
        acc[j] = 0.f, sd[j] = 0.f;
        wv[j] = c < FD ? bf2f(Pc[(int64_t)wrow(j) * dp + c]) : 0.f;
      }
      for (int t = 0; t < kDcnChunk / kWaves; ++t) {
        const int64_t b = ch * kDcnChunk + w + kWaves * t;
        if (b >= B) break;  // (wave-uniform)
        float m[L1], ds[L1];
        sample_rule<L1>(p, kk, dwide, b, m, ds);
#pragma unroll
        for (int j = 0; j < L1; ++j) sd[j] = sd[j] + ds[j];
        if (c >= d) continue;
        const float x = bf2f(X[b * ldx + c]);
#pragma unroll
        for (int j = 0; j < L1; ++j) {
          const float t2 = m[j] * x;
          acc[j] = acc[j] + t2;
        }
        if (c < FD) {
          const int f = c / D;
          const int64_t q = b * F + f;
          const int64_t r = perm ? (int64_t)perm[q] : q;
          if ((uint64_t)r < (uint64_t)n) {
            float g = m[0] * wv[0];
#pragma unroll
            for (int j = 1; j < L1; ++j) {
              const float t2 = m[j] * wv[j];
              g = g + t2;
            }
            bf16_t* gp = dX + r * D + (c - f * D);
            *gp = f2bf(bf2f(*gp) + g);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < L1; ++j) lds[w][j][lane] = acc[j];
      if (cb == 0 && lane == 0) {
#pragma unroll
        for (int j = 0; j < L1; ++j) sds[w][j] = sd[j];
      }
      __syncthreads();
      for (int i = threadIdx.x; i < L1 * 64; i += kBlock) {
        const int j = i >> 6, cl = i & 63;
        if (cb + cl < dp)
          prow[(int64_t)j * dp + cb + cl] = ((lds[0][j][cl] + lds[1][j][cl]) + lds[2][j][cl]) + lds[3][j][cl];
      }
      if (cb == 0) store_sd<L1>(sds, prow, dp);
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------------------------------------- fold
// wave j of a workgroup is row j of 64 columns: T_jc and Sd_j in chunk order, then the rule's gradients
template <int L1>
__global__ __launch_bounds__(64 * L1) void cross_fold_kernel(const float* __restrict__ part, int64_t pcols,
                                                             int64_t nchunks, const bf16_t* __restrict__ Pc, int d,
                                                             int dp, float* __restrict__ Gc) {
#pragma clang fp contract(off)
  constexpr int L = L1 - 1;
  __shared__ float sds[8];
  const int lane = threadIdx.x & 63, j = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const bool act = c < d;
  float T = 0.f, s = 0.f;
  const float* pt = part + (int64_t)j * dp + (act ? c : 0);
  const float* ps = part + (int64_t)L1 * dp + j;
#pragma unroll 16
  for (int64_t ch = 0; ch < nchunks; ++ch) {
    T = T + pt[ch * pcols];
    s = s + ps[ch * pcols];
  }
  if (lane == 0) sds[j] = s;
  __syncthreads();
  if (!act) return;
  float Bc = 0.f;  // B_jc
  for (int l = 0; l < j; ++l) Bc = Bc + bf2f(Pc[(int64_t)(wrow(l) + 1) * dp + c]);
  const float t = Bc * sds[j];
  const float dw = T + t;
  float* gw = Gc + (int64_t)wrow(j) * dp + c;
  *gw = *gw + dw;
  if (j < L) {  // db_j = Sd_L w_Lc + Sd_{L-1} w_{L-1,c} + ... + Sd_{j+1} w_{j+1,c}, added in that order
    float r = sds[L] * bf2f(Pc[(int64_t)wrow(L) * dp + c]);
    for (int l = L - 1; l > j; --l) {
      const float t2 = sds[l] * bf2f(Pc[(int64_t)wrow(l) * dp + c]);
      r = r + t2;
    }
    float* gb = Gc + (int64_t)(wrow(j) + 1) * dp + c;
    *gb = *gb + r;
  }
}

// workgroups of kBlock threads of kernel f that the current device holds at once (1024 if it will not say)
inline int resident_blocks(const void* f) {
  int dev = 0, cus = 0, per = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, f, kBlock, 0) != hipSuccess || cus < 1 || per < 1) {
    (void)hipGetLastError();
    return 1024;
  }
  return cus * per;
}

void check_shape(const char* op, int64_t ldx, int64_t B, int d, int L, int blocks) {
  if (d < 1 || d > kDcnMaxD || d > ldx)
    throw std::runtime_error(std::string(op) + ": d outside [1, " + std::to_string(kDcnMaxD) + "] or above ldx");
  if (L < 1 || L > kDcnMaxL) throw std::runtime_error(std::string(op) + ": L outside [1, 4]");
  if (blocks < 0 || blocks > kDcnMaxBlocks) throw std::runtime_error(std::string(op) + ": blocks outside [0, 65535]");
  if (B < 0 || B >= (1ll << 31)) throw std::runtime_error(std::string(op) + ": B must be below 2^31");
}

// f.run<NP, L1>() for (pieces per lane, L + 1); NP = 0 is the scalar form
template <int NP, typename Fn>
void dispatch_l(int L, const Fn& f) {
  switch (L) {
    case 1: return f.template run<NP, 2>();
    case 2: return f.template run<NP, 3>();
    case 3: return f.template run<NP, 4>();
    default: return f.template run<NP, 5>();
  }
}

template <typename Fn>
void dispatch(int d, int L, bool vec, const Fn& f) {
  if (!vec) return dispatch_l<0>(L, f);
  switch ((dcn_dp(d) / 8 + 63) / 64) {
    case 1: return dispatch_l<1>(L, f);
    case 2: return dispatch_l<2>(L, f);
    case 3: return dispatch_l<3>(L, f);
    default: return dispatch_l<4>(L, f);
  }
}

struct FwdLaunch {
  const bf16_t* X;
  int64_t ldx, B;
  int d;
  const bf16_t* Pc;
  float *wide, *p, *k;
  int blocks;
  hipStream_t s;
  template <int NP, int L1>
  void run() const {
    const int dp = dcn_dp(d);
    if constexpr (NP == 0) {
      const int grid = blocks > 0 ? blocks : grid_for(B * 16, kBlock, 1024);
      hipLaunchKernelGGL((cross_fwd_scalar<L1>), grid, kBlock, 0, s, X, ldx, B, d, Pc, dp, wide, p, k);
    } else {
      // every wave loads its weight slices and derives k once, so the grid is one resident generation of workgroups
      // (measured at d = 845, L = 3, B = 16384: 18.6 us at 768 = 3 per CU, 26.3 at 1024, 42.0 at 4096)
      static const int resident = resident_blocks(reinterpret_cast<const void*>(&cross_fwd_vec<NP, L1>));
      const int grid = blocks > 0 ? blocks : grid_for(B * 16, kBlock, resident);
      hipLaunchKernelGGL((cross_fwd_vec<NP, L1>), grid, kBlock, 0, s, X, ldx, B, d, Pc, dp, wide, p, k);
    }
  }
};

struct BwdLaunch {
  const bf16_t* X;
  int64_t ldx, B;
  int d;
  const float *p, *k, *dwide;
  const bf16_t* Pc;
  const int32_t* perm;
  bf16_t* dX;
  int F, D;
  float* part;
  int blocks;
  hipStream_t s;
  template <int NP, int L1>
  void run() const {
    const int64_t nchunks = dcn_nchunks(B), pcols = dcn_part_cols(d, L1 - 1);
    const int grid = blocks > 0 ? blocks : (int)(nchunks < 8192 ? nchunks : 8192);
    const int dp = dcn_dp(d);
    if constexpr (NP == 0)
      hipLaunchKernelGGL((cross_bwd_scalar<L1>), grid, kBlock, 0, s, X, ldx, B, d, p, k, dwide, Pc, dp, perm, dX, F, D,
                         part, pcols, nchunks);
    else
      hipLaunchKernelGGL((cross_bwd_vec<NP, L1>), grid, kBlock, 0, s, X, ldx, B, d, p, k, dwide, Pc, dp, perm, dX, F,
                         D, part, pcols, nchunks);
  }
};

struct FoldLaunch {
  const float* part;
  int64_t nchunks;
  const bf16_t* Pc;
  int d;
  float* Gc;
  hipStream_t s;
  template <int NP, int L1>
  void run() const {
    const int dp = dcn_dp(d);
    hipLaunchKernelGGL((cross_fold_kernel<L1>), (d + 63) / 64, 64 * L1, 0, s, part, dcn_part_cols(d, L1 - 1), nchunks,
                       Pc, d, dp, Gc);
  }
};

}  // namespace

void wd_cross_forward(const uint16_t* X, int64_t ldx, int64_t B, int d, const uint16_t* Pc, int L, float* wide,
                      float* p, float* k, int blocks, hipStream_t s) {
  check_shape("wd_cross_forward", ldx, B, d, L, blocks);
  if (B <= 0) return;
  const bool vec = ldx % 8 == 0 && aligned16(X) && aligned16(Pc);
  dispatch(d, L, vec, FwdLaunch{X, ldx, B, d, Pc, wide, p, k, blocks, s});
  MINIPS_HIP_CHECK(hipGetLastError());
}

void wd_cross_backward(const uint16_t* X, int64_t ldx, int64_t B, int d, const float* p, const float* k,
                       const float* dwide, const uint16_t* Pc, int L, const int32_t* perm, uint16_t* dX, int F, int D,
                       float* part, int blocks, hipStream_t s) {
  check_shape("wd_cross_backward", ldx, B, d, L, blocks);
  if (D < 1 || D > kDcnMaxEmb || F < 1 || (int64_t)F * D > d)
    throw std::runtime_error("wd_cross_backward: 1 <= D <= 64, F >= 1 and F * D <= d");
  if (B >= (1ll << 31) / F) throw std::runtime_error("wd_cross_backward: B * F must be below 2^31");
  if (B <= 0) return;
  const bool vec = D % 8 == 0 && ldx % 8 == 0 && aligned16(X) && aligned16(Pc) && aligned16(dX);
  dispatch(d, L, vec, BwdLaunch{X, ldx, B, d, p, k, dwide, Pc, perm, dX, F, D, part, blocks, s});
  MINIPS_HIP_CHECK(hipGetLastError());
}

void wd_cross_fold(const float* part, int64_t nchunks, const uint16_t* Pc, int d, int L, float* Gc, hipStream_t s) {
  check_shape("wd_cross_fold", d, 0, d, L, 0);
  if (nchunks < 0 || nchunks >= (1ll << 31) / kDcnChunk)
    throw std::runtime_error("wd_cross_fold: nchunks outside [0, 2^31 / 64)");
  if (nchunks == 0) return;
  dispatch_l<0>(L, FoldLaunch{part, nchunks, Pc, d, Gc, s});
  MINIPS_HIP_CHECK(hipGetLastError());
}

}  // namespace minips_k
