// DeepFM's FM interaction term over the assembled Wide & Deep input (deepfm.h states the rule and the mapping).
// Both kernels are memory-bound streams of short bf16 rows: E values per lane (8: one 16-byte load, or 1: the
// fallback for a D or a buffer that is not 16-byte friendly), L lanes per field row, 64 / L lane groups per wave.
#include <stdexcept>
#include <string>

#include "common.h"
#include "deepfm.h"

namespace minips_k {

namespace {

constexpr int kBlock = 256;

template <int E>
__device__ __forceinline__ void load_bf(const bf16_t* p, float (&a)[E]) {
  if constexpr (E == 8) {
    const uint4 w = *reinterpret_cast<const uint4*>(p);
    const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a[2 * i] = __uint_as_float(u[i] << 16);
      a[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
    }
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) a[e] = bf2f(p[e]);
  }
}

template <int E>
__device__ __forceinline__ void store_bf(bf16_t* p, const float (&a)[E]) {
  if constexpr (E == 8) {
    *reinterpret_cast<uint4*>(p) =
        make_uint4(pack_bf2(a[0], a[1]), pack_bf2(a[2], a[3]), pack_bf2(a[4], a[5]), pack_bf2(a[6], a[7]));
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) p[e] = f2bf(a[e]);
  }
}

template <int E>
__device__ __forceinline__ void load_f(const float* p, float (&a)[E]) {
  if constexpr (E == 8) {
    const float4 x = reinterpret_cast<const float4*>(p)[0], y = reinterpret_cast<const float4*>(p)[1];
    a[0] = x.x, a[1] = x.y, a[2] = x.z, a[3] = x.w, a[4] = y.x, a[5] = y.y, a[6] = y.z, a[7] = y.w;
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) a[e] = p[e];
  }
}

template <int E>
__device__ __forceinline__ void store_f(float* p, const float (&a)[E]) {
  if constexpr (E == 8) {
    reinterpret_cast<float4*>(p)[0] = make_float4(a[0], a[1], a[2], a[3]);
    reinterpret_cast<float4*>(p)[1] = make_float4(a[4], a[5], a[6], a[7]);
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) p[e] = a[e];
  }
}

// One wave per sample. Lane group g (L lanes, lane l owns columns [E l, E l + E)) takes the fields g, g + G, ...
template <int E, int L>
__global__ __launch_bounds__(kBlock) void wd_fm_forward_kernel(const bf16_t* __restrict__ X, int64_t ldx, int64_t B,
                                                               int F, int D, float* __restrict__ wide,
                                                               float* __restrict__ S) {
#pragma clang fp contract(off)
  constexpr int G = 64 / L;
  const int lane = threadIdx.x & 63, g = lane / L, l = lane % L;
  const int c0 = E * l;
  const bool act = c0 < D;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t b = wave; b < B; b += nwaves) {
    const bf16_t* xb = X + b * ldx + c0;
    float s[E], q[E];
#pragma unroll
    for (int e = 0; e < E; ++e) s[e] = 0.f, q[e] = 0.f;
    if (act) {
#pragma unroll 2
      for (int f = g; f < F; f += G) {
        float v[E];
        load_bf<E>(xb + (int64_t)f * D, v);
#pragma unroll
        for (int e = 0; e < E; ++e) {
          s[e] += v[e];
          q[e] += v[e] * v[e];
        }
      }
    }
    // the groups' partial sums, folded in a fixed order: afterwards every group holds the totals
#pragma unroll
    for (int o = L; o < 64; o <<= 1) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        s[e] += __shfl_xor(s[e], o, 64);
        q[e] += __shfl_xor(q[e], o, 64);
      }
    }
    if (act && g == 0) store_f<E>(S + b * D + c0, s);
    float t = 0.f;  // (a lane without columns holds zeros)
#pragma unroll
    for (int e = 0; e < E; ++e) t += s[e] * s[e] - q[e];
#pragma unroll
    for (int o = 1; o < L; o <<= 1) t += __shfl_xor(t, o, 64);
    if (lane == 0) wide[b] += 0.5f * t;
  }
}

// One lane group per lookup, grid-stride: dX[r] += dwide[b] (S[b] - v), three roundings and the bf16 conversion.
template <int E, int L>
__global__ __launch_bounds__(kBlock) void wd_fm_backward_kernel(const bf16_t* __restrict__ X, int64_t ldx,
                                                                const float* __restrict__ S,
                                                                const float* __restrict__ dwide,
                                                                const int32_t* __restrict__ perm,
                                                                bf16_t* __restrict__ dX, int64_t n, int F, int D) {
#pragma clang fp contract(off)
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t ngroups = ((int64_t)gridDim.x * blockDim.x) / L;
  const int c0 = E * (int)(tid % L);
  if (c0 >= D) return;
  for (int64_t i = tid / L; i < n; i += ngroups) {
    const int64_t r = perm ? (int64_t)perm[i] : i;
    if ((uint64_t)r >= (uint64_t)n) continue;  // nothing of that row is touched
    const uint32_t b = (uint32_t)i / (uint32_t)F, f = (uint32_t)i - b * (uint32_t)F;
    float v[E], sv[E], gx[E];
    load_bf<E>(X + (int64_t)b * ldx + (int64_t)f * D + c0, v);
    load_bf<E>(dX + r * D + c0, gx);
    load_f<E>(S + (int64_t)b * D + c0, sv);
    const float dz = dwide[b];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const float d = sv[e] - v[e];
      const float p = dz * d;
      gx[e] = gx[e] + p;
    }
    store_bf<E>(dX + r * D + c0, gx);
  }
}

void check_shape(const char* op, int64_t ldx, int64_t B, int F, int D, int blocks) {
  if (!dfm_shape_ok(F, D, ldx)) throw std::runtime_error(std::string(op) + ": 1 <= D <= 64, F >= 1 and F * D <= ldx");
  if (blocks < 0 || blocks > kDfmMaxBlocks) throw std::runtime_error(std::string(op) + ": blocks outside [0, 65535]");
  if (B < 0 || B >= (1ll << 31) / F) throw std::runtime_error(std::string(op) + ": B * F must be below 2^31");
}

// f.run<E, L>() for the lane shape of (D, vec)
template <typename Fn>
void dispatch_shape(int D, bool vec, const Fn& f) {
  if (vec) {
    switch (D / 8) {
      case 1: return f.template run<8, 1>();
      case 2: return f.template run<8, 2>();
      case 4: return f.template run<8, 4>();
      default: return f.template run<8, 8>();
    }
  }
  switch (pow2ceil(D)) {
    case 1: return f.template run<1, 1>();
    case 2: return f.template run<1, 2>();
    case 4: return f.template run<1, 4>();
    case 8: return f.template run<1, 8>();
    case 16: return f.template run<1, 16>();
    case 32: return f.template run<1, 32>();
    default: return f.template run<1, 64>();
  }
}

inline bool vec_d(int D) { return D == 8 || D == 16 || D == 32 || D == 64; }

struct FwdLaunch {
  const bf16_t* X;
  int64_t ldx, B;
  int F, D;
  float *wide, *S;
  int blocks;
  hipStream_t s;
  template <int E, int L>
  void run() const {
    const int grid = blocks > 0 ? blocks : grid_for(B * 64, kBlock, 8192);
    hipLaunchKernelGGL((wd_fm_forward_kernel<E, L>), grid, kBlock, 0, s, X, ldx, B, F, D, wide, S);
  }
};

struct BwdLaunch {
  const bf16_t* X;
  int64_t ldx;
  const float *S, *dwide;
  const int32_t* perm;
  bf16_t* dX;
  int64_t n;
  int F, D, blocks;
  hipStream_t s;
  template <int E, int L>
  void run() const {
    const int grid = blocks > 0 ? blocks : grid_for(n * L, kBlock, 8192);
    hipLaunchKernelGGL((wd_fm_backward_kernel<E, L>), grid, kBlock, 0, s, X, ldx, S, dwide, perm, dX, n, F, D);
  }
};

}  // namespace

void wd_fm_forward(const uint16_t* X, int64_t ldx, int64_t B, int F, int D, float* wide, float* S, int blocks,
                   hipStream_t s) {
  check_shape("wd_fm_forward", ldx, B, F, D, blocks);
  if (B <= 0) return;
  const bool vec = vec_d(D) && ldx % 8 == 0 && aligned16(X) && aligned16(S);
  dispatch_shape(D, vec, FwdLaunch{X, ldx, B, F, D, wide, S, blocks, s});
  MINIPS_HIP_CHECK(hipGetLastError());
}

void wd_fm_backward(const uint16_t* X, int64_t ldx, const float* S, const float* dwide, const int32_t* perm,
                    uint16_t* dX, int64_t B, int F, int D, int blocks, hipStream_t s) {
  check_shape("wd_fm_backward", ldx, B, F, D, blocks);
  if (B <= 0) return;
  const bool vec = vec_d(D) && ldx % 8 == 0 && aligned16(X) && aligned16(S) && aligned16(dX);
  dispatch_shape(D, vec, BwdLaunch{X, ldx, S, dwide, perm, dX, B * F, F, D, blocks, s});
  MINIPS_HIP_CHECK(hipGetLastError());
}

}  // namespace minips_k
