// AutoInt's interacting layers over the assembled Wide & Deep input (attnint.h states the rule and the design): one
// wave carries one sample through a layer, every intermediate stays in registers as the next MFMA's operand.
#include <stdexcept>
#include <string>

#include "attnint.h"
#include "common.h"

namespace minips_k {

namespace {

typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

__device__ __forceinline__ v4f mfma(v8s a, v8s b, v4f c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, b), c, 0, 0, 0);
}

constexpr v4f kZero4 = {0.f, 0.f, 0.f, 0.f};

// Two accumulator tiles -> one operand fragment: contraction indices 4 g + r (lo) and 16 + 4 g + r (hi).
__device__ __forceinline__ v8s pack2(v4f lo, v4f hi) {
  const uint4 u = make_uint4(pack_bf2(lo[0], lo[1]), pack_bf2(lo[2], lo[3]), pack_bf2(hi[0], hi[1]),
                             pack_bf2(hi[2], hi[3]));
  return __builtin_bit_cast(v8s, u);
}

template <int HD>
__device__ __forceinline__ v8s pack_hd(const v4f (&c)[HD]) {
  if constexpr (HD == 2) return pack2(c[0], c[1]);
  return pack2(c[0], kZero4);
}

__device__ __forceinline__ v8s frag8(const bf16_t (&v)[8]) {
  const uint4 u = make_uint4(v[0] | (uint32_t)v[1] << 16, v[2] | (uint32_t)v[3] << 16, v[4] | (uint32_t)v[5] << 16,
                             v[6] | (uint32_t)v[7] << 16);
  return __builtin_bit_cast(v8s, u);
}

// bf16_rne as fp32
__device__ __forceinline__ float rbf(float v) { return bf2f(f2bf(v)); }

// 8 consecutive bf16 at p: one 16-byte load, or element by element
__device__ __forceinline__ v8s load8(const bf16_t* p, bool vec) {
  if (vec) return *reinterpret_cast<const v8s*>(p);
  bf16_t v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = p[e];
  return frag8(v);
}

// W^l [Din, 4 A] -> LDS transposed [4 A][pitch], columns k >= Din zero
__device__ __forceinline__ void stage_w(const bf16_t* __restrict__ W, int Din, int N4, int pitch, bf16_t* Wt) {
  for (int idx = threadIdx.x; idx < N4 * pitch; idx += kBlock) Wt[idx] = 0;
  __syncthreads();
  for (int idx = threadIdx.x; idx < Din * N4; idx += kBlock) {
    const int k = idx / N4, n = idx - k * N4;
    Wt[n * pitch + k] = W[idx];
  }
  __syncthreads();
}

// The fragments of E^{l-1}: rows l15 + 16 it, columns 32 ks + 8 g .. + 8 (zero outside m x Din)
template <int KS>
__device__ __forceinline__ void load_e(const bf16_t* Es, int rs, bool vec, int m, int Din, int l15, int g,
                                       v8s (&ef)[2][KS]) {
#pragma unroll
  for (int it = 0; it < 2; ++it)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int i = l15 + 16 * it, k = 32 * ks + 8 * g;
      ef[it][ks] = (i < m && k < Din) ? load8(Es + i * rs + k, vec) : v8s{0, 0, 0, 0, 0, 0, 0, 0};
    }
}

// c[ct][it] += the accumulator tile of W_n^T E^T: rows n0 + 16 ct + 4 g + r of the projection, column (sample row)
// l15 + 16 it. Packed over ct it is the fragment "row i, head columns" of E W_n.
template <int KS, int HD>
__device__ __forceinline__ void proj_t(const bf16_t* Wt, int pitch, int n0, int l15, int g, const v8s (&ef)[2][KS],
                                       v4f (&c)[2][HD]) {
#pragma unroll
  for (int ct = 0; ct < HD; ++ct)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const v8s w = *reinterpret_cast<const v8s*>(Wt + (n0 + 16 * ct + l15) * pitch + 32 * ks + 8 * g);
#pragma unroll
      for (int it = 0; it < 2; ++it) c[it][ct] = mfma(w, ef[it][ks], c[it][ct]);
    }
}

// c[ct][it] += the accumulator tile of E W_n: sample rows 4 g + r + 16 it, projection column n0 + 16 ct + l15. Packed
// over it it is the fragment "head column, all sample rows" of (E W_n)^T.
template <int KS, int HD>
__device__ __forceinline__ void proj_n(const bf16_t* Wt, int pitch, int n0, int l15, int g, const v8s (&ef)[2][KS],
                                       v4f (&c)[HD][2]) {
#pragma unroll
  for (int ct = 0; ct < HD; ++ct)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const v8s w = *reinterpret_cast<const v8s*>(Wt + (n0 + 16 * ct + l15) * pitch + 32 * ks + 8 * g);
#pragma unroll
      for (int it = 0; it < 2; ++it) c[ct][it] = mfma(ef[it][ks], w, c[ct][it]);
    }
}

// fragments "row, head columns" of E W_n (rounded to bf16)
template <int KS, int HD>
__device__ __forceinline__ void proj_rows(const bf16_t* Wt, int pitch, int n0, int l15, int g,
                                          const v8s (&ef)[2][KS], v8s (&f)[2]) {
  v4f c[2][HD];
#pragma unroll
  for (int it = 0; it < 2; ++it)
#pragma unroll
    for (int ct = 0; ct < HD; ++ct) c[it][ct] = kZero4;
  proj_t<KS, HD>(Wt, pitch, n0, l15, g, ef, c);
  f[0] = pack_hd<HD>(c[0]);
  f[1] = pack_hd<HD>(c[1]);
}

// fragments "head column, sample rows" of (E W_n)^T (rounded to bf16)
template <int KS, int HD>
__device__ __forceinline__ void proj_cols(const bf16_t* Wt, int pitch, int n0, int l15, int g,
                                          const v8s (&ef)[2][KS], v8s (&f)[HD]) {
  v4f c[HD][2];
#pragma unroll
  for (int ct = 0; ct < HD; ++ct) c[ct][0] = c[ct][1] = kZero4;
  proj_n<KS, HD>(Wt, pitch, n0, l15, g, ef, c);
#pragma unroll
  for (int ct = 0; ct < HD; ++ct) f[ct] = pack2(c[ct][0], c[ct][1]);
}

// The softmax of row i = l15 + 16 it, whose scores s[jt][r] (j = 16 jt + 4 g + r) lie in the four lanes of equal l15:
// p receives bf16_rne(P) as fp32; mx and l are the row's maximum and sum, equal in the four lanes.
__device__ __forceinline__ void softmax_row(const v4f (&s)[2], int m, int g, v4f (&p)[2], float& mx, float& l) {
  mx = -INFINITY;
#pragma unroll
  for (int jt = 0; jt < 2; ++jt)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (16 * jt + 4 * g + r < m) mx = fmaxf(mx, s[jt][r]);
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  l = 0.f;
#pragma unroll
  for (int jt = 0; jt < 2; ++jt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p[jt][r] = 16 * jt + 4 * g + r < m ? __expf(s[jt][r] - mx) : 0.f;
      l += p[jt][r];
    }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
#pragma unroll
  for (int jt = 0; jt < 2; ++jt)
#pragma unroll
    for (int r = 0; r < 4; ++r) p[jt][r] = rbf(p[jt][r] / l);
}

// ---------------------------------------------------------------------------------------------- forward
// Ein: E^{l-1} (sample stride es, row stride er); Eout: E^l (sample stride os, row stride A)
template <int KS, int HD>
__global__ __launch_bounds__(kBlock) void attn_fwd(const bf16_t* __restrict__ Ein, int64_t es, int er, bool evec,
                                                   int64_t B, int m, int Din, int H, const bf16_t* __restrict__ W,
                                                   bf16_t* __restrict__ Eout, int64_t os) {
  extern __shared__ __attribute__((aligned(16))) bf16_t Wt[];
  constexpr int d = 16 * HD, pitch = 32 * KS + 8;
  const int A = H * d;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
  stage_w(W, Din, 4 * A, pitch, Wt);

  for (int64_t b = (int64_t)blockIdx.x * kWaves + wave; b < B; b += (int64_t)gridDim.x * kWaves) {
    v8s ef[2][KS];
    load_e<KS>(Ein + b * es, er, evec, m, Din, l15, g, ef);
    for (int h = 0; h < H; ++h) {
      asm volatile("" ::: "memory");  // (W's fragments are re-read from LDS, not hoisted into registers)
      v8s qf[2], kf[2], vt[HD];
      proj_rows<KS, HD>(Wt, pitch, h * d, l15, g, ef, qf);
      proj_rows<KS, HD>(Wt, pitch, A + h * d, l15, g, ef, kf);
      proj_cols<KS, HD>(Wt, pitch, 2 * A + h * d, l15, g, ef, vt);
      v4f o[2][HD];  // starts from R: rows a = 4 g + r + 16 ct of R_h^T, column i = l15 + 16 it
#pragma unroll
      for (int it = 0; it < 2; ++it)
#pragma unroll
        for (int ct = 0; ct < HD; ++ct) o[it][ct] = kZero4;
      proj_t<KS, HD>(Wt, pitch, 3 * A + h * d, l15, g, ef, o);
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        v4f s[2], p[2];
        float mx, l;
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) s[jt] = mfma(kf[jt], qf[it], kZero4);  // S^T: rows j, column i
        softmax_row(s, m, g, p, mx, l);
        const v8s pf = pack2(p[0], p[1]);
        const int i = l15 + 16 * it;
#pragma unroll
        for (int ct = 0; ct < HD; ++ct) {
          const v4f acc = mfma(vt[ct], pf, o[it][ct]);  // (P V)^T on top of R^T
          if (i < m) {
            const uint2 u = make_uint2(pack_bf2(fmaxf(acc[0], 0.f), fmaxf(acc[1], 0.f)),
                                       pack_bf2(fmaxf(acc[2], 0.f), fmaxf(acc[3], 0.f)));
            *reinterpret_cast<uint2*>(Eout + b * os + i * A + h * d + 16 * ct + 4 * g) = u;
          }
        }
      }
    }
  }
}

// wide[b] += <w_out, E^T_b>: one wave per sample
__global__ __launch_bounds__(kBlock) void attn_out(const bf16_t* __restrict__ ET, int64_t es, int64_t B, int n,
                                                   const bf16_t* __restrict__ w_out, float* wide) {
  const int lane = threadIdx.x & 63;
  for (int64_t b = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); b < B; b += (int64_t)gridDim.x * kWaves) {
    float s = 0.f;
    for (int o = lane; o < n; o += 64) s += bf2f(w_out[o]) * bf2f(ET[b * es + o]);
    s = warp_sum(s);
    if (lane == 0) wide[b] += s;
  }
}

// ---------------------------------------------------------------------------------------------- backward
struct BwdArgs {
  const bf16_t* Ein;   // E^{l-1}: sample stride es, row stride er
  int64_t es;
  int er;
  bool evec;
  int64_t B;
  int m, Din;
  const bf16_t* W;
  const bf16_t* Ek;    // E^l (sample stride ks, row stride A)
  const bf16_t* dEk;   // dE^l, null at the last layer (formed from dwide and w_out)
  int64_t ks;
  const bf16_t* w_out;
  const float* dwide;
  bf16_t* dEprev;      // dE^{l-1} (sample stride ks, row stride Din), null at layer 1
  const int32_t* perm;
  bf16_t* dX;          // layer 1: [B m, Din]
  float* part;         // [nchunks, Din, 4 A]
  int64_t chunk, nchunks;
};

// The four waves of a workgroup carry ONE sample together: wave w owns gradient part w of [dQ | dK | dV | dY] -- it
// recomputes what that part needs, forms the part in both orientations, keeps the part's A / 16 x 2 KS tiles of dW in
// its accumulators across the chunk's samples, and its share of dE^{l-1} is folded over the waves through LDS.
template <int KS, int H, int HD>
__global__ __launch_bounds__(kBlock) void attn_bwd(BwdArgs p) {
  extern __shared__ __attribute__((aligned(16))) bf16_t Wt[];
  constexpr int d = 16 * HD, A = H * d, N4 = 4 * A, pitch = 32 * KS + 8, KT = 2 * KS, NTP = A / 16;
  float4* deb = reinterpret_cast<float4*>(Wt + N4 * pitch);  // [2][2 KT][64]: a lane's dE tiles, two samples deep
  const int m = p.m, Din = p.Din;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, l15 = lane & 15;
  const int part = __builtin_amdgcn_readfirstlane(tid >> 6);  // (wave-uniform)
  stage_w(p.W, Din, N4, pitch, Wt);
  int parity = 0;

  for (int64_t chunk = blockIdx.x; chunk < p.nchunks; chunk += gridDim.x) {
    v4f dw[NTP][KT];  // dW^T tiles of this part: rows n = part A + 16 nt + 4 g + r, column k = l15 + 16 kt
#pragma unroll
    for (int nt = 0; nt < NTP; ++nt)
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) dw[nt][kt] = kZero4;

    for (int64_t sidx = 0; sidx < p.chunk; ++sidx, parity ^= 1) {
      const int64_t b = chunk * p.chunk + sidx;
      if (b >= p.B) break;  // (workgroup-uniform)
      const bf16_t* Es = p.Ein + b * p.es;
      const bf16_t* Ys = p.Ek + b * p.ks;
      const bf16_t* dYs = p.dEk ? p.dEk + b * p.ks : nullptr;
      const float dz = p.dwide[b];
      auto dy = [&](int i, int a) -> bf16_t {  // dY[i, a]; zero outside the sample
        if (i >= m) return (bf16_t)0;
        const int idx = i * A + a;
        if (!(bf2f(Ys[idx]) > 0.f)) return (bf16_t)0;
        return dYs ? dYs[idx] : f2bf(dz * bf2f(p.w_out[idx]));
      };
      auto dy4 = [&](int i, int a, bf16_t* v) {  // dY[i, a .. a + 4): 8-byte loads (a % 4 == 0)
        v[0] = v[1] = v[2] = v[3] = 0;
        if (i >= m) return;
        const int idx = i * A + a;
        const uint2 y = *reinterpret_cast<const uint2*>(Ys + idx);
        const bf16_t yv[4] = {(bf16_t)y.x, (bf16_t)(y.x >> 16), (bf16_t)y.y, (bf16_t)(y.y >> 16)};
        uint2 gv = make_uint2(0u, 0u);
        if (dYs) gv = *reinterpret_cast<const uint2*>(dYs + idx);
        const bf16_t gb[4] = {(bf16_t)gv.x, (bf16_t)(gv.x >> 16), (bf16_t)gv.y, (bf16_t)(gv.y >> 16)};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (bf2f(yv[e]) > 0.f) v[e] = dYs ? gb[e] : f2bf(dz * bf2f(p.w_out[idx + e]));
      };
      auto load_yf = [&](int h, v8s(&yf)[2]) {  // dY rows i = l15 + 16 it, head columns {4 g + r, 16 + 4 g + r}
#pragma unroll
        for (int it = 0; it < 2; ++it) {
          bf16_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
          dy4(l15 + 16 * it, h * d + 4 * g, v);
          if constexpr (HD == 2) dy4(l15 + 16 * it, h * d + 16 + 4 * g, v + 4);
          yf[it] = frag8(v);
        }
      };
      auto load_yt = [&](int h, v8s(&yt)[HD]) {  // dY^T: column a = l15 + 16 ct of the head, rows {4 g + r, 16 + ..}
#pragma unroll
        for (int ct = 0; ct < HD; ++ct) {
          bf16_t v[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = dy(4 * g + (e & 3) + 16 * (e >> 2), h * d + 16 * ct + l15);
          yt[ct] = frag8(v);
        }
      };

      v8s ef[2][KS], et[KT];
      load_e<KS>(Es, p.er, p.evec, m, Din, l15, g, ef);
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {  // E^T: column k = l15 + 16 kt, rows {4 g + r, 16 + 4 g + r}
        const int k = l15 + 16 * kt;
        bf16_t v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int i = 4 * g + (e & 3) + 16 * (e >> 2);
          v[e] = (i < m && k < Din) ? Es[i * p.er + k] : (bf16_t)0;
        }
        et[kt] = frag8(v);
      }
      v4f de[2][KT];  // this part's share of dE^{l-1 T}: rows k = 16 kt + 4 g + r, column i = l15 + 16 it
#pragma unroll
      for (int it = 0; it < 2; ++it)
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) de[it][kt] = kZero4;

#pragma unroll
      for (int h = 0; h < H; ++h) {
        asm volatile("" ::: "memory");  // (W's fragments are re-read from LDS per head, not hoisted into registers)
        // the part as "row i, head columns" (gr) and "column n, rows i" (gc), from x (rows) and y (columns)
        v8s gr[2], gc[HD], x[2], y[HD];
        if (part == 3) {
          load_yf(h, gr);
          load_yt(h, gc);
        } else {
          v8s qf[2], kf[2], vf[2], yf[2];
          proj_rows<KS, HD>(Wt, pitch, h * d, l15, g, ef, qf);
          proj_rows<KS, HD>(Wt, pitch, A + h * d, l15, g, ef, kf);
          if (part <= 1) {
            proj_rows<KS, HD>(Wt, pitch, 2 * A + h * d, l15, g, ef, vf);
            load_yf(h, yf);
          }
          // rows i in the lane's column: the softmax statistics, and (parts 0, 1) dS
          asm volatile("" ::: "memory");
          float mx[2], ls[2], rs[2] = {0.f, 0.f};
#pragma unroll
          for (int it = 0; it < 2; ++it) {
            v4f s[2], pp[2];
#pragma unroll
            for (int jt = 0; jt < 2; ++jt) s[jt] = mfma(kf[jt], qf[it], kZero4);  // S^T
            softmax_row(s, m, g, pp, mx[it], ls[it]);
            if (part <= 1) {
              v4f dp[2];
              float r = 0.f;
#pragma unroll
              for (int jt = 0; jt < 2; ++jt) {
                dp[jt] = mfma(vf[jt], yf[it], kZero4);  // dP^T = V dY^T
#pragma unroll
                for (int e = 0; e < 4; ++e) r += dp[jt][e] * pp[jt][e];
              }
              r += __shfl_xor(r, 16, 64);
              r += __shfl_xor(r, 32, 64);
              rs[it] = r;
#pragma unroll
              for (int jt = 0; jt < 2; ++jt)
#pragma unroll
                for (int e = 0; e < 4; ++e) dp[jt][e] = pp[jt][e] * (dp[jt][e] - r);
              x[it] = pack2(dp[0], dp[1]);  // dS rows i (part 0)
            }
          }
          if (part == 0) {  // dQ = dS K
            proj_cols<KS, HD>(Wt, pitch, A + h * d, l15, g, ef, y);
          } else {
            // P^T / dS^T: column j = l15 + 16 jt, rows i = 4 g + r + 16 it; the row statistics come from lane 4 g + r
#pragma unroll
            for (int jt = 0; jt < 2; ++jt) {
              v4f pp[2];
              const bool live = l15 + 16 * jt < m;
#pragma unroll
              for (int it = 0; it < 2; ++it) {
                const v4f s = mfma(qf[it], kf[jt], kZero4);  // S
                v4f dp = kZero4;
                if (part == 1) dp = mfma(yf[it], vf[jt], kZero4);  // dP
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                  const float mxi = __shfl(mx[it], 4 * g + e, 64), li = __shfl(ls[it], 4 * g + e, 64);
                  const float ri = __shfl(rs[it], 4 * g + e, 64);
                  const float pv = live ? rbf(__expf(s[e] - mxi) / li) : 0.f;
                  pp[it][e] = part == 1 ? pv * (dp[e] - ri) : pv;
                }
              }
              x[jt] = pack2(pp[0], pp[1]);  // dS^T rows j (part 1), P^T rows j (part 2)
            }
            if (part == 1)
              proj_cols<KS, HD>(Wt, pitch, h * d, l15, g, ef, y);  // dK = dS^T Q
            else
              load_yt(h, y);  // dV = P^T dY
          }
          v4f cr[2][HD], cc[HD][2];
#pragma unroll
          for (int it = 0; it < 2; ++it)
#pragma unroll
            for (int ct = 0; ct < HD; ++ct) {
              cr[it][ct] = mfma(y[ct], x[it], kZero4);
              cc[ct][it] = mfma(x[it], y[ct], kZero4);
            }
          gr[0] = pack_hd<HD>(cr[0]);
          gr[1] = pack_hd<HD>(cr[1]);
#pragma unroll
          for (int ct = 0; ct < HD; ++ct) gc[ct] = pack2(cc[ct][0], cc[ct][1]);
        }
        const int n0 = part * A + h * d;
        asm volatile("" ::: "memory");  // (the same for the gathers below: no loads are moved above the products)
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
          bf16_t v[8];  // W[k = l15 + 16 kt, n0 + {4 g + r, 16 + 4 g + r}] from the transposed copy
#pragma unroll
          for (int e = 0; e < 8; ++e)
            v[e] = (HD == 2 || e < 4) ? Wt[(n0 + 4 * g + (e & 3) + 16 * (e >> 2)) * pitch + l15 + 16 * kt] : (bf16_t)0;
          const v8s wf = frag8(v);
#pragma unroll
          for (int it = 0; it < 2; ++it) de[it][kt] = mfma(wf, gr[it], de[it][kt]);
#pragma unroll
          for (int ct = 0; ct < HD; ++ct) dw[h * HD + ct][kt] = mfma(gc[ct], et[kt], dw[h * HD + ct][kt]);
        }
      }

      // dE^{l-1} = ((Q's share + K's) + V's) + Y's: a lane meets its own tiles of the wave before in LDS
      float4* buf = deb + parity * (2 * KT * 64);
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        if (part == w) {
#pragma unroll
          for (int it = 0; it < 2; ++it)
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
              float4* q = buf + (it * KT + kt) * 64 + lane;
              if (w > 0) {
                const float4 u = *q;
                de[it][kt][0] += u.x, de[it][kt][1] += u.y, de[it][kt][2] += u.z, de[it][kt][3] += u.w;
              }
              if (w + 1 < kWaves) *q = make_float4(de[it][kt][0], de[it][kt][1], de[it][kt][2], de[it][kt][3]);
            }
        }
        if (w + 1 < kWaves) __syncthreads();
      }
      if (part == kWaves - 1) {  // row i = l15 + 16 it, columns 16 kt + 4 g .. + 4
#pragma unroll
        for (int it = 0; it < 2; ++it) {
          const int i = l15 + 16 * it;
          if (i >= m) continue;
          bf16_t* row = nullptr;
          if (p.dEprev) {
            row = p.dEprev + b * p.ks + i * Din;
          } else {
            const int64_t n = p.B * m;
            const int64_t r = p.perm ? (int64_t)p.perm[b * m + i] : b * m + i;
            if (r >= 0 && r < n) row = p.dX + r * Din;
          }
          if (!row) continue;
#pragma unroll
          for (int kt = 0; kt < KT; ++kt) {
            const int k = 16 * kt + 4 * g;
            if (k >= Din) continue;
            v4f v = de[it][kt];
            uint2* q = reinterpret_cast<uint2*>(row + k);
            if (!p.dEprev) {
              const uint2 u = *q;
              v[0] += __uint_as_float(u.x << 16), v[1] += __uint_as_float(u.x & 0xffff0000u);
              v[2] += __uint_as_float(u.y << 16), v[3] += __uint_as_float(u.y & 0xffff0000u);
            }
            *q = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
          }
        }
      }
    }

    // the chunk's partial: every wave stores its own part's columns
    float* pc = p.part + chunk * (int64_t)Din * N4 + part * A;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      const int k = l15 + 16 * kt;
      if (k >= Din) continue;
#pragma unroll
      for (int nt = 0; nt < NTP; ++nt)
        *reinterpret_cast<float4*>(pc + (int64_t)k * N4 + 16 * nt + 4 * g) =
            make_float4(dw[nt][kt][0], dw[nt][kt][1], dw[nt][kt][2], dw[nt][kt][3]);
    }
  }
}

// part[chunk, o] = sum over the chunk's samples (ascending) of dwide[b] E^T_b[o]
__global__ __launch_bounds__(kBlock) void attn_wout(const bf16_t* __restrict__ ET, int64_t es, int64_t B, int n,
                                                    const float* __restrict__ dwide, int64_t chunk, float* part) {
  const int64_t b0 = blockIdx.x * chunk, b1 = b0 + chunk < B ? b0 + chunk : B;
  for (int o = threadIdx.x; o < n; o += kBlock) {
    float s = 0.f;
    for (int64_t b = b0; b < b1; ++b) s += dwide[b] * bf2f(ET[b * es + o]);
    part[(int64_t)blockIdx.x * n + o] = s;
  }
}

__global__ __launch_bounds__(kBlock) void attn_fold(const float* __restrict__ part, int64_t nchunks, int64_t n,
                                                    float* G) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int64_t c = 0; c < nchunks; ++c) s += part[c * n + i];
  G[i] += s;
}

// ---------------------------------------------------------------------------------------------- launchers
void check_layer(const char* op, int64_t ldx, int64_t B, const AttnLayer& L, int blocks) {
  const std::string o(op);
  if (L.m < 1 || L.m > kAttnMaxM) throw std::runtime_error(o + ": F outside [1, 32]");
  if (L.D < 8 || L.D > kAttnMaxD || L.D % 8) throw std::runtime_error(o + ": D must be a multiple of 8 in [8, 64]");
  if (L.T < 1 || L.T > kAttnMaxT || L.l < 1 || L.l > L.T) throw std::runtime_error(o + ": layer outside 1 .. T <= 3");
  if ((L.d != 16 && L.d != 32) || L.H < 1 || L.H * L.d > kAttnMaxA)
    throw std::runtime_error(o + ": heads outside the rule (d in {16, 32}, H d <= 64)");
  if (L.l == 1 && (int64_t)L.m * L.D > ldx) throw std::runtime_error(o + ": X has fewer than F D columns");
  if (blocks < 0 || blocks > kAttnMaxBlocks) throw std::runtime_error(o + ": blocks outside [0, 65535]");
  if (B < 0 || B >= (1ll << 31) / ((int64_t)L.T * L.m * L.A()))
    throw std::runtime_error(o + ": B T F A must be below 2^31");
}

inline int lds_bytes(const AttnLayer& L) { return 2 * 4 * L.A() * (32 * ((L.Din() + 31) / 32) + 8); }
// + the lanes' dE tiles, two samples deep
inline int bwd_lds_bytes(const AttnLayer& L) { return lds_bytes(L) + 2 * 4 * ((L.Din() + 31) / 32) * 64 * 16; }

template <int KS, int HD>
void launch_fwd(const bf16_t* Ein, int64_t es, int er, int64_t B, const AttnLayer& L, const bf16_t* W, bf16_t* Eout,
                int64_t os, int blocks, hipStream_t s) {
  const bool evec = aligned16(Ein) && es % 8 == 0 && er % 8 == 0;
  const int64_t want = (B + kWaves - 1) / kWaves;
  const int grid = blocks > 0 ? blocks : (int)(want < 1024 ? want : 1024);
  hipLaunchKernelGGL((attn_fwd<KS, HD>), grid, kBlock, lds_bytes(L), s, Ein, es, er, evec, B, L.m, L.Din(), L.H, W,
                     Eout, os);
}

template <int KS, int H>
void launch_bwd_hd(const BwdArgs& a, const AttnLayer& L, int grid, hipStream_t s) {
  if constexpr (H <= 2) {
    if (L.d == 32) {
      hipLaunchKernelGGL((attn_bwd<KS, H, 2>), grid, kBlock, bwd_lds_bytes(L), s, a);
      return;
    }
  }
  hipLaunchKernelGGL((attn_bwd<KS, H, 1>), grid, kBlock, bwd_lds_bytes(L), s, a);
}

template <int KS>
void launch_bwd(const BwdArgs& a, const AttnLayer& L, int grid, hipStream_t s) {
  switch (L.H) {
    case 1: return launch_bwd_hd<KS, 1>(a, L, grid, s);
    case 2: return launch_bwd_hd<KS, 2>(a, L, grid, s);
    case 3: return launch_bwd_hd<KS, 3>(a, L, grid, s);
    default: return launch_bwd_hd<KS, 4>(a, L, grid, s);
  }
}

}  // namespace

void wd_attn_layer_forward(const uint16_t* X, int64_t ldx, int64_t B, const AttnLayer& L, const uint16_t* W,
                           uint16_t* EK, int blocks, hipStream_t s) {
  check_layer("wd_attn_layer_forward", ldx, B, L, blocks);
  if (reinterpret_cast<uintptr_t>(EK) % 16)
    throw std::runtime_error("wd_attn_layer_forward: EK must be 16-byte aligned");
  if (B <= 0) return;
  const int A = L.A();
  const int64_t ks = (int64_t)L.T * L.m * A;
  const bf16_t* Ein = L.l == 1 ? X : EK + (int64_t)(L.l - 2) * L.m * A;
  const int64_t es = L.l == 1 ? ldx : ks;
  const int er = L.l == 1 ? L.D : A;
  bf16_t* Eout = EK + (int64_t)(L.l - 1) * L.m * A;
  const bool two = L.Din() > 32;
  if (L.d == 32) {
    if (two) launch_fwd<2, 2>(Ein, es, er, B, L, W, Eout, ks, blocks, s);
    else launch_fwd<1, 2>(Ein, es, er, B, L, W, Eout, ks, blocks, s);
  } else {
    if (two) launch_fwd<2, 1>(Ein, es, er, B, L, W, Eout, ks, blocks, s);
    else launch_fwd<1, 1>(Ein, es, er, B, L, W, Eout, ks, blocks, s);
  }
  MINIPS_HIP_CHECK(hipGetLastError());
}

void wd_attn_output(const uint16_t* EK, int64_t B, const AttnLayer& L, const uint16_t* w_out, float* wide, int blocks,
                    hipStream_t s) {
  check_layer("wd_attn_output", (int64_t)L.m * L.D, B, L, blocks);
  if (B <= 0) return;
  const int n = L.m * L.A();
  const int grid = blocks > 0 ? blocks : grid_for(B * 64, kBlock, 2048);
  hipLaunchKernelGGL(attn_out, grid, kBlock, 0, s, EK + (int64_t)(L.T - 1) * n, (int64_t)L.T * n, B, n, w_out, wide);
  MINIPS_HIP_CHECK(hipGetLastError());
}

void wd_attn_layer_backward(const uint16_t* X, int64_t ldx, int64_t B, const AttnLayer& L, const uint16_t* W,
                            const uint16_t* EK, uint16_t* dEK, const uint16_t* w_out, const float* dwide,
                            const int32_t* perm, uint16_t* dX, float* part, int blocks, hipStream_t s) {
  check_layer("wd_attn_layer_backward", ldx, B, L, blocks);
  if (reinterpret_cast<uintptr_t>(EK) % 16 || reinterpret_cast<uintptr_t>(dEK) % 16 ||
      reinterpret_cast<uintptr_t>(part) % 16 || reinterpret_cast<uintptr_t>(dX) % 8)
    throw std::runtime_error("wd_attn_layer_backward: EK, dEK and part must be 16-byte, dX 8-byte aligned");
  if (B >= (1ll << 31) / L.m) throw std::runtime_error("wd_attn_layer_backward: B F must be below 2^31");
  if (B <= 0) return;
  const int A = L.A(), mA = L.m * A;
  const int64_t ks = (int64_t)L.T * mA;
  BwdArgs a{};
  a.Ein = L.l == 1 ? X : EK + (int64_t)(L.l - 2) * mA;
  a.es = L.l == 1 ? ldx : ks;
  a.er = L.l == 1 ? L.D : A;
  a.evec = aligned16(a.Ein) && a.es % 8 == 0 && a.er % 8 == 0;
  a.B = B, a.m = L.m, a.Din = L.Din(), a.W = W;
  a.Ek = EK + (int64_t)(L.l - 1) * mA;
  a.dEk = L.l == L.T ? nullptr : dEK + (int64_t)(L.l - 1) * mA;
  a.ks = ks, a.w_out = w_out, a.dwide = dwide;
  a.dEprev = L.l == 1 ? nullptr : dEK + (int64_t)(L.l - 2) * mA;
  a.perm = perm, a.dX = dX, a.part = part;
  a.chunk = attn_chunk(B), a.nchunks = attn_nchunks(B);
  const int grid = blocks > 0 ? blocks : (int)a.nchunks;
  if (L.Din() > 32) launch_bwd<2>(a, L, grid, s);
  else launch_bwd<1>(a, L, grid, s);
  MINIPS_HIP_CHECK(hipGetLastError());
}

void wd_attn_wout_partial(const uint16_t* EK, int64_t B, const AttnLayer& L, const float* dwide, float* part,
                          hipStream_t s) {
  check_layer("wd_attn_wout_partial", (int64_t)L.m * L.D, B, L, 0);
  if (B <= 0) return;
  const int n = L.m * L.A();
  hipLaunchKernelGGL(attn_wout, (unsigned)attn_nchunks(B), kBlock, 0, s, EK + (int64_t)(L.T - 1) * n, (int64_t)L.T * n,
                     B, n, dwide, attn_chunk(B), part);
  MINIPS_HIP_CHECK(hipGetLastError());
}

void wd_attn_fold(const float* part, int64_t nchunks, int64_t n, float* G, hipStream_t s) {
  if (nchunks < 0 || nchunks > kAttnMaxChunks) throw std::runtime_error("wd_attn_fold: nchunks outside [0, 512]");
  if (n < 0 || n >= (1ll << 31)) throw std::runtime_error("wd_attn_fold: n outside [0, 2^31)");
  if (nchunks == 0 || n == 0) return;
  hipLaunchKernelGGL(attn_fold, (unsigned)((n + kBlock - 1) / kBlock), kBlock, 0, s, part, nchunks, n, G);
  MINIPS_HIP_CHECK(hipGetLastError());
}

}  // namespace minips_k
