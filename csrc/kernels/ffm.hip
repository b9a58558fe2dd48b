// Field-aware factorization-machine forward and backward over a CSR batch of pulled rows (ffm.h states the
// rule, the mapping and which member counts take which backward path). Both kernels are latency-bound gathers
// of k-float slots: E floats per lane and load (4: one float4, or 1: the form for buffers that are not 16-byte
// friendly).
#include <stdexcept>
#include <string>

#include "common.h"
#include "ffm.h"
#include "member_rows.h"

namespace minips_k {

namespace {

constexpr int kBlock = 256;
constexpr int kRedW = kFfmMaxFK + 8;  // a gradient row in LDS (W <= 516)

// One wave per sample; lane l takes the pairs l, l + 64, ... of the round-robin enumeration (ffm.h) and the
// lookups l, l + 64, ... of the linear term.
template <int E>
__global__ __launch_bounds__(kBlock) void ffm_forward_kernel(
    const int64_t* __restrict__ rowptr, const int64_t* __restrict__ inv, const float* __restrict__ vals,
    const int32_t* __restrict__ fields, const float* __restrict__ labels, const float* __restrict__ rows, int64_t ld,
    int64_t cap, int F, int k, const float* __restrict__ w0, float gscale, int64_t B, int64_t n,
    float* __restrict__ z, float* __restrict__ dz, float* __restrict__ loss, int32_t* __restrict__ rowid) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const float w0v = w0 ? *w0 : 0.f;
  const int FK = F * k;
  for (int64_t b = wave; b < B; b += nwaves) {
    int64_t st = rowptr[b], en = rowptr[b + 1];
    st = st < 0 ? 0 : st;
    en = en > n ? n : en;  // a rowptr outside [0, n] reads and writes nothing
    const int64_t m = en > st ? en - st : 0;
    float lin = 0.f, acc = 0.f;
    for (int64_t j = st + lane; j < en; j += 64) {
      const int64_t rj = inv[j];
      const int fj = fields[j];
      rowid[j] = (int32_t)b;
      if ((uint64_t)rj < (uint64_t)cap && (unsigned)fj < (unsigned)F) lin += rows[rj * ld + FK] * vals[j];
    }
    const int64_t D = m >> 1, Q = m * D;
    if (D > 0) {
      const bool even = (m & 1) == 0;
      const int64_t si = 64 / D, sd = 64 % D;
      int64_t i = lane / D, d0 = lane % D;  // pair q = i D + d0, d = d0 + 1
      for (int64_t q = lane; q < Q; q += 64) {
        int64_t j = i + d0 + 1;
        j = j >= m ? j - m : j;
        if (!(even && d0 + 1 == D && i >= D)) {  // the half round of an even m
          const int64_t ri = inv[st + i], rj = inv[st + j];
          const int fi = fields[st + i], fj = fields[st + j];
          if ((uint64_t)ri < (uint64_t)cap && (uint64_t)rj < (uint64_t)cap && (unsigned)fi < (unsigned)F &&
              (unsigned)fj < (unsigned)F) {
            const float* pa = rows + ri * ld + fj * k;
            const float* pb = rows + rj * ld + fi * k;
            float dot = 0.f;
            for (int c = 0; c < k; c += E) {
              float va[E], vb[E];
              load_e<E>(pa + c, va);
              load_e<E>(pb + c, vb);
#pragma unroll
              for (int e = 0; e < E; ++e) dot += va[e] * vb[e];
            }
            acc += dot * (vals[st + i] * vals[st + j]);
          }
        }
        i += si, d0 += sd;
        if (d0 >= D) d0 -= D, ++i;
      }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      acc += __shfl_xor(acc, o, 64);
      lin += __shfl_xor(lin, o, 64);
    }
    if (lane == 0) {
      const float zz = (w0v + lin) + acc;
      float dzb, lossb;
      logistic_head(zz, labels[b] > 0.5f, gscale, &dzb, &lossb);
      z[b] = zz;
      dz[b] = dzb;
      loss[b] = lossb;
    }
  }
}

struct BwdArgs {
  const int32_t* members;
  const int32_t* memrow;
  const int32_t* rowid;
  const int64_t* rowptr;
  const int64_t* inv;
  const float* vals;
  const int32_t* fields;
  const float* dz;
  const float* rows;
  int64_t ld, cap, B;
  int F, k, n;
  float* grad;
  float* part;
};

// what lane t of a lane group of L lanes does: as a loader, part `cc` of partner `p` of a step of PP partners;
// as an owner, the columns [(ch L + t) E, + E) of the gradient row for ch < C -- slot[ch] is their field
// (-2: none), sl[ch] the part of a partner's vector that lands there, lin[ch]: the linear column is the first
template <int E, int L, int C>
struct Lane {
  int t, gbase, sub, PP, p, cc;
  int slot[C], sl[C];
  bool lin[C];
  __device__ __forceinline__ Lane(int lane, int F, int k) {
    t = lane % L, gbase = lane - t, sub = k / E, PP = L / sub, p = t / sub, cc = t % sub;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      const int col = (ch * L + t) * E;
      slot[ch] = col < F * k ? col / k : -2;
      sl[ch] = (col % k) / E;
      lin[ch] = col == F * k;
    }
  }
};

// the terms of member m: acc[g k + c] += (c_m x_j) v_{inv[j], fields[m], c} over the partners j of field g
template <int E, int L, int C>
__device__ __forceinline__ void ffm_member(const BwdArgs& a, int m, const Lane<E, L, C>& ln, float (&acc)[C][E]) {
  const int j = a.members[m];
  if ((unsigned)j >= (unsigned)a.n) return;
  const int b = a.rowid[j];
  if ((uint64_t)(int64_t)b >= (uint64_t)a.B) return;
  const int fm = a.fields[j];
  if ((unsigned)fm >= (unsigned)a.F) return;
  const float c = a.dz[b] * a.vals[j];
  int64_t st = a.rowptr[b], en = a.rowptr[b + 1];
  st = st < 0 ? 0 : st;
  en = en > a.n ? a.n : en;
  for (int64_t base = st; base < en; base += ln.PP) {
    // the lanes as loaders: every gather of the step is in flight at once
    const int64_t jj = base + ln.p;
    int fp = -1;
    float tv[E];
#pragma unroll
    for (int e = 0; e < E; ++e) tv[e] = 0.f;
    if (ln.p < ln.PP && jj < en && jj != j) {
      const int64_t rj = a.inv[jj];
      const int fj = a.fields[jj];
      if ((uint64_t)rj < (uint64_t)a.cap && (unsigned)fj < (unsigned)a.F) {
        load_e<E>(a.rows + rj * a.ld + fm * a.k + ln.cc * E, tv);
        const float s = c * a.vals[jj];
#pragma unroll
        for (int e = 0; e < E; ++e) tv[e] *= s;
        fp = fj;
      }
    }
    // the lanes as owners: the step's partners in order
    const int cnt = (int)((en - base) < ln.PP ? (en - base) : ln.PP);  // uniform over the group
    for (int q = 0; q < cnt; ++q) {
      const int src = ln.gbase + q * ln.sub;
      const int fq = __shfl(fp, src, 64);
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const float tt = __shfl(tv[e], src + ln.sl[ch], 64);
          if (fq == ln.slot[ch]) acc[ch][e] += tt;
        }
      }
    }
  }
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    if (ln.lin[ch]) acc[ch][0] += c;
  }
}

template <int E, int C>
__device__ __forceinline__ void zero_acc(float (&acc)[C][E]) {
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
#pragma unroll
    for (int e = 0; e < E; ++e) acc[ch][e] = 0.f;
  }
}

// the groups' sums folded in a fixed order: afterwards every group holds the totals
template <int E, int L, int C>
__device__ __forceinline__ void fold_groups(float (&acc)[C][E]) {
#pragma unroll
  for (int o = L; o < 64; o <<= 1) {
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
#pragma unroll
      for (int e = 0; e < E; ++e) acc[ch][e] += __shfl_xor(acc[ch][e], o, 64);
    }
  }
}

template <int E, int L, int C>
__device__ __forceinline__ void store_row(float* dst, int W, const Lane<E, L, C>& ln, const float (&acc)[C][E]) {
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    const int col = (ch * L + ln.t) * E;
    if (col < W) store_e<E>(dst + col, acc[ch]);  // W % E == 0
  }
}

// Rows of up to kFfmWaveMax members: a tile of G consecutive unique rows per wave and iteration, one lane group
// per row; the rows of a tile that have more than kFfmGroupMax members are then walked by the whole wave.
template <int E, int L, int C>
__global__ __launch_bounds__(kBlock) void ffm_backward_kernel(BwdArgs a) {
  constexpr int G = 64 / L;
  const int lane = threadIdx.x & 63, g = lane / L, l = lane % L;
  const int W = a.F * a.k + 4;
  const Lane<E, L, C> ln(lane, a.F, a.k);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int U = member_unique(a.memrow, a.n, a.cap);
  const int64_t ntiles = ((int64_t)U + G - 1) / G;
  // consecutive tiles per wave: one binary search of memrow per wave, every later row starts by a gallop from
  // where the tile before it ended (`carry`)
  const int64_t per = (ntiles + nwaves - 1) / nwaves;
  const int64_t t0 = wave * per, t1 = (t0 + per) < ntiles ? (t0 + per) : ntiles;
  int carry = -1;
  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t u64 = tile * G + g;
    const bool valid = u64 < U;
    const int u = valid ? (int)u64 : 0;
    // a row ends where the next group's row begins, and the tile's last row gallops from its own start
    int lo = a.n;
    if (valid) lo = carry < 0 ? lower_bound_i32(a.memrow, 0, a.n, u) : first_ge_i32(a.memrow, carry, a.n, u);
    const int lo_next = __shfl_down(lo, L, 64);
    int hi = lo;
    if (valid) {
      if (g < G - 1 && u + 1 < U) hi = lo_next;  // the next group holds row u + 1
      else if (lo < a.n && a.memrow[lo] == u) hi = gallop_i32(a.memrow, lo, a.n, u + 1);
    }
    carry = __shfl(hi, 63, 64);  // (the last group is invalid in the last tile only)
    const int M = hi - lo;
    if (valid && M > 0 && M <= kFfmGroupMax) {
      float acc[C][E];
      zero_acc<E, C>(acc);
      for (int m = lo; m < hi; ++m) ffm_member<E, L, C>(a, m, ln, acc);
      store_row<E, L, C>(a.grad + (int64_t)u * W, W, ln, acc);
    }
    unsigned long long big = __ballot(valid && l == 0 && M > kFfmGroupMax && M <= kFfmWaveMax);
    while (big) {
      const int src = __ffsll(big) - 1;
      big &= big - 1;
      const int ru = __shfl(u, src, 64), rlo = __shfl(lo, src, 64), rhi = __shfl(hi, src, 64);
      float acc[C][E];
      zero_acc<E, C>(acc);
      for (int m = rlo + g; m < rhi; m += G) ffm_member<E, L, C>(a, m, ln, acc);
      fold_groups<E, L, C>(acc);
      if (g == 0) store_row<E, L, C>(a.grad + (int64_t)ru * W, W, ln, acc);
    }
  }
}

// block p sums the members of chunk p that belong to a heavy row into part[(2 p + s) * W ...] (member_rows.h)
template <int E, int L, int C>
__global__ __launch_bounds__(kBlock) void ffm_backward_heavy_kernel(BwdArgs a) {
  constexpr int G = 64 / L, NG = G * (kBlock / 64);
  __shared__ float red[kBlock / 64][kRedW];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane / L;
  const int W = a.F * a.k + 4;
  const Lane<E, L, C> ln(lane, a.F, a.k);
  const int64_t p = blockIdx.x;
  const int64_t c_lo = p * kFfmChunk, c_hi = (c_lo + kFfmChunk) < a.n ? (c_lo + kFfmChunk) : a.n;
  for (int s = 0; s < 2; ++s) {
    int r, lo, hi;
    if (!member_heavy_row<kFfmChunk, kFfmWaveMax>(a.memrow, a.n, a.cap, p, s, r, lo, hi)) continue;  // block-uniform
    const int m0 = lo > c_lo ? lo : (int)c_lo, m1 = hi < c_hi ? hi : (int)c_hi;
    float acc[C][E];
    zero_acc<E, C>(acc);
    for (int m = m0 + wv * G + g; m < m1; m += NG) ffm_member<E, L, C>(a, m, ln, acc);
    fold_groups<E, L, C>(acc);
    __syncthreads();  // (the previous candidate's reads of red)
    if (g == 0) {
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
        const int col = (ch * L + ln.t) * E;
        if (col < W) {
#pragma unroll
          for (int e = 0; e < E; ++e) red[wv][col + e] = acc[ch][e];
        }
      }
    }
    __syncthreads();
    for (int col = threadIdx.x; col < W; col += kBlock) {
      float t = red[0][col];
#pragma unroll
      for (int w = 1; w < kBlock / 64; ++w) t += red[w][col];
      a.part[(2 * p + s) * W + col] = t;
    }
  }
}

void check_shape(const char* op, int F, int k, int64_t ld, int64_t cap, int64_t B, int64_t n, int blocks) {
  if (!ffm_shape_ok(F, k))
    throw std::runtime_error(std::string(op) + ": k % 4 == 0, 4 <= k <= 16, 1 <= F <= 64 and F * k <= 512");
  if (ld < F * k + 4) throw std::runtime_error(std::string(op) + ": ld < F * k + 4");
  if (blocks < 0 || blocks > kFfmMaxBlocks)
    throw std::runtime_error(std::string(op) + ": blocks outside [0, 65535]");
  if (n >= (1ll << 31) || B >= (1ll << 31) || cap >= (1ll << 31))
    throw std::runtime_error(std::string(op) + ": n, B and cap must be below 2^31");
}

// f.run<E, L, C>() for the lane shape of (W, vec)
template <typename F>
void dispatch_shape(int W, bool vec, const F& f) {
  if (vec) {
    const int cols = W / 4;  // 2 .. 129
    if (cols <= 2) return f.template run<4, 2, 1>();
    if (cols <= 4) return f.template run<4, 4, 1>();
    if (cols <= 8) return f.template run<4, 8, 1>();
    if (cols <= 16) return f.template run<4, 16, 1>();
    if (cols <= 32) return f.template run<4, 32, 1>();
    if (cols <= 64) return f.template run<4, 64, 1>();
    if (cols <= 128) return f.template run<4, 64, 2>();
    return f.template run<4, 64, 3>();
  }
  if (W <= 64) return f.template run<1, 64, 1>();
  if (W <= 128) return f.template run<1, 64, 2>();
  if (W <= 256) return f.template run<1, 64, 4>();
  return f.template run<1, 64, 9>();  // W <= 516
}

struct BwdLaunch {
  BwdArgs a;
  int blocks;
  hipStream_t s;
  template <int E, int L, int C>
  void run() const {
    const int64_t n = a.n, urows = a.cap < n ? a.cap : n;  // at most this many unique rows
    const int grid = blocks > 0 ? blocks : grid_for(urows * L, kBlock, 8192);
    hipLaunchKernelGGL((ffm_backward_kernel<E, L, C>), grid, kBlock, 0, s, a);
    if (n > kFfmWaveMax) {
      const int chunks = member_chunks(n, kFfmChunk);
      hipLaunchKernelGGL((ffm_backward_heavy_kernel<E, L, C>), chunks, kBlock, 0, s, a);
      hipLaunchKernelGGL((member_heavy_fold_kernel<float, float, kFfmChunk, kFfmWaveMax>), chunks, kBlock, 0, s,
                         a.memrow, a.n, a.cap, a.F * a.k + 4, a.part, a.grad);
    }
  }
};

}  // namespace

void ffm_forward(const int64_t* rowptr, const int64_t* inv, const float* vals, const int32_t* fields,
                 const float* labels, const float* rows, int64_t ld, int64_t cap, int F, int k, const float* w0,
                 float gscale, int64_t B, int64_t n, float* z, float* dz, float* loss, int32_t* rowid, int blocks,
                 hipStream_t s) {
  check_shape("ffm_forward", F, k, ld, cap, B, n, blocks);
  if (B <= 0) return;
  const bool vec = ld % 4 == 0 && aligned16(rows);
  const int grid = blocks > 0 ? blocks : grid_for(B * 64, kBlock, 16384);
  if (vec)
    hipLaunchKernelGGL((ffm_forward_kernel<4>), grid, kBlock, 0, s, rowptr, inv, vals, fields, labels, rows, ld, cap,
                       F, k, w0, gscale, B, n, z, dz, loss, rowid);
  else
    hipLaunchKernelGGL((ffm_forward_kernel<1>), grid, kBlock, 0, s, rowptr, inv, vals, fields, labels, rows, ld, cap,
                       F, k, w0, gscale, B, n, z, dz, loss, rowid);
  MINIPS_HIP_CHECK(hipGetLastError());
}

int64_t ffm_backward_part_floats(int64_t n, int W) {
  return member_part_elems(n, W, kFfmChunk, kFfmWaveMax);
}

void ffm_backward(const int32_t* members, const int32_t* memrow, const int32_t* rowid, const int64_t* rowptr,
                  const int64_t* inv, const float* vals, const int32_t* fields, const float* dz, const float* rows,
                  int64_t ld, int64_t cap, int F, int k, int64_t B, int64_t n, float* grad_rows, float* part,
                  int blocks, hipStream_t s) {
  static_assert(kFfmMaxFK + 4 <= kRedW, "a gradient row must fit the LDS fold");
  check_shape("ffm_backward", F, k, ld, cap, B, n, blocks);
  if (n <= 0 || B <= 0 || cap <= 0) return;
  const bool heavy = n > kFfmWaveMax;
  if (heavy && part == nullptr) throw std::runtime_error("ffm_backward: part workspace missing");
  const bool vec = ld % 4 == 0 && aligned16(rows) && aligned16(grad_rows);
  const BwdArgs a{members, memrow, rowid, rowptr, inv, vals, fields, dz, rows, ld, cap, B, F, k, (int)n, grad_rows,
                  part};
  dispatch_shape(F * k + 4, vec, BwdLaunch{a, blocks, s});
  MINIPS_HIP_CHECK(hipGetLastError());
}

}  // namespace minips_k
