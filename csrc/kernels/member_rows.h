// One row of output per unique pulled row, summed from the lookups grouped by row: the shared device code of
// fm.hip, ffm.hip and lda.hip (as dense_update.h is the dense clock's). members / memrow [n] are a plan's lookup
// CSR: memrow ascending, members[m] the lookup whose pulled row is memrow[m]; rows at or beyond cap do not exist.
// Every unique row is written exactly once, without float atomics and with the same bits for every grid size.
//
// The models keep what differs -- what a member contributes, how a row of up to WaveMax members finds its
// members and is summed, and the kernel that sums one chunk of a heavier row into a partial. From here come the
// searches, the rule for rows of more than WaveMax members and the kernel that adds their partials:
//   memrow is cut into chunks of Chunk members, one workgroup per chunk. A row of more than WaveMax >= 2 Chunk
//   members covers at least one whole chunk, so in every chunk it touches it is the first row or the last one:
//   workgroup p looks at those two candidates only (member_heavy_row) and sums the members of chunk p that belong
//   to candidate s into part[(2 p + s) * W ...] (the model's kernel). In a second launch the workgroup whose chunk
//   holds the row's first member adds the row's partials in chunk order and stores the row
//   (member_heavy_fold_kernel). A later chunk always has the row as its first candidate (s = 0).
// Also here because the FM and the FFM share them word for word: load_e / store_e and the logistic head.
#pragma once

#include "common.h"

namespace minips_k {

// E floats as one float4 (E = 4, 16-byte aligned) or one by one
template <int E>
__device__ __forceinline__ void load_e(const float* p, float (&a)[E]) {
  if constexpr (E == 4) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    a[0] = v.x, a[1] = v.y, a[2] = v.z, a[3] = v.w;
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) a[e] = p[e];
  }
}

template <int E>
__device__ __forceinline__ void store_e(float* p, const float (&a)[E]) {
  if constexpr (E == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(a[0], a[1], a[2], a[3]);
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) p[e] = a[e];
  }
}

// Logistic loss of the logit zz against y, and its derivative times gscale: sigmoid(z) - y without the
// cancellation of sigmoid - 1 (sigmoid = big for z >= 0, small below). Sums and quotients only: no product
// feeds an addition, so there is nothing for the compiler to contract differently from one caller to the next.
__device__ __forceinline__ void logistic_head(float zz, bool y, float gscale, float* dz, float* loss) {
  const float ex = expf(-fabsf(zz));  // in (0, 1]
  const float big = 1.f / (1.f + ex), small = ex / (1.f + ex);
  const float sg = zz >= 0.f ? big : small, one_m = zz >= 0.f ? small : big;
  *dz = (y ? -one_m : sg) * gscale;
  *loss = fmaxf(zz, 0.f) - (y ? zz : 0.f) + log1pf(ex);
}

// the first index in [lo, hi) of the ascending a with a[i] >= key (hi: none)
__device__ __forceinline__ int lower_bound_i32(const int32_t* __restrict__ a, int lo, int hi, int64_t key) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (a[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// first index in (lo, n) whose value is >= key, given a[lo] < key: doubling steps from lo, then a binary search
// inside the last step (a short segment costs two or three reads, not log2 n)
__device__ __forceinline__ int gallop_i32(const int32_t* __restrict__ a, int lo, int n, int64_t key) {
  int step = 1;
  while (lo + step < n && a[lo + step] < key) {
    lo += step;
    step <<= 1;
  }
  return lower_bound_i32(a, lo + 1, lo + step < n ? lo + step : n, key);
}

// first index in [lo, n) whose value is >= key
__device__ __forceinline__ int first_ge_i32(const int32_t* __restrict__ a, int lo, int n, int64_t key) {
  if (lo >= n || a[lo] >= key) return lo < n ? lo : n;
  return gallop_i32(a, lo, n, key);
}

// the number of unique rows: memrow[n - 1] + 1, clamped into [0, cap] (n >= 1)
__device__ __forceinline__ int member_unique(const int32_t* __restrict__ memrow, int n, int64_t cap) {
  const int64_t U = (int64_t)memrow[n - 1] + 1;
  return (int)(U < 0 ? 0 : (U > cap ? cap : U));
}

// Candidate s of chunk p = [c_lo, c_hi): its first row (s = 0), or its last row if that is another (s = 1).
// True when the candidate has more than WaveMax members; then r is the row and [lo, hi) its members.
//
// Before the two searches, two reads: a heavy row that touches the chunk also holds the member H = Chunk / 2
// before the chunk or the member H after its last one. For if row [lo, hi) has a member in [c_lo, c_hi) and
// holds neither member c_lo - H nor member c_hi - 1 + H, then, being contiguous, lo > c_lo - H and
// hi <= c_hi - 1 + H, so hi - lo <= (c_hi - c_lo) + 2 H - 2 <= 2 Chunk - 2 < WaveMax: not heavy. A side that does
// not exist only makes its bound hold by itself: in the first chunk (c_lo < H) lo >= 0 > c_lo - H, and at the
// tail (c_hi - 1 + H >= n) hi <= n <= c_hi - 1 + H; neither is read. So the reads reject no heavy row for any
// Chunk, and they spare most chunks the searches.
template <int Chunk, int WaveMax>
__device__ __forceinline__ bool member_heavy_row(const int32_t* __restrict__ memrow, int n, int64_t cap, int64_t p,
                                                 int s, int& r, int& lo, int& hi) {
  static_assert(WaveMax >= 2 * Chunk, "a heavy row must be first or last in every chunk it touches");
  const int64_t c_lo = p * Chunk, c_hi = (c_lo + Chunk) < n ? (c_lo + Chunk) : n;
  const int ra = memrow[c_lo], rb = memrow[c_hi - 1];
  if (s == 1 && rb == ra) return false;
  r = s ? rb : ra;
  if ((uint64_t)(int64_t)r >= (uint64_t)cap) return false;
  constexpr int H = Chunk / 2;
  const int64_t after = c_hi - 1 + H;
  if (!((c_lo >= H && memrow[c_lo - H] == r) || (after < n && memrow[after] == r))) return false;
  lo = lower_bound_i32(memrow, 0, n, r);
  hi = lower_bound_i32(memrow, lo, n, (int64_t)r + 1);
  return hi - lo > WaveMax;
}

constexpr int kMemberFoldMaxBlock = 256;

// One workgroup per chunk, any block size up to kMemberFoldMaxBlock (columns strided over the threads). The
// workgroup whose chunk holds a heavy row's first member adds that row's partials, its own first and then the
// later chunks' ascending, in Acc and stores the row as floats: <float, float> sums gradients in one fixed
// order, <int32_t, int64_t> sums counts exactly.
template <typename Part, typename Acc, int Chunk, int WaveMax>
__global__ __launch_bounds__(kMemberFoldMaxBlock) void member_heavy_fold_kernel(const int32_t* __restrict__ memrow,
                                                                                int n, int64_t cap, int W,
                                                                                const Part* __restrict__ part,
                                                                                float* __restrict__ out) {
  const int64_t p = blockIdx.x;
  const int64_t c_lo = p * Chunk;
  for (int s = 0; s < 2; ++s) {
    int r, lo, hi;
    if (!member_heavy_row<Chunk, WaveMax>(memrow, n, cap, p, s, r, lo, hi)) continue;
    if (lo < c_lo) continue;  // the row began in an earlier chunk
    const int64_t q1 = (hi - 1) / Chunk;
    for (int col = threadIdx.x; col < W; col += blockDim.x) {
      Acc t = part[(2 * p + s) * W + col];
      for (int64_t qc = p + 1; qc <= q1; ++qc) t += part[(2 * qc) * W + col];
      out[(int64_t)r * W + col] = (float)t;
    }
  }
}

// chunks of n members, and the elements of the `part` workspace: 2 W per chunk when a row can be heavy at all
inline int member_chunks(int64_t n, int Chunk) { return (int)((n + Chunk - 1) / Chunk); }

inline int64_t member_part_elems(int64_t n, int W, int Chunk, int WaveMax) {
  return n > WaveMax ? 2 * ((n + Chunk - 1) / Chunk) * W : 0;
}

}  // namespace minips_k
