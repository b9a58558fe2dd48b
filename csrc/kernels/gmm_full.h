// Gaussian mixture model with full covariances, fitted by (stepwise) EM on the dense PS (gmm_full.hip; binding in
// csrc/bindings/gmm_full_py.cpp, module minips_amd._gmmfk). The diagonal model's kernel (gmm.h) scores a point by one
// GEMM and keeps K x 2D accumulators in registers; here a score is a D x D product per component and the second moment
// is K weighted D x D SYRKs, so the work is split into a scores kernel and a statistics kernel. The rule is the same in
// the kernels and in the CPU references ops.gmm_full_prepare / ops.gmm_full_estep.
//
// Shapes    1 <= K <= 128 components, 1 <= D <= 64 dimensions, KP = 16 ceil(K / 16), DP = 16 ceil(D / 16)
//           (gmm_full_shape_ok).
// State     the normalised sufficient statistics s [K, W] fp32, W = D + D*D + 1: s[k, 0:D] = E[r_k x],
//           s[k, D:D + D*D] = E[r_k x x^T] (row-major, exactly symmetric), s[k, W - 1] = E[r_k], and a fixed shift
//           [D]; x always means point - shift, formed as the point is read.
// Prepare   gmm_full_prepare(s, reg_covar) -> Wh [K, DP, DP], b [K, DP], cst [K], per component:
//             s0 = s[k, W - 1]   pi = s0 / sum_j s0_j (over the j with a finite s0_j > 0)   mu = s1 / s0
//             Sigma = S2 / s0 - mu mu^T + reg_covar I (its lower triangle is read)      Sigma = L L^T (Cholesky)
//             Wh = L^-1 (lower triangular; pad rows and columns 0)      b = Wh mu
//             cst = log pi - sum_d log L_dd - (D / 2) log 2 pi
//           A component with s0 <= 0, a non-finite statistic, a pivot that is non-positive or non-finite, or a
//           non-finite cst is dead: cst = -inf, Wh and b 0.
// E-step    gmm_full_estep(X [n, D] fp32 with row stride ld >= D, shift, Wh, b, cst), per point i:
//             y_k = Wh_k x - b_k        t_ik = cst_k - 0.5 |y_k|^2       (a sum of squares: no cancellation)
//             m_i = max_k t_ik    lse_i = m_i + log sum_k exp(t_ik - m_i)    r_ik = exp(t_ik - lse_i)
//           S [K, W] = the sums over i of r_ik x_i | r_ik x_i x_i^T | r_ik (not normalised), ll = sum_i lse_i (fp64),
//           assign [n] int32 = argmax_k t_ik (the lowest index on ties), logp [n] fp32 = lse_i. Without S only assign,
//           logp and ll are computed: the predict path. The D x D block is computed on its lower-triangle tiles and
//           mirrored, so it is symmetric to the bit.
// Bad       a point whose lse is not finite (a non-finite feature; every component dead) contributes nothing to S and
//           ll and is counted in the int32 counter `bad`; its assign is -1 and its logp NaN.
// Bits      the points are cut into chunks of gmm_full_chunk(n, K, D) consecutive points: 2048, lengthened in steps of
//           2048 until there are at most gmm_full_max_chunks(K, D) = min(kGmmFullMaxChunks, kGmmFullPartCap /
//           (K W)) of them, so the partials' workspace never exceeds kGmmFullPartCap floats (256 MiB) whatever n is
//           (at 2048 points a chunk, K = 128, D = 64 and a million points would take a gigabyte). A chunk's partial S
//           is a function of the data alone (fixed MFMA order); the fold adds the partials in chunk order. ll is folded
//           from per-tile fp64 partials (256 points) in a fixed order. The same bits on every run and for every grid
//           size; no float atomics anywhere.
//
// Kernels (wave64, 256-thread workgroups; DPB = DP is a template parameter: 16, 32, 48 or 64)
//   gmmf_prepare_kernel<DPB>  a workgroup per component. Sigma's lower triangle is built in LDS [DPB][DPB + 1]; a
//                           left-looking Cholesky, a thread per row, every dot product serial in ascending order; the
//                           triangular inverse by forward substitution, a thread per column; b a thread per row; the
//                           log-determinant serial. __fdiv_rn and __fsqrt_rn throughout.
//   gmmf_scores_kernel<DPB> persistent over tiles of 256 points. Wave w owns the points 64 w .. 64 w + 63 of the tile
//                           as four row tiles of 16 and keeps their x in registers as the MFMA A operand (4 * DPB / 4
//                           VGPRs) for the whole component loop. Wh_k [DPB][DPB + 4] and b_k stream through two LDS
//                           buffers: the next component's global loads are in flight during the math, one barrier a
//                           component, and a staged Wh_k feeds 256 points. Y = X Wh_k^T by v_mfma_f32_16x16x4_f32, one
//                           B operand read feeding the four row tiles; the k-steps above the diagonal tile are skipped
//                           (Wh is lower triangular). Per lane q = sum over its columns of (y - b)^2 for 16 points;
//                           a halving fold over the 16 lanes of a lane group (15 shuffles for the 16 sums) leaves every
//                           lane with the whole |y|^2 of one point of the wave: no LDS, no barrier. So the softmax over
//                           k is online and per lane: running max, sum and argmax of one point in ascending component
//                           order. The scores go to the global workspace T [n, KP] four components a store; logp,
//                           assign, the tile's fp64 ll partial and the bad count follow at the end of the tile.
//   Why T goes to global memory: the diagonal kernel keeps the responsibilities in LDS only. Here the second-moment
//                           accumulators of all components (K DP^2 floats, a megabyte at 128 x 64) do not fit one
//                           workgroup, and recomputing the scores per component group would multiply the dominant
//                           flops. T costs 4 K bytes a point against 4 K D^2 flops. r = exp(t - lse) is formed as the
//                           statistics kernel reads T, each value once.
//   gmmf_stats_kernel<DPB>  grid (chunk, component group); a group is G = 8 components at DPB >= 48 and 16 below: what
//                           fits in accumulator VGPRs. Tiles of 64 points are staged into two LDS buffers [64][DPB +
//                           4] (float4 loads, scalar loads for the last quad of a row and when ld or the base is not
//                           16-byte friendly; shift subtracted on the way in; pad columns, rows past n and the rows of
//                           bad points zero) beside R [64][16 + 4], r = exp(t - lse). Wave w owns G / 4 components and
//                           all their lower-triangle tiles of (r_k o X)^T X (A operand r x formed as read, at most 80
//                           accumulator VGPRs), and deals itself the tiles of R^T [X | 1] (the column of ones gives
//                           sum r). The accumulators live for the chunk; one partial is written. One barrier a tile.
//   gmmf_fold_kernel        S[j] = the chunks' partials added in chunk order, a thread per lower-triangle entry, which
//                           writes its mirror image too; one more workgroup adds the fp64 ll partials (lane-strided
//                           ascending, then a butterfly).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace minips_k {

constexpr int kGmmFullMaxBlocks = 65535;
constexpr int kGmmFullMaxK = 128;
constexpr int kGmmFullMaxD = 64;
constexpr int kGmmFullTile = 256;               // points per scores tile and per ll partial
constexpr int kGmmFullChunk = 2048;             // the shortest chunk
constexpr int kGmmFullMaxChunks = 256;          // partials per statistic at the most
constexpr int64_t kGmmFullPartCap = 1ll << 26;  // floats of S partials at the most (256 MiB)

inline int gmm_full_pad(int64_t v) { return (int)((v + 15) / 16 * 16); }
inline bool gmm_full_shape_ok(int64_t K, int64_t D) {
  return K >= 1 && K <= kGmmFullMaxK && D >= 1 && D <= kGmmFullMaxD;
}
inline int64_t gmm_full_width(int64_t D) { return D + D * D + 1; }
inline int64_t gmm_full_max_chunks(int64_t K, int64_t D) {
  const int64_t c = kGmmFullPartCap / (K * gmm_full_width(D));
  return c < kGmmFullMaxChunks ? c : kGmmFullMaxChunks;
}
// a function of (n, K, D) only: a multiple of 2048
inline int64_t gmm_full_chunk(int64_t n, int64_t K, int64_t D) {
  const int64_t base = (n + kGmmFullChunk - 1) / kGmmFullChunk, cap = gmm_full_max_chunks(K, D);
  const int64_t mult = base <= cap ? 1 : (base + cap - 1) / cap;
  return mult * kGmmFullChunk;
}
inline int64_t gmm_full_chunks(int64_t n, int64_t K, int64_t D) {
  const int64_t c = gmm_full_chunk(n, K, D);
  return (n + c - 1) / c;
}
inline int64_t gmm_full_tiles(int64_t n) { return (n + kGmmFullTile - 1) / kGmmFullTile; }

// s [K, D + D*D + 1] -> Wh [K, DP, DP], b [K, DP], cst [K]
void gmm_full_prepare(const float* s, int K, int D, float reg_covar, float* Wh, float* b, float* cst,
                      hipStream_t stream);

// X [n, ld], shift [D], Wh [K, DP, DP], b [K, DP], cst [K]. S [K, W] or null (the predict path), ll fp64 [1], assign
// int32 [n] or null, logp fp32 [n] (required with S: the statistics kernel reads it) or null, bad int32 [1] or null
// (added to). Workspaces: T n * KP floats and part gmm_full_chunks(n, K, D) * K * W floats (both unused without S),
// llpart gmm_full_tiles(n) doubles. blocks > 0 forces the grid size. n == 0 writes zeros.
void gmm_full_estep(const float* X, int64_t ld, int64_t n, int D, int K, const float* shift, const float* Wh,
                    const float* b, const float* cst, float* S, double* ll, int32_t* assign, float* logp,
                    int32_t* bad, float* T, float* part, double* llpart, int blocks, hipStream_t stream);

}  // namespace minips_k
