// Gaussian mixture model with diagonal covariances, fitted by (stepwise) EM on the dense PS (gmm.hip; binding in
// csrc/bindings/gmm_py.cpp, module minips_amd._gmmk): the E-step and the sufficient statistics of a batch of points in
// one fused kernel -- "attention with the sum taken over the queries". The rule is the same in the kernels and in the
// CPU references ops.gmm_prepare / ops.gmm_estep.
//
// Shapes    1 <= K <= 128 components, 1 <= D <= 128 dimensions, KP = 16 ceil(K / 16), DP = 16 ceil(D / 16),
//           KP * DP <= 8192 (gmm_shape_ok).
// State     the normalised sufficient statistics s [K, 2D + 1] fp32: s[k, 0:D] = E[r_k x], s[k, D:2D] = E[r_k x^2],
//           s[k, 2D] = E[r_k], and a fixed shift [D]; x always means point - shift, formed as the point is read.
// Prepare   gmm_prepare(s, var_floor) -> coef [K, 2 DP], cst [K]:
//             s0 = s[k, 2D]   pi = s0 / sum_j s0_j (over the j with a finite s0_j > 0)   mu = s1 / s0
//             v = s2 / s0 - mu^2, var = v if v > var_floor else var_floor
//             coef[k, d] = -0.5 / var     coef[k, DP + d] = mu / var     (the pad columns are 0)
//             cst_k = log pi_k - 0.5 sum_d (mu^2 / var + log var) - (D / 2) log 2 pi
//           A component with s0 <= 0, a non-finite statistic or a non-finite cst is dead: cst = -inf, its coef row 0.
// E-step    gmm_estep(X [n, D] fp32 with row stride ld >= D, shift, coef, cst), per point i:
//             t_ik = cst_k + sum_d (coef[k, d] x_d^2 + coef[k, DP + d] x_d)
//             m_i = max_k t_ik    lse_i = m_i + log sum_k exp(t_ik - m_i)    r_ik = exp(t_ik - lse_i)
//           S [K, 2D + 1] = the sums over i of r_ik x_i | r_ik x_i^2 | r_ik (not normalised), ll = sum_i lse_i (fp64),
//           assign [n] int32 = argmax_k t_ik (the lowest index on ties), logp [n] fp32 = lse_i. Without S only assign,
//           logp and ll are computed: the predict path.
// Bad       a point whose lse is not finite (a non-finite feature; every component dead) contributes nothing to S and
//           ll and is counted in the int32 counter `bad`; its assign is -1 and its logp NaN.
// Bits      the points are cut into chunks of kGmmChunk consecutive points. A chunk's partial (S, ll) is a function of
//           the data alone (fixed MFMA and cross-lane orders); gmm_fold_kernel adds the partials in chunk order. The
//           result is the same bits on every run and for every grid size; no float atomics anywhere.
//
// Kernels (wave64, 256-thread workgroups; KPB x DPB the padded bucket of the instantiation, >= KP x DP)
//   gmm_prepare_kernel      a wave per component; the folds over K and D are lane-strided sums in ascending order
//                           followed by a xor butterfly.
//   gmm_estep_kernel<KPB, DPB, ACC>  persistent over chunks. coef [KPB][2 DPB + 4], cst and shift are resident in LDS
//                           for the whole kernel. A tile of 64 points is staged into LDS [64][DPB + 4] (float4 loads,
//                           scalar loads for the last quad of a row and when ld or the base is not 16-byte friendly;
//                           shift subtracted on the way in; pad columns and the rows past n zero). Two tiles: the next
//                           tile's global loads are in flight during the math. Scores: wave w owns the points 16 w ..
//                           16 w + 15 of the tile and every component tile; T = [x^2 | x] coef^T comes from
//                           v_mfma_f32_16x16x4_f32 with the [x^2 | x] operand formed as x is read from LDS. In the
//                           MFMA's C layout a point's scores lie in the 16 lanes of one lane group, so the row max,
//                           the argmax and the row sum are a per-lane pass in ascending component order and a
//                           four-step xor butterfly: no LDS, no barrier. R goes to an LDS tile [64][KPB + 4] only;
//                           the rows of bad points are zeroed in both tiles. Accumulation (ACC): R^T [x | x^2] by the
//                           same MFMA into register accumulators that live for the whole chunk; the KPB * 2 DPB / 256
//                           output tiles are dealt to the waves as a grid of min(4, DPB / 8) column groups by the
//                           rest as row groups, so an R value read feeds several MFMAs (at most 18 tiles = 72
//                           accumulator VGPRs a lane, in the 96 x 96 bucket; 64 at 128 x 64 and 64 x 128); tiles
//                           wholly past K or D are skipped. sum_i r_ik is a per-lane sum in the softmax pass, folded
//                           through LDS in a fixed order at the end of the chunk. Two barriers a tile.
//   gmm_fold_kernel         S[j] = the chunks' partials added in chunk order, a thread per entry; one more workgroup
//                           adds the fp64 ll partials (lane-strided ascending, then a butterfly).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace minips_k {

constexpr int kGmmMaxBlocks = 65535;
constexpr int kGmmMaxK = 128;
constexpr int kGmmMaxD = 128;
constexpr int kGmmMaxKD = 8192;   // KP * DP
constexpr int kGmmTile = 64;      // points per LDS tile
constexpr int kGmmChunk = 2048;   // points per partial

inline int gmm_pad(int64_t v) { return (int)((v + 15) / 16 * 16); }
inline bool gmm_shape_ok(int64_t K, int64_t D) {
  return K >= 1 && K <= kGmmMaxK && D >= 1 && D <= kGmmMaxD && gmm_pad(K) * gmm_pad(D) <= kGmmMaxKD;
}
inline int64_t gmm_chunks(int64_t n) { return (n + kGmmChunk - 1) / kGmmChunk; }

// s [K, 2D + 1] -> coef [K, 2 DP], cst [K]
void gmm_prepare(const float* s, int K, int D, float var_floor, float* coef, float* cst, hipStream_t stream);

// X [n, ld], shift [D], coef [K, 2 DP], cst [K]. S [K, 2D + 1] or null (the predict path), ll fp64 [1], assign int32
// [n] or null, logp fp32 [n] or null, bad int32 [1] or null (added to). part: gmm_chunks(n) * K * (2D + 1) floats
// (unused without S), llpart: gmm_chunks(n) doubles. blocks > 0 forces the grid size. n == 0 writes zeros.
void gmm_estep(const float* X, int64_t ld, int64_t n, int D, int K, const float* shift, const float* coef,
               const float* cst, float* S, double* ll, int32_t* assign, float* logp, int32_t* bad, float* part,
               double* llpart, int blocks, hipStream_t stream);

}  // namespace minips_k
