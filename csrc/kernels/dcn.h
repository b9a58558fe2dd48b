// Deep & Cross (DCN, Wang et al., 2017) on the Wide & Deep step (dcn.hip; binding in csrc/bindings/dcn_py.cpp,
// module minips_amd._dcnk): L cross layers with vector weights over the whole assembled input -- the field
// embeddings and the dense features together -- whose output feeds the wide logit through one more vector.
// (2L+1) d dense parameters, trained by the dense table's Adam.
//
// X [B, ldx] bf16 is the assembled input (wd_assemble / wd_assemble_tab); d = F D + n_dense is every column left of
// the ones column. x_0 = float(X[b, 0:d]) (bf16 values, exact in fp32). Pc [(2L+1), dp] bf16, dp = align8(d), holds
// the rows w_0, b_0, ..., w_{L-1}, b_{L-1}, w_c as the dense table's pulled values; below w_L means w_c. The model:
//     s_l = <x_l, w_l>,   x_{l+1} = x_0 s_l + b_l + x_l   (l = 0 .. L-1),    wide[b] += <x_L, w_c>
// With a_0 = 1, B_0 = 0, a_{l+1} = a_l + s_l, B_{l+1} = B_l + b_l it is exactly x_l = a_l x_0 + B_l, so a sample
// needs only the L+1 dot products p_j = <x_0, w_j> and the parameter-only constants k_j = <B_j, w_j> (k_0 = 0).
//
// THE RULE. Everything in fp32, every operation rounded on its own (contraction off, as in ftrl_rule.h); "x = y op z"
// below is one rounded operation.
//   reductions over d (forward only: p [B, L+1] and k [L+1], kept for the backward, which recomputes nothing over d):
//     a lane adds its products x_c w_jc (for k: B_jc w_jc, B_jc the running sum b_0c + ... + b_{j-1}c) in ascending
//     column order into one accumulator per j that starts at +0, and the 64 lanes are folded by __shfl_xor with
//     offsets 32, 16, 8, 4, 2, 1. The lane mapping (below) fixes the bits; a reference that sums in another order
//     agrees within the rounding of a length-d dot product.
//   forward, per sample:    a = 1;  for l = 0 .. L-1: t = a p_l; s_l = t + k_l; a_{l+1} = a_l + s_l
//                           t = a_L p_L; c = t + k_L; wide[b] = wide[b] + c
//   backward, per sample:   dz = dwide[b]; a_0 .. a_L as in the forward;  ds_L = dz;  r = dz p_L
//                           for l = L-1 .. 0: ds_l = r;  t = ds_l p_l;  r = r + t
//                           m_j = ds_j a_j   (j = 0 .. L)
//     embedding gradient, columns c < F D:  g = m_0 w_0c;  for j = 1 .. L: t = m_j w_jc; g = g + t   (w_c's term last)
//                           field f = c / D, row r = perm[b F + f] (b F + f without perm) of dX viewed as [B F, D]:
//                           dX[r, c % D] = bf16_rne(float(dX[r, c % D]) + g)   (common.h's pack_bf2 / f2bf)
//                           a perm entry outside [0, B F) is skipped whole; columns F D <= c < d get no gradient.
//     batch sums:           T_jc = sum_b m_j x_0c and Sd_j = sum_b ds_j, in the order of the mapping below
//   fold, per column c:     Bc = 0;  for l = 0 .. L: t = Bc Sd_l; dw = T_lc + t; Gc[w_l, c] = Gc[w_l, c] + dw;
//                                                    (l < L) Bc = Bc + b_lc
//                           r = Sd_L w_Lc;  for l = L-1 .. 0: Gc[b_l, c] = Gc[b_l, c] + r;  t = Sd_l w_lc;  r = r + t
//
// Mapping (wave64, 256 threads per workgroup).
//   vector form -- D % 8 == 0 (backward), ldx % 8 == 0, X, Pc (dX, part) 16-byte aligned: a piece is 8 consecutive
//     columns, one 16-byte load; lane n owns the pieces n, n + 64, ... (at most 4: d <= 2048). A lane always owns the
//     same columns, so it keeps its slice of the L+1 weight rows in registers (packed bf16) across samples. The last
//     piece of a d that is no multiple of 8 is loaded element by element: columns >= d of X and of Pc are never read.
//   scalar form -- anything else: lane n owns the columns n, n + 64, ..., one element per lane-step, the weights
//     re-read per sample. Slower, never refused.
//   forward   one wave per sample, grid-stride. Every wave derives k itself (no cross-workgroup dependency), wave 0
//             stores it; lane 0 finishes the scalar rule, stores p[b, :] and updates wide[b].
//   backward  a chunk of kDcnChunk consecutive samples is one workgroup's job (grid-stride over chunks): wave w takes
//             the chunk's samples w, w + 4, ... in ascending order, every lane runs the scalar rule uniformly, updates
//             its pieces of dX and adds m_j x_0 and ds_j into register accumulators that start at +0; the four waves
//             are folded through LDS as ((w0 + w1) + w2) + w3 and stored in part [nchunks, (L+1) dp + kDcnTrailer]:
//             the L+1 partial T_j rows, then the L+1 partial Sd_j. No float atomics. A wave loads its next sample's
//             X and dX pieces one sample ahead: the in-range entries of perm must be distinct (a permutation, as the
//             planner's is), so that the next sample's rows are not the ones being written.
//   fold      one thread per (row j, column c) adds the chunks in chunk order and adds the gradients into Gc.
// Every output is a function of the inputs alone: the same bits on every run and for every grid size.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace minips_k {

constexpr int kDcnMaxBlocks = 65535;
constexpr int kDcnMaxD = 2048;    // columns of x_0 (4 pieces per lane)
constexpr int kDcnMaxL = 4;       // cross layers
constexpr int kDcnMaxEmb = 64;    // D
constexpr int kDcnChunk = 32;     // samples per partial row of the batch sums: independent of the grid
constexpr int kDcnTrailer = 8;    // fp32 slots behind a chunk's rows (the first L+1 hold the scalar sums)

inline int dcn_dp(int d) { return (d + 7) / 8 * 8; }
inline int64_t dcn_part_cols(int d, int L) { return (int64_t)(L + 1) * dcn_dp(d) + kDcnTrailer; }
inline int64_t dcn_nchunks(int64_t B) { return (B + kDcnChunk - 1) / kDcnChunk; }

// bf16 travels as raw uint16_t (common.h's bf16_t). X [B, ldx] bf16 (columns < d are read), Pc [(2L+1), dp] bf16,
// wide [B] fp32 (updated in place), p [B, L+1] and k [L+1] fp32 (written). blocks > 0 forces the grid size.
// 1 <= d <= kDcnMaxD, d <= ldx, 1 <= L <= kDcnMaxL. B == 0 launches nothing.
void wd_cross_forward(const uint16_t* X, int64_t ldx, int64_t B, int d, const uint16_t* Pc, int L, float* wide,
                      float* p, float* k, int blocks, hipStream_t stream);

// X, Pc, p, k as above, dwide [B], perm nullable int32 [B F], dX bf16 [B F, D] contiguous (updated in place),
// part fp32 [dcn_nchunks(B), dcn_part_cols(d, L)] (written). F >= 1, 1 <= D <= kDcnMaxEmb, F D <= d, B F < 2^31.
// B == 0 launches nothing.
void wd_cross_backward(const uint16_t* X, int64_t ldx, int64_t B, int d, const float* p, const float* k,
                       const float* dwide, const uint16_t* Pc, int L, const int32_t* perm, uint16_t* dX, int F, int D,
                       float* part, int blocks, hipStream_t stream);

// part as written by the backward for nchunks chunks, Gc fp32 [(2L+1), dp] (added to). nchunks == 0 launches nothing.
void wd_cross_fold(const float* part, int64_t nchunks, const uint16_t* Pc, int d, int L, float* Gc,
                   hipStream_t stream);

}  // namespace minips_k
