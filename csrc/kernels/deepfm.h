// DeepFM's second-order term (Guo et al., 2017) on the Wide & Deep step (deepfm.hip; binding in
// csrc/bindings/deepfm_py.cpp, module minips_amd._dfmk): the factorization-machine interaction of the F field
// embeddings the deep tower already reads, added to the wide logit in the forward and to the embedding
// gradient in the backward. No new parameter, table state or collective.
//
// X [B, ldx] bf16 is the assembled input (wd_assemble / wd_assemble_tab): the embedding of field f of sample b
// lies in columns [f D, f D + D). v_fc = float(X[b, f D + c]) (a bf16 value, exact in fp32). Everything in
// fp32, every operation rounded on its own (contraction off, as in ftrl_rule.h):
//
// forward   S_bc = sum_f v_fc
//           q_bc = sum_f v_fc v_fc
//           fm_b = 0.5 sum_c (S_bc S_bc - q_bc)         (the difference per column, not between two large sums)
//           wide[b] += fm_b;  S [B, D] is kept for the backward
// backward  per lookup (b, f): row r = perm[b F + f] (b F + f without perm) of dX viewed as [B F, D]
//           dX[r, c] = bf16_rne( float(dX[r, c]) + dwide[b] * (S_bc - v_fc) )
//           the subtraction, the product and the sum are three roundings; the conversion is common.h's
//           pack_bf2 / f2bf. A perm entry outside [0, B F) is skipped: nothing of that row is touched.
// This is the exact gradient of fm_b = sum_{f<g} <v_f, v_g> with respect to the embedding of lookup (b, f),
// added to the deep tower's before the embedding backward sums the lookups of a row.
//
// Mapping (wave64). Vector form -- D in {8, 16, 32, 64}, X (S, dX) 16-byte aligned, ldx % 8 == 0: L = D / 8
// lanes own one 16-byte load of 8 bf16 of a field row each, so a wave holds 64 / L lane groups. Any other D in
// [1, 64] or alignment: one lane per column (L = pow2ceil(D)); slower, never refused.
//   forward   one wave per sample; group g takes the fields g, g + 64/L, ...; the groups are folded by
//             __shfl_xor in a fixed order; lanes 0 .. L-1 store S (two float4 each in vector form), lane 0
//             finishes fm and updates wide[b]. Columns >= F D of X are never read.
//   backward  grid-stride over the lookups, one lane group per lookup: one 16-byte load each of X and dX, two
//             float4 of S and one 16-byte store per lane in vector form. With a permutation in perm every dX
//             row is written at most once.
// No atomics, no LDS, no cross-workgroup communication. Every output is a function of the inputs alone: the
// same bits on every run and for every grid size.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace minips_k {

constexpr int kDfmMaxBlocks = 65535;
constexpr int kDfmMaxD = 64;

inline bool dfm_shape_ok(int64_t F, int64_t D, int64_t ldx) {
  return D >= 1 && D <= kDfmMaxD && F >= 1 && F <= (1ll << 31) / D && F * D <= ldx;
}

// bf16 travels as raw uint16_t (common.h's bf16_t). X [B, ldx] bf16 (columns < F D are read), wide [B] fp32
// (updated in place), S [B, D] fp32 (written). blocks > 0 forces the grid size. B == 0 launches nothing.
void wd_fm_forward(const uint16_t* X, int64_t ldx, int64_t B, int F, int D, float* wide, float* S, int blocks,
                   hipStream_t stream);

// X as above, S [B, D], dwide [B], perm nullable int32 [B F], dX bf16 [B F, D] contiguous (updated in place).
// B F < 2^31. B == 0 launches nothing.
void wd_fm_backward(const uint16_t* X, int64_t ldx, const float* S, const float* dwide, const int32_t* perm,
                    uint16_t* dX, int64_t B, int F, int D, int blocks, hipStream_t stream);

}  // namespace minips_k
