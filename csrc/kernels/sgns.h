// Word2vec by skip-gram with negative sampling (Mikolov et al., 2013) over the pulled rows of a window of pairs
// (sgns.hip; binding in csrc/bindings/sgns_py.cpp, module minips_amd._w2vk): the integer negative sampler, a fused
// forward and an atomic-free backward that writes the gradient of every unique pulled row once. The rule is the
// same in the kernels and in the CPU references ops.sgns_*.
//
// Rows      one sparse table of 2 V rows of d floats, d % 4 == 0, 4 <= d <= 512: key 2 w is word w's input vector
//           v_w, key 2 w + 1 its output vector u_w. 1 <= N <= 64 negatives per pair.
// Negatives integers only; mix (the splitmix64 finaliser) and mulhi_u64 are lda.h's. Once per corpus, on the host,
//           from the word counts c_w (int64, all ranks'): q_w = c_w > 0 ? max(1, llrint(c_w^0.75 2^20)) : 0 in
//           fp64, T = sum q_w, and an integer Vose alias table over V buckets of capacity T with the masses q_w V:
//           thr uint64 [V] (the part of bucket i that is word i's) and alias int32 [V] (whose the rest is). Exactly
//             thr[w] + sum_{i : alias[i] == w} (T - thr[i]) == q_w V        for every w,
//           so word w is drawn with probability q_w / T up to the 2^-64 of mulhi, and a word of count 0 never.
//           T < 2^59: with fewer than 2^40 tokens and V < 2^31, q_w <= c_w^0.75 2^20 + 1, and by the concavity of
//           x^0.75, sum_w c_w^0.75 <= V^0.25 (sum_w c_w)^0.75 < 2^7.75 2^30, so T < 2^57.75 + 2^31 < 2^59; thr <= T
//           fits an int64 and x below never overflows.
//           Draw t (0 <= t < N) of global pair g in epoch ep:
//             r = mix(mix(seed + ep * 0x9E3779B97F4A7C15) ^ (g * 64 + t));  i = mulhi_u64(r, V);
//             x = mulhi_u64(mix(r), T);  neg = x < thr[i] ? i : alias[i].
// lookups   the int64 key matrix [P, N + 2] of P pairs (centre c, context o): column 0 is 2 c, column 1 is 2 o + 1,
//           column 2 + t is 2 neg_t + 1 (drawn with g = pair_base + p, or read from explicit negatives int32
//           [P, N]). A word outside [0, V) (read from centres, contexts, negatives or alias) gives the key -1.
// forward   fp32, from inv [P (N + 2)] and rows [cap, ld] of the plan's Get. Pair p has the centre row
//           a = inv[p (N + 2)] and the targets t = 0 .. N with rows b_t = inv[p (N + 2) + 1 + t], y_t = [t == 0].
//           Target t >= 1 is masked when b_t == b_0 (word2vec's `if (target == word) continue`: the same pulled
//           row is the same key). A target whose row is outside [0, cap) does not exist; a pair whose centre row
//           is outside [0, cap) contributes nothing anywhere (its e, loss and h are written as 0).
//             s_t = <v_a, u_{b_t}>;  (e_t, loss_t) = logistic_head(s_t, y_t, gscale)      (member_rows.h's head)
//             e [P, N + 1], masked and missing entries exactly 0.0;  loss [P] = sum of the live loss_t, t ascending;
//             h [P, d],  h_p = sum_t e[p, t] u_{b_t}, t ascending            (the centre's gradient, as the FM's S)
//           gscale = 1 / (P * world): the mean loss over the global batch.
// backward  per unique pulled row r, its member lookups m in the lookup CSR's order (members / memrow, memrow
//           sorted): j = members[m], p = j / (N + 2), col = j % (N + 2). The member contributes h_p if col == 0,
//           else e[p, col - 1] * v_{a_p} (a_p = inv[p (N + 2)], read from rows). g_r = the sum over the members,
//           written exactly once; rows without lookups are untouched. A member outside [0, P (N + 2)) or a centre
//           row outside [0, cap) is skipped.
//
// Mapping (wave64, 256-thread workgroups). L = min(64, pow2ceil(d / 4)) lanes own a pair (forward) or a row
// (backward), lane l the float4 l and, when d > 256, also the float4 64 + l: several pairs share a wave at small d,
// one pair takes a wave at d >= 256. When rows, ld, h or grad_rows are not 16-byte friendly the same kernels run
// with one lane per element (L = min(64, pow2ceil(d)), up to 8 elements a lane): slower, never refused.
//   lookups   one thread per key.
//   forward   a lane group per pair; a dot product is the lane's own products in column order, then a __shfl_xor
//             fold in a fixed order; the row of target t + 1 is in flight while target t is folded. No LDS.
//   backward  by the member count M of the row (a row starts at its binary search in memrow):
//             M <= kSgnsGroupMax (32)              one lane group walks the members in order
//             kSgnsGroupMax < M <= kSgnsWaveMax    a whole wave: members strided over its groups, fixed-order fold
//             M > kSgnsWaveMax (512)               workgroups, by the chunk rule of member_rows.h: a 256-thread
//                                                  block (waves folded through LDS) per kSgnsChunk (256) members
//           A member's term is three dependent loads (member -> centre row index -> row), so a walk fetches several
//           members before it adds the first, in the order of the plain loop; and the wave limit is lower than the
//           FM's 2048, because at d >= 128 a wave holds two rows' lane groups or one and a hot row would be its
//           long serial chain (frequent words are this model's normal case).
// No float atomics anywhere. Every output is a function of the inputs alone: the same bits on every run and for
// every grid size. Every index read from a tensor is checked on the device and skipped. Empty inputs launch nothing.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace minips_k {

constexpr int kSgnsMaxBlocks = 65535;
constexpr int kSgnsMinDim = 4;
constexpr int kSgnsMaxDim = 512;
constexpr int kSgnsMaxNeg = 64;      // g * 64 + t keys a draw
constexpr int kSgnsGroupMax = 32;    // members one lane group walks alone
constexpr int kSgnsWaveMax = 512;    // members one wave walks; more go to the chunked workgroup path
constexpr int kSgnsChunk = 256;      // members per block of the workgroup path (kSgnsWaveMax >= 2 * kSgnsChunk)

inline bool sgns_dim_ok(int64_t d) { return d >= kSgnsMinDim && d <= kSgnsMaxDim && d % 4 == 0; }
inline bool sgns_neg_ok(int64_t N) { return N >= 1 && N <= kSgnsMaxNeg; }

// centres / contexts int64 [P]; thr [V] (uint64), alias int32 [V], 1 <= T; negatives int32 [P, N] or nullptr (then
// thr and alias are not read and may be null); keys int64 [P, N + 2]. P == 0 launches nothing.
void sgns_lookups(const int64_t* centres, const int64_t* contexts, const uint64_t* thr, const int32_t* alias,
                  int64_t V, uint64_t T, uint64_t seed, uint64_t epoch, uint64_t pair_base, int N,
                  const int32_t* negatives, int64_t P, int64_t* keys, hipStream_t stream);

// inv int64 [P (N + 2)], rows [cap, ld] (ld >= d); e [P, N + 1], loss [P], h [P, d] contiguous. blocks > 0 forces
// the grid size. P == 0 launches nothing.
void sgns_forward(const int64_t* inv, const float* rows, int64_t ld, int64_t cap, int d, int N, float gscale,
                  int64_t P, float* e, float* loss, float* h, int blocks, hipStream_t stream);

// floats of the workspace `part` sgns_backward needs for n lookups of d-wide rows (0: none)
int64_t sgns_backward_part_floats(int64_t n, int d);

// members / memrow int32 [n], n = P (N + 2) (memrow sorted; the unique count memrow[n - 1] + 1 is read on the
// device), inv [n], e [P, N + 1], h [P, d], rows [cap, ld]; grad_rows [cap, d] contiguous. part:
// sgns_backward_part_floats(n, d) floats. n == 0 launches nothing.
void sgns_backward(const int32_t* members, const int32_t* memrow, const int64_t* inv, const float* e, const float* h,
                   const float* rows, int64_t ld, int64_t cap, int d, int N, int64_t P, float* grad_rows, float* part,
                   int blocks, hipStream_t stream);

}  // namespace minips_k
