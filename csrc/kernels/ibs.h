// Two-tower retrieval with the in-batch sampled softmax (Yi et al., 2019, "Sampling-bias-corrected neural modeling
// for large corpus item recommendations") over the pulled rows of a batch of (user, item) pairs (ibs.hip; binding in
// csrc/bindings/ibs_py.cpp, module minips_amd._ibsk): a fused forward, two fused gradient sweeps and an atomic-free
// row reduce. The P x P logit matrix never reaches memory. The rule is the same in the kernels and in the CPU
// references ops.ibs_*.
//
// Inputs    P pairs. inv int64 [2 P], a plan's row indices of the key matrix [P, 2]: lookup 2 p is pair p's user row,
//           lookup 2 p + 1 its item row. rows fp32 [cap, ld], width d, d % 4 == 0 and 8 <= d <= 128;
//           KP = 16 ceil(d / 16). Temperature tau > 0. logq fp32 [P] or none: the log sampling probability of pair
//           q's item (the bias correction). gscale = 1 / (P * world).
//           a_p = rows[inv[2 p]], b_q = rows[inv[2 q + 1]].
// Validity  a pair is valid iff both its inv lie in [0, cap). An invalid pair is neither a query nor a candidate:
//           its loss and lse are written as 0 and its lookups add exactly 0 to their rows.
// Live      for query p, candidate q is live iff both are valid and (q == p or inv[2 q + 1] != inv[2 p + 1]): another
//           pair carrying the same item is an accidental hit and is left out of the softmax, not counted as a
//           negative.
// forward   fp32:  s_pq = <a_p, b_q> * rtau - logq_q   (rtau = 1 / tau rounded to fp32; no logq: 0)
//                  lse_p = log sum_{q live} exp(s_pq),  loss_p = lse_p - s_pp
// backward  G_pq = (exp(s_pq - lse_p) - [p == q]) * gs for live q, else 0   (gs = gscale / tau rounded to fp32)
//           dA_p = sum_q G_pq b_q,  dB_q = sum_p G_pq a_p
//           For every unique pulled row u with an in-range lookup: grad_rows[u] = the sum over its member lookups, in
//           member order (members / memrow: the plan's lookup CSR), of that lookup's dA row (even lookup) or dB row
//           (odd lookup). Rows without lookups stay untouched; columns >= d of the rows are never read or written.
//
// Mapping (wave64, 256-thread workgroups, one instantiation per KP, scratch 0). One tile routine, resident side
// against streamed side: a workgroup owns 64 pairs of the resident side, staged once into an LDS tile [64][KP + 4]
// (float4 loads when ld and the base are 16-byte friendly, scalar ones otherwise); the other side is streamed in
// tiles of 64 pairs through two LDS buffers, tile t + 1's global loads in flight while tile t is multiplied. Each of
// the four waves owns a 16-row strip of the 64 x 64 logit tile, v_mfma_f32_16x16x4_f32 over d; the live mask comes
// from the item rows staged with the tiles.
//   forward   resident = the queries. Online softmax per row: running maximum and sum, folded across the 16 lanes of
//             a row by __shfl_xor in a fixed order; s_pp is the diagonal tile's own accumulator. Writes lse, loss.
//   gradient  the same routine twice, templated on the resident side: users (dA; the query's lse is the resident
//             row's) and items (dB; the query's lse is the streamed column's). The logit tile is recomputed, G parked
//             in an LDS tile [64][68] whose rows are the resident pairs, and G x (streamed tile) accumulated by the
//             same MFMA in registers over the whole sweep, K = 64 a tile. Every resident pair's dA or dB row is
//             written once to the workspace ws [2 P, KP], row = its lookup. No float atomics, no cross-workgroup sum.
//   reduce    on member_rows.h: a row of up to kIbsWaveMax members is summed by a lane group (a float4 a lane) in
//             member order; a heavier row by the chunk rule, a 256-thread block per kIbsChunk members.
// LDS: (3 (KP + 4) + 6) 256 B forward, 17408 B more for G in the gradient sweeps: 120320 B at KP = 128.
// Every output is a function of the inputs alone: the same bits on every run and for every grid size. Every index
// read from a tensor is checked on the device. Empty inputs launch nothing.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace minips_k {

constexpr int kIbsMaxBlocks = 65535;
constexpr int kIbsMinD = 8;
constexpr int kIbsMaxD = 128;
constexpr int kIbsTile = 64;       // pairs per resident / streamed tile
constexpr int kIbsWaveMax = 512;   // members a lane group sums alone; more go to the chunked workgroup path
constexpr int kIbsChunk = 256;     // members per block of the workgroup path (kIbsWaveMax >= 2 * kIbsChunk)

inline bool ibs_d_ok(int64_t d) { return d >= kIbsMinD && d <= kIbsMaxD && d % 4 == 0; }
inline int ibs_kp(int d) { return 16 * ((d + 15) / 16); }

// inv int64 [2 P], rows [cap, ld] (ld >= d), logq [P] or nullptr; lse, loss [P]. blocks > 0 forces the grid size.
// P == 0 launches nothing.
void ibs_forward(const int64_t* inv, const float* rows, int64_t ld, int64_t cap, int d, float tau, const float* logq,
                 int64_t P, float* lse, float* loss, int blocks, hipStream_t stream);

// floats of the workspaces ibs_backward needs: ws [2 P, KP] and the chunk rule's partials (0: none)
int64_t ibs_backward_ws_floats(int64_t P, int d);
int64_t ibs_backward_part_floats(int64_t P, int d);

// members / memrow int32 [2 P] (memrow sorted; the unique count memrow[2 P - 1] + 1 is read on the device), lse [P]
// from ibs_forward on the same inputs; grad_rows [cap, d] contiguous. P == 0 launches nothing.
void ibs_backward(const int32_t* members, const int32_t* memrow, const int64_t* inv, const float* rows, int64_t ld,
                  int64_t cap, int d, float tau, const float* logq, const float* lse, float gscale, int64_t P,
                  float* grad_rows, float* ws, float* part, int blocks, hipStream_t stream);

}  // namespace minips_k
