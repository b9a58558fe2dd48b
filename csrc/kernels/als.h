// Collaborative filtering by alternating least squares (Zhou et al. 2008, "ALS-WR"; Hu, Koren and Volinsky 2008 for
// implicit feedback) over the pulled rows of one half-sweep (als.hip; binding in csrc/bindings/als_py.cpp, module
// minips_amd._alsk): a gathered SYRK and a small SPD solve per entity, fused in one workgroup. Not a gradient method:
// the new row is solved for and the table is pushed x_new - x_old. The rule is the same in the kernels and in the CPU
// references ops.als_*.
//
// Rows      one sparse table of U + I fp32 rows of k floats, k % 4 == 0, 4 <= k <= 128: key u < U is user u's
//           factor, key U + i item i's. A half-sweep solves one side (its entities) from the other side's rows.
// Lookups   entity e (0 <= e < B) has the lookups j in [rowptr[e], rowptr[e + 1]) (rowptr int64, clamped to [0, n]).
//           Lookup j reads the pulled row y_j = rows[inv[j]] (rows [cap, ld], ld >= k) with two fp32 weights a_j
//           and c_j. A lookup whose inv[j] lies outside [0, cap) contributes nothing.
// System    with reg_e (fp32 per entity) and an optional shared G0 [k, k] (fp32, symmetric, its lower triangle read):
//             A_e = (sum_j a_j y_j y_j^T + G0) + reg_e I        b_e = sum_j c_j y_j        x_e = A_e^-1 b_e
//           by a Cholesky factorisation A = L L^T and two triangular solves, all in fp32.
//             explicit ALS-WR   a = 1, c = r, reg = lambda n_e (or lambda), no G0
//             implicit          a = alpha r, c = 1 + alpha r, reg = lambda, G0 = Y^T Y over the whole other side
// Skip      an entity with no contributing lookup is skipped: x_out = x_old, delta = 0. An entity whose factorisation
//           meets a pivot that is <= 0 or not finite is skipped the same way and counted in the int32 counter `bad`.
// Outputs   x_out[slot[e]] = x_e, delta[slot[e]] = x_e - x_old[slot[e]] (x_old, x_out, delta [m, k] contiguous; slot
//           int64 [B], a slot outside [0, m) writes nothing). slot is a permutation in the model (the entity plan's
//           inv), so every output row is written exactly once: no atomics.
// Chunks    fixed on the host, once (ops.als_chunks): entity e gets max(1, ceil(n_e / chunk)) descriptors
//           (entity, lo, hi) int32 of consecutive lookup ranges. The descriptors of the entities with more than one
//           come first, in entity order (n_multi_desc of them); `multi` int32 [n_multi, 3] lists those entities as
//           (entity, first descriptor, descriptors). Every sum's order is a function of the descriptors alone, so a
//           result is the same bits on every run and for every grid size. desc and multi must come from
//           ops.als_chunks of the same rowptr: the kernels keep every index in bounds (a descriptor whose entity
//           lies outside [0, B) is skipped, its workspace slot zeroed), but descriptors that do not tile an
//           entity's lookups give that entity a wrong system, not an error.
//
// Kernels (wave64, 256-thread workgroups, KP = 16 ceil(k / 16) the padded width, templated)
//   als_solve_kernel<KP>   a workgroup per descriptor. 64 member rows a stage are gathered into an LDS tile
//                          [64][KP + 4] (k / 4 lanes a row, a float4 each; a scalar load path when rows or ld are not
//                          16-byte friendly; columns k .. KP, missing rows and their weights zero). Two tiles: the
//                          next stage's global loads are in flight while this one is multiplied. The lower-triangle
//                          16 x 16 tiles of the Gram matrix (at most 36) are dealt round-robin to the four waves and
//                          accumulated in registers by v_mfma_f32_16x16x4_f32, four members an instruction in CSR
//                          order, a_t applied to the A operand as it is read; thread c < k adds c_t y_t[c] in member
//                          order. A single-descriptor entity is then solved in the same workgroup: the accumulators
//                          go to LDS as a KP x (KP + 1) lower triangle over the staging tiles (about 68 KiB at KP =
//                          128: two workgroups a CU), G0 and reg are added, and a blocked right-looking Cholesky of
//                          panel width 16 runs -- one wave factors the diagonal block in registers, every row below
//                          solves its 16 entries against it, the trailing tiles are updated by MFMA, three barriers a
//                          panel, loops bounded by k -- followed by both triangular solves in one wave,
//                          column-oriented, two elements a lane at k = 128, no barriers. A descriptor of a
//                          multi-chunk entity writes its packed (A, b, count) partial to a workspace slot instead.
//   als_fold_solve_kernel<KP>  a workgroup per multi-chunk entity: adds its partials in chunk order, same solve.
//   als_gram_kernel<KP>    G = sum_r y_r y_r^T over a contiguous strip of kAlsGramStrip shard rows a workgroup (the
//                          same tile code, a = 1), one packed partial per workgroup; als_gram_fold_kernel adds the
//                          partials in index order and writes the symmetric [k, k].
// Every index read from a tensor is checked on the device and skipped. Empty inputs launch nothing.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace minips_k {

constexpr int kAlsMaxBlocks = 65535;
constexpr int kAlsMinK = 4;
constexpr int kAlsMaxK = 128;
constexpr int kAlsStage = 64;        // member rows per LDS tile
constexpr int kAlsGramStrip = 256;   // shard rows per workgroup of als_gram
constexpr int kAlsMaxChunk = 1 << 20;  // a partial's lookup count is kept in a float

inline bool als_k_ok(int64_t k) { return k >= kAlsMinK && k <= kAlsMaxK && k % 4 == 0; }
inline int als_kp(int k) { return (k + 15) / 16 * 16; }
// floats of one multi-chunk partial: the packed lower triangle, b and the contributing-lookup count (padded)
inline int64_t als_slot_floats(int k) {
  const int64_t kp = als_kp(k);
  return kp * (kp + 1) / 2 + kp + 4;
}
// floats of als_gram's workspace for R rows
inline int64_t als_gram_part_floats(int64_t R, int k) {
  const int64_t kp = als_kp(k);
  return (R + kAlsGramStrip - 1) / kAlsGramStrip * (kp * (kp + 1) / 2);
}

// rowptr int64 [B + 1], inv int64 [n], a / c fp32 [n], rows [cap, ld], reg fp32 [B], slot int64 [B], x_old / x_out /
// delta [m, k], desc int32 [n_desc, 3], multi int32 [n_multi, 3], ws n_multi_desc * als_slot_floats(k) floats (may
// be null when n_multi_desc == 0), gram0 [k, k] or null, bad int32 [1] or null. blocks > 0 forces the grid size.
// n_desc == 0 launches nothing.
void als_solve(const int64_t* rowptr, const int64_t* inv, const float* a, const float* c, int64_t n, const float* rows,
               int64_t ld, int64_t cap, int k, const float* reg, const int64_t* slot, int64_t B, const float* x_old,
               float* x_out, float* delta, int64_t m, const int32_t* desc, int64_t n_desc, int64_t n_multi_desc,
               const int32_t* multi, int64_t n_multi, float* ws, const float* gram0, int32_t* bad, int blocks,
               hipStream_t stream);

// rows [R, ld] -> out [k, k] contiguous; part: als_gram_part_floats(R, k) floats. R == 0 writes zeros.
void als_gram(const float* rows, int64_t ld, int64_t R, int k, float* part, float* out, hipStream_t stream);

}  // namespace minips_k
