// Field-aware factorization machine (Juan et al., 2016) over a CSR batch of pulled split rows (ffm.hip; binding
// in csrc/bindings/ffm_py.cpp, module minips_amd._ffmk): a fused pairwise forward and an atomic-free backward
// that writes the gradient of every unique pulled row once.
//
// Row of feature u: [v_u,0,0..k-1 | v_u,1,0..k-1 | ... | v_u,F-1,0..k-1 | w_u | 0 0 0], width W = F k + 4; slot g
// (columns [g k, g k + k)) is the vector u uses against a partner of field g. k % 4 == 0, 4 <= k <= 16,
// 1 <= F <= 64, F k <= 512. Sample b holds the lookups j in [rowptr[b], rowptr[b+1]); lookup j reads pulled
// row inv[j] with value x_j and field fields[j] (int32 in [0, F)); a feature occurring twice in a sample is two
// lookups, several lookups of a sample may share a field. y = label > 0.5. Everything in fp32:
//
// forward   z_b    = w0 + sum_j w_{inv[j]} x_j + sum_{i<j} <v_{inv[i],fields[j]}, v_{inv[j],fields[i]}> x_i x_j
//           loss_b = max(z, 0) - z y + log1p(exp(-|z|))                 (an empty sample: z = w0)
//           dz_b   = (sigmoid(z_b) - y) * gscale                        (gscale = 1 / (B * world): mean loss)
//           rowid[j] = b
//           the pairs are formed one by one: no aggregate-and-subtract, no cancellation. F = 1 is the FM.
// backward  per unique pulled row u, its member lookups m (inv[m] == u, sample b_m, c_m = dz[b_m] x_m):
//           g_u[g k + c] = sum_m c_m sum_{j in b_m, j != m, fields[j] == g} v_{inv[j],fields[m],c} x_j
//           g_u[F k]     = sum_m c_m;  columns F k + 1 .. F k + 3 are written as 0
//           rows without lookups are left untouched. Self is skipped, not subtracted: the exact gradient,
//           also with duplicates and shared fields. Everything is recomputed from rows: no per-lookup gradient
//           rows and no per-sample aggregate exist anywhere.
// skipped   a lookup whose inv is outside [0, cap) or whose field is outside [0, F) contributes nothing anywhere
//           and receives nothing; a member or sample index out of range likewise; rowptr is clamped to [0, n].
//
// Mapping. E floats per lane and load (4: one float4; 1: the form for rows / ld / grad_rows that are not 16-byte
// friendly -- slower, never refused).
//   forward   one wave per sample. The m (m - 1) / 2 pairs are enumerated round-robin, pair q = (i, d):
//             j = (i + d) mod m, d = 1 .. m / 2 (the last round of an even m covers i < m / 2 only), q = i (m / 2)
//             + d - 1 -- so the 64 lanes of a step hold a few i and consecutive j: with a sample's lookups in
//             field order the v_{i, f_j} side is read as consecutive slots of a few rows. Lane l takes the pairs
//             l, l + 64, ... in order (the (i, d) of the next pair by two adds, no division in the loop); the
//             lanes' sums are folded by __shfl_xor in a fixed order. No LDS.
//   backward  L = pow2ceil(W / E) lanes (at most 64, then C = ceil(W / (64 E)) columns chunks per lane) own the
//             columns of a row's gradient; 64 / L lane groups per wave. For one member the group's lanes first
//             take *partners*: lane t loads the k / E-th part t % (k / E) of partner t / (k / E)'s vector against
//             the member's field (all gathers of a step in flight at once, no lane idles with one feature per
//             field), scaled by c_m x_j; then the owners of the columns walk the step's partners in order with
//             shuffles and add those whose field is their slot. By the member count M of the row:
//             M <= kFfmGroupMax                 one lane group walks the members in order
//             kFfmGroupMax < M <= kFfmWaveMax   a whole wave: members strided over its groups, fixed-order fold
//             M > kFfmWaveMax                   workgroups, by the chunk rule of member_rows.h: a 256-thread block
//                                               (waves folded through LDS) per kFfmChunk members
//             (a member costs nnz_b gathers and a walk over them, not one gather as in the FM: the limits are
//             far below fm.h's -- with 512 | 256 a Zipf(1.05) batch spent 2.2 ms in rows that one wave walked
//             alone (profiles/ffm/kernels.txt). A wave takes consecutive tiles of rows, so memrow is searched once
//             per wave and a row starts where the row before it ended. `part` holds 2 W floats per chunk:
//             n W / 4 bytes.)
// No float atomics anywhere. Every output is a function of the inputs alone: the same bits on every run and for
// every grid size.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace minips_k {

constexpr int kFfmMaxBlocks = 65535;
constexpr int kFfmMaxF = 64;
constexpr int kFfmMaxK = 16;
constexpr int kFfmMaxFK = 512;
constexpr int kFfmGroupMax = 8;    // members one lane group walks alone
constexpr int kFfmWaveMax = 64;    // members one wave walks; more go to the chunked workgroup path
constexpr int kFfmChunk = 32;      // members per block of the workgroup path (kFfmWaveMax >= 2 * kFfmChunk)

inline bool ffm_shape_ok(int64_t F, int64_t k) {
  return k >= 4 && k <= kFfmMaxK && k % 4 == 0 && F >= 1 && F <= kFfmMaxF && F * k <= kFfmMaxFK;
}

// rowptr [B+1], inv / vals / fields [n] (n = rowptr[B], given by the caller), labels [B], rows [cap, ld]
// (ld >= F k + 4), w0 nullable device scalar. Outputs z / dz / loss [B], rowid [n]. blocks > 0 forces the grid
// size. B == 0 launches nothing.
void ffm_forward(const int64_t* rowptr, const int64_t* inv, const float* vals, const int32_t* fields,
                 const float* labels, const float* rows, int64_t ld, int64_t cap, int F, int k, const float* w0,
                 float gscale, int64_t B, int64_t n, float* z, float* dz, float* loss, int32_t* rowid, int blocks,
                 hipStream_t stream);

// floats of the workspace `part` ffm_backward needs for n lookups of width-W rows (0: none)
int64_t ffm_backward_part_floats(int64_t n, int W);

// members / memrow [n] (memrow sorted, the unique count memrow[n-1] + 1 is read on the device), rowid / vals /
// fields / inv [n], rowptr [B+1], dz [B], rows [cap, ld]; grad_rows [cap, F k + 4] contiguous. part:
// ffm_backward_part_floats(n, F k + 4) floats. n == 0 launches nothing.
void ffm_backward(const int32_t* members, const int32_t* memrow, const int32_t* rowid, const int64_t* rowptr,
                  const int64_t* inv, const float* vals, const int32_t* fields, const float* dz, const float* rows,
                  int64_t ld, int64_t cap, int F, int k, int64_t B, int64_t n, float* grad_rows, float* part,
                  int blocks, hipStream_t stream);

}  // namespace minips_k
