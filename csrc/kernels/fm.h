// 2-way factorization machine (Rendle, 2010) over a CSR batch of pulled split rows (fm.hip; binding in
// csrc/bindings/fm_py.cpp, module minips_amd._fmk): a fused forward and an atomic-free backward that
// writes the gradient of every unique pulled row once.
//
// Row of feature u: [v_u0 .. v_u,k-1 | w_u | 0 0 0], width W = k + 4, k % 4 == 0, 4 <= k <= 60 (SparseTable
// split rows, the layout of Wide & Deep). Sample b holds the lookups j in [rowptr[b], rowptr[b+1]); lookup j
// reads pulled row inv[j] with value x_j (a feature occurring twice in a sample is two lookups).
// y = label > 0.5 (covers {0,1} and {-1,1}). Everything in fp32:
//
// forward   S_bf  = sum_j v_{inv[j],f} x_j
//           Q_b   = sum_j sum_f (v_{inv[j],f} x_j)^2
//           lin_b = sum_j w_{inv[j]} x_j
//           z_b   = w0 + lin_b + (sum_f S_bf^2 - Q_b) / 2              (an empty sample: z = w0)
//           loss_b = max(z, 0) - z y + log1p(exp(-|z|))
//           dz_b  = (sigmoid(z_b) - y) * gscale                         (gscale = 1 / (B * world): mean loss)
//           rowid[j] = b
// backward  per unique pulled row u, its member lookups m in CSR (members) order, c_m = dz[b_m] x_m:
//           g_uf  = sum_m c_m (S[b_m, f] - v_uf x_m)   f < k             (exact with duplicates in a sample)
//           g_uk  = sum_m c_m;  columns k+1 .. k+3 are written as 0
//           rows without lookups are left untouched
//
// Mapping. L = pow2ceil(W / 4) lanes own one float4 of a row each (L = 2 / 4 / 8 / 16 for k = 4 / 8-12 / 16-28 /
// 32-60), so a wave holds 64 / L lane groups; the lane of the last float4 carries the linear column. When
// rows, ld, S or grad_rows are not 16-byte friendly the same kernels run with one lane per element
// (L = pow2ceil(W)): slower, never refused.
//   forward   one wave per sample; inv / vals of 64 lookups are read coalesced and handed to the groups by
//             shuffles, group g takes the lookups g, g + 64/L, ...; groups folded by __shfl_xor in a fixed order.
//   backward  by the member count M of the row (a row starts at its binary search in memrow and ends where the
//             next row starts):
//             M <= kFmGroupMax (32)            one lane group walks the members in order
//             kFmGroupMax < M <= kFmWaveMax    a whole wave: members strided over its groups, fixed-order fold
//             M > kFmWaveMax (2048)            workgroups, by the chunk rule of member_rows.h: a 256-thread block
//                                              (waves folded through LDS) per kFmChunk (1024) members
// No atomics anywhere; the forward needs no LDS. Every output is a function of the inputs alone: the same
// bits on every run and for every grid size.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace minips_k {

constexpr int kFmMaxBlocks = 65535;
constexpr int kFmGroupMax = 32;    // members one lane group walks alone
constexpr int kFmWaveMax = 2048;   // members one wave walks; more go to the chunked workgroup path
constexpr int kFmChunk = 1024;     // members per block of the workgroup path (kFmWaveMax >= 2 * kFmChunk)

inline bool fm_k_ok(int64_t k) { return k >= 4 && k <= 60 && k % 4 == 0; }

// rowptr [B+1], inv / vals [n] (n = rowptr[B], given by the caller), labels [B], rows [cap, ld] (ld >= k + 4),
// w0 nullable device scalar. Outputs S [B, k], z / dz / loss [B], rowid [n]. A lookup whose inv is outside
// [0, cap) contributes nothing. blocks > 0 forces the grid size. B == 0 launches nothing.
void fm_forward(const int64_t* rowptr, const int64_t* inv, const float* vals, const float* labels, const float* rows,
                int64_t ld, int64_t cap, int k, const float* w0, float gscale, int64_t B, int64_t n, float* S, float* z,
                float* dz, float* loss, int32_t* rowid, int blocks, hipStream_t stream);

// floats of the workspace `part` fm_backward needs for n lookups of width-W rows (0: none)
int64_t fm_backward_part_floats(int64_t n, int W);

// members / memrow [n] (memrow sorted, the unique count memrow[n-1] + 1 is read on the device), rowid / vals
// [n], dz [B], S [B, k], rows [cap, ld]; grad_rows [cap, k + 4] contiguous. A member or sample index out of
// range is skipped. part: fm_backward_part_floats(n, k + 4) floats. n == 0 launches nothing.
void fm_backward(const int32_t* members, const int32_t* memrow, const int32_t* rowid, const float* vals,
                 const float* dz, const float* S, const float* rows, int64_t ld, int64_t cap, int k, int64_t B,
                 int64_t n, float* grad_rows, float* part, int blocks, hipStream_t stream);

}  // namespace minips_k
