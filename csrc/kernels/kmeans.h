// K-Means' fused step on dense points (kmeans.hip; binding in csrc/bindings/kmeans_py.cpp, module minips_amd._kmk):
// the nearest centre of every point by an fp32 MFMA sweep that never writes a score, and the per-centre sums and
// counts by a stable integer group-by and the atomic-free row reduce of member_rows.h. The rule is the same in the
// kernels and in the CPU references ops.km_nearest / ops.km_sums.
//
// Shapes    X fp32 [n, D] with row stride ld >= D and any alignment, C fp32 [K, D] contiguous, 1 <= K <= 4096,
//           1 <= D <= 256, n < 2^31 (km_shape_ok). D is padded to 16 inside (km_bucket: the instantiation's width).
// Nearest   km_nearest(X, C) -> assign int32 [n], dist fp32 [n], sse fp64 [1], bad int32 [1] (added to)
//             cn_k = sum_d c_kd^2 in fp32; a centre whose cn_k is not finite is dead and never chosen
//             t_ik = cn_k - 2 <x_i, c_k>, the dot product accumulated in fp32 by MFMA
//             assign_i = argmin_k t_ik over the live centres, the lowest index on exact ties of t. Identical centre
//             rows give identical t (one reduction order for every centre), so the lower duplicate always wins.
//             dist_i = sum_d (x_id - c_ad)^2, a = assign_i: from the winner's row directly, no cancellation
//             sse = sum_i dist_i in fp64: one partial per chunk of kKmChunk points, the partials folded in chunk order
// Bad       a point whose sum_d x_id^2 is not finite, or that finds no live centre: assign -1, dist NaN, nothing added
//           to sse, 1 added to bad. n == 0 writes sse = 0 and launches nothing else.
// Sums      km_sums(X, assign, K) -> sums fp32 [K, D], counts int32 [K]: sums[k] = the sum of the x_i with
//           assign_i == k, added in ascending i; counts[k] their number. An assign outside [0, K) contributes nothing.
//           Every row and every count is written; an empty centre gets zeros.
// Bits      every output is a function of the inputs alone: fixed MFMA, cross-lane and fold orders, a centre's
//           members in ascending point index, a heavy centre by member_rows.h's chunk rule with the partials folded
//           in chunk order. No float atomics; integer LDS atomics for the histograms only. The same bits on every run
//           and for every grid size (`blocks`).
//
// Kernels (wave64, 256-thread workgroups, scratch 0)
//   km_norms_kernel         a wave per centre: lane-strided ascending sum of squares, then a xor butterfly -> cn [K].
//   km_nearest_kernel<DPB>  persistent over chunks (= tiles of 64 points). The tile is staged through LDS (float4
//                           loads; scalar ones for a ragged last quad and when ld or the base is not 16-byte
//                           friendly; rows past n and pad columns zero) into registers: wave w owns the points 16 w ..
//                           16 w + 15 as the MFMA A operand for the whole sweep, DPB / 4 VGPRs a lane. The centres
//                           stream in strips of 64 through two LDS buffers [64][DPB + 4] with their cn beside them
//                           (+inf: dead or past K); strip s + 1's global loads are in flight during strip s's MFMAs
//                           (v_mfma_f32_16x16x4_f32; a lane's four consecutive floats feed four MFMAs, so every LDS
//                           read is 16 bytes). 16-centre tiles wholly past K are skipped. A lane keeps a running
//                           (best, index) with a strict < in ascending centre order; one xor butterfly over the 16
//                           lanes that share a point carries (value, index) with the lower index on ties. The exact
//                           distance re-reads the winner's row from global memory against the registers; sum x^2 from
//                           the same registers is the bad-point test. One fp64 sse partial and one bad count a chunk.
//   km_fold_kernel          sse = the partials in chunk order (thread-strided ascending, then a fixed tree); bad +=.
//   km_hist / km_colscan / km_start / km_place   the group-by: per-block centre histograms in LDS (K + 1 bins, the
//                           last for the points without a centre), a column scan over the blocks, an exclusive scan
//                           over the centres (-> counts), and a placement that ranks a point among the earlier points
//                           of its block with the same centre: members / memrow sorted by (centre, point index).
//   km_sums_kernel          a lane group of L = pow2ceil(ceil(D / 4)) lanes per centre of up to kKmWaveMax members: a
//                           float4 a lane (columns 4 l .. 4 l + 3, or l, l + L, l + 2 L, l + 3 L with scalar loads when
//                           X is not 16-byte friendly), members in order; empty centres are zero-filled here.
//   km_sums_heavy_kernel + member_heavy_fold_kernel   a centre of more members, by the chunk rule of member_rows.h.
// LDS of the nearest kernel: 2 * 64 * (DPB + 4) * 4 + 512 + 48 bytes: 133680 B at DPB = 256.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace minips_k {

constexpr int kKmMaxBlocks = 65535;
constexpr int kKmMaxK = 4096;
constexpr int kKmMaxD = 256;
constexpr int kKmTile = 64;         // points per resident tile
constexpr int kKmStrip = 64;        // centres per streamed strip
constexpr int kKmChunk = 64;        // points per sse partial (one tile)
constexpr int kKmGroup = 256;       // points per round of a group-by block
constexpr int kKmMaxGroups = 1024;  // group-by blocks at most (a block takes several rounds beyond 2^18 points)
constexpr int kKmWaveMax = 512;     // members a lane group sums alone; more go to the chunk rule
constexpr int kKmRowChunk = 256;    // members per block of the chunk rule (kKmWaveMax >= 2 * kKmRowChunk)

inline bool km_shape_ok(int64_t K, int64_t D) { return K >= 1 && K <= kKmMaxK && D >= 1 && D <= kKmMaxD; }
// the padded width of the instantiation that serves D
inline int km_bucket(int D) {
  const int dp = (D + 15) / 16 * 16;
  return dp <= 32 ? dp : dp <= 64 ? 64 : dp <= 96 ? 96 : dp <= 128 ? 128 : dp <= 192 ? 192 : 256;
}
inline int64_t km_chunks(int64_t n) { return (n + kKmChunk - 1) / kKmChunk; }
// the group-by: points per block (a multiple of kKmGroup) and blocks
inline int64_t km_group_points(int64_t n) {
  const int64_t per = (int64_t)kKmGroup * kKmMaxGroups;
  return kKmGroup * ((n + per - 1) / per > 1 ? (n + per - 1) / per : 1);
}
inline int64_t km_groups(int64_t n) { return (n + km_group_points(n) - 1) / km_group_points(n); }

// workspace of km_nearest: cn [K] floats; ssepart [km_chunks(n)] doubles; badpart [km_chunks(n)] int32
// X [n, ld], C [K, D]; assign [n], dist [n], sse [1], bad [1] or null (added to). blocks > 0 forces the grid size.
void km_nearest(const float* X, int64_t ld, int64_t n, int D, const float* C, int K, int32_t* assign, float* dist,
                double* sse, int32_t* bad, float* cn, double* ssepart, int32_t* badpart, int blocks,
                hipStream_t stream);

// int32 workspace of km_sums: hist [km_groups(n) * (K + 1)], tot [K + 1], start [K + 2], members [n], memrow [n]
int64_t km_sums_ws_ints(int64_t n, int K);
// float workspace (the chunk rule's partials; 0: none)
int64_t km_sums_part_floats(int64_t n, int D);

// X [n, ld], assign [n]; sums [K, D] contiguous, counts [K]. n == 0 writes zeros.
void km_sums(const float* X, int64_t ld, int64_t n, int D, const int32_t* assign, int K, float* sums, int32_t* counts,
             int32_t* ws, float* part, int blocks, hipStream_t stream);

}  // namespace minips_k
