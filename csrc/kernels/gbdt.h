// Histogram gradient-boosted decision trees, binary logistic objective, in exact fixed point (gbdt.hip; binding
// in csrc/bindings/gbdt_py.cpp, module minips_amd._gbdtk). Gradients are quantised to integers once per round;
// everything summed afterwards is an integer, so histograms, splits and trees are the same bits for every launch
// shape, path, batch split and rank count, and on the CPU reference (minips_amd/ops).
//
// Constants: S = 2^20; 2 <= NB <= 256 bins; 1 <= depth <= 8 (a level has nodes = 2^d <= 128); 1 <= F <= 4096.
//
// bin       cuts fp32 [F, NB - 1], ascending per feature, padded with +inf. bin(x, f) = #{j : x > cuts[f, j]}: a
//           NaN lands in bin 0, +inf past every finite cut. Comparisons only (an upper-bound search over the
//           ascending cuts: the same count). bins uint8 [N, ldb] row-major, ldb >= F; columns >= F are not
//           written.
// grad      fp32: zc = clamp(z, -30, 30); p = 1 / (1 + expf(-zc)); y = label > 0.5; qg = llrintf((p - y) S);
//           qh = llrintf(max(p (1 - p), 2^-20) S) >= 1; gh int32 [N, 2] = (qg, qh). |qg| <= S, qh <= S / 4.
//           The same pass adds sum_i llrintf(loss_i 2^24) to one int64: loss = max(zl, 0) - zl y +
//           log1pf(expf(-|zl|)), zl = clamp(z, -64, 64) (the formula of evalmetrics.h). z must not be NaN.
// hist      at a level with `nodes` nodes ADDS into hist int64 [nodes, F, NB, 3] (sum qg, sum qh, count): sample
//           i with 0 <= node[i] < nodes contributes once per feature f at bins[i, f]; a node id out of range
//           contributes nothing, a bin >= NB nothing for that feature. Integer sums only.
// split     per node from hist alone. Candidate (f, t), t in [0, NB - 2], left = bins <= t of feature f; the
//           totals of a candidate are the sums of its own feature's bins. Prefix sums exact in int64;
//           GL = (double)sum_qg_left 2^-20 and so on (exact below 2^33 samples);
//           gain = (GL GL / (HL + lambda) + GR GR / (HR + lambda)) - G G / (H + lambda), every operation rounded
//           on its own in fp64 (contraction off). Valid: countL >= min_child_count, countR >= min_child_count,
//           gain > min_gain. Best: largest gain, then lowest f, then lowest t. None valid: feat = -1, thr = 0,
//           gain = 0 (a pass-through node: everything goes left). child int64 [nodes, 2, 3]: the left and right
//           sums of the chosen split; for feat = -1 left holds feature 0's totals and right zeros. lambda > 0.
// leaf      from a level's child: leaf[2 n + s] = (float)(-(Gs 2^-20) / (Hs 2^-20 + lambda) * lr), in fp64 with
//           every operation rounded on its own, then rounded to fp32; a child with count 0 gets +0.0.
// advance   node'[i] = 2 node[i] + (feat[node[i]] >= 0 && bins[i, feat] > thr). A node id outside [0, nodes) or
//           a feat >= F gives node' = -1 (out of range for every later level). With `leaf` (the last level) also
//           z[i] += leaf[node'[i]] for node' >= 0.
// predict   trees are complete binary trees of fixed depth, level-major (node n of level d at 2^d - 1 + n):
//           feat int32 [T, 2^depth - 1], thr uint8 likewise, leaf fp32 [T, 2^depth]. z[i] = base + leaf_0[..] +
//           leaf_1[..] + ..., summed in fp32 in tree order; optionally leaf_index int32 [N, T]. A feat outside
//           [0, F) is a pass-through node.
//
// Mapping (wave64, 256-thread workgroups).
//   hist  LDS path: a workgroup owns a tile of tf features, tf the largest with nodes x tf x NB x 3 int32
//         accumulators <= kGbdtLdsBytes (64 KiB of the CU's 160: two workgroups per CU), and streams chunks of
//         kGbdtFlushRows samples, a thread per sample: node, (qg, qh), then the row of bins -- by 16-byte loads
//         when bins and ldb are 16-byte friendly and the row is addressable to align16(F), else byte by byte --
//         and three LDS integer atomics per feature. After EVERY chunk the accumulators are flushed with 64-bit
//         global integer atomics (zero entries skipped) and cleared. The bound: between two flushes a workgroup
//         adds at most kGbdtFlushRows = 1792 samples to an accumulator, each of magnitude <= S = 2^20, so
//         |sum| <= 1792 * 2^20 < 2^31 for any input of the rule. A sample whose |qg| or |qh| exceeds S (not
//         the rule's gradients: a caller's own gh) goes straight to the global atomics, so the result is the
//         exact int64 sum for every int32 input.
//         Global path: a thread per (sample, feature), three 64-bit global integer atomics. Taken by `auto`
//         where one feature of the level does not fit the LDS budget (nodes x NB x 12 bytes > 64 KiB).
//         path: 0 auto, 1 LDS (an error where one feature does not fit), 2 global. blocks > 0 forces the number
//         of workgroups along the samples.
//   split one wave per (node, feature): lane l takes the bins [l R, l R + R), R = ceil(NB / 64); the int64 prefix
//         goes by __shfl_up; every lane keeps its best (gain, t) and a __shfl_xor fold carries the key (gain,
//         f, t) -- a total order, so the fold order cannot matter. A second launch, one wave per node, folds the
//         features with the same key and writes feat / thr / gain / child. No float atomics.
//   bin / grad / advance / predict / leaf are element-wise. bin stores four bins as one word when bins and ldb
//         are 4-byte friendly, else a byte per lane; unaligned pointers are never refused.
// Every index read from a tensor is checked on the device and skipped, never trusted. Empty inputs launch
// nothing.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace minips_k {

constexpr int kGbdtMaxBlocks = 65535;
constexpr int kGbdtMaxBins = 256;
constexpr int kGbdtMaxDepth = 8;
constexpr int kGbdtMaxNodes = 1 << (kGbdtMaxDepth - 1);  // nodes of the deepest level
constexpr int kGbdtMaxF = 4096;
constexpr int kGbdtMaxTrees = 1 << 16;
constexpr int kGbdtScaleBits = 20;                       // S = 2^20
constexpr int kGbdtFlushRows = 1792;                     // samples a workgroup adds between two LDS flushes
constexpr int kGbdtLdsBytes = 64 * 1024;                 // LDS accumulators of one workgroup
static_assert((int64_t)kGbdtFlushRows << kGbdtScaleBits < (1ll << 31), "the LDS accumulators are int32");

// features per workgroup of the LDS path (0: one feature does not fit)
inline int gbdt_hist_tile(int nodes, int F, int NB) {
  const int64_t per = (int64_t)nodes * NB * 3 * 4;
  const int64_t t = kGbdtLdsBytes / per;
  return (int)(t < F ? t : F);
}

// X [N, ldx] fp32, cuts [F, NB - 1]; bins [N, ldb].
void gbdt_bin(const float* X, int64_t ldx, const float* cuts, int64_t N, int F, int NB, uint8_t* bins, int64_t ldb,
              int blocks, hipStream_t stream);

// z / labels [N]; gh [N, 2]; loss_acc one int64 (added to).
void gbdt_grad(const float* z, const float* labels, int64_t N, int32_t* gh, int64_t* loss_acc, int blocks,
               hipStream_t stream);

// bins [N, ldb] with `width` addressable columns per row (F <= width <= ldb), node [N], gh [N, 2]; hist
// [nodes, F, NB, 3] (added to).
void gbdt_hist(const uint8_t* bins, int64_t ldb, int64_t width, const int32_t* node, const int32_t* gh, int64_t N,
               int F, int NB, int nodes, int64_t* hist, int path, int blocks, hipStream_t stream);

// hist [nodes, F, NB, 3]; outputs feat / thr [nodes], gain [nodes], child [nodes, 2, 3]; workspace wgain
// [nodes * F] doubles and wthr [nodes * F] int32.
void gbdt_split(const int64_t* hist, int nodes, int F, int NB, double lambda, int64_t min_child_count,
                double min_gain, int32_t* feat, int32_t* thr, double* gain, int64_t* child, double* wgain,
                int32_t* wthr, hipStream_t stream);

// child [nodes, 2, 3] -> leaf [2 * nodes]
void gbdt_leaf(const int64_t* child, int nodes, double lambda, double lr, float* leaf, hipStream_t stream);

// bins [N, ldb], node [N] (updated in place), feat / thr [nodes]; leaf [2 * nodes] and z [N] nullable together.
void gbdt_advance(const uint8_t* bins, int64_t ldb, int32_t* node, const int32_t* feat, const int32_t* thr,
                  int64_t N, int F, int nodes, const float* leaf, float* z, int blocks, hipStream_t stream);

// bins [N, ldb]; feat / thr [T, 2^depth - 1] and leaf [T, 2^depth] contiguous; z [N]; leaf_index [N, T] nullable.
void gbdt_predict(const uint8_t* bins, int64_t ldb, int64_t N, int F, const int32_t* feat, const uint8_t* thr,
                  const float* leaf, int T, int depth, float base, float* z, int32_t* leaf_index, int blocks,
                  hipStream_t stream);

}  // namespace minips_k
