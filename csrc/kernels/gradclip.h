// Global-norm gradient clipping as a device-side part of the dense clock (gradclip.hip; bindings in
// csrc/bindings/optim_py.cpp, module minips_amd._optk).
//
// The rule, with x_i the fp32 gradient element the Adam consumes (g[i] plus its split-K planes in the
// grouped order slab_fold<true> of dense_update.h: groups of four as (a0+a1)+(a2+a3), then the remainder
// one by one; the dense clock's other order, plane by plane, is only what slab_pack and ps_push_dense ship
// and differs in rounding from 4 planes on):
//   total  = sum_i (double)x_i * (double)x_i      (over every rank's shard; non-finite iff an element is)
//   norm   = sqrt(total);  scale_d = max_norm / (norm + 1e-6)
//   scale  = scale_d < 1 ? (float)scale_d : 1.0f
//   total non-finite: the clock is SKIPPED (w, m, v, the bf16 copy untouched; g still cleared on zero_g)
//   otherwise the update is adam_kernel's with gscale = scale.
#pragma once

#include "kernels.h"

namespace minips_k {

constexpr int kSumsqMaxBlocks = 1024;  // workgroups (= partial sums) of one grad_sumsq launch
constexpr int kClipMaxParts = 4096;    // partial sums one adam_clip_apply folds

// part[b] = the fp64 sum of squares of workgroup b's grid-stride share of g[0:n] (+ slabs), b < L; zero
// for a workgroup without elements. No atomics: a function of the data and L only. n % 4 == 0, 16-byte
// aligned g, 1 <= L <= kSumsqMaxBlocks.
void grad_sumsq(const float* g, int64_t n, const AdamSlabs* slabs, double* part, int L, hipStream_t s);

// Every workgroup folds part[0:np] in one fixed order (so every launch and every replay of a clock
// derives the same bits of scale), then applies the rule above. stats (fp64 [4]: norm, scale,
// n_clipped, n_skipped) is updated by one thread when write_stats; scale reads 0 on a skipped clock.
// n % 4 == 0, 16-byte aligned w / m / v / g, 8-byte aligned w_bf16 (nullable), 1 <= np <= kClipMaxParts.
void adam_clip_apply(float* w, float* m, float* v, float* g, int64_t n, const AdamSlabs* slabs, float lr,
                     float beta1, float beta2, float eps, float weight_decay, int step, const int* step_dev,
                     bf16_t* w_bf16, bool zero_g, const double* part, int np, double max_norm, double* stats,
                     bool write_stats, hipStream_t s);

}  // namespace minips_k
