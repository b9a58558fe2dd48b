// Split rows with two rules (wideftrl.hip; binding in csrc/bindings/wideftrl_py.cpp, module
// minips_amd._wdftrlk): Wide & Deep's recipe, the deep embedding on row-wise Adagrad and the wide (linear)
// columns on FTRL-Proximal with L1 / L2, applied in one pass over the touched rows.
//
// Per owned row r = key - base with gradient row g[0:W), D1 = split, Wf = W - D1, all in fp32:
//   columns c <  D1   st = state[r] + (sum_c g_c^2) / (float)D1;  state[r] = st
//                     w_c -= lr / (sqrtf(st) + eps) * g_c          (sparse_rowwise_adagrad's rule and order)
//   columns c >= D1   gs = g_c * grad_scale (its own rounded product), then ftrl.h's coordinate rule on
//                     (w_c, z, n, gs) with alpha, beta, l1, l2, no contraction
// State: state [rows] (the deep accumulator) and zn [rows, 2*Wf] (z in columns [0, Wf), n in [Wf, 2*Wf)):
// ftrl.h's layout over the wide columns. A column with g = 0 and w = z = n = 0 stays there (den = 0).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace minips_k {

constexpr int kWideFtrlMaxBlocks = 65535;

// keys[0:n) distinct (n_dev: optional device count bounding the prefix, no host sync). A key whose row
// falls outside [0, rows) is skipped -- nothing of it is read or written -- and counted into oor (optional
// device int64). 1 <= D1 < W <= ld; grads [n, W] contiguous. blocks > 0 forces the grid size
// (<= kWideFtrlMaxBlocks). No atomics but the oor counter, no LDS: the output is a function of the inputs.
void sparse_adagrad_ftrl(float* table, int64_t ld, float* state, float* zn, int64_t rows, int D1, int W,
                         const int64_t* keys, int64_t n, const int64_t* n_dev, int64_t base, const float* grads,
                         float lr, float eps, float alpha, float beta, float l1, float l2, float grad_scale,
                         int64_t* oor, int blocks, hipStream_t stream);

}  // namespace minips_k
