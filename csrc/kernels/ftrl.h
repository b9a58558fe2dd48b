// Per-coordinate FTRL-Proximal on sparse table rows (ftrl.hip; binding in csrc/bindings/ftrl_py.cpp,
// module minips_amd._ftrlk). McMahan et al., "Ad Click Prediction: a View from the Trenches" (2013),
// Algorithm 1, with sigma written without its cancellation.
//
// The rule, per owned row r = key - base and column c, all in fp32, every operation rounded on its own
// (no contraction; ops.sparse_ftrl's CPU reference runs the same sequence):
//   g2    = g * g
//   n'    = n + g2
//   s'    = sqrt(n');  s = sqrt(n)
//   den   = alpha * (s' + s)
//   sigma = den > 0 ? g2 / den : 0            (== (sqrt(n') - sqrt(n)) / alpha)
//   z'    = z + (g - sigma * w)
//   w'    = |z'| <= l1 ? 0 : -(z' - sign(z') * l1) / ((beta + s') / alpha + l2)
// State: zn [rows, 2*W] fp32, row r = z in columns [0, W), n in [W, 2W): one contiguous 8*W-byte segment
// per touched row.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace minips_k {

constexpr int kFtrlMaxBlocks = 65535;

// keys[0:n) distinct (n_dev: optional device count bounding the prefix, no host sync). A key whose row
// falls outside [0, rows) is skipped -- nothing of it is read or written -- and counted into oor (optional
// device int64). W >= 1 columns of table rows of leading dimension ld >= W; grads [n, W] contiguous.
// blocks > 0 forces the grid size (<= kFtrlMaxBlocks). No atomics but the oor counter: the output is a
// function of the inputs alone.
void sparse_ftrl(float* table, int64_t ld, float* zn, int64_t rows, const int64_t* keys, int64_t n,
                 const int64_t* n_dev, int64_t base, int W, const float* grads, float alpha, float beta, float l1,
                 float l2, int64_t* oor, int blocks, hipStream_t stream);

}  // namespace minips_k
