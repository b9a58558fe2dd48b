// Host-callable launchers of the held-out evaluation kernels (evalmetrics.hip): raw pointers +
// stream, no torch types. The torch-facing validation layer is csrc/bindings/eval_py.cpp
// (module minips_amd._evalk).
//
// Accumulator ``acc`` (int64, 2*NB + 2 words): neg[NB] | pos[NB] | loss_fx | n_nan, NB a power of
// two in [kEvalMinBins, kEvalMaxBins]. Per sample, with fp32 logit z and label y = label > 0.5:
//   NaN z          n_nan += 1, nothing else
//   bin            min(NB-1, (int)floorf((clamp(z, -16, 16) + 16) * (NB/32)))   -> neg / pos [bin] += 1
//   loss           zl = clamp(z, -64, 64); l = max(zl,0) - zl*y + log1pf(expf(-|zl|));
//                  loss_fx += llrintf(l * 2^24)
// Everything accumulated is an integer, so the sums do not depend on order, launch shape or rank count.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace minips_k {

typedef uint16_t bf16_t;

constexpr int kEvalMinBins = 32;
constexpr int kEvalMaxBins = 8192;  // two uint32 LDS histograms: 64 KB per workgroup

void binary_hist(const float* logits, const float* labels, int64_t n, int NB, int64_t* acc, hipStream_t s);

// z[b] = H[b, :Hd] . w + b0 + wide[b] (fp32 accumulate; wide may be null), then the rule above;
// logits_out (nullable) receives z. H rows are ld elements apart; Hd % 8 == 0, 8 <= Hd <= 1024,
// ld % 8 == 0, H and w 16-byte aligned (16-byte row loads).
void eval_head_hist(const bf16_t* H, int64_t B, int Hd, int64_t ld, const bf16_t* w, const bf16_t* b0,
                    const float* wide, const float* labels, int NB, int64_t* acc, float* logits_out,
                    hipStream_t s);

}  // namespace minips_k
