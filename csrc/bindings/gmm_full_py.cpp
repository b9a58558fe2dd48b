// Torch-facing binding of the full-covariance Gaussian-mixture EM-step kernels (module minips_amd._gmmfk; launchers and
// the rule in csrc/kernels/gmm_full.h). A torch extension of its own, like _gmmk. Every device pointer comes from a
// checked accessor of tensor_access.h, the ops launch on the current HIP stream of their first tensor's device under a
// device guard (no sync, no host read), and a bad argument raises before anything is launched.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <cmath>

#include "../kernels/gmm_full.h"
#include "tensor_access.h"

namespace {

using namespace minips_access;  // NOLINT: the accessors are this file's vocabulary
using OptTensor = c10::optional<at::Tensor>;
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// s fp32 [K, D + D*D + 1] contiguous -> Wh fp32 [K, DP, DP], b fp32 [K, DP] and cst fp32 [K], all contiguous
void gmm_full_prepare(const at::Tensor& s, int64_t D, double reg_covar, at::Tensor& Wh, at::Tensor& b,
                      at::Tensor& cst) {
  TORCH_CHECK(s.dim() == 2 && D >= 1 && s.size(1) == minips_k::gmm_full_width(D), "s must be a [K, D + D*D + 1] ",
              "matrix, got ", s.sizes(), " with D = ", D);
  const int64_t K = s.size(0), dp = minips_k::gmm_full_pad(D);
  TORCH_CHECK(minips_k::gmm_full_shape_ok(K, D), "s says K = ", K, ", D = ", D, ": 1 <= K <= ",
              minips_k::kGmmFullMaxK, " and 1 <= D <= ", minips_k::kGmmFullMaxD);
  TORCH_CHECK(std::isfinite(reg_covar) && reg_covar >= 0, "reg_covar is ", reg_covar, ", expected a finite value >= 0");
  TORCH_CHECK(Wh.dim() == 3 && Wh.size(0) == K && Wh.size(1) == dp && Wh.size(2) == dp, "Wh has shape ", Wh.sizes(),
              ", expected [", K, ", ", dp, ", ", dp, "]");
  TORCH_CHECK(b.dim() == 2 && b.size(0) == K && b.size(1) == dp, "b has shape ", b.sizes(), ", expected [", K, ", ",
              dp, "]");
  TORCH_CHECK(cst.dim() == 1 && cst.numel() == K, "cst has shape ", cst.sizes(), ", expected [", K, "]");
  DeviceGuard gd(gpu_of(s, "s"));
  const float* sp = dev<float>(s, "s", K * minips_k::gmm_full_width(D));
  float* wp = dev<float>(Wh, "Wh", K * dp * dp);
  float* bp = dev<float>(b, "b", K * dp);
  float* tp = dev<float>(cst, "cst", K);
  minips_k::gmm_full_prepare(sp, (int)K, (int)D, (float)reg_covar, wp, bp, tp, stream_of(s));
}

// X fp32 [n, D] (row-major, padded ld allowed), shift fp32 [D], Wh fp32 [K, DP, DP] (16-byte aligned), b fp32 [K, DP],
// cst fp32 [K], S optional fp32 [K, D + D*D + 1] (absent: the predict path), ll fp64 [1], assign optional int32 [n],
// logp optional fp32 [n], bad optional int32 [1] (added to).
void gmm_full_estep(const at::Tensor& X, const at::Tensor& shift, const at::Tensor& Wh, const at::Tensor& b,
                    const at::Tensor& cst, const OptTensor& S, at::Tensor& ll, const OptTensor& assign,
                    const OptTensor& logp, const OptTensor& bad, int64_t blocks) {
  TORCH_CHECK(X.dim() == 2, "X must be a [n, D] matrix");
  TORCH_CHECK(shift.dim() == 1 && cst.dim() == 1, "shift and cst must be vectors");
  const int64_t n = X.size(0), D = shift.numel(), K = cst.numel(), dp = minips_k::gmm_full_pad(D);
  const int64_t kp = minips_k::gmm_full_pad(K), W = minips_k::gmm_full_width(D);
  TORCH_CHECK(minips_k::gmm_full_shape_ok(K, D), "cst and shift say K = ", K, ", D = ", D, ": 1 <= K <= ",
              minips_k::kGmmFullMaxK, " and 1 <= D <= ", minips_k::kGmmFullMaxD);
  TORCH_CHECK(X.size(1) == D, "X has shape ", X.sizes(), ", shift says D = ", D);
  TORCH_CHECK(n < (1ll << 31) - minips_k::kGmmFullChunk, "X holds ", n, " points, expected fewer than 2^31 - ",
              minips_k::kGmmFullChunk);
  TORCH_CHECK(Wh.dim() == 3 && Wh.size(0) == K && Wh.size(1) == dp && Wh.size(2) == dp, "Wh has shape ", Wh.sizes(),
              ", cst and shift say [", K, ", ", dp, ", ", dp, "]");
  TORCH_CHECK(b.dim() == 2 && b.size(0) == K && b.size(1) == dp, "b has shape ", b.sizes(), ", cst and shift say [", K,
              ", ", dp, "]");
  TORCH_CHECK(blocks >= 0 && blocks <= minips_k::kGmmFullMaxBlocks, "blocks is ", blocks,
              ", expected 0 <= blocks <= ", minips_k::kGmmFullMaxBlocks);
  if (present(S))
    TORCH_CHECK(S->dim() == 2 && S->size(0) == K && S->size(1) == W, "S has shape ", S->sizes(), ", expected [", K,
                ", ", W, "]");
  TORCH_CHECK(ll.numel() == 1, "ll holds ", ll.numel(), " values, expected 1");
  if (present(assign)) TORCH_CHECK(assign->dim() == 1 && assign->numel() == n, "assign has shape ", assign->sizes(),
                                   ", expected [", n, "]");
  if (present(logp)) TORCH_CHECK(logp->dim() == 1 && logp->numel() == n, "logp has shape ", logp->sizes(),
                                 ", expected [", n, "]");
  if (present(bad)) TORCH_CHECK(bad->numel() == 1, "bad holds ", bad->numel(), " counters, expected 1");
  DeviceGuard gd(gpu_of(X, "X"));
  const float* xp = dev_rows<float>(X, "X", n, D);
  const float* hp = dev<float>(shift, "shift", D);
  const float* wp = dev<float>(Wh, "Wh", K * dp * dp);
  TORCH_CHECK(aligned16(wp), "Wh must start at a 16-byte boundary");
  const float* bp = dev<float>(b, "b", K * dp);
  const float* tp = dev<float>(cst, "cst", K);
  float* sp = dev_opt<float>(S, "S", K * W);
  double* lp = dev<double>(ll, "ll", 1);
  int32_t* ap = dev_opt<int32_t>(assign, "assign", n);
  float* gp = dev_opt<float>(logp, "logp", n);
  int32_t* cp = dev_opt<int32_t>(bad, "bad", 1);
  // the workspaces: fresh allocations are 16-byte aligned
  at::Tensor T, part, llpart, lse;
  if (n > 0) {
    llpart = at::empty({minips_k::gmm_full_tiles(n)}, X.options().dtype(at::kDouble));
    if (sp != nullptr) {
      T = at::empty({n * kp}, X.options());
      part = at::empty({minips_k::gmm_full_chunks(n, K, D) * K * W}, X.options());
      if (gp == nullptr) {  // the statistics kernel reads lse
        lse = at::empty({n}, X.options());
        gp = lse.data_ptr<float>();
      }
    }
  }
  minips_k::gmm_full_estep(xp, n > 1 ? X.stride(0) : X.size(1), n, (int)D, (int)K, hp, wp, bp, tp, sp, lp, ap, gp, cp,
                           T.defined() ? T.data_ptr<float>() : nullptr,
                           part.defined() ? part.data_ptr<float>() : nullptr,
                           llpart.defined() ? llpart.data_ptr<double>() : nullptr, (int)blocks, stream_of(X));
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "minips_amd full-covariance Gaussian-mixture EM-step kernels (gfx950)";
  m.def("gmm_full_prepare", &gmm_full_prepare, py::arg("s"), py::arg("D"), py::arg("reg_covar"), py::arg("Wh"),
        py::arg("b"), py::arg("cst"));
  m.def("gmm_full_estep", &gmm_full_estep, py::arg("X"), py::arg("shift"), py::arg("Wh"), py::arg("b"),
        py::arg("cst"), py::arg("S"), py::arg("ll"), py::arg("assign"), py::arg("logp"), py::arg("bad"),
        py::arg("blocks"));
  m.attr("MAX_K") = minips_k::kGmmFullMaxK;
  m.attr("MAX_D") = minips_k::kGmmFullMaxD;
  m.attr("CHUNK") = minips_k::kGmmFullChunk;
  m.attr("MAX_CHUNKS") = minips_k::kGmmFullMaxChunks;
  m.attr("PART_CAP") = minips_k::kGmmFullPartCap;
  m.attr("TILE") = minips_k::kGmmFullTile;
}
