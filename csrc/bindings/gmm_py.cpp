// Torch-facing binding of the Gaussian-mixture EM-step kernels (module minips_amd._gmmk; launchers and the rule in
// csrc/kernels/gmm.h). A torch extension of its own, like _alsk: the module and the table of its validation test
// (tests/test_gmmk_validation.py) stay the complete description of each other. Every device pointer comes from a
// checked accessor of tensor_access.h, the ops launch on the current HIP stream of their first tensor's device under a
// device guard (no sync, no host read), and a bad argument raises before anything is launched.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <cmath>

#include "../kernels/gmm.h"
#include "tensor_access.h"

namespace {

using namespace minips_access;  // NOLINT: the accessors are this file's vocabulary
using OptTensor = c10::optional<at::Tensor>;
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

// s fp32 [K, 2D + 1] contiguous -> coef fp32 [K, 2 DP] and cst fp32 [K], both contiguous
void gmm_prepare(const at::Tensor& s, double var_floor, at::Tensor& coef, at::Tensor& cst) {
  TORCH_CHECK(s.dim() == 2 && s.size(1) % 2 == 1, "s must be a [K, 2D + 1] matrix");
  const int64_t K = s.size(0), D = (s.size(1) - 1) / 2, dp = minips_k::gmm_pad(D);
  TORCH_CHECK(minips_k::gmm_shape_ok(K, D), "s says K = ", K, ", D = ", D, ": 1 <= K, D <= 128 and KP * DP <= ",
              minips_k::kGmmMaxKD);
  TORCH_CHECK(std::isfinite(var_floor) && var_floor > 0, "var_floor is ", var_floor, ", expected a finite value > 0");
  TORCH_CHECK(coef.dim() == 2 && coef.size(0) == K && coef.size(1) == 2 * dp, "coef has shape ", coef.sizes(),
              ", expected [", K, ", ", 2 * dp, "]");
  TORCH_CHECK(cst.dim() == 1 && cst.numel() == K, "cst has shape ", cst.sizes(), ", expected [", K, "]");
  DeviceGuard gd(gpu_of(s, "s"));
  const float* sp = dev<float>(s, "s", K * (2 * D + 1));
  float* cp = dev<float>(coef, "coef", K * 2 * dp);
  float* tp = dev<float>(cst, "cst", K);
  minips_k::gmm_prepare(sp, (int)K, (int)D, (float)var_floor, cp, tp, stream_of(s));
}

// X fp32 [n, D] (row-major, padded ld allowed), shift fp32 [D], coef fp32 [K, 2 DP], cst fp32 [K], S optional fp32
// [K, 2D + 1] (absent: the predict path), ll fp64 [1], assign optional int32 [n], logp optional fp32 [n], bad optional
// int32 [1] (added to).
void gmm_estep(const at::Tensor& X, const at::Tensor& shift, const at::Tensor& coef, const at::Tensor& cst,
               const OptTensor& S, at::Tensor& ll, const OptTensor& assign, const OptTensor& logp,
               const OptTensor& bad, int64_t blocks) {
  TORCH_CHECK(X.dim() == 2, "X must be a [n, D] matrix");
  TORCH_CHECK(shift.dim() == 1 && cst.dim() == 1, "shift and cst must be vectors");
  const int64_t n = X.size(0), D = shift.numel(), K = cst.numel(), dp = minips_k::gmm_pad(D);
  TORCH_CHECK(minips_k::gmm_shape_ok(K, D), "cst and shift say K = ", K, ", D = ", D,
              ": 1 <= K, D <= 128 and KP * DP <= ", minips_k::kGmmMaxKD);
  TORCH_CHECK(X.size(1) == D, "X has shape ", X.sizes(), ", shift says D = ", D);
  TORCH_CHECK(n < (1ll << 31) - minips_k::kGmmChunk, "X holds ", n, " points, expected fewer than 2^31 - ",
              minips_k::kGmmChunk);
  TORCH_CHECK(coef.dim() == 2 && coef.size(0) == K && coef.size(1) == 2 * dp, "coef has shape ", coef.sizes(),
              ", cst and shift say [", K, ", ", 2 * dp, "]");
  TORCH_CHECK(blocks >= 0 && blocks <= minips_k::kGmmMaxBlocks, "blocks is ", blocks, ", expected 0 <= blocks <= ",
              minips_k::kGmmMaxBlocks);
  if (present(S))
    TORCH_CHECK(S->dim() == 2 && S->size(0) == K && S->size(1) == 2 * D + 1, "S has shape ", S->sizes(),
                ", expected [", K, ", ", 2 * D + 1, "]");
  TORCH_CHECK(ll.numel() == 1, "ll holds ", ll.numel(), " values, expected 1");
  if (present(assign)) TORCH_CHECK(assign->dim() == 1 && assign->numel() == n, "assign has shape ", assign->sizes(),
                                   ", expected [", n, "]");
  if (present(logp)) TORCH_CHECK(logp->dim() == 1 && logp->numel() == n, "logp has shape ", logp->sizes(),
                                 ", expected [", n, "]");
  if (present(bad)) TORCH_CHECK(bad->numel() == 1, "bad holds ", bad->numel(), " counters, expected 1");
  DeviceGuard gd(gpu_of(X, "X"));
  const float* xp = dev_rows<float>(X, "X", n, D);
  const float* hp = dev<float>(shift, "shift", D);
  const float* cp = dev<float>(coef, "coef", K * 2 * dp);
  const float* tp = dev<float>(cst, "cst", K);
  float* sp = dev_opt<float>(S, "S", K * (2 * D + 1));
  double* lp = dev<double>(ll, "ll", 1);
  int32_t* ap = dev_opt<int32_t>(assign, "assign", n);
  float* gp = dev_opt<float>(logp, "logp", n);
  int32_t* bp = dev_opt<int32_t>(bad, "bad", 1);
  const int64_t nchunks = minips_k::gmm_chunks(n);
  at::Tensor part, llpart;
  if (nchunks > 0) {
    llpart = at::empty({nchunks}, X.options().dtype(at::kDouble));
    if (sp != nullptr) part = at::empty({nchunks * K * (2 * D + 1)}, X.options());
  }
  minips_k::gmm_estep(xp, n > 1 ? X.stride(0) : X.size(1), n, (int)D, (int)K, hp, cp, tp, sp, lp, ap, gp, bp,
                      part.defined() ? part.data_ptr<float>() : nullptr,
                      llpart.defined() ? llpart.data_ptr<double>() : nullptr, (int)blocks, stream_of(X));
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "minips_amd Gaussian-mixture EM-step kernels (gfx950)";
  m.def("gmm_prepare", &gmm_prepare, py::arg("s"), py::arg("var_floor"), py::arg("coef"), py::arg("cst"));
  m.def("gmm_estep", &gmm_estep, py::arg("X"), py::arg("shift"), py::arg("coef"), py::arg("cst"), py::arg("S"),
        py::arg("ll"), py::arg("assign"), py::arg("logp"), py::arg("bad"), py::arg("blocks"));
  m.attr("MAX_K") = minips_k::kGmmMaxK;
  m.attr("MAX_D") = minips_k::kGmmMaxD;
  m.attr("MAX_KD") = minips_k::kGmmMaxKD;
  m.attr("CHUNK") = minips_k::kGmmChunk;
  m.attr("TILE") = minips_k::kGmmTile;
}
