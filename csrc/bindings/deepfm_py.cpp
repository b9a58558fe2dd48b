// Torch-facing binding of DeepFM's FM interaction term on the Wide & Deep step (module minips_amd._dfmk;
// launchers and the rule in csrc/kernels/deepfm.h). A torch extension of its own, like _evalk, _optk, _ftrlk,
// _wdftrlk and _fmk: the module and the table of its validation test (tests/test_dfmk_validation.py) stay the
// complete description of each other. Every device pointer comes from a checked accessor of tensor_access.h,
// the ops launch on the current HIP stream of X's device under a device guard (no sync, no host read, no
// allocation), and a bad argument raises before anything is launched.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include "../kernels/deepfm.h"
#include "tensor_access.h"

namespace {

using namespace minips_access;  // NOLINT: the accessors are this file's vocabulary
using OptTensor = c10::optional<at::Tensor>;
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

// X must be a [B, >= F * D] row-major matrix; returns its leading dimension
int64_t check_common(const at::Tensor& X, int64_t F, int64_t D, int64_t blocks) {
  TORCH_CHECK(D >= 1 && D <= minips_k::kDfmMaxD, "D is ", D, ", expected 1 <= D <= ", minips_k::kDfmMaxD);
  TORCH_CHECK(F >= 1 && F < (1ll << 24), "F is ", F, ", expected 1 <= F < 2^24");
  TORCH_CHECK(blocks >= 0 && blocks <= minips_k::kDfmMaxBlocks, "blocks is ", blocks, ", expected 0 <= blocks <= ",
              minips_k::kDfmMaxBlocks);
  TORCH_CHECK(X.dim() == 2, "X must be a [B, >= F * D] matrix");
  const int64_t B = X.size(0), ldx = B > 1 ? X.stride(0) : X.size(1);
  TORCH_CHECK(B * F < (1ll << 31), "X holds ", B, " samples of F = ", F, " fields, expected B * F < 2^31");
  TORCH_CHECK(F * D <= X.size(1) && F * D <= ldx, "X has shape ", X.sizes(), " (ld ", ldx, "), F * D = ", F * D,
              " columns are read");
  return ldx;
}

// X bf16 [B, >= F * D] (row-major, padded ld allowed), wide fp32 [B] (updated), S fp32 [B, D] (written)
void wd_fm_forward(const at::Tensor& X, int64_t F, int64_t D, at::Tensor& wide, at::Tensor& S, int64_t blocks) {
  const int64_t ldx = check_common(X, F, D, blocks), B = X.size(0);
  TORCH_CHECK(wide.dim() == 1 && wide.numel() == B, "wide has shape ", wide.sizes(), ", expected [", B, "]");
  TORCH_CHECK(S.dim() == 2 && S.size(0) == B && S.size(1) == D, "S has shape ", S.sizes(), ", expected [", B, ", ", D,
              "]");
  DeviceGuard gd(gpu_of(X, "X"));
  const bf16_t* xp = dev_rows<bf16_t>(X, "X", B, F * D);
  float* wp = dev<float>(wide, "wide", B);
  float* sp = dev<float>(S, "S", B * D);
  TORCH_CHECK(wide.device() == X.device() && S.device() == X.device(), "wide and S must be on X's device");
  minips_k::wd_fm_forward(xp, ldx, B, (int)F, (int)D, wp, sp, (int)blocks, stream_of(X));
}

// X as above, S fp32 [B, D], dwide fp32 [B], perm optional int32 [B * F], dX bf16 with B * F * D elements,
// contiguous ([B, F * D] in lookup order or [B * F, D] in the permuted order; updated in place)
void wd_fm_backward(const at::Tensor& X, const at::Tensor& S, const at::Tensor& dwide, const OptTensor& perm,
                    at::Tensor& dX, int64_t F, int64_t D, int64_t blocks) {
  const int64_t ldx = check_common(X, F, D, blocks), B = X.size(0);
  TORCH_CHECK(dwide.dim() == 1 && dwide.numel() == B, "dwide has shape ", dwide.sizes(), ", expected [", B, "]");
  TORCH_CHECK(S.dim() == 2 && S.size(0) == B && S.size(1) == D, "S has shape ", S.sizes(), ", expected [", B, ", ", D,
              "]");
  TORCH_CHECK(dX.dim() == 2 && dX.numel() == B * F * D && (dX.size(1) == D || dX.size(1) == F * D),
              "dX has shape ", dX.sizes(), ", expected [", B, ", ", F * D, "] or [", B * F, ", ", D, "]");
  if (present(perm))
    TORCH_CHECK(perm->dim() == 1 && perm->numel() == B * F, "perm has shape ", perm->sizes(), ", expected [", B * F,
                "]");
  DeviceGuard gd(gpu_of(X, "X"));
  const bf16_t* xp = dev_rows<bf16_t>(X, "X", B, F * D);
  const float* sp = dev<float>(S, "S", B * D);
  const float* dp = dev<float>(dwide, "dwide", B);
  const int32_t* pp = dev_opt<int32_t>(perm, "perm", B * F);
  bf16_t* gp = dev<bf16_t>(dX, "dX", B * F * D);
  TORCH_CHECK(S.device() == X.device() && dwide.device() == X.device() && dX.device() == X.device() &&
                  (!present(perm) || perm->device() == X.device()),
              "S, dwide, perm and dX must be on X's device");
  minips_k::wd_fm_backward(xp, ldx, sp, dp, pp, gp, B, (int)F, (int)D, (int)blocks, stream_of(X));
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "minips_amd DeepFM interaction-term kernels on the Wide & Deep input (gfx950)";
  m.def("wd_fm_forward", &wd_fm_forward, py::arg("X"), py::arg("F"), py::arg("D"), py::arg("wide"), py::arg("S"),
        py::arg("blocks"));
  m.def("wd_fm_backward", &wd_fm_backward, py::arg("X"), py::arg("S"), py::arg("dwide"), py::arg("perm"),
        py::arg("dX"), py::arg("F"), py::arg("D"), py::arg("blocks"));
  m.attr("MAX_D") = minips_k::kDfmMaxD;
}
