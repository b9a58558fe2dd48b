// Torch-facing bindings of the held-out evaluation kernels (module minips_amd._evalk; launchers in
// csrc/kernels/evalmetrics.h). A torch extension of its own: minips_amd._kernels and the table of
// tests/test_bindings_validation.py stay the complete description of each other, and this module
// has its own table (tests/test_evalk_validation.py). As in ops_py.cpp, every device pointer comes
// from a checked accessor of tensor_access.h, ops launch on the current HIP stream of the tensors'
// device under a device guard, and a bad argument raises before anything is launched.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include "../kernels/evalmetrics.h"
#include "tensor_access.h"

namespace {

using minips_k::bf16_t;
using namespace minips_access;  // NOLINT: the accessors are this file's vocabulary
using OptTensor = c10::optional<at::Tensor>;
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

// acc: neg[NB] | pos[NB] | loss_fx | n_nan -> NB
int bins_of(const at::Tensor& acc) {
  const int64_t n = acc.numel();
  const int64_t NB = (n - 2) / 2;
  TORCH_CHECK(n == 2 * NB + 2 && NB >= minips_k::kEvalMinBins && NB <= minips_k::kEvalMaxBins && !(NB & (NB - 1)),
              "acc holds ", n, " elements, expected 2*NB + 2 with NB a power of two in [", minips_k::kEvalMinBins,
              ", ", minips_k::kEvalMaxBins, "]");
  return (int)NB;
}

void binary_hist(const at::Tensor& logits, const at::Tensor& labels, at::Tensor& acc) {
  TORCH_CHECK(logits.dim() == 1, "logits: [n]");
  const int64_t n = logits.numel();
  TORCH_CHECK(labels.dim() == 1 && labels.numel() == n, "labels holds ", labels.numel(), " elements, logits ", n);
  const int NB = bins_of(acc);
  DeviceGuard g(gpu_of(acc, "acc"));
  int64_t* ap = dev<int64_t>(acc, "acc", 2 * NB + 2);
  const float* zp = dev<float>(logits, "logits", n);
  const float* yp = dev<float>(labels, "labels", n);
  minips_k::binary_hist(zp, yp, n, NB, ap, stream_of(acc));
}

void eval_head_hist(const at::Tensor& H, const at::Tensor& w, const at::Tensor& b0, const OptTensor& wide,
                    const at::Tensor& labels, at::Tensor& acc, const OptTensor& logits_out) {
  TORCH_CHECK(H.dim() == 2, "H: [B, Hd]");
  const int64_t B = H.size(0), Hd = H.size(1);
  const int64_t ld = B > 1 ? H.stride(0) : Hd;
  TORCH_CHECK(Hd % 8 == 0 && Hd >= 8 && Hd <= 1024, "H has ", Hd, " columns: Hd % 8 == 0 and 8 <= Hd <= 1024");
  TORCH_CHECK(ld >= Hd && ld % 8 == 0, "H has row stride ", ld, ": ld >= Hd and ld % 8 == 0");
  TORCH_CHECK(w.dim() == 1 && w.numel() == Hd, "w holds ", w.numel(), " elements, H has ", Hd, " columns");
  TORCH_CHECK(labels.dim() == 1 && labels.numel() == B, "labels holds ", labels.numel(), " elements, H has ", B,
              " rows");
  TORCH_CHECK(!present(wide) || (wide->dim() == 1 && wide->numel() == B), "wide must be [B], H has ", B, " rows");
  TORCH_CHECK(!present(logits_out) || (logits_out->dim() == 1 && logits_out->numel() == B),
              "logits_out must be [B], H has ", B, " rows");
  const int NB = bins_of(acc);
  DeviceGuard g(gpu_of(acc, "acc"));
  int64_t* ap = dev<int64_t>(acc, "acc", 2 * NB + 2);
  const bf16_t* hp = dev_rows<bf16_t>(H, "H", B, Hd);
  const bf16_t* wp = dev<bf16_t>(w, "w", Hd);
  aligned16(H, "H");
  aligned16(w, "w");
  const bf16_t* bp = dev<bf16_t>(b0, "b0", 1);
  const float* wd = dev_opt<float>(wide, "wide", B);
  const float* yp = dev<float>(labels, "labels", B);
  float* zo = dev_opt<float>(logits_out, "logits_out", B);
  minips_k::eval_head_hist(hp, B, (int)Hd, ld, wp, bp, wd, yp, NB, ap, zo, stream_of(acc));
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "minips_amd held-out evaluation kernels (gfx950)";
  m.def("binary_hist", &binary_hist, py::arg("logits"), py::arg("labels"), py::arg("acc"));
  m.def("eval_head_hist", &eval_head_hist, py::arg("H"), py::arg("w"), py::arg("b0"), py::arg("wide"),
        py::arg("labels"), py::arg("acc"), py::arg("logits_out") = py::none());
}
