// Torch-facing binding of the split-row apply with two rules -- row-wise Adagrad on the deep columns,
// FTRL-Proximal on the wide ones (module minips_amd._wdftrlk; launcher in csrc/kernels/wideftrl.h). A torch
// extension of its own, like _evalk, _optk and _ftrlk: each module and the table of its validation test stay
// the complete description of each other (this one: tests/test_wdftrlk_validation.py). As in ftrl_py.cpp,
// every device pointer comes from a checked accessor of tensor_access.h, the op launches on the current HIP
// stream of the table's device under a device guard (graph-capture safe: no sync in here), and a bad
// argument raises before anything is launched.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <cmath>

#include "../kernels/wideftrl.h"
#include "tensor_access.h"

namespace {

using namespace minips_access;  // NOLINT: the accessors are this file's vocabulary
using OptTensor = c10::optional<at::Tensor>;
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

// table [rows, >= W] fp32 rows (row-major, padded ld allowed), state [rows], zn [rows, 2 * (W - D1)]
// contiguous, keys int64 [n], grads [n, W] contiguous; W is the gradient's width, rows the table's row count.
void sparse_adagrad_ftrl(at::Tensor& table, at::Tensor& state, at::Tensor& zn, int64_t D1, const at::Tensor& keys,
                         int64_t base, const at::Tensor& grads, double lr, double eps, double alpha, double beta,
                         double l1, double l2, double grad_scale, const OptTensor& n_dev, const OptTensor& oor,
                         int64_t blocks) {
  TORCH_CHECK(alpha > 0, "alpha is ", alpha, ", expected a positive rate");
  TORCH_CHECK(beta >= 0, "beta is ", beta, ", expected >= 0");
  TORCH_CHECK(l1 >= 0, "l1 is ", l1, ", expected >= 0");
  TORCH_CHECK(l2 >= 0, "l2 is ", l2, ", expected >= 0");
  TORCH_CHECK(std::isfinite((float)grad_scale) && (float)grad_scale > 0, "grad_scale is ", grad_scale,
              ", expected a finite positive factor");
  TORCH_CHECK(blocks >= 0 && blocks <= minips_k::kWideFtrlMaxBlocks, "blocks is ", blocks,
              ", expected 0 <= blocks <= ", minips_k::kWideFtrlMaxBlocks);
  TORCH_CHECK(grads.dim() == 2 && grads.size(1) >= 2, "grads must be a [n, W] matrix of W >= 2 columns");
  TORCH_CHECK(table.dim() == 2, "table must be a [rows, >= W] matrix");
  const int64_t n = keys.numel(), W = grads.size(1), rows = table.size(0);
  TORCH_CHECK(W <= (1 << 20), "grads is ", W, " wide, expected <= 2^20 columns");
  TORCH_CHECK(D1 >= 1 && D1 < W, "D1 (split) is ", D1, ", expected 1 <= D1 < W = ", W);
  const int64_t Wf = W - D1;
  DeviceGuard gd(gpu_of(table, "table"));
  float* tp = dev_rows<float>(table, "table", rows, W);
  TORCH_CHECK(state.dim() == 1 && state.size(0) == rows, "state has shape ", state.sizes(), ", expected [", rows,
              "] (one accumulator per table row)");
  float* sp = dev<float>(state, "state", rows);
  TORCH_CHECK(zn.dim() == 2 && zn.size(0) == rows && zn.size(1) == 2 * Wf, "zn has shape ", zn.sizes(),
              ", expected [", rows, ", ", 2 * Wf, "] (z | n of the wide columns per table row)");
  float* zp = dev<float>(zn, "zn", rows * 2 * Wf);
  const int64_t* kp = dev<int64_t>(keys, "keys", n);
  TORCH_CHECK(grads.size(0) >= n, "grads holds ", grads.size(0), " rows, keys ", n);
  const float* gp = dev<float>(grads, "grads", n * W);
  const int64_t* nd = dev_opt<int64_t>(n_dev, "n_dev", 1);
  int64_t* op = dev_opt<int64_t>(oor, "oor", 1);
  minips_k::sparse_adagrad_ftrl(tp, table.stride(0), sp, zp, rows, (int)D1, (int)W, kp, n, nd, base, gp, (float)lr,
                                (float)eps, (float)alpha, (float)beta, (float)l1, (float)l2, (float)grad_scale, op,
                                (int)blocks, stream_of(table));
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "minips_amd row-wise Adagrad + FTRL-Proximal split-row kernel (gfx950)";
  m.def("sparse_adagrad_ftrl", &sparse_adagrad_ftrl, py::arg("table"), py::arg("state"), py::arg("zn"),
        py::arg("D1"), py::arg("keys"), py::arg("base"), py::arg("grads"), py::arg("lr"), py::arg("eps"),
        py::arg("alpha"), py::arg("beta"), py::arg("l1"), py::arg("l2"), py::arg("grad_scale"), py::arg("n_dev"),
        py::arg("oor"), py::arg("blocks"));
}
