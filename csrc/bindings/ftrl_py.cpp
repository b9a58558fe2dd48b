// Torch-facing binding of the FTRL-Proximal sparse apply (module minips_amd._ftrlk; launcher in
// csrc/kernels/ftrl.h). A torch extension of its own, like _evalk and _optk: each module and the table of
// its validation test stay the complete description of each other (this one: tests/test_ftrlk_validation.py).
// As in ops_py.cpp, every device pointer comes from a checked accessor of tensor_access.h, the op launches
// on the current HIP stream of the table's device under a device guard (graph-capture safe: no sync in
// here), and a bad argument raises before anything is launched.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include "../kernels/ftrl.h"
#include "tensor_access.h"

namespace {

using namespace minips_access;  // NOLINT: the accessors are this file's vocabulary
using OptTensor = c10::optional<at::Tensor>;
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

// table [rows, >= W] fp32 rows (row-major, padded ld allowed), zn [rows, 2W] contiguous, keys int64 [n],
// grads [n, W] contiguous; W is the gradient's width, rows the table's row count.
void sparse_ftrl(at::Tensor& table, at::Tensor& zn, const at::Tensor& keys, int64_t base, const at::Tensor& grads,
                 double alpha, double beta, double l1, double l2, const OptTensor& n_dev, const OptTensor& oor,
                 int64_t blocks) {
  TORCH_CHECK(alpha > 0, "alpha is ", alpha, ", expected a positive rate");
  TORCH_CHECK(beta >= 0, "beta is ", beta, ", expected >= 0");
  TORCH_CHECK(l1 >= 0, "l1 is ", l1, ", expected >= 0");
  TORCH_CHECK(l2 >= 0, "l2 is ", l2, ", expected >= 0");
  TORCH_CHECK(blocks >= 0 && blocks <= minips_k::kFtrlMaxBlocks, "blocks is ", blocks, ", expected 0 <= blocks <= ",
              minips_k::kFtrlMaxBlocks);
  TORCH_CHECK(grads.dim() == 2 && grads.size(1) >= 1, "grads must be a [n, W] matrix");
  TORCH_CHECK(table.dim() == 2, "table must be a [rows, >= W] matrix");
  const int64_t n = keys.numel(), W = grads.size(1), rows = table.size(0);
  TORCH_CHECK(W <= (1 << 20), "grads is ", W, " wide, expected <= 2^20 columns");
  DeviceGuard gd(gpu_of(table, "table"));
  float* tp = dev_rows<float>(table, "table", rows, W);
  TORCH_CHECK(zn.dim() == 2 && zn.size(0) == rows && zn.size(1) == 2 * W, "zn has shape ", zn.sizes(),
              ", expected [", rows, ", ", 2 * W, "] (z | n per table row)");
  float* zp = dev<float>(zn, "zn", rows * 2 * W);
  const int64_t* kp = dev<int64_t>(keys, "keys", n);
  TORCH_CHECK(grads.size(0) >= n, "grads holds ", grads.size(0), " rows, keys ", n);
  const float* gp = dev<float>(grads, "grads", n * W);
  const int64_t* nd = dev_opt<int64_t>(n_dev, "n_dev", 1);
  int64_t* op = dev_opt<int64_t>(oor, "oor", 1);
  minips_k::sparse_ftrl(tp, table.stride(0), zp, rows, kp, n, nd, base, (int)W, gp, (float)alpha, (float)beta,
                        (float)l1, (float)l2, op, (int)blocks, stream_of(table));
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "minips_amd FTRL-Proximal sparse-table kernel (gfx950)";
  m.def("sparse_ftrl", &sparse_ftrl, py::arg("table"), py::arg("zn"), py::arg("keys"), py::arg("base"),
        py::arg("grads"), py::arg("alpha"), py::arg("beta"), py::arg("l1"), py::arg("l2"), py::arg("n_dev"),
        py::arg("oor"), py::arg("blocks"));
}
