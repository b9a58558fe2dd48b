// Torch-facing bindings of the gradient-clipping kernels (module minips_amd._optk; launchers in
// csrc/kernels/gradclip.h). A torch extension of its own, like _evalk: minips_amd._kernels and the table
// of tests/test_bindings_validation.py stay the complete description of each other, and this module has
// its own table (tests/test_optk_validation.py). As in ops_py.cpp, every device pointer comes from a
// checked accessor of tensor_access.h, ops launch on the current HIP stream of the tensors' device under
// a device guard (graph-capture safe: no sync in here), and a bad argument raises before anything is
// launched.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include "../kernels/gradclip.h"
#include "tensor_access.h"

namespace {

using minips_k::bf16_t;
using namespace minips_access;  // NOLINT: the accessors are this file's vocabulary
using OptTensor = c10::optional<at::Tensor>;
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

void grad_sumsq(const at::Tensor& g, const SlabList& slabs, at::Tensor& part, int64_t L) {
  const int64_t n = g.numel();
  TORCH_CHECK(L >= 1 && L <= minips_k::kSumsqMaxBlocks, "L is ", L, ", expected 1 <= L <= ",
              minips_k::kSumsqMaxBlocks);
  TORCH_CHECK(n % 4 == 0, "g holds ", n, " elements, expected a multiple of 4");
  DeviceGuard gd(gpu_of(g, "g"));
  const float* gp = dev<float>(g, "g", n);
  aligned16(g, "g");
  const minips_k::AdamSlabs sl = parse_slabs(slabs, n, "grad_sumsq");
  double* pp = dev<double>(part, "part", L);
  minips_k::grad_sumsq(gp, n, sl.n ? &sl : nullptr, pp, (int)L, stream_of(g));
}

void adam_clip_apply(at::Tensor& w, at::Tensor& m, at::Tensor& v, at::Tensor& g, const SlabList& slabs, double lr,
                     double beta1, double beta2, double eps, double weight_decay, int64_t step,
                     const OptTensor& step_dev, const OptTensor& w_bf16, bool zero_g, const at::Tensor& part,
                     int64_t np, double max_norm, at::Tensor& stats, bool write_stats) {
  const int64_t n = w.numel();
  TORCH_CHECK(n % 4 == 0, "w holds ", n, " elements, expected a multiple of 4");
  TORCH_CHECK(np >= 1 && np <= minips_k::kClipMaxParts, "np is ", np, ", expected 1 <= np <= ",
              minips_k::kClipMaxParts);
  TORCH_CHECK(max_norm > 0, "max_norm is ", max_norm, ", expected a positive norm");
  TORCH_CHECK(m.numel() == n, "m holds ", m.numel(), " elements, w ", n);
  TORCH_CHECK(v.numel() == n, "v holds ", v.numel(), " elements, w ", n);
  TORCH_CHECK(g.numel() == n, "g holds ", g.numel(), " elements, w ", n);
  TORCH_CHECK(!present(w_bf16) || w_bf16->numel() == n, "w_bf16 holds ", present(w_bf16) ? w_bf16->numel() : 0,
              " elements, w ", n);
  DeviceGuard gd(gpu_of(w, "w"));
  float* wp = dev<float>(w, "w", n);
  float* mp = dev<float>(m, "m", n);
  float* vp = dev<float>(v, "v", n);
  float* gp = dev<float>(g, "g", n);
  aligned16(w, "w");
  aligned16(m, "m");
  aligned16(v, "v");
  aligned16(g, "g");
  const minips_k::AdamSlabs sl = parse_slabs(slabs, n, "adam_clip_apply");
  const int* sd = dev_opt<int>(step_dev, "step_dev", 1);
  bf16_t* wb = dev_opt<bf16_t>(w_bf16, "w_bf16", n);
  TORCH_CHECK(!wb || reinterpret_cast<uintptr_t>(wb) % 8 == 0, "w_bf16 must be 8-byte aligned");
  const double* pp = dev<double>(part, "part", np);
  double* sp = dev<double>(stats, "stats", 4);
  minips_k::adam_clip_apply(wp, mp, vp, gp, n, sl.n ? &sl : nullptr, (float)lr, (float)beta1, (float)beta2,
                            (float)eps, (float)weight_decay, (int)step, sd, wb, zero_g, pp, (int)np, max_norm, sp,
                            write_stats, stream_of(w));
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "minips_amd gradient-clipping kernels (gfx950)";
  m.def("grad_sumsq", &grad_sumsq, py::arg("g"), py::arg("slabs"), py::arg("part"), py::arg("L"));
  m.def("adam_clip_apply", &adam_clip_apply, py::arg("w"), py::arg("m"), py::arg("v"), py::arg("g"),
        py::arg("slabs"), py::arg("lr"), py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
        py::arg("weight_decay"), py::arg("step"), py::arg("step_dev"), py::arg("w_bf16"), py::arg("zero_g"),
        py::arg("part"), py::arg("np"), py::arg("max_norm"), py::arg("stats"), py::arg("write_stats"));
}
