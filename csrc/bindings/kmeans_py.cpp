// Torch-facing binding of K-Means' fused step kernels (module minips_amd._kmk; launchers and the rule in
// csrc/kernels/kmeans.h). A torch extension of its own, like _gmmk: the module and the table of its validation test
// (tests/test_kmk_validation.py) stay the complete description of each other. Every device pointer comes from a
// checked accessor of tensor_access.h, the ops launch on the current HIP stream of their first tensor's device under a
// device guard (no sync, no host read), and a bad argument raises before anything is launched.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include "../kernels/kmeans.h"
#include "tensor_access.h"

namespace {

using namespace minips_access;  // NOLINT: the accessors are this file's vocabulary
using OptTensor = c10::optional<at::Tensor>;
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

void check_n(int64_t n) {
  TORCH_CHECK(n < (1ll << 31) - minips_k::kKmGroup, "X holds ", n, " points, expected fewer than 2^31 - ",
              minips_k::kKmGroup);
}

void check_blocks(int64_t blocks) {
  TORCH_CHECK(blocks >= 0 && blocks <= minips_k::kKmMaxBlocks, "blocks is ", blocks, ", expected 0 <= blocks <= ",
              minips_k::kKmMaxBlocks);
}

// X fp32 [n, D] (row-major, padded ld allowed, any alignment), C fp32 [K, D] contiguous; assign int32 [n], dist fp32
// [n], sse fp64 [1], bad optional int32 [1] (added to).
void km_nearest(const at::Tensor& X, const at::Tensor& C, at::Tensor& assign, at::Tensor& dist, at::Tensor& sse,
                const OptTensor& bad, int64_t blocks) {
  TORCH_CHECK(X.dim() == 2, "X must be a [n, D] matrix");
  TORCH_CHECK(C.dim() == 2, "C must be a [K, D] matrix");
  const int64_t n = X.size(0), D = C.size(1), K = C.size(0);
  TORCH_CHECK(minips_k::km_shape_ok(K, D), "C has shape ", C.sizes(), ", expected 1 <= K <= ", minips_k::kKmMaxK,
              " and 1 <= D <= ", minips_k::kKmMaxD);
  TORCH_CHECK(X.size(1) == D, "X has shape ", X.sizes(), ", C says D = ", D);
  check_n(n);
  check_blocks(blocks);
  TORCH_CHECK(assign.dim() == 1 && assign.numel() == n, "assign has shape ", assign.sizes(), ", expected [", n, "]");
  TORCH_CHECK(dist.dim() == 1 && dist.numel() == n, "dist has shape ", dist.sizes(), ", expected [", n, "]");
  TORCH_CHECK(sse.numel() == 1, "sse holds ", sse.numel(), " values, expected 1");
  if (present(bad)) TORCH_CHECK(bad->numel() == 1, "bad holds ", bad->numel(), " counters, expected 1");
  DeviceGuard gd(gpu_of(X, "X"));
  const float* xp = dev_rows<float>(X, "X", n, D);
  const float* cp = dev<float>(C, "C", K * D);
  int32_t* ap = dev<int32_t>(assign, "assign", n);
  float* dp = dev<float>(dist, "dist", n);
  double* sp = dev<double>(sse, "sse", 1);
  int32_t* bp = dev_opt<int32_t>(bad, "bad", 1);
  const int64_t nt = minips_k::km_chunks(n);
  at::Tensor cn = at::empty({K}, X.options());
  at::Tensor ssepart = at::empty({nt}, X.options().dtype(at::kDouble));
  at::Tensor badpart = at::empty({nt}, X.options().dtype(at::kInt));
  minips_k::km_nearest(xp, n > 1 ? X.stride(0) : D, n, (int)D, cp, (int)K, ap, dp, sp, bp, cn.data_ptr<float>(),
                       ssepart.data_ptr<double>(), badpart.data_ptr<int32_t>(), (int)blocks, stream_of(X));
}

// X fp32 [n, D] (as above), assign int32 [n]; sums fp32 [K, D] contiguous, counts int32 [K].
void km_sums(const at::Tensor& X, const at::Tensor& assign, at::Tensor& sums, at::Tensor& counts, int64_t blocks) {
  TORCH_CHECK(X.dim() == 2, "X must be a [n, D] matrix");
  TORCH_CHECK(sums.dim() == 2, "sums must be a [K, D] matrix");
  const int64_t n = X.size(0), D = sums.size(1), K = sums.size(0);
  TORCH_CHECK(minips_k::km_shape_ok(K, D), "sums has shape ", sums.sizes(), ", expected 1 <= K <= ",
              minips_k::kKmMaxK, " and 1 <= D <= ", minips_k::kKmMaxD);
  TORCH_CHECK(X.size(1) == D, "X has shape ", X.sizes(), ", sums says D = ", D);
  check_n(n);
  check_blocks(blocks);
  TORCH_CHECK(assign.dim() == 1 && assign.numel() == n, "assign has shape ", assign.sizes(), ", expected [", n, "]");
  TORCH_CHECK(counts.dim() == 1 && counts.numel() == K, "counts has shape ", counts.sizes(), ", expected [", K, "]");
  DeviceGuard gd(gpu_of(X, "X"));
  const float* xp = dev_rows<float>(X, "X", n, D);
  const int32_t* ap = dev<int32_t>(assign, "assign", n);
  float* sp = dev<float>(sums, "sums", K * D);
  int32_t* cp = dev<int32_t>(counts, "counts", K);
  at::Tensor ws = at::empty({minips_k::km_sums_ws_ints(n, (int)K)}, X.options().dtype(at::kInt));
  const int64_t pf = minips_k::km_sums_part_floats(n, (int)D);
  at::Tensor part;
  if (pf > 0) part = at::empty({pf}, X.options());
  minips_k::km_sums(xp, n > 1 ? X.stride(0) : D, n, (int)D, ap, (int)K, sp, cp, ws.data_ptr<int32_t>(),
                    part.defined() ? part.data_ptr<float>() : nullptr, (int)blocks, stream_of(X));
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "minips_amd K-Means fused step kernels (gfx950)";
  m.def("km_nearest", &km_nearest, py::arg("X"), py::arg("C"), py::arg("assign"), py::arg("dist"), py::arg("sse"),
        py::arg("bad"), py::arg("blocks"));
  m.def("km_sums", &km_sums, py::arg("X"), py::arg("assign"), py::arg("sums"), py::arg("counts"), py::arg("blocks"));
  m.attr("MAX_K") = minips_k::kKmMaxK;
  m.attr("MAX_D") = minips_k::kKmMaxD;
  m.attr("TILE") = minips_k::kKmTile;
  m.attr("STRIP") = minips_k::kKmStrip;
  m.attr("CHUNK") = minips_k::kKmChunk;
  m.attr("WAVE_MAX") = minips_k::kKmWaveMax;
  m.attr("ROW_CHUNK") = minips_k::kKmRowChunk;
}
