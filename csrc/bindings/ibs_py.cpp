// Torch-facing binding of the in-batch sampled softmax kernels (module minips_amd._ibsk; launchers and the rule in
// csrc/kernels/ibs.h). A torch extension of its own, like _w2vk, _alsk and _gmmk: the module and the table of its
// validation test (tests/test_ibsk_validation.py) stay the complete description of each other. Every device pointer
// comes from a checked accessor of tensor_access.h, the ops launch on the current HIP stream of their first tensor's
// device under a device guard (no sync, no host read), and a bad argument raises before anything is launched.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <cmath>

#include "../kernels/ibs.h"
#include "tensor_access.h"

namespace {

using namespace minips_access;  // NOLINT: the accessors are this file's vocabulary
using OptTensor = c10::optional<at::Tensor>;
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

// the checks both ops share; returns P
int64_t check_common(const at::Tensor& inv, const at::Tensor& rows, int64_t d, double tau, const OptTensor& logq,
                     int64_t blocks) {
  TORCH_CHECK(minips_k::ibs_d_ok(d), "d is ", d, ", expected d % 4 == 0 and ", minips_k::kIbsMinD, " <= d <= ",
              minips_k::kIbsMaxD);
  TORCH_CHECK((float)tau > 0.f && std::isfinite((float)tau) && std::isfinite(1.f / (float)tau), "tau is ", tau,
              ", expected a positive finite temperature");
  TORCH_CHECK(blocks >= 0 && blocks <= minips_k::kIbsMaxBlocks, "blocks is ", blocks, ", expected 0 <= blocks <= ",
              minips_k::kIbsMaxBlocks);
  TORCH_CHECK(rows.dim() == 2, "rows must be a [cap, >= d] matrix");
  TORCH_CHECK(rows.size(0) < (1ll << 31), "rows holds ", rows.size(0), " rows, expected fewer than 2^31");
  TORCH_CHECK(inv.dim() == 1 && inv.numel() % 2 == 0, "inv must be a vector of 2 P lookups, it holds ", inv.numel());
  const int64_t P = inv.numel() / 2;
  TORCH_CHECK(P < (1ll << 30), "inv holds ", P, " pairs, expected fewer than 2^30");
  if (present(logq)) TORCH_CHECK(logq->dim() == 1 && logq->numel() == P, "logq has shape ", logq->sizes(),
                                 ", expected [P] = [", P, "]");
  return P;
}

// inv int64 [2 P], rows fp32 [cap, >= d] (row-major, padded ld allowed), logq optional fp32 [P]; outputs lse and
// loss fp32 [P].
void ibs_forward(const at::Tensor& inv, const at::Tensor& rows, int64_t d, double tau, const OptTensor& logq,
                 at::Tensor& lse, at::Tensor& loss, int64_t blocks) {
  const int64_t P = check_common(inv, rows, d, tau, logq, blocks);
  TORCH_CHECK(lse.dim() == 1 && lse.numel() == P, "lse has shape ", lse.sizes(), ", expected [P] = [", P, "]");
  TORCH_CHECK(loss.dim() == 1 && loss.numel() == P, "loss has shape ", loss.sizes(), ", expected [P] = [", P, "]");
  const int64_t cap = rows.size(0);
  DeviceGuard gd(gpu_of(rows, "rows"));
  const float* rp = dev_rows<float>(rows, "rows", cap, d);
  const int64_t* ip = dev<int64_t>(inv, "inv", 2 * P);
  const float* qp = dev_opt<float>(logq, "logq", P);
  float* sp = dev<float>(lse, "lse", P);
  float* lp = dev<float>(loss, "loss", P);
  minips_k::ibs_forward(ip, rp, cap > 1 ? rows.stride(0) : rows.size(1), cap, (int)d, (float)tau, qp, P, sp, lp,
                        (int)blocks, stream_of(rows));
}

// members / memrow int32 [2 P] (memrow sorted), inv int64 [2 P], rows fp32 [cap, >= d], lse fp32 [P] (ibs_forward's),
// logq optional fp32 [P]; grad_rows fp32 [>= cap, d] contiguous.
void ibs_backward(const at::Tensor& members, const at::Tensor& memrow, const at::Tensor& inv, const at::Tensor& rows,
                  int64_t d, double tau, const OptTensor& logq, const at::Tensor& lse, double gscale,
                  at::Tensor& grad_rows, int64_t blocks) {
  const int64_t P = check_common(inv, rows, d, tau, logq, blocks);
  TORCH_CHECK(std::isfinite((float)gscale), "gscale is ", gscale, ", expected a finite factor");
  TORCH_CHECK(members.dim() == 1 && members.numel() == 2 * P, "members holds ", members.numel(),
              " lookups, inv says ", 2 * P);
  TORCH_CHECK(memrow.dim() == 1 && memrow.numel() == 2 * P, "memrow holds ", memrow.numel(), " entries, inv says ",
              2 * P);
  TORCH_CHECK(lse.dim() == 1 && lse.numel() == P, "lse has shape ", lse.sizes(), ", expected [P] = [", P, "]");
  const int64_t cap = rows.size(0);
  TORCH_CHECK(grad_rows.dim() == 2 && grad_rows.size(0) >= cap && grad_rows.size(1) == d, "grad_rows has shape ",
              grad_rows.sizes(), ", expected [>= ", cap, ", ", d, "]");
  DeviceGuard gd(gpu_of(rows, "rows"));
  const float* rp = dev_rows<float>(rows, "rows", cap, d);
  const int32_t* mp = dev<int32_t>(members, "members", 2 * P);
  const int32_t* mr = dev<int32_t>(memrow, "memrow", 2 * P);
  const int64_t* ip = dev<int64_t>(inv, "inv", 2 * P);
  const float* qp = dev_opt<float>(logq, "logq", P);
  const float* sp = dev<float>(lse, "lse", P);
  float* gp = dev<float>(grad_rows, "grad_rows", cap * d);
  if (P == 0 || cap == 0) return;
  const int64_t wf = minips_k::ibs_backward_ws_floats(P, (int)d), pf = minips_k::ibs_backward_part_floats(P, (int)d);
  at::Tensor ws = at::empty({wf}, rows.options()), part;
  if (pf > 0) part = at::empty({pf}, rows.options());
  minips_k::ibs_backward(mp, mr, ip, rp, cap > 1 ? rows.stride(0) : rows.size(1), cap, (int)d, (float)tau, qp, sp,
                         (float)gscale, P, gp, ws.data_ptr<float>(), pf > 0 ? part.data_ptr<float>() : nullptr,
                         (int)blocks, stream_of(rows));
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "minips_amd in-batch sampled softmax (two-tower retrieval) kernels (gfx950)";
  m.def("ibs_forward", &ibs_forward, py::arg("inv"), py::arg("rows"), py::arg("d"), py::arg("tau"), py::arg("logq"),
        py::arg("lse"), py::arg("loss"), py::arg("blocks"));
  m.def("ibs_backward", &ibs_backward, py::arg("members"), py::arg("memrow"), py::arg("inv"), py::arg("rows"),
        py::arg("d"), py::arg("tau"), py::arg("logq"), py::arg("lse"), py::arg("gscale"), py::arg("grad_rows"),
        py::arg("blocks"));
  m.attr("MIN_D") = minips_k::kIbsMinD;
  m.attr("MAX_D") = minips_k::kIbsMaxD;
  m.attr("TILE") = minips_k::kIbsTile;
  m.attr("WAVE_MAX") = minips_k::kIbsWaveMax;
  m.attr("CHUNK") = minips_k::kIbsChunk;
}
