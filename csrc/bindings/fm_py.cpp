// Torch-facing binding of the factorization-machine forward and backward (module minips_amd._fmk; launchers
// and the rule in csrc/kernels/fm.h). A torch extension of its own, like _evalk, _optk, _ftrlk and _wdftrlk:
// the module and the table of its validation test (tests/test_fmk_validation.py) stay the complete
// description of each other. Every device pointer comes from a checked accessor of tensor_access.h, the ops
// launch on the current HIP stream of the rows' device under a device guard (no sync, no host read: the
// unique count is taken on the device), and a bad argument raises before anything is launched.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <cmath>

#include "../kernels/fm.h"
#include "tensor_access.h"

namespace {

using namespace minips_access;  // NOLINT: the accessors are this file's vocabulary
using OptTensor = c10::optional<at::Tensor>;
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

void check_common(int64_t k, int64_t blocks, const at::Tensor& rows) {
  TORCH_CHECK(minips_k::fm_k_ok(k), "k is ", k, ", expected k % 4 == 0 and 4 <= k <= 60");
  TORCH_CHECK(blocks >= 0 && blocks <= minips_k::kFmMaxBlocks, "blocks is ", blocks, ", expected 0 <= blocks <= ",
              minips_k::kFmMaxBlocks);
  TORCH_CHECK(rows.dim() == 2, "rows must be a [cap, >= k + 4] matrix");
  TORCH_CHECK(rows.size(0) < (1ll << 31), "rows holds ", rows.size(0), " rows, expected fewer than 2^31");
}

// rowptr int64 [B + 1], inv int64 [n], vals fp32 [n], labels fp32 [B], rows fp32 [cap, >= k + 4] (row-major,
// padded ld allowed), w0 optional fp32 [>= 1]; outputs S [B, k], z / dz / loss [B], rowid int32 [n].
void fm_forward(const at::Tensor& rowptr, const at::Tensor& inv, const at::Tensor& vals, const at::Tensor& labels,
                const at::Tensor& rows, int64_t k, const OptTensor& w0, double gscale, at::Tensor& S, at::Tensor& z,
                at::Tensor& dz, at::Tensor& loss, at::Tensor& rowid, int64_t blocks) {
  check_common(k, blocks, rows);
  TORCH_CHECK(std::isfinite((float)gscale), "gscale is ", gscale, ", expected a finite factor");
  TORCH_CHECK(rowptr.dim() == 1 && rowptr.numel() >= 1, "rowptr must be a [B + 1] vector");
  TORCH_CHECK(inv.dim() == 1 && vals.dim() == 1 && labels.dim() == 1 && rowid.dim() == 1 && z.dim() == 1 &&
                  dz.dim() == 1 && loss.dim() == 1,
              "inv, vals, labels, rowid, z, dz and loss must be vectors");
  const int64_t B = rowptr.numel() - 1, n = inv.numel(), cap = rows.size(0);
  TORCH_CHECK(B < (1ll << 31) && n < (1ll << 31), "B is ", B, " and n is ", n, ", expected fewer than 2^31");
  TORCH_CHECK(vals.numel() == n, "vals holds ", vals.numel(), " values, inv ", n, " lookups");
  TORCH_CHECK(labels.numel() == B, "labels holds ", labels.numel(), " values, rowptr says ", B, " samples");
  TORCH_CHECK(S.dim() == 2 && S.size(1) == k, "S has shape ", S.sizes(), ", expected [", B, ", ", k, "]");
  DeviceGuard gd(gpu_of(rows, "rows"));
  const float* rp = dev_rows<float>(rows, "rows", cap, k + 4);
  const int64_t* pp = dev<int64_t>(rowptr, "rowptr", B + 1);
  const int64_t* ip = dev<int64_t>(inv, "inv", n);
  const float* vp = dev<float>(vals, "vals", n);
  const float* lp = dev<float>(labels, "labels", B);
  const float* wp = dev_opt<float>(w0, "w0", 1);
  float* Sp = dev<float>(S, "S", B * k);
  float* zp = dev<float>(z, "z", B);
  float* dp = dev<float>(dz, "dz", B);
  float* op = dev<float>(loss, "loss", B);
  int32_t* ri = dev<int32_t>(rowid, "rowid", n);
  minips_k::fm_forward(pp, ip, vp, lp, rp, cap > 1 ? rows.stride(0) : rows.size(1), cap, (int)k, wp, (float)gscale, B,
                       n, Sp, zp, dp, op, ri, (int)blocks, stream_of(rows));
}

// members / memrow / rowid int32 [n] (memrow sorted), vals fp32 [n], dz fp32 [B], S fp32 [B, k], rows fp32
// [cap, >= k + 4]; grad_rows fp32 [cap, k + 4] contiguous.
void fm_backward(const at::Tensor& members, const at::Tensor& memrow, const at::Tensor& rowid, const at::Tensor& vals,
                 const at::Tensor& dz, const at::Tensor& S, const at::Tensor& rows, int64_t k, at::Tensor& grad_rows,
                 int64_t blocks) {
  check_common(k, blocks, rows);
  TORCH_CHECK(members.dim() == 1 && memrow.dim() == 1 && rowid.dim() == 1 && vals.dim() == 1 && dz.dim() == 1,
              "members, memrow, rowid, vals and dz must be vectors");
  const int64_t n = members.numel(), B = dz.numel(), cap = rows.size(0), W = k + 4;
  TORCH_CHECK(B < (1ll << 31) && n < (1ll << 31), "B is ", B, " and n is ", n, ", expected fewer than 2^31");
  TORCH_CHECK(memrow.numel() == n && rowid.numel() == n && vals.numel() == n, "memrow holds ", memrow.numel(),
              ", rowid ", rowid.numel(), " and vals ", vals.numel(), " entries, members ", n, " lookups");
  TORCH_CHECK(S.dim() == 2 && S.size(0) == B && S.size(1) == k, "S has shape ", S.sizes(), ", expected [", B, ", ", k,
              "]");
  TORCH_CHECK(grad_rows.dim() == 2 && grad_rows.size(0) >= cap && grad_rows.size(1) == W, "grad_rows has shape ",
              grad_rows.sizes(), ", expected [>= ", cap, ", ", W, "]");
  DeviceGuard gd(gpu_of(rows, "rows"));
  const float* rp = dev_rows<float>(rows, "rows", cap, W);
  const int32_t* mp = dev<int32_t>(members, "members", n);
  const int32_t* mr = dev<int32_t>(memrow, "memrow", n);
  const int32_t* ri = dev<int32_t>(rowid, "rowid", n);
  const float* vp = dev<float>(vals, "vals", n);
  const float* dp = dev<float>(dz, "dz", B);
  const float* Sp = dev<float>(S, "S", B * k);
  float* gp = dev<float>(grad_rows, "grad_rows", cap * W);
  if (n == 0 || B == 0 || cap == 0) return;
  const int64_t pf = minips_k::fm_backward_part_floats(n, (int)W);
  at::Tensor part;
  if (pf > 0) part = at::empty({pf}, rows.options());
  minips_k::fm_backward(mp, mr, ri, vp, dp, Sp, rp, cap > 1 ? rows.stride(0) : rows.size(1), cap, (int)k, B, n, gp,
                        pf > 0 ? part.data_ptr<float>() : nullptr, (int)blocks, stream_of(rows));
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "minips_amd factorization-machine forward / backward kernels (gfx950)";
  m.def("fm_forward", &fm_forward, py::arg("rowptr"), py::arg("inv"), py::arg("vals"), py::arg("labels"),
        py::arg("rows"), py::arg("k"), py::arg("w0"), py::arg("gscale"), py::arg("S"), py::arg("z"), py::arg("dz"),
        py::arg("loss"), py::arg("rowid"), py::arg("blocks"));
  m.def("fm_backward", &fm_backward, py::arg("members"), py::arg("memrow"), py::arg("rowid"), py::arg("vals"),
        py::arg("dz"), py::arg("S"), py::arg("rows"), py::arg("k"), py::arg("grad_rows"), py::arg("blocks"));
  m.attr("GROUP_MAX") = minips_k::kFmGroupMax;
  m.attr("WAVE_MAX") = minips_k::kFmWaveMax;
  m.attr("CHUNK") = minips_k::kFmChunk;
}
