// Torch-facing binding of the field-aware factorization-machine forward and backward (module minips_amd._ffmk;
// launchers and the rule in csrc/kernels/ffm.h). A torch extension of its own, like _fmk: the module and the
// table of its validation test (tests/test_ffmk_validation.py) stay the complete description of each other.
// Every device pointer comes from a checked accessor of tensor_access.h, the ops launch on the current HIP
// stream of the rows' device under a device guard (no sync, no host read: the unique count is taken on the
// device), and a bad argument raises before anything is launched.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <cmath>

#include "../kernels/ffm.h"
#include "tensor_access.h"

namespace {

using namespace minips_access;  // NOLINT: the accessors are this file's vocabulary
using OptTensor = c10::optional<at::Tensor>;
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

void check_common(int64_t F, int64_t k, int64_t blocks, const at::Tensor& rows) {
  TORCH_CHECK(k >= 4 && k <= minips_k::kFfmMaxK && k % 4 == 0, "k is ", k, ", expected k % 4 == 0 and 4 <= k <= ",
              minips_k::kFfmMaxK);
  TORCH_CHECK(F >= 1 && F <= minips_k::kFfmMaxF && F * k <= minips_k::kFfmMaxFK, "F is ", F, " (k ", k,
              "), expected 1 <= F <= ", minips_k::kFfmMaxF, " and F * k <= ", minips_k::kFfmMaxFK);
  TORCH_CHECK(blocks >= 0 && blocks <= minips_k::kFfmMaxBlocks, "blocks is ", blocks, ", expected 0 <= blocks <= ",
              minips_k::kFfmMaxBlocks);
  TORCH_CHECK(rows.dim() == 2, "rows must be a [cap, >= F * k + 4] matrix");
  TORCH_CHECK(rows.size(0) < (1ll << 31), "rows holds ", rows.size(0), " rows, expected fewer than 2^31");
}

// rowptr int64 [B + 1], inv int64 [n], vals fp32 [n], fields int32 [n], labels fp32 [B], rows fp32
// [cap, >= F k + 4] (row-major, padded ld allowed), w0 optional fp32 [>= 1]; outputs z / dz / loss [B], rowid
// int32 [n].
void ffm_forward(const at::Tensor& rowptr, const at::Tensor& inv, const at::Tensor& vals, const at::Tensor& fields,
                 const at::Tensor& labels, const at::Tensor& rows, int64_t F, int64_t k, const OptTensor& w0,
                 double gscale, at::Tensor& z, at::Tensor& dz, at::Tensor& loss, at::Tensor& rowid, int64_t blocks) {
  check_common(F, k, blocks, rows);
  TORCH_CHECK(std::isfinite((float)gscale), "gscale is ", gscale, ", expected a finite factor");
  TORCH_CHECK(rowptr.dim() == 1 && rowptr.numel() >= 1, "rowptr must be a [B + 1] vector");
  TORCH_CHECK(inv.dim() == 1 && vals.dim() == 1 && fields.dim() == 1 && labels.dim() == 1 && rowid.dim() == 1 &&
                  z.dim() == 1 && dz.dim() == 1 && loss.dim() == 1,
              "inv, vals, fields, labels, rowid, z, dz and loss must be vectors");
  const int64_t B = rowptr.numel() - 1, n = inv.numel(), cap = rows.size(0);
  TORCH_CHECK(B < (1ll << 31) && n < (1ll << 31), "B is ", B, " and n is ", n, ", expected fewer than 2^31");
  TORCH_CHECK(vals.numel() == n, "vals holds ", vals.numel(), " values, inv ", n, " lookups");
  TORCH_CHECK(fields.numel() == n, "fields holds ", fields.numel(), " values, inv ", n, " lookups");
  TORCH_CHECK(labels.numel() == B, "labels holds ", labels.numel(), " values, rowptr says ", B, " samples");
  DeviceGuard gd(gpu_of(rows, "rows"));
  const float* rp = dev_rows<float>(rows, "rows", cap, F * k + 4);
  const int64_t* pp = dev<int64_t>(rowptr, "rowptr", B + 1);
  const int64_t* ip = dev<int64_t>(inv, "inv", n);
  const float* vp = dev<float>(vals, "vals", n);
  const int32_t* fp = dev<int32_t>(fields, "fields", n);
  const float* lp = dev<float>(labels, "labels", B);
  const float* wp = dev_opt<float>(w0, "w0", 1);
  float* zp = dev<float>(z, "z", B);
  float* dp = dev<float>(dz, "dz", B);
  float* op = dev<float>(loss, "loss", B);
  int32_t* ri = dev<int32_t>(rowid, "rowid", n);
  minips_k::ffm_forward(pp, ip, vp, fp, lp, rp, cap > 1 ? rows.stride(0) : rows.size(1), cap, (int)F, (int)k, wp,
                        (float)gscale, B, n, zp, dp, op, ri, (int)blocks, stream_of(rows));
}

// members / memrow / rowid / fields int32 [n] (memrow sorted), rowptr int64 [B + 1], inv int64 [n], vals fp32
// [n], dz fp32 [B], rows fp32 [cap, >= F k + 4]; grad_rows fp32 [cap, F k + 4] contiguous.
void ffm_backward(const at::Tensor& members, const at::Tensor& memrow, const at::Tensor& rowid,
                  const at::Tensor& rowptr, const at::Tensor& inv, const at::Tensor& vals, const at::Tensor& fields,
                  const at::Tensor& dz, const at::Tensor& rows, int64_t F, int64_t k, at::Tensor& grad_rows,
                  int64_t blocks) {
  check_common(F, k, blocks, rows);
  TORCH_CHECK(members.dim() == 1 && memrow.dim() == 1 && rowid.dim() == 1 && inv.dim() == 1 && vals.dim() == 1 &&
                  fields.dim() == 1 && dz.dim() == 1,
              "members, memrow, rowid, inv, vals, fields and dz must be vectors");
  TORCH_CHECK(rowptr.dim() == 1 && rowptr.numel() >= 1, "rowptr must be a [B + 1] vector");
  const int64_t n = members.numel(), B = dz.numel(), cap = rows.size(0), W = F * k + 4;
  TORCH_CHECK(B < (1ll << 31) && n < (1ll << 31), "B is ", B, " and n is ", n, ", expected fewer than 2^31");
  TORCH_CHECK(rowptr.numel() == B + 1, "rowptr holds ", rowptr.numel(), " entries, dz says ", B, " samples");
  TORCH_CHECK(memrow.numel() == n && rowid.numel() == n && inv.numel() == n && vals.numel() == n &&
                  fields.numel() == n,
              "memrow holds ", memrow.numel(), ", rowid ", rowid.numel(), ", inv ", inv.numel(), ", vals ",
              vals.numel(), " and fields ", fields.numel(), " entries, members ", n, " lookups");
  TORCH_CHECK(grad_rows.dim() == 2 && grad_rows.size(0) >= cap && grad_rows.size(1) == W, "grad_rows has shape ",
              grad_rows.sizes(), ", expected [>= ", cap, ", ", W, "]");
  DeviceGuard gd(gpu_of(rows, "rows"));
  const float* rp = dev_rows<float>(rows, "rows", cap, W);
  const int32_t* mp = dev<int32_t>(members, "members", n);
  const int32_t* mr = dev<int32_t>(memrow, "memrow", n);
  const int32_t* ri = dev<int32_t>(rowid, "rowid", n);
  const int64_t* pp = dev<int64_t>(rowptr, "rowptr", B + 1);
  const int64_t* ip = dev<int64_t>(inv, "inv", n);
  const float* vp = dev<float>(vals, "vals", n);
  const int32_t* fp = dev<int32_t>(fields, "fields", n);
  const float* dp = dev<float>(dz, "dz", B);
  float* gp = dev<float>(grad_rows, "grad_rows", cap * W);
  if (n == 0 || B == 0 || cap == 0) return;
  const int64_t pf = minips_k::ffm_backward_part_floats(n, (int)W);
  at::Tensor part;
  if (pf > 0) part = at::empty({pf}, rows.options());
  minips_k::ffm_backward(mp, mr, ri, pp, ip, vp, fp, dp, rp, cap > 1 ? rows.stride(0) : rows.size(1), cap, (int)F,
                         (int)k, B, n, gp, pf > 0 ? part.data_ptr<float>() : nullptr, (int)blocks, stream_of(rows));
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "minips_amd field-aware factorization-machine forward / backward kernels (gfx950)";
  m.def("ffm_forward", &ffm_forward, py::arg("rowptr"), py::arg("inv"), py::arg("vals"), py::arg("fields"),
        py::arg("labels"), py::arg("rows"), py::arg("F"), py::arg("k"), py::arg("w0"), py::arg("gscale"), py::arg("z"),
        py::arg("dz"), py::arg("loss"), py::arg("rowid"), py::arg("blocks"));
  m.def("ffm_backward", &ffm_backward, py::arg("members"), py::arg("memrow"), py::arg("rowid"), py::arg("rowptr"),
        py::arg("inv"), py::arg("vals"), py::arg("fields"), py::arg("dz"), py::arg("rows"), py::arg("F"),
        py::arg("k"), py::arg("grad_rows"), py::arg("blocks"));
  m.attr("GROUP_MAX") = minips_k::kFfmGroupMax;
  m.attr("WAVE_MAX") = minips_k::kFfmWaveMax;
  m.attr("CHUNK") = minips_k::kFfmChunk;
  m.attr("MAX_F") = minips_k::kFfmMaxF;
  m.attr("MAX_K") = minips_k::kFfmMaxK;
  m.attr("MAX_FK") = minips_k::kFfmMaxFK;
}
