// Torch-facing binding of the ALS normal-equation kernels (module minips_amd._alsk; launchers and the rule in
// csrc/kernels/als.h). A torch extension of its own, like _fmk, _ldak and _w2vk: the module and the table of its
// validation test (tests/test_alsk_validation.py) stay the complete description of each other. Every device pointer
// comes from a checked accessor of tensor_access.h, the ops launch on the current HIP stream of their first tensor's
// device under a device guard (no sync, no host read), and a bad argument raises before anything is launched.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include "../kernels/als.h"
#include "tensor_access.h"

namespace {

using namespace minips_access;  // NOLINT: the accessors are this file's vocabulary
using OptTensor = c10::optional<at::Tensor>;
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

// rowptr int64 [B + 1], inv int64 [n], a / c fp32 [n], rows fp32 [cap, >= k] (row-major, padded ld allowed), reg
// fp32 [B], slot int64 [B], x_old / x_out / delta fp32 [m, k] contiguous (k is x_out's width), desc int32
// [n_desc, 3], multi int32 [n_multi, 3] (n_multi_desc: the leading descriptors that belong to them), gram0 optional
// fp32 [k, k], bad optional int32 [1].
void als_solve(const at::Tensor& rowptr, const at::Tensor& inv, const at::Tensor& a, const at::Tensor& c,
               const at::Tensor& rows, const at::Tensor& reg, const at::Tensor& slot, const at::Tensor& x_old,
               at::Tensor& x_out, at::Tensor& delta, const at::Tensor& desc, const at::Tensor& multi,
               int64_t n_multi_desc, const OptTensor& gram0, const OptTensor& bad, int64_t blocks) {
  TORCH_CHECK(x_out.dim() == 2, "x_out must be a [m, k] matrix");
  const int64_t m = x_out.size(0), k = x_out.size(1);
  TORCH_CHECK(minips_k::als_k_ok(k), "x_out is ", k, " wide: k % 4 == 0 and ", minips_k::kAlsMinK, " <= k <= ",
              minips_k::kAlsMaxK);
  TORCH_CHECK(blocks >= 0 && blocks <= minips_k::kAlsMaxBlocks, "blocks is ", blocks, ", expected 0 <= blocks <= ",
              minips_k::kAlsMaxBlocks);
  TORCH_CHECK(rows.dim() == 2, "rows must be a [cap, >= k] matrix");
  TORCH_CHECK(rows.size(0) < (1ll << 31), "rows holds ", rows.size(0), " rows, expected fewer than 2^31");
  TORCH_CHECK(rowptr.dim() == 1 && rowptr.numel() >= 1, "rowptr must be a vector of B + 1 entries");
  TORCH_CHECK(inv.dim() == 1 && a.dim() == 1 && c.dim() == 1, "inv, a and c must be vectors");
  TORCH_CHECK(reg.dim() == 1 && slot.dim() == 1, "reg and slot must be vectors");
  const int64_t B = rowptr.numel() - 1, n = inv.numel(), cap = rows.size(0);
  TORCH_CHECK(n < (1ll << 31) && B < (1ll << 31), "inv holds ", n, " lookups of ", B, " entities, expected < 2^31");
  TORCH_CHECK(a.numel() == n, "a holds ", a.numel(), " weights, inv ", n, " lookups");
  TORCH_CHECK(c.numel() == n, "c holds ", c.numel(), " weights, inv ", n, " lookups");
  TORCH_CHECK(reg.numel() == B, "reg holds ", reg.numel(), " values, rowptr says ", B, " entities");
  TORCH_CHECK(slot.numel() == B, "slot holds ", slot.numel(), " values, rowptr says ", B, " entities");
  TORCH_CHECK(x_old.dim() == 2 && x_old.size(0) == m && x_old.size(1) == k, "x_old has shape ", x_old.sizes(),
              ", expected x_out's [", m, ", ", k, "]");
  TORCH_CHECK(delta.dim() == 2 && delta.size(0) == m && delta.size(1) == k, "delta has shape ", delta.sizes(),
              ", expected x_out's [", m, ", ", k, "]");
  TORCH_CHECK(desc.dim() == 2 && desc.size(1) == 3, "desc has shape ", desc.sizes(), ", expected [n_desc, 3]");
  TORCH_CHECK(multi.dim() == 2 && multi.size(1) == 3, "multi has shape ", multi.sizes(), ", expected [n_multi, 3]");
  const int64_t n_desc = desc.size(0), n_multi = multi.size(0);
  TORCH_CHECK(n_desc < (1ll << 31), "desc holds ", n_desc, " descriptors, expected fewer than 2^31");
  TORCH_CHECK(n_multi_desc >= 0 && n_multi_desc <= n_desc && n_multi <= n_multi_desc, "n_multi_desc is ",
              n_multi_desc, ", expected n_multi = ", n_multi, " <= n_multi_desc <= n_desc = ", n_desc);
  if (present(gram0))
    TORCH_CHECK(gram0->dim() == 2 && gram0->size(0) == k && gram0->size(1) == k, "gram0 has shape ", gram0->sizes(),
                ", expected [", k, ", ", k, "]");
  if (present(bad)) TORCH_CHECK(bad->numel() == 1, "bad holds ", bad->numel(), " counters, expected 1");
  DeviceGuard gd(gpu_of(rows, "rows"));
  const float* rp = dev_rows<float>(rows, "rows", cap, k);
  const int64_t* pp = dev<int64_t>(rowptr, "rowptr", B + 1);
  const int64_t* ip = dev<int64_t>(inv, "inv", n);
  const float* ap = dev<float>(a, "a", n);
  const float* cp = dev<float>(c, "c", n);
  const float* gp = dev<float>(reg, "reg", B);
  const int64_t* sp = dev<int64_t>(slot, "slot", B);
  const float* xo = dev<float>(x_old, "x_old", m * k);
  float* xn = dev<float>(x_out, "x_out", m * k);
  float* dp = dev<float>(delta, "delta", m * k);
  const int32_t* de = dev<int32_t>(desc, "desc", n_desc * 3);
  const int32_t* mu = dev<int32_t>(multi, "multi", n_multi * 3);
  const float* g0 = dev_opt<float>(gram0, "gram0", k * k);
  int32_t* bp = dev_opt<int32_t>(bad, "bad", 1);
  if (n_desc == 0) return;
  at::Tensor ws;
  if (n_multi_desc > 0) ws = at::empty({n_multi_desc * minips_k::als_slot_floats((int)k)}, rows.options());
  minips_k::als_solve(pp, ip, ap, cp, n, rp, cap > 1 ? rows.stride(0) : rows.size(1), cap, (int)k, gp, sp, B, xo, xn,
                      dp, m, de, n_desc, n_multi_desc, mu, n_multi, n_multi_desc > 0 ? ws.data_ptr<float>() : nullptr,
                      g0, bp, (int)blocks, stream_of(rows));
}

// rows fp32 [R, >= k] (row-major, padded ld allowed) -> out fp32 [k, k] contiguous = rows[:, :k]^T rows[:, :k]
void als_gram(const at::Tensor& rows, at::Tensor& out) {
  TORCH_CHECK(out.dim() == 2 && out.size(0) == out.size(1), "out must be a [k, k] matrix");
  const int64_t k = out.size(0);
  TORCH_CHECK(minips_k::als_k_ok(k), "out is ", k, " wide: k % 4 == 0 and ", minips_k::kAlsMinK, " <= k <= ",
              minips_k::kAlsMaxK);
  TORCH_CHECK(rows.dim() == 2, "rows must be a [R, >= k] matrix");
  const int64_t R = rows.size(0);
  TORCH_CHECK(R < (1ll << 31), "rows holds ", R, " rows, expected fewer than 2^31");
  DeviceGuard gd(gpu_of(rows, "rows"));
  const float* rp = dev_rows<float>(rows, "rows", R, k);
  float* op = dev<float>(out, "out", k * k);
  const int64_t pf = minips_k::als_gram_part_floats(R, (int)k);
  at::Tensor part;
  if (pf > 0) part = at::empty({pf}, rows.options());
  minips_k::als_gram(rp, R > 1 ? rows.stride(0) : rows.size(1), R, (int)k, pf > 0 ? part.data_ptr<float>() : nullptr,
                     op, stream_of(rows));
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "minips_amd alternating-least-squares normal-equation kernels (gfx950)";
  m.def("als_solve", &als_solve, py::arg("rowptr"), py::arg("inv"), py::arg("a"), py::arg("c"), py::arg("rows"),
        py::arg("reg"), py::arg("slot"), py::arg("x_old"), py::arg("x_out"), py::arg("delta"), py::arg("desc"),
        py::arg("multi"), py::arg("n_multi_desc"), py::arg("gram0"), py::arg("bad"), py::arg("blocks"));
  m.def("als_gram", &als_gram, py::arg("rows"), py::arg("out"));
  m.attr("MIN_K") = minips_k::kAlsMinK;
  m.attr("MAX_K") = minips_k::kAlsMaxK;
  m.attr("STAGE") = minips_k::kAlsStage;
  m.attr("GRAM_STRIP") = minips_k::kAlsGramStrip;
  m.attr("MAX_CHUNK") = minips_k::kAlsMaxChunk;
}
