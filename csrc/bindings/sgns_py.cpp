// Torch-facing binding of the skip-gram negative-sampling kernels (module minips_amd._w2vk; launchers and the rule
// in csrc/kernels/sgns.h). A torch extension of its own, like _fmk, _ffmk and _ldak: the module and the table of its
// validation test (tests/test_w2vk_validation.py) stay the complete description of each other. Every device pointer
// comes from a checked accessor of tensor_access.h, the ops launch on the current HIP stream of their first
// tensor's device under a device guard (no sync, no host read: the unique count is taken on the device), and a bad
// argument raises before anything is launched.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <cmath>

#include "../kernels/sgns.h"
#include "tensor_access.h"

namespace {

using namespace minips_access;  // NOLINT: the accessors are this file's vocabulary
using OptTensor = c10::optional<at::Tensor>;
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

void check_common(int64_t d, int64_t N, int64_t blocks, const at::Tensor& rows) {
  TORCH_CHECK(minips_k::sgns_neg_ok(N), "N is ", N, ", expected 1 <= N <= ", minips_k::kSgnsMaxNeg);
  TORCH_CHECK(blocks >= 0 && blocks <= minips_k::kSgnsMaxBlocks, "blocks is ", blocks, ", expected 0 <= blocks <= ",
              minips_k::kSgnsMaxBlocks);
  TORCH_CHECK(rows.dim() == 2, "rows must be a [cap, >= d] matrix");
  TORCH_CHECK(minips_k::sgns_dim_ok(d), "h is ", d, " wide: rows and h hold d floats, d % 4 == 0 and 4 <= d <= ",
              minips_k::kSgnsMaxDim);
  TORCH_CHECK(rows.size(0) < (1ll << 31), "rows holds ", rows.size(0), " rows, expected fewer than 2^31");
}

// centres / contexts int64 [P], thr int64 [V] (the bits of the uint64 thresholds), alias int32 [V], negatives
// optional int32 [P, N]; keys int64 [P, N + 2]. seed, epoch and pair_base are the bits of uint64 values.
void sgns_lookups(const at::Tensor& centres, const at::Tensor& contexts, const at::Tensor& thr,
                  const at::Tensor& alias, int64_t T, int64_t seed, int64_t epoch, int64_t pair_base, int64_t N,
                  const OptTensor& negatives, at::Tensor& keys) {
  TORCH_CHECK(minips_k::sgns_neg_ok(N), "N is ", N, ", expected 1 <= N <= ", minips_k::kSgnsMaxNeg);
  TORCH_CHECK(centres.dim() == 1 && contexts.dim() == 1, "centres and contexts must be vectors");
  TORCH_CHECK(thr.dim() == 1 && alias.dim() == 1, "thr and alias must be vectors");
  const int64_t P = centres.numel(), V = thr.numel();
  TORCH_CHECK(contexts.numel() == P, "contexts holds ", contexts.numel(), " words, centres ", P);
  TORCH_CHECK(V >= 1 && V < (1ll << 31), "thr holds ", V, " words, expected 1 <= V < 2^31");
  TORCH_CHECK(alias.numel() == V, "alias holds ", alias.numel(), " entries, thr ", V);
  TORCH_CHECK(T >= 1 && T < (1ll << 59), "T is ", T, ", expected 1 <= T < 2^59");
  TORCH_CHECK(epoch >= 0, "epoch is ", epoch, ", expected >= 0");
  TORCH_CHECK(pair_base >= 0 && pair_base < (1ll << 56), "pair_base is ", pair_base, ", expected in [0, 2^56)");
  TORCH_CHECK(P * (N + 2) < (1ll << 31), "centres holds ", P, " pairs, expected P (N + 2) < 2^31");
  TORCH_CHECK(keys.dim() == 2 && keys.size(0) == P && keys.size(1) == N + 2, "keys has shape ", keys.sizes(),
              ", expected [P, N + 2] = [", P, ", ", N + 2, "]");
  if (present(negatives))
    TORCH_CHECK(negatives->dim() == 2 && negatives->size(0) == P && negatives->size(1) == N, "negatives has shape ",
                negatives->sizes(), ", expected [P, N] = [", P, ", ", N, "]");
  DeviceGuard gd(gpu_of(centres, "centres"));
  const int64_t* cp = dev<int64_t>(centres, "centres", P);
  const int64_t* op = dev<int64_t>(contexts, "contexts", P);
  const int64_t* tp = dev<int64_t>(thr, "thr", V);
  const int32_t* ap = dev<int32_t>(alias, "alias", V);
  const int32_t* np = dev_opt<int32_t>(negatives, "negatives", P * N);
  int64_t* kp = dev<int64_t>(keys, "keys", P * (N + 2));
  minips_k::sgns_lookups(cp, op, reinterpret_cast<const uint64_t*>(tp), ap, V, (uint64_t)T, (uint64_t)seed,
                         (uint64_t)epoch, (uint64_t)pair_base, (int)N, np, P, kp, stream_of(centres));
}

// inv int64 [P (N + 2)], rows fp32 [cap, >= d] (row-major, padded ld allowed); outputs e [P, N + 1], loss [P],
// h [P, d] contiguous (d is h's width).
void sgns_forward(const at::Tensor& inv, const at::Tensor& rows, int64_t N, double gscale, at::Tensor& e,
                  at::Tensor& loss, at::Tensor& h, int64_t blocks) {
  TORCH_CHECK(h.dim() == 2, "h must be a [P, d] matrix");
  const int64_t d = h.size(1), P = h.size(0);
  check_common(d, N, blocks, rows);
  TORCH_CHECK(std::isfinite((float)gscale), "gscale is ", gscale, ", expected a finite factor");
  TORCH_CHECK(inv.dim() == 1 && loss.dim() == 1, "inv and loss must be vectors");
  TORCH_CHECK(P * (N + 2) < (1ll << 31), "h holds ", P, " pairs, expected P (N + 2) < 2^31");
  TORCH_CHECK(inv.numel() == P * (N + 2), "inv holds ", inv.numel(), " lookups, h says ", P, " pairs of N + 2 = ",
              N + 2);
  TORCH_CHECK(e.dim() == 2 && e.size(0) == P && e.size(1) == N + 1, "e has shape ", e.sizes(), ", expected [", P,
              ", ", N + 1, "]");
  TORCH_CHECK(loss.numel() == P, "loss holds ", loss.numel(), " values, h says ", P, " pairs");
  const int64_t cap = rows.size(0);
  DeviceGuard gd(gpu_of(rows, "rows"));
  const float* rp = dev_rows<float>(rows, "rows", cap, d);
  const int64_t* ip = dev<int64_t>(inv, "inv", P * (N + 2));
  float* ep = dev<float>(e, "e", P * (N + 1));
  float* lp = dev<float>(loss, "loss", P);
  float* hp = dev<float>(h, "h", P * d);
  minips_k::sgns_forward(ip, rp, cap > 1 ? rows.stride(0) : rows.size(1), cap, (int)d, (int)N, (float)gscale, P, ep,
                         lp, hp, (int)blocks, stream_of(rows));
}

// members / memrow int32 [n], inv int64 [n], n = P (N + 2) (memrow sorted), e fp32 [P, N + 1], h fp32 [P, d],
// rows fp32 [cap, >= d]; grad_rows fp32 [>= cap, d] contiguous.
void sgns_backward(const at::Tensor& members, const at::Tensor& memrow, const at::Tensor& inv, const at::Tensor& e,
                   const at::Tensor& h, const at::Tensor& rows, int64_t N, at::Tensor& grad_rows, int64_t blocks) {
  TORCH_CHECK(h.dim() == 2, "h must be a [P, d] matrix");
  const int64_t d = h.size(1), P = h.size(0);
  check_common(d, N, blocks, rows);
  TORCH_CHECK(members.dim() == 1 && memrow.dim() == 1 && inv.dim() == 1, "members, memrow and inv must be vectors");
  TORCH_CHECK(P * (N + 2) < (1ll << 31), "h holds ", P, " pairs, expected P (N + 2) < 2^31");
  const int64_t n = P * (N + 2), cap = rows.size(0);
  TORCH_CHECK(members.numel() == n, "members holds ", members.numel(), " lookups, h says ", P, " pairs of N + 2 = ",
              N + 2);
  TORCH_CHECK(memrow.numel() == n, "memrow holds ", memrow.numel(), " entries, members ", n);
  TORCH_CHECK(inv.numel() == n, "inv holds ", inv.numel(), " lookups, members ", n);
  TORCH_CHECK(e.dim() == 2 && e.size(0) == P && e.size(1) == N + 1, "e has shape ", e.sizes(), ", expected [", P,
              ", ", N + 1, "]");
  TORCH_CHECK(grad_rows.dim() == 2 && grad_rows.size(0) >= cap && grad_rows.size(1) == d, "grad_rows has shape ",
              grad_rows.sizes(), ", expected [>= ", cap, ", ", d, "]");
  DeviceGuard gd(gpu_of(rows, "rows"));
  const float* rp = dev_rows<float>(rows, "rows", cap, d);
  const int32_t* mp = dev<int32_t>(members, "members", n);
  const int32_t* mr = dev<int32_t>(memrow, "memrow", n);
  const int64_t* ip = dev<int64_t>(inv, "inv", n);
  const float* ep = dev<float>(e, "e", P * (N + 1));
  const float* hp = dev<float>(h, "h", P * d);
  float* gp = dev<float>(grad_rows, "grad_rows", cap * d);
  if (n == 0 || cap == 0) return;
  const int64_t pf = minips_k::sgns_backward_part_floats(n, (int)d);
  at::Tensor part;
  if (pf > 0) part = at::empty({pf}, rows.options());
  minips_k::sgns_backward(mp, mr, ip, ep, hp, rp, cap > 1 ? rows.stride(0) : rows.size(1), cap, (int)d, (int)N, P, gp,
                          pf > 0 ? part.data_ptr<float>() : nullptr, (int)blocks, stream_of(rows));
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "minips_amd skip-gram negative-sampling (word2vec) kernels (gfx950)";
  m.def("sgns_lookups", &sgns_lookups, py::arg("centres"), py::arg("contexts"), py::arg("thr"), py::arg("alias"),
        py::arg("T"), py::arg("seed"), py::arg("epoch"), py::arg("pair_base"), py::arg("N"), py::arg("negatives"),
        py::arg("keys"));
  m.def("sgns_forward", &sgns_forward, py::arg("inv"), py::arg("rows"), py::arg("N"), py::arg("gscale"), py::arg("e"),
        py::arg("loss"), py::arg("h"), py::arg("blocks"));
  m.def("sgns_backward", &sgns_backward, py::arg("members"), py::arg("memrow"), py::arg("inv"), py::arg("e"),
        py::arg("h"), py::arg("rows"), py::arg("N"), py::arg("grad_rows"), py::arg("blocks"));
  m.attr("MIN_DIM") = minips_k::kSgnsMinDim;
  m.attr("MAX_DIM") = minips_k::kSgnsMaxDim;
  m.attr("MAX_NEG") = minips_k::kSgnsMaxNeg;
  m.attr("GROUP_MAX") = minips_k::kSgnsGroupMax;
  m.attr("WAVE_MAX") = minips_k::kSgnsWaveMax;
  m.attr("CHUNK") = minips_k::kSgnsChunk;
}
