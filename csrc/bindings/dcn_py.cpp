// Torch-facing binding of the Deep & Cross layers on the Wide & Deep step (module minips_amd._dcnk; launchers and
// the rule in csrc/kernels/dcn.h). A torch extension of its own, like _evalk, _optk, _ftrlk, _wdftrlk, _fmk and
// _dfmk: the module and the table of its validation test (tests/test_dcnk_validation.py) stay the complete
// description of each other. Every device pointer comes from a checked accessor of tensor_access.h, the ops launch
// on the current HIP stream of X's (part's) device under a device guard (no sync, no host read, no allocation), and
// a bad argument raises before anything is launched.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include "../kernels/dcn.h"
#include "tensor_access.h"

namespace {

using namespace minips_access;  // NOLINT: the accessors are this file's vocabulary
using OptTensor = c10::optional<at::Tensor>;
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

void check_dl(int64_t d, int64_t L) {
  TORCH_CHECK(d >= 1 && d <= minips_k::kDcnMaxD, "d is ", d, ", expected 1 <= d <= ", minips_k::kDcnMaxD);
  TORCH_CHECK(L >= 1 && L <= minips_k::kDcnMaxL, "L is ", L, ", expected 1 <= L <= ", minips_k::kDcnMaxL);
}

// X must be a [B, >= d] row-major matrix; returns its leading dimension
int64_t check_x(const at::Tensor& X, int64_t d, int64_t L, int64_t blocks) {
  check_dl(d, L);
  TORCH_CHECK(blocks >= 0 && blocks <= minips_k::kDcnMaxBlocks, "blocks is ", blocks, ", expected 0 <= blocks <= ",
              minips_k::kDcnMaxBlocks);
  TORCH_CHECK(X.dim() == 2, "X must be a [B, >= d] matrix");
  const int64_t B = X.size(0), ldx = B > 1 ? X.stride(0) : X.size(1);
  TORCH_CHECK(B < (1ll << 31), "X holds ", B, " samples, expected B < 2^31");
  TORCH_CHECK(d <= X.size(1) && d <= ldx, "X has shape ", X.sizes(), " (ld ", ldx, "), d = ", d, " columns are read");
  return ldx;
}

void check_pc(const at::Tensor& Pc, int64_t d, int64_t L) {
  const int64_t dp = minips_k::dcn_dp((int)d);
  TORCH_CHECK(Pc.dim() == 2 && Pc.size(0) == 2 * L + 1 && Pc.size(1) == dp, "Pc has shape ", Pc.sizes(),
              ", expected [", 2 * L + 1, ", ", dp, "]");
}

void check_pk(const at::Tensor& p, const at::Tensor& k, int64_t B, int64_t L) {
  TORCH_CHECK(p.dim() == 2 && p.size(0) == B && p.size(1) == L + 1, "p has shape ", p.sizes(), ", expected [", B, ", ",
              L + 1, "]");
  TORCH_CHECK(k.dim() == 1 && k.numel() == L + 1, "k has shape ", k.sizes(), ", expected [", L + 1, "]");
}

// X bf16 [B, >= d] (row-major, padded ld allowed), Pc bf16 [(2L+1), align8(d)], wide fp32 [B] (updated), p fp32
// [B, L+1] and k fp32 [L+1] (written)
void wd_cross_forward(const at::Tensor& X, int64_t d, const at::Tensor& Pc, int64_t L, at::Tensor& wide, at::Tensor& p,
                      at::Tensor& k, int64_t blocks) {
  const int64_t ldx = check_x(X, d, L, blocks), B = X.size(0);
  check_pc(Pc, d, L);
  TORCH_CHECK(wide.dim() == 1 && wide.numel() == B, "wide has shape ", wide.sizes(), ", expected [", B, "]");
  check_pk(p, k, B, L);
  DeviceGuard gd(gpu_of(X, "X"));
  const bf16_t* xp = dev_rows<bf16_t>(X, "X", B, d);
  const bf16_t* cp = dev<bf16_t>(Pc, "Pc", Pc.numel());
  float* wp = dev<float>(wide, "wide", B);
  float* pp = dev<float>(p, "p", B * (L + 1));
  float* kp = dev<float>(k, "k", L + 1);
  TORCH_CHECK(Pc.device() == X.device() && wide.device() == X.device() && p.device() == X.device() &&
                  k.device() == X.device(),
              "Pc, wide, p and k must be on X's device");
  minips_k::wd_cross_forward(xp, ldx, B, (int)d, cp, (int)L, wp, pp, kp, (int)blocks, stream_of(X));
}

// X, Pc, p, k as above, dwide fp32 [B], perm optional int32 [B * F], dX bf16 with B * F * D elements, contiguous
// ([B, F * D] in lookup order or [B * F, D] in the permuted order; updated in place), part fp32
// [ceil(B / CHUNK), (L+1) * align8(d) + TRAILER] (written)
void wd_cross_backward(const at::Tensor& X, int64_t d, const at::Tensor& p, const at::Tensor& k,
                       const at::Tensor& dwide, const at::Tensor& Pc, int64_t L, const OptTensor& perm, at::Tensor& dX,
                       int64_t F, int64_t D, at::Tensor& part, int64_t blocks) {
  const int64_t ldx = check_x(X, d, L, blocks), B = X.size(0);
  TORCH_CHECK(D >= 1 && D <= minips_k::kDcnMaxEmb, "D is ", D, ", expected 1 <= D <= ", minips_k::kDcnMaxEmb);
  TORCH_CHECK(F >= 1 && F * D <= d, "F is ", F, ", expected F >= 1 and F * D <= d = ", d);
  TORCH_CHECK(B * F < (1ll << 31), "X holds ", B, " samples of F = ", F, " fields, expected B * F < 2^31");
  check_pc(Pc, d, L);
  check_pk(p, k, B, L);
  TORCH_CHECK(dwide.dim() == 1 && dwide.numel() == B, "dwide has shape ", dwide.sizes(), ", expected [", B, "]");
  TORCH_CHECK(dX.dim() == 2 && dX.numel() == B * F * D && (dX.size(1) == D || dX.size(1) == F * D),
              "dX has shape ", dX.sizes(), ", expected [", B, ", ", F * D, "] or [", B * F, ", ", D, "]");
  if (present(perm))
    TORCH_CHECK(perm->dim() == 1 && perm->numel() == B * F, "perm has shape ", perm->sizes(), ", expected [", B * F,
                "]");
  const int64_t nchunks = minips_k::dcn_nchunks(B), pcols = minips_k::dcn_part_cols((int)d, (int)L);
  TORCH_CHECK(part.dim() == 2 && part.size(0) == nchunks && part.size(1) == pcols, "part has shape ", part.sizes(),
              ", expected [", nchunks, ", ", pcols, "]");
  DeviceGuard gd(gpu_of(X, "X"));
  const bf16_t* xp = dev_rows<bf16_t>(X, "X", B, d);
  const float* pp = dev<float>(p, "p", B * (L + 1));
  const float* kp = dev<float>(k, "k", L + 1);
  const float* dp = dev<float>(dwide, "dwide", B);
  const bf16_t* cp = dev<bf16_t>(Pc, "Pc", Pc.numel());
  const int32_t* mp = dev_opt<int32_t>(perm, "perm", B * F);
  bf16_t* gp = dev<bf16_t>(dX, "dX", B * F * D);
  float* tp = dev<float>(part, "part", nchunks * pcols);
  TORCH_CHECK(p.device() == X.device() && k.device() == X.device() && dwide.device() == X.device() &&
                  Pc.device() == X.device() && dX.device() == X.device() && part.device() == X.device() &&
                  (!present(perm) || perm->device() == X.device()),
              "p, k, dwide, Pc, perm, dX and part must be on X's device");
  minips_k::wd_cross_backward(xp, ldx, B, (int)d, pp, kp, dp, cp, (int)L, mp, gp, (int)F, (int)D, tp, (int)blocks,
                              stream_of(X));
}

// part as the backward wrote it ([nchunks, (L+1) * align8(d) + TRAILER]), Gc fp32 [(2L+1), align8(d)] (added to)
void wd_cross_fold(const at::Tensor& part, int64_t nchunks, const at::Tensor& Pc, int64_t d, int64_t L,
                   at::Tensor& Gc) {
  check_dl(d, L);
  const int64_t dp = minips_k::dcn_dp((int)d), pcols = minips_k::dcn_part_cols((int)d, (int)L);
  TORCH_CHECK(nchunks >= 0 && nchunks < (1ll << 31) / minips_k::kDcnChunk, "nchunks is ", nchunks,
              ", expected 0 <= nchunks < 2^31 / ", minips_k::kDcnChunk);
  TORCH_CHECK(part.dim() == 2 && part.size(0) == nchunks && part.size(1) == pcols, "part has shape ", part.sizes(),
              ", expected [nchunks = ", nchunks, ", (L + 1) * align8(d) + ", minips_k::kDcnTrailer, " = ", pcols, "]");
  check_pc(Pc, d, L);
  TORCH_CHECK(Gc.dim() == 2 && Gc.size(0) == 2 * L + 1 && Gc.size(1) == dp, "Gc has shape ", Gc.sizes(),
              ", expected [", 2 * L + 1, ", ", dp, "]");
  DeviceGuard gd(gpu_of(part, "part"));
  const float* tp = dev<float>(part, "part", nchunks * pcols);
  const bf16_t* cp = dev<bf16_t>(Pc, "Pc", Pc.numel());
  float* gp = dev<float>(Gc, "Gc", Gc.numel());
  TORCH_CHECK(Pc.device() == part.device() && Gc.device() == part.device(), "Pc and Gc must be on part's device");
  minips_k::wd_cross_fold(tp, nchunks, cp, (int)d, (int)L, gp, stream_of(part));
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "minips_amd Deep & Cross layer kernels on the Wide & Deep input (gfx950)";
  m.def("wd_cross_forward", &wd_cross_forward, py::arg("X"), py::arg("d"), py::arg("Pc"), py::arg("L"),
        py::arg("wide"), py::arg("p"), py::arg("k"), py::arg("blocks"));
  m.def("wd_cross_backward", &wd_cross_backward, py::arg("X"), py::arg("d"), py::arg("p"), py::arg("k"),
        py::arg("dwide"), py::arg("Pc"), py::arg("L"), py::arg("perm"), py::arg("dX"), py::arg("F"), py::arg("D"),
        py::arg("part"), py::arg("blocks"));
  m.def("wd_cross_fold", &wd_cross_fold, py::arg("part"), py::arg("nchunks"), py::arg("Pc"), py::arg("d"),
        py::arg("L"), py::arg("Gc"));
  m.attr("MAX_D") = minips_k::kDcnMaxD;
  m.attr("MAX_L") = minips_k::kDcnMaxL;
  m.attr("CHUNK") = minips_k::kDcnChunk;
  m.attr("TRAILER") = minips_k::kDcnTrailer;
}
