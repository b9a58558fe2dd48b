// Torch-facing binding of AutoInt's interacting layers on the Wide & Deep step (module minips_amd._aink; launchers and
// the rule in csrc/kernels/attnint.h). A torch extension of its own, like _cink: the module and the table of its
// validation test (tests/test_aink_validation.py) stay the complete description of each other. Every device pointer
// comes from a checked accessor of tensor_access.h, the ops launch on the current HIP stream of their first tensor's
// device under a device guard (no sync, no host read, no allocation), and a bad argument raises before anything is
// launched.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include "../kernels/attnint.h"
#include "tensor_access.h"

namespace {

using namespace minips_access;  // NOLINT: the accessors are this file's vocabulary
using OptTensor = c10::optional<at::Tensor>;
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;
using minips_k::AttnLayer;

// T layers of H heads of size d over F fields of D columns; l in [1, T]
AttnLayer layer_of(int64_t F, int64_t D, int64_t T, int64_t H, int64_t d, int64_t l) {
  TORCH_CHECK(F >= 1 && F <= minips_k::kAttnMaxM, "F is ", F, ", expected 1 <= F <= ", minips_k::kAttnMaxM);
  TORCH_CHECK(D >= 8 && D <= minips_k::kAttnMaxD && D % 8 == 0, "D is ", D, ", expected a multiple of 8 in [8, ",
              minips_k::kAttnMaxD, "]");
  TORCH_CHECK(T >= 1 && T <= minips_k::kAttnMaxT, "T is ", T, ", expected 1 <= T <= ", minips_k::kAttnMaxT);
  TORCH_CHECK(d == 16 || d == 32, "d is ", d, ", expected 16 or 32");
  TORCH_CHECK(H >= 1 && H * d <= minips_k::kAttnMaxA, "H is ", H, ", expected 1 <= H and H * d <= ",
              minips_k::kAttnMaxA);
  TORCH_CHECK(l >= 1 && l <= T, "l is ", l, ", expected 1 <= l <= ", T);
  return AttnLayer{(int)F, (int)D, (int)T, (int)H, (int)d, (int)l};
}

// the last layer as EK bf16 [B, T, F, H d] itself describes it (the ops that read only EK; D takes no part)
AttnLayer last_layer_of(const at::Tensor& EK, int64_t d) {
  TORCH_CHECK(d == 16 || d == 32, "d is ", d, ", expected 16 or 32");
  TORCH_CHECK(EK.dim() == 4 && EK.size(1) >= 1 && EK.size(1) <= minips_k::kAttnMaxT && EK.size(2) >= 1 &&
                  EK.size(2) <= minips_k::kAttnMaxM && EK.size(3) >= d && EK.size(3) <= minips_k::kAttnMaxA &&
                  EK.size(3) % d == 0,
              "EK has shape ", EK.sizes(), ", expected [B, 1 .. ", minips_k::kAttnMaxT, ", 1 .. ", minips_k::kAttnMaxM,
              ", a multiple of d = ", d, " up to ", minips_k::kAttnMaxA, "]");
  return AttnLayer{(int)EK.size(2), 8, (int)EK.size(1), (int)(EK.size(3) / d), (int)d, (int)EK.size(1)};
}

void check_blocks(int64_t blocks) {
  TORCH_CHECK(blocks >= 0 && blocks <= minips_k::kAttnMaxBlocks, "blocks is ", blocks, ", expected 0 <= blocks <= ",
              minips_k::kAttnMaxBlocks);
}

// X must be a [B, >= F D] row-major matrix; returns its leading dimension
int64_t check_x(const at::Tensor& X, const AttnLayer& L) {
  TORCH_CHECK(X.dim() == 2, "X must be a [B, >= F * D] matrix");
  const int64_t B = X.size(0), ldx = B > 1 ? X.stride(0) : X.size(1), fd = (int64_t)L.m * L.D;
  TORCH_CHECK(B < (1ll << 31) / ((int64_t)L.T * L.m * L.A()), "X holds ", B, " samples, expected B * T * F * A < 2^31");
  TORCH_CHECK(fd <= X.size(1) && fd <= ldx, "X has shape ", X.sizes(), " (ld ", ldx, "), F * D = ", fd,
              " columns are read");
  return ldx;
}

void check_w(const at::Tensor& W, const AttnLayer& L) {
  TORCH_CHECK(W.dim() == 2 && W.size(0) == L.Din() && W.size(1) == 4 * L.A(), "W has shape ", W.sizes(),
              ", expected [", L.Din(), ", ", 4 * L.A(), "]");
}

void check_stack(const at::Tensor& t, const char* name, int64_t B, const AttnLayer& L) {
  TORCH_CHECK(t.dim() == 4 && t.size(0) == B && t.size(1) == L.T && t.size(2) == L.m && t.size(3) == L.A(), name,
              " has shape ", t.sizes(), ", expected [", B, ", ", L.T, ", ", L.m, ", ", L.A(), "]");
  aligned16(t, name);
}

void check_vec(const at::Tensor& t, const char* name, int64_t n) {
  TORCH_CHECK(t.dim() == 1 && t.numel() == n, name, " has shape ", t.sizes(), ", expected [", n, "]");
}

// X bf16 [B, >= F D], W bf16 [Din_l, 4 H d], EK bf16 [B, T, F, H d] (slot l - 2 read for l > 1, slot l - 1 written)
void wd_attn_layer_forward(const at::Tensor& X, int64_t F, int64_t D, const at::Tensor& W, int64_t T, int64_t H,
                           int64_t d, int64_t l, at::Tensor& EK, int64_t blocks) {
  const AttnLayer L = layer_of(F, D, T, H, d, l);
  check_blocks(blocks);
  const int64_t ldx = check_x(X, L), B = X.size(0);
  check_w(W, L);
  check_stack(EK, "EK", B, L);
  DeviceGuard gd(gpu_of(X, "X"));
  const bf16_t* xp = dev_rows<bf16_t>(X, "X", B, F * D);
  const bf16_t* wp = dev<bf16_t>(W, "W", W.numel());
  bf16_t* kp = dev<bf16_t>(EK, "EK", EK.numel());
  TORCH_CHECK(W.device() == X.device() && EK.device() == X.device(), "W and EK must be on X's device");
  minips_k::wd_attn_layer_forward(xp, ldx, B, L, wp, kp, (int)blocks, stream_of(X));
}

// EK bf16 [B, T, F, A], w_out bf16 [F A], wide fp32 [B] (updated)
void wd_attn_output(const at::Tensor& EK, int64_t d, const at::Tensor& w_out, at::Tensor& wide, int64_t blocks) {
  check_blocks(blocks);
  const AttnLayer L = last_layer_of(EK, d);
  const int64_t B = EK.size(0);
  check_stack(EK, "EK", B, L);
  TORCH_CHECK(B < (1ll << 31) / ((int64_t)L.T * L.m * L.A()), "EK holds ", B,
              " samples, expected B * T * F * A < 2^31");
  check_vec(w_out, "w_out", (int64_t)L.m * L.A());
  check_vec(wide, "wide", B);
  DeviceGuard gd(gpu_of(EK, "EK"));
  const bf16_t* kp = dev<bf16_t>(EK, "EK", EK.numel());
  const bf16_t* op = dev<bf16_t>(w_out, "w_out", w_out.numel());
  float* wp = dev<float>(wide, "wide", B);
  TORCH_CHECK(w_out.device() == EK.device() && wide.device() == EK.device(), "w_out and wide must be on EK's device");
  minips_k::wd_attn_output(kp, B, L, op, wp, (int)blocks, stream_of(EK));
}

// X, W, EK as the forward; dEK bf16 like EK (slot l - 1 read unless l = T, slot l - 2 written unless l = 1); w_out bf16
// [F A]; dwide fp32 [B]; perm optional int32 [B F]; dX bf16 with B F D elements (updated by l = 1); part fp32
// [nchunks(B), Din_l, 4 A] (written: the chunks' partial weight gradients)
void wd_attn_layer_backward(const at::Tensor& X, int64_t F, int64_t D, const at::Tensor& W, int64_t T, int64_t H,
                            int64_t d, int64_t l, const at::Tensor& EK, at::Tensor& dEK, const at::Tensor& w_out,
                            const at::Tensor& dwide, const OptTensor& perm, at::Tensor& dX, at::Tensor& part,
                            int64_t blocks) {
  const AttnLayer L = layer_of(F, D, T, H, d, l);
  check_blocks(blocks);
  const int64_t ldx = check_x(X, L), B = X.size(0);
  TORCH_CHECK(B * F < (1ll << 31), "X holds ", B, " samples of F = ", F, " fields, expected B * F < 2^31");
  check_w(W, L);
  check_stack(EK, "EK", B, L);
  check_stack(dEK, "dEK", B, L);
  check_vec(w_out, "w_out", (int64_t)L.m * L.A());
  check_vec(dwide, "dwide", B);
  TORCH_CHECK(dX.dim() == 2 && dX.numel() == B * F * D && (dX.size(1) == D || dX.size(1) == F * D), "dX has shape ",
              dX.sizes(), ", expected [", B, ", ", F * D, "] or [", B * F, ", ", D, "]");
  aligned16(dX, "dX");
  if (present(perm))
    TORCH_CHECK(perm->dim() == 1 && perm->numel() == B * F, "perm has shape ", perm->sizes(), ", expected [", B * F,
                "]");
  const int64_t nch = minips_k::attn_nchunks(B);
  TORCH_CHECK(part.dim() == 3 && part.size(0) == nch && part.size(1) == L.Din() && part.size(2) == 4 * L.A(),
              "part has shape ", part.sizes(), ", expected [", nch, ", ", L.Din(), ", ", 4 * L.A(), "]");
  aligned16(part, "part");
  DeviceGuard gd(gpu_of(X, "X"));
  const bf16_t* xp = dev_rows<bf16_t>(X, "X", B, F * D);
  const bf16_t* wp = dev<bf16_t>(W, "W", W.numel());
  const bf16_t* kp = dev<bf16_t>(EK, "EK", EK.numel());
  bf16_t* dkp = dev<bf16_t>(dEK, "dEK", dEK.numel());
  const bf16_t* op = dev<bf16_t>(w_out, "w_out", w_out.numel());
  const float* dp = dev<float>(dwide, "dwide", B);
  const int32_t* mp = dev_opt<int32_t>(perm, "perm", B * F);
  bf16_t* xg = dev<bf16_t>(dX, "dX", B * F * D);
  float* pp = dev<float>(part, "part", part.numel());
  for (const at::Tensor* t : {&W, &EK, (const at::Tensor*)&dEK, &w_out, &dwide, (const at::Tensor*)&dX,
                              (const at::Tensor*)&part})
    TORCH_CHECK(t->device() == X.device(), "W, EK, dEK, w_out, dwide, dX and part must be on X's device");
  TORCH_CHECK(!present(perm) || perm->device() == X.device(), "perm must be on X's device");
  minips_k::wd_attn_layer_backward(xp, ldx, B, L, wp, kp, dkp, op, dp, mp, xg, pp, (int)blocks, stream_of(X));
}

// EK bf16 [B, T, F, A], dwide fp32 [B], part fp32 [nchunks(B), F A] (written)
void wd_attn_wout_partial(const at::Tensor& EK, int64_t d, const at::Tensor& dwide, at::Tensor& part) {
  const AttnLayer L = last_layer_of(EK, d);
  const int64_t B = EK.size(0), nch = minips_k::attn_nchunks(B);
  check_stack(EK, "EK", B, L);
  TORCH_CHECK(B < (1ll << 31) / ((int64_t)L.T * L.m * L.A()), "EK holds ", B,
              " samples, expected B * T * F * A < 2^31");
  check_vec(dwide, "dwide", B);
  const int64_t n = (int64_t)L.m * L.A();
  TORCH_CHECK(part.dim() == 2 && part.size(0) == nch && part.size(1) == n, "part has shape ", part.sizes(),
              ", expected [", nch, ", ", n, "]");
  DeviceGuard gd(gpu_of(EK, "EK"));
  const bf16_t* kp = dev<bf16_t>(EK, "EK", EK.numel());
  const float* dp = dev<float>(dwide, "dwide", B);
  float* tp = dev<float>(part, "part", nch * n);
  TORCH_CHECK(dwide.device() == EK.device() && part.device() == EK.device(), "dwide and part must be on EK's device");
  minips_k::wd_attn_wout_partial(kp, B, L, dp, tp, stream_of(EK));
}

// part fp32 [nchunks, ...] with nchunks <= MAX_CHUNKS, G fp32 with as many elements as one chunk of part (added to)
void wd_attn_fold(const at::Tensor& part, at::Tensor& G) {
  TORCH_CHECK(part.dim() >= 2 && part.size(0) <= minips_k::kAttnMaxChunks, "part has shape ", part.sizes(),
              ", expected [nchunks <= ", minips_k::kAttnMaxChunks, ", ...]");
  const int64_t nch = part.size(0), n = nch ? part.numel() / nch : G.numel();
  TORCH_CHECK(G.numel() == n && n < (1ll << 31), "G holds ", G.numel(), " elements, a chunk of part ", n);
  DeviceGuard gd(gpu_of(part, "part"));
  const float* tp = dev<float>(part, "part", nch * n);
  float* gp = dev<float>(G, "G", n);
  TORCH_CHECK(G.device() == part.device(), "G must be on part's device");
  minips_k::wd_attn_fold(tp, nch, n, gp, stream_of(part));
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "minips_amd AutoInt multi-head field self-attention kernels on the Wide & Deep input (gfx950)";
  m.def("wd_attn_layer_forward", &wd_attn_layer_forward, py::arg("X"), py::arg("F"), py::arg("D"), py::arg("W"),
        py::arg("T"), py::arg("H"), py::arg("d"), py::arg("l"), py::arg("EK"), py::arg("blocks"));
  m.def("wd_attn_output", &wd_attn_output, py::arg("EK"), py::arg("d"), py::arg("w_out"), py::arg("wide"),
        py::arg("blocks"));
  m.def("wd_attn_layer_backward", &wd_attn_layer_backward, py::arg("X"), py::arg("F"), py::arg("D"), py::arg("W"),
        py::arg("T"), py::arg("H"), py::arg("d"), py::arg("l"), py::arg("EK"), py::arg("dEK"), py::arg("w_out"),
        py::arg("dwide"), py::arg("perm"), py::arg("dX"), py::arg("part"), py::arg("blocks"));
  m.def("wd_attn_wout_partial", &wd_attn_wout_partial, py::arg("EK"), py::arg("d"), py::arg("dwide"),
        py::arg("part"));
  m.def("wd_attn_fold", &wd_attn_fold, py::arg("part"), py::arg("G"));
  m.attr("MAX_T") = minips_k::kAttnMaxT;
  m.attr("MAX_F") = minips_k::kAttnMaxM;
  m.attr("MAX_D") = minips_k::kAttnMaxD;
  m.attr("MAX_A") = minips_k::kAttnMaxA;
  m.attr("CHUNK") = minips_k::kAttnChunk;
  m.attr("MAX_CHUNKS") = minips_k::kAttnMaxChunks;
}
