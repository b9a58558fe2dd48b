// Torch-facing binding of the Compressed Interaction Network layers on the Wide & Deep step (module minips_amd._cink;
// launchers and the rule in csrc/kernels/cin.h). A torch extension of its own, like _dcnk and _dfmk: the module and the
// table of its validation test (tests/test_cink_validation.py) stay the complete description of each other. Every
// device pointer comes from a checked accessor of tensor_access.h, the ops launch on the current HIP stream of their
// first tensor's device under a device guard (no sync, no host read, no allocation), and a bad argument raises before
// anything is launched.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <vector>

#include "../kernels/cin.h"
#include "tensor_access.h"

namespace {

using namespace minips_access;  // NOLINT: the accessors are this file's vocabulary
using OptTensor = c10::optional<at::Tensor>;
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;
using minips_k::CinLayer;

// layers = (H_1 .. H_T), k in [1, T]: the layer's place in the stacked buffers
CinLayer layer_of(int64_t F, int64_t D, const std::vector<int64_t>& layers, int64_t k) {
  TORCH_CHECK(F >= 1 && F <= minips_k::kCinMaxM, "F is ", F, ", expected 1 <= F <= ", minips_k::kCinMaxM);
  TORCH_CHECK(D >= 8 && D <= minips_k::kCinMaxD && D % 8 == 0, "D is ", D, ", expected a multiple of 8 in [8, ",
              minips_k::kCinMaxD, "]");
  const int64_t T = (int64_t)layers.size();
  TORCH_CHECK(T >= 1 && T <= minips_k::kCinMaxT, "layers has ", T, " entries, expected 1 .. ", minips_k::kCinMaxT);
  int64_t Hs = 0;
  for (int64_t H : layers) {
    TORCH_CHECK(H >= 16 && H <= minips_k::kCinMaxH && H % 16 == 0, "layers holds ", H,
                ", expected multiples of 16 in [16, ", minips_k::kCinMaxH, "]");
    Hs += H;
  }
  TORCH_CHECK(k >= 1 && k <= T, "k is ", k, ", expected 1 <= k <= ", T);
  CinLayer L{};
  L.m = (int)F, L.D = (int)D, L.Hs = (int)Hs, L.first = k == 1, L.last = k == T;
  L.H = (int)layers[k - 1];
  L.Hp = k == 1 ? (int)F : (int)layers[k - 2];
  for (int64_t i = 0; i + 1 < k; ++i) L.off += (int)layers[i];
  L.off_prev = k == 1 ? 0 : L.off - L.Hp;
  return L;
}

void check_blocks(int64_t blocks) {
  TORCH_CHECK(blocks >= 0 && blocks <= minips_k::kCinMaxBlocks, "blocks is ", blocks, ", expected 0 <= blocks <= ",
              minips_k::kCinMaxBlocks);
}

// X must be a [B, >= F D] row-major matrix; returns its leading dimension
int64_t check_x(const at::Tensor& X, const CinLayer& L) {
  TORCH_CHECK(X.dim() == 2, "X must be a [B, >= F * D] matrix");
  const int64_t B = X.size(0), ldx = B > 1 ? X.stride(0) : X.size(1), fd = (int64_t)L.m * L.D;
  TORCH_CHECK(B < (1ll << 31) / ((int64_t)L.Hs * L.D), "X holds ", B, " samples, expected B * sum(layers) * D < 2^31");
  TORCH_CHECK(fd <= X.size(1) && fd <= ldx, "X has shape ", X.sizes(), " (ld ", ldx, "), F * D = ", fd,
              " columns are read");
  return ldx;
}

void check_w(const at::Tensor& W, const CinLayer& L) {
  const int64_t mp = minips_k::cin_mp(L.m);
  TORCH_CHECK(W.dim() == 3 && W.size(0) == L.H && W.size(1) == L.Hp && W.size(2) == mp, "W has shape ", W.sizes(),
              ", expected [", L.H, ", ", L.Hp, ", ", mp, "]");
}

void check_stack(const at::Tensor& t, const char* name, int64_t B, const CinLayer& L) {
  TORCH_CHECK(t.dim() == 3 && t.size(0) == B && t.size(1) == L.Hs && t.size(2) == L.D, name, " has shape ", t.sizes(),
              ", expected [", B, ", ", L.Hs, ", ", L.D, "]");
  aligned16(t, name);
}

void check_vec(const at::Tensor& t, const char* name, int64_t n) {
  TORCH_CHECK(t.dim() == 1 && t.numel() == n, name, " has shape ", t.sizes(), ", expected [", n, "]");
}

// X bf16 [B, >= F D], W bf16 [H_k, H_{k-1}, align8(F)], XK bf16 [B, sum(layers), D] (layer k - 1 read, layer k written)
void wd_cin_layer_forward(const at::Tensor& X, int64_t F, int64_t D, const at::Tensor& W,
                          const std::vector<int64_t>& layers, int64_t k, at::Tensor& XK, int64_t blocks) {
  const CinLayer L = layer_of(F, D, layers, k);
  check_blocks(blocks);
  const int64_t ldx = check_x(X, L), B = X.size(0);
  check_w(W, L);
  check_stack(XK, "XK", B, L);
  DeviceGuard gd(gpu_of(X, "X"));
  const bf16_t* xp = dev_rows<bf16_t>(X, "X", B, F * D);
  const bf16_t* wp = dev<bf16_t>(W, "W", W.numel());
  bf16_t* kp = dev<bf16_t>(XK, "XK", XK.numel());
  TORCH_CHECK(W.device() == X.device() && XK.device() == X.device(), "W and XK must be on X's device");
  minips_k::wd_cin_layer_forward(xp, ldx, B, L, wp, kp, (int)blocks, stream_of(X));
}

// XK bf16 [B, Hs, D], w_out bf16 [Hs], wide fp32 [B] (updated), p fp32 [B, Hs] (written)
void wd_cin_output(const at::Tensor& XK, const at::Tensor& w_out, at::Tensor& wide, at::Tensor& p, int64_t blocks) {
  check_blocks(blocks);
  TORCH_CHECK(XK.dim() == 3, "XK must be a [B, sum(layers), D] tensor");
  const int64_t B = XK.size(0), Hs = XK.size(1), D = XK.size(2);
  TORCH_CHECK(Hs >= 16 && Hs <= minips_k::kCinMaxT * minips_k::kCinMaxH && D >= 8 && D <= minips_k::kCinMaxD &&
                  D % 8 == 0 && B < (1ll << 31) / std::max<int64_t>(1, Hs * D),
              "XK has shape ", XK.sizes(), ", outside the rule");
  aligned16(XK, "XK");
  check_vec(w_out, "w_out", Hs);
  check_vec(wide, "wide", B);
  TORCH_CHECK(p.dim() == 2 && p.size(0) == B && p.size(1) == Hs, "p has shape ", p.sizes(), ", expected [", B, ", ",
              Hs, "]");
  DeviceGuard gd(gpu_of(XK, "XK"));
  const bf16_t* kp = dev<bf16_t>(XK, "XK", XK.numel());
  const bf16_t* op = dev<bf16_t>(w_out, "w_out", Hs);
  float* wp = dev<float>(wide, "wide", B);
  float* pp = dev<float>(p, "p", B * Hs);
  TORCH_CHECK(w_out.device() == XK.device() && wide.device() == XK.device() && p.device() == XK.device(),
              "w_out, wide and p must be on XK's device");
  minips_k::wd_cin_output(kp, B, (int)Hs, (int)D, op, wp, pp, (int)blocks, stream_of(XK));
}

// X, W, XK as the forward; dXK bf16 like XK (layer k read unless k = T, layer k - 1 written unless k = 1); w_out bf16
// [Hs]; dwide fp32 [B]; g0 fp32 [B, F, D] (the layers' running embedding gradient); perm optional int32 [B F]; dX bf16
// with B F D elements (updated by k = 1)
void wd_cin_layer_backward(const at::Tensor& X, int64_t F, int64_t D, const at::Tensor& W,
                           const std::vector<int64_t>& layers, int64_t k, const at::Tensor& XK, at::Tensor& dXK,
                           const at::Tensor& w_out, const at::Tensor& dwide, at::Tensor& g0, const OptTensor& perm,
                           at::Tensor& dX, int64_t blocks) {
  const CinLayer L = layer_of(F, D, layers, k);
  check_blocks(blocks);
  const int64_t ldx = check_x(X, L), B = X.size(0);
  TORCH_CHECK(B * F < (1ll << 31), "X holds ", B, " samples of F = ", F, " fields, expected B * F < 2^31");
  check_w(W, L);
  check_stack(XK, "XK", B, L);
  check_stack(dXK, "dXK", B, L);
  check_vec(w_out, "w_out", L.Hs);
  check_vec(dwide, "dwide", B);
  TORCH_CHECK(g0.dim() == 3 && g0.size(0) == B && g0.size(1) == F && g0.size(2) == D, "g0 has shape ", g0.sizes(),
              ", expected [", B, ", ", F, ", ", D, "]");
  TORCH_CHECK(dX.dim() == 2 && dX.numel() == B * F * D && (dX.size(1) == D || dX.size(1) == F * D), "dX has shape ",
              dX.sizes(), ", expected [", B, ", ", F * D, "] or [", B * F, ", ", D, "]");
  if (present(perm))
    TORCH_CHECK(perm->dim() == 1 && perm->numel() == B * F, "perm has shape ", perm->sizes(), ", expected [", B * F,
                "]");
  DeviceGuard gd(gpu_of(X, "X"));
  const bf16_t* xp = dev_rows<bf16_t>(X, "X", B, F * D);
  const bf16_t* wp = dev<bf16_t>(W, "W", W.numel());
  const bf16_t* kp = dev<bf16_t>(XK, "XK", XK.numel());
  bf16_t* dkp = dev<bf16_t>(dXK, "dXK", dXK.numel());
  const bf16_t* op = dev<bf16_t>(w_out, "w_out", L.Hs);
  const float* dp = dev<float>(dwide, "dwide", B);
  float* gp = dev<float>(g0, "g0", B * F * D);
  const int32_t* mp = dev_opt<int32_t>(perm, "perm", B * F);
  bf16_t* xg = dev<bf16_t>(dX, "dX", B * F * D);
  for (const at::Tensor* t : {&W, &XK, (const at::Tensor*)&dXK, &w_out, &dwide, (const at::Tensor*)&g0,
                              (const at::Tensor*)&dX})
    TORCH_CHECK(t->device() == X.device(), "W, XK, dXK, w_out, dwide, g0 and dX must be on X's device");
  TORCH_CHECK(!present(perm) || perm->device() == X.device(), "perm must be on X's device");
  minips_k::wd_cin_layer_backward(xp, ldx, B, L, wp, kp, dkp, op, dp, gp, mp, xg, (int)blocks, stream_of(X));
}

// part fp32 [nchunks(B), H_k, H_{k-1} align8(F)] (written): the per-chunk partial weight gradients of layer k
void wd_cin_layer_wgrad(const at::Tensor& X, int64_t F, int64_t D, const std::vector<int64_t>& layers, int64_t k,
                        const at::Tensor& XK, const at::Tensor& dXK, const at::Tensor& w_out,
                        const at::Tensor& dwide, at::Tensor& part) {
  const CinLayer L = layer_of(F, D, layers, k);
  const int64_t ldx = check_x(X, L), B = X.size(0);
  check_stack(XK, "XK", B, L);
  check_stack(dXK, "dXK", B, L);
  check_vec(w_out, "w_out", L.Hs);
  check_vec(dwide, "dwide", B);
  const int64_t nch = minips_k::cin_nchunks(B), K = (int64_t)L.Hp * minips_k::cin_mp(L.m);
  TORCH_CHECK(part.dim() == 3 && part.size(0) == nch && part.size(1) == L.H && part.size(2) == K, "part has shape ",
              part.sizes(), ", expected [", nch, ", ", L.H, ", ", K, "]");
  DeviceGuard gd(gpu_of(X, "X"));
  const bf16_t* xp = dev_rows<bf16_t>(X, "X", B, F * D);
  const bf16_t* kp = dev<bf16_t>(XK, "XK", XK.numel());
  const bf16_t* dkp = dev<bf16_t>(dXK, "dXK", dXK.numel());
  const bf16_t* op = dev<bf16_t>(w_out, "w_out", L.Hs);
  const float* dp = dev<float>(dwide, "dwide", B);
  float* pp = dev<float>(part, "part", nch * L.H * K);
  for (const at::Tensor* t : {&XK, &dXK, &w_out, &dwide, (const at::Tensor*)&part})
    TORCH_CHECK(t->device() == X.device(), "XK, dXK, w_out, dwide and part must be on X's device");
  minips_k::wd_cin_layer_wgrad(xp, ldx, B, L, kp, dkp, op, dp, pp, stream_of(X));
}

// dwide fp32 [B], p fp32 [B, Hs], part fp32 [nchunks(B), Hs] (written)
void wd_cin_wout_partial(const at::Tensor& dwide, const at::Tensor& p, at::Tensor& part) {
  TORCH_CHECK(p.dim() == 2 && p.size(1) >= 16 && p.size(1) <= minips_k::kCinMaxT * minips_k::kCinMaxH &&
                  p.size(0) < (1ll << 31) / 512,
              "p has shape ", p.sizes(), ", expected [B, sum(layers)]");
  const int64_t B = p.size(0), Hs = p.size(1), nch = minips_k::cin_nchunks(B);
  check_vec(dwide, "dwide", B);
  TORCH_CHECK(part.dim() == 2 && part.size(0) == nch && part.size(1) == Hs, "part has shape ", part.sizes(),
              ", expected [", nch, ", ", Hs, "]");
  DeviceGuard gd(gpu_of(p, "p"));
  const float* dp = dev<float>(dwide, "dwide", B);
  const float* pp = dev<float>(p, "p", B * Hs);
  float* tp = dev<float>(part, "part", nch * Hs);
  TORCH_CHECK(dwide.device() == p.device() && part.device() == p.device(), "dwide and part must be on p's device");
  minips_k::wd_cin_wout_partial(dp, pp, B, (int)Hs, tp, stream_of(p));
}

// part fp32 [nchunks, ...] with nchunks <= MAX_CHUNKS, G fp32 with as many elements as one chunk of part (added to)
void wd_cin_fold(const at::Tensor& part, at::Tensor& G) {
  TORCH_CHECK(part.dim() >= 2 && part.size(0) <= minips_k::kCinMaxChunks, "part has shape ", part.sizes(),
              ", expected [nchunks <= ", minips_k::kCinMaxChunks, ", ...]");
  const int64_t nch = part.size(0), n = nch ? part.numel() / nch : G.numel();
  TORCH_CHECK(G.numel() == n && n < (1ll << 31), "G holds ", G.numel(), " elements, a chunk of part ", n);
  DeviceGuard gd(gpu_of(part, "part"));
  const float* tp = dev<float>(part, "part", nch * n);
  float* gp = dev<float>(G, "G", n);
  TORCH_CHECK(G.device() == part.device(), "G must be on part's device");
  minips_k::wd_cin_fold(tp, nch, n, gp, stream_of(part));
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "minips_amd Compressed Interaction Network (xDeepFM) kernels on the Wide & Deep input (gfx950)";
  m.def("wd_cin_layer_forward", &wd_cin_layer_forward, py::arg("X"), py::arg("F"), py::arg("D"), py::arg("W"),
        py::arg("layers"), py::arg("k"), py::arg("XK"), py::arg("blocks"));
  m.def("wd_cin_output", &wd_cin_output, py::arg("XK"), py::arg("w_out"), py::arg("wide"), py::arg("p"),
        py::arg("blocks"));
  m.def("wd_cin_layer_backward", &wd_cin_layer_backward, py::arg("X"), py::arg("F"), py::arg("D"), py::arg("W"),
        py::arg("layers"), py::arg("k"), py::arg("XK"), py::arg("dXK"), py::arg("w_out"), py::arg("dwide"),
        py::arg("g0"), py::arg("perm"), py::arg("dX"), py::arg("blocks"));
  m.def("wd_cin_layer_wgrad", &wd_cin_layer_wgrad, py::arg("X"), py::arg("F"), py::arg("D"), py::arg("layers"),
        py::arg("k"), py::arg("XK"), py::arg("dXK"), py::arg("w_out"), py::arg("dwide"), py::arg("part"));
  m.def("wd_cin_wout_partial", &wd_cin_wout_partial, py::arg("dwide"), py::arg("p"), py::arg("part"));
  m.def("wd_cin_fold", &wd_cin_fold, py::arg("part"), py::arg("G"));
  m.attr("MAX_T") = minips_k::kCinMaxT;
  m.attr("MAX_H") = minips_k::kCinMaxH;
  m.attr("MAX_F") = minips_k::kCinMaxM;
  m.attr("MAX_D") = minips_k::kCinMaxD;
  m.attr("CHUNK") = minips_k::kCinChunk;
  m.attr("MAX_CHUNKS") = minips_k::kCinMaxChunks;
}
