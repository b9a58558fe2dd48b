// Torch-facing binding of the histogram GBDT kernels (module minips_amd._gbdtk; launchers and the rule in
// csrc/kernels/gbdt.h). A torch extension of its own, like _ffmk: the module and the table of its validation test
// (tests/test_gbdtk_validation.py) stay the complete description of each other. Every device pointer comes from
// a checked accessor of tensor_access.h, the ops launch on the current HIP stream of their first tensor's device
// under a device guard (no sync, no host read), and a bad argument raises before anything is launched.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <cmath>

#include "../kernels/gbdt.h"
#include "tensor_access.h"

namespace {

using namespace minips_access;  // NOLINT: the accessors are this file's vocabulary
using OptTensor = c10::optional<at::Tensor>;
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

void check_F(int64_t F) {
  TORCH_CHECK(F >= 1 && F <= minips_k::kGbdtMaxF, "F is ", F, ", expected 1 <= F <= ", minips_k::kGbdtMaxF);
}

void check_blocks(int64_t blocks) {
  TORCH_CHECK(blocks >= 0 && blocks <= minips_k::kGbdtMaxBlocks, "blocks is ", blocks, ", expected 0 <= blocks <= ",
              minips_k::kGbdtMaxBlocks);
}

int64_t ld_of(const at::Tensor& t) { return t.size(0) > 1 ? t.stride(0) : t.size(1); }

// bins uint8 [N, >= F] row-major (padded ld allowed)
const uint8_t* bins_of(const at::Tensor& bins, int64_t N, int64_t F) {
  TORCH_CHECK(bins.dim() == 2, "bins must be a [N, >= F] matrix");
  TORCH_CHECK(bins.size(0) == N, "bins holds ", bins.size(0), " rows, expected ", N);
  return dev_rows<uint8_t>(bins, "bins", N, F);
}

// the shape of a level's histogram: [nodes, F, NB, 3]
void hist_shape(const at::Tensor& hist, int64_t* nodes, int64_t* F, int64_t* NB) {
  TORCH_CHECK(hist.dim() == 4 && hist.size(3) == 3, "hist must be [nodes, F, NB, 3]");
  *nodes = hist.size(0), *F = hist.size(1), *NB = hist.size(2);
  TORCH_CHECK(*nodes >= 1 && *nodes <= minips_k::kGbdtMaxNodes && !(*nodes & (*nodes - 1)), "hist has ", *nodes,
              " nodes, expected a power of two in [1, ", minips_k::kGbdtMaxNodes, "]");
  TORCH_CHECK(*F >= 1 && *F <= minips_k::kGbdtMaxF, "hist has F = ", *F, ", expected 1 <= F <= ", minips_k::kGbdtMaxF);
  TORCH_CHECK(*NB >= 2 && *NB <= minips_k::kGbdtMaxBins, "hist has NB = ", *NB, ", expected 2 <= NB <= ",
              minips_k::kGbdtMaxBins);
}

// X fp32 [N, F] row-major, cuts fp32 [F, NB - 1] contiguous; bins uint8 [N, >= F].
void gbdt_bin(const at::Tensor& X, const at::Tensor& cuts, at::Tensor& bins, int64_t blocks) {
  check_blocks(blocks);
  TORCH_CHECK(X.dim() == 2, "X must be a [N, F] matrix");
  TORCH_CHECK(cuts.dim() == 2, "cuts must be a [F, NB - 1] matrix");
  const int64_t N = X.size(0), F = cuts.size(0), NB = cuts.size(1) + 1;
  TORCH_CHECK(F >= 1 && F <= minips_k::kGbdtMaxF, "cuts has ", F, " rows, expected 1 <= F <= ", minips_k::kGbdtMaxF);
  TORCH_CHECK(NB >= 2 && NB <= minips_k::kGbdtMaxBins, "cuts has ", NB - 1,
              " columns, expected NB - 1 with 2 <= NB <= ", minips_k::kGbdtMaxBins);
  TORCH_CHECK(X.size(1) == F, "X has ", X.size(1), " columns, cuts says ", F, " features");
  DeviceGuard gd(gpu_of(X, "X"));
  const float* xp = dev_rows<float>(X, "X", N, F);
  const float* cp = dev<float>(cuts, "cuts", F * (NB - 1));
  uint8_t* bp = const_cast<uint8_t*>(bins_of(bins, N, F));
  minips_k::gbdt_bin(xp, ld_of(X), cp, N, (int)F, (int)NB, bp, ld_of(bins), (int)blocks, stream_of(X));
}

// z / labels fp32 [N]; gh int32 [N, 2]; loss_acc int64 [1] (added to).
void gbdt_grad(const at::Tensor& z, const at::Tensor& labels, at::Tensor& gh, at::Tensor& loss_acc, int64_t blocks) {
  check_blocks(blocks);
  TORCH_CHECK(z.dim() == 1 && labels.dim() == 1, "z and labels must be vectors");
  const int64_t N = z.numel();
  TORCH_CHECK(labels.numel() == N, "labels holds ", labels.numel(), " values, z ", N);
  TORCH_CHECK(gh.dim() == 2 && gh.size(0) == N && gh.size(1) == 2, "gh has shape ", gh.sizes(), ", expected [", N,
              ", 2]");
  TORCH_CHECK(loss_acc.dim() == 1 && loss_acc.numel() == 1, "loss_acc must hold one int64");
  DeviceGuard gd(gpu_of(z, "z"));
  const float* zp = dev<float>(z, "z", N);
  const float* lp = dev<float>(labels, "labels", N);
  int32_t* gp = dev<int32_t>(gh, "gh", 2 * N);
  int64_t* ap = dev<int64_t>(loss_acc, "loss_acc", 1);
  minips_k::gbdt_grad(zp, lp, N, gp, ap, (int)blocks, stream_of(z));
}

// bins uint8 [N, >= F]; node int32 [N]; gh int32 [N, 2]; hist int64 [nodes, F, NB, 3] contiguous (added to).
void gbdt_hist(const at::Tensor& bins, const at::Tensor& node, const at::Tensor& gh, at::Tensor& hist, int64_t path,
               int64_t blocks) {
  check_blocks(blocks);
  TORCH_CHECK(path >= 0 && path <= 2, "path is ", path, ", expected 0 (auto), 1 (LDS) or 2 (global)");
  int64_t nodes, F, NB;
  hist_shape(hist, &nodes, &F, &NB);
  TORCH_CHECK(path != 1 || minips_k::gbdt_hist_tile((int)nodes, (int)F, (int)NB) >= 1, "path is 1 (LDS), but one ",
              "feature of ", nodes, " nodes x ", NB, " bins does not fit the LDS accumulators");
  TORCH_CHECK(node.dim() == 1, "node must be a vector");
  const int64_t N = node.numel();
  TORCH_CHECK(gh.dim() == 2 && gh.size(0) == N && gh.size(1) == 2, "gh has shape ", gh.sizes(), ", expected [", N,
              ", 2]");
  DeviceGuard gd(gpu_of(hist, "hist"));
  const uint8_t* bp = bins_of(bins, N, F);
  const int32_t* np = dev<int32_t>(node, "node", N);
  const int32_t* gp = dev<int32_t>(gh, "gh", 2 * N);
  int64_t* hp = dev<int64_t>(hist, "hist", nodes * F * NB * 3);
  minips_k::gbdt_hist(bp, ld_of(bins), bins.size(1), np, gp, N, (int)F, (int)NB, (int)nodes, hp, (int)path,
                      (int)blocks, stream_of(hist));
}

// hist int64 [nodes, F, NB, 3]; feat / thr int32 [nodes], gain fp64 [nodes], child int64 [nodes, 2, 3].
void gbdt_split(const at::Tensor& hist, double reg_lambda, int64_t min_child_count, double min_gain, at::Tensor& feat,
                at::Tensor& thr, at::Tensor& gain, at::Tensor& child) {
  int64_t nodes, F, NB;
  hist_shape(hist, &nodes, &F, &NB);
  TORCH_CHECK(reg_lambda > 0.0 && std::isfinite(reg_lambda), "reg_lambda is ", reg_lambda, ", expected > 0");
  TORCH_CHECK(min_child_count >= 1, "min_child_count is ", min_child_count, ", expected >= 1");
  TORCH_CHECK(min_gain >= 0.0 && std::isfinite(min_gain), "min_gain is ", min_gain, ", expected >= 0");
  TORCH_CHECK(feat.dim() == 1 && feat.numel() == nodes, "feat has shape ", feat.sizes(), ", expected [", nodes, "]");
  TORCH_CHECK(thr.dim() == 1 && thr.numel() == nodes, "thr has shape ", thr.sizes(), ", expected [", nodes, "]");
  TORCH_CHECK(gain.dim() == 1 && gain.numel() == nodes, "gain has shape ", gain.sizes(), ", expected [", nodes, "]");
  TORCH_CHECK(child.dim() == 3 && child.size(0) == nodes && child.size(1) == 2 && child.size(2) == 3,
              "child has shape ", child.sizes(), ", expected [", nodes, ", 2, 3]");
  DeviceGuard gd(gpu_of(hist, "hist"));
  const int64_t* hp = dev<int64_t>(hist, "hist", nodes * F * NB * 3);
  int32_t* fp = dev<int32_t>(feat, "feat", nodes);
  int32_t* tp = dev<int32_t>(thr, "thr", nodes);
  double* gp = dev<double>(gain, "gain", nodes);
  int64_t* cp = dev<int64_t>(child, "child", nodes * 6);
  at::Tensor wgain = at::empty({nodes * F}, gain.options());
  at::Tensor wthr = at::empty({nodes * F}, feat.options());
  minips_k::gbdt_split(hp, (int)nodes, (int)F, (int)NB, reg_lambda, min_child_count, min_gain, fp, tp, gp, cp,
                       wgain.data_ptr<double>(), wthr.data_ptr<int32_t>(), stream_of(hist));
}

// child int64 [nodes, 2, 3] -> leaf fp32 [2 * nodes]
void gbdt_leaf(const at::Tensor& child, double reg_lambda, double lr, at::Tensor& leaf) {
  TORCH_CHECK(child.dim() == 3 && child.size(1) == 2 && child.size(2) == 3, "child must be [nodes, 2, 3]");
  const int64_t nodes = child.size(0);
  TORCH_CHECK(nodes >= 1 && nodes <= minips_k::kGbdtMaxNodes && !(nodes & (nodes - 1)), "child has ", nodes,
              " nodes, expected a power of two in [1, ", minips_k::kGbdtMaxNodes, "]");
  TORCH_CHECK(reg_lambda > 0.0 && std::isfinite(reg_lambda), "reg_lambda is ", reg_lambda, ", expected > 0");
  TORCH_CHECK(lr > 0.0 && std::isfinite(lr), "lr is ", lr, ", expected > 0");
  TORCH_CHECK(leaf.dim() == 1 && leaf.numel() == 2 * nodes, "leaf has shape ", leaf.sizes(), ", expected [",
              2 * nodes, "]");
  DeviceGuard gd(gpu_of(child, "child"));
  const int64_t* cp = dev<int64_t>(child, "child", nodes * 6);
  float* lp = dev<float>(leaf, "leaf", 2 * nodes);
  minips_k::gbdt_leaf(cp, (int)nodes, reg_lambda, lr, lp, stream_of(child));
}

// bins uint8 [N, >= F]; node int32 [N] (in place); feat / thr int32 [nodes]; leaf fp32 [2 nodes] and z fp32 [N]
// optional, together.
void gbdt_advance(const at::Tensor& bins, at::Tensor& node, const at::Tensor& feat, const at::Tensor& thr, int64_t F,
                  const OptTensor& leaf, const OptTensor& z, int64_t blocks) {
  check_blocks(blocks);
  check_F(F);
  TORCH_CHECK(node.dim() == 1 && feat.dim() == 1 && thr.dim() == 1, "node, feat and thr must be vectors");
  const int64_t N = node.numel(), nodes = feat.numel();
  TORCH_CHECK(nodes >= 1 && nodes <= minips_k::kGbdtMaxNodes && !(nodes & (nodes - 1)), "feat holds ", nodes,
              " nodes, expected a power of two in [1, ", minips_k::kGbdtMaxNodes, "]");
  TORCH_CHECK(thr.numel() == nodes, "thr holds ", thr.numel(), " values, feat ", nodes);
  TORCH_CHECK(present(leaf) == present(z), "leaf and z come together");
  if (present(leaf)) {
    TORCH_CHECK(leaf->dim() == 1 && leaf->numel() == 2 * nodes, "leaf has shape ", leaf->sizes(), ", expected [",
                2 * nodes, "]");
    TORCH_CHECK(z->dim() == 1 && z->numel() == N, "z has shape ", z->sizes(), ", expected [", N, "]");
  }
  DeviceGuard gd(gpu_of(node, "node"));
  const uint8_t* bp = bins_of(bins, N, F);
  int32_t* np = dev<int32_t>(node, "node", N);
  const int32_t* fp = dev<int32_t>(feat, "feat", nodes);
  const int32_t* tp = dev<int32_t>(thr, "thr", nodes);
  const float* lp = dev_opt<float>(leaf, "leaf", 2 * nodes);
  float* zp = dev_opt<float>(z, "z", N);
  minips_k::gbdt_advance(bp, ld_of(bins), np, fp, tp, N, (int)F, (int)nodes, lp, zp, (int)blocks, stream_of(node));
}

// bins uint8 [N, >= F]; feat int32 / thr uint8 [T, 2^depth - 1], leaf fp32 [T, 2^depth] contiguous; z fp32 [N];
// leaf_index int32 [N, T] optional.
void gbdt_predict(const at::Tensor& bins, const at::Tensor& feat, const at::Tensor& thr, const at::Tensor& leaf,
                  int64_t F, int64_t depth, double base, at::Tensor& z, const OptTensor& leaf_index, int64_t blocks) {
  check_blocks(blocks);
  check_F(F);
  TORCH_CHECK(depth >= 1 && depth <= minips_k::kGbdtMaxDepth, "depth is ", depth, ", expected 1 <= depth <= ",
              minips_k::kGbdtMaxDepth);
  TORCH_CHECK(std::isfinite((float)base), "base is ", base, ", expected a finite score");
  const int64_t nn = (1ll << depth) - 1, nl = 1ll << depth;
  TORCH_CHECK(feat.dim() == 2 && feat.size(1) == nn, "feat has shape ", feat.sizes(), ", expected [T, ", nn, "]");
  const int64_t T = feat.size(0);
  TORCH_CHECK(T <= minips_k::kGbdtMaxTrees, "feat holds ", T, " trees, expected at most ", minips_k::kGbdtMaxTrees);
  TORCH_CHECK(thr.dim() == 2 && thr.size(0) == T && thr.size(1) == nn, "thr has shape ", thr.sizes(), ", expected [",
              T, ", ", nn, "]");
  TORCH_CHECK(leaf.dim() == 2 && leaf.size(0) == T && leaf.size(1) == nl, "leaf has shape ", leaf.sizes(),
              ", expected [", T, ", ", nl, "]");
  TORCH_CHECK(z.dim() == 1, "z must be a vector");
  const int64_t N = z.numel();
  if (present(leaf_index))
    TORCH_CHECK(leaf_index->dim() == 2 && leaf_index->size(0) == N && leaf_index->size(1) == T,
                "leaf_index has shape ", leaf_index->sizes(), ", expected [", N, ", ", T, "]");
  DeviceGuard gd(gpu_of(z, "z"));
  const uint8_t* bp = bins_of(bins, N, F);
  const int32_t* fp = dev<int32_t>(feat, "feat", T * nn);
  const uint8_t* tp = dev<uint8_t>(thr, "thr", T * nn);
  const float* lp = dev<float>(leaf, "leaf", T * nl);
  float* zp = dev<float>(z, "z", N);
  int32_t* ip = dev_opt<int32_t>(leaf_index, "leaf_index", N * T);
  minips_k::gbdt_predict(bp, ld_of(bins), N, (int)F, fp, tp, lp, (int)T, (int)depth, (float)base, zp, ip,
                         (int)blocks, stream_of(z));
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "minips_amd histogram GBDT kernels in exact fixed point (gfx950)";
  m.def("gbdt_bin", &gbdt_bin, py::arg("X"), py::arg("cuts"), py::arg("bins"), py::arg("blocks"));
  m.def("gbdt_grad", &gbdt_grad, py::arg("z"), py::arg("labels"), py::arg("gh"), py::arg("loss_acc"),
        py::arg("blocks"));
  m.def("gbdt_hist", &gbdt_hist, py::arg("bins"), py::arg("node"), py::arg("gh"), py::arg("hist"), py::arg("path"),
        py::arg("blocks"));
  m.def("gbdt_split", &gbdt_split, py::arg("hist"), py::arg("reg_lambda"), py::arg("min_child_count"),
        py::arg("min_gain"), py::arg("feat"), py::arg("thr"), py::arg("gain"), py::arg("child"));
  m.def("gbdt_leaf", &gbdt_leaf, py::arg("child"), py::arg("reg_lambda"), py::arg("lr"), py::arg("leaf"));
  m.def("gbdt_advance", &gbdt_advance, py::arg("bins"), py::arg("node"), py::arg("feat"), py::arg("thr"), py::arg("F"),
        py::arg("leaf"), py::arg("z"), py::arg("blocks"));
  m.def("gbdt_predict", &gbdt_predict, py::arg("bins"), py::arg("feat"), py::arg("thr"), py::arg("leaf"), py::arg("F"),
        py::arg("depth"), py::arg("base"), py::arg("z"), py::arg("leaf_index"), py::arg("blocks"));
  m.attr("MAX_BINS") = minips_k::kGbdtMaxBins;
  m.attr("MAX_DEPTH") = minips_k::kGbdtMaxDepth;
  m.attr("MAX_F") = minips_k::kGbdtMaxF;
  m.attr("FLUSH_ROWS") = minips_k::kGbdtFlushRows;
  m.attr("LDS_BYTES") = minips_k::kGbdtLdsBytes;
  m.attr("SCALE_BITS") = minips_k::kGbdtScaleBits;
}
