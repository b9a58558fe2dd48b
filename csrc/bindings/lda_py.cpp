// Torch-facing binding of the LDA Gibbs kernels (module minips_amd._ldak; launchers and the rule in
// csrc/kernels/lda.h). A torch extension of its own, like _gbdtk: the module and the table of its validation test
// (tests/test_ldak_validation.py) stay the complete description of each other. Every device pointer comes from
// a checked accessor of tensor_access.h, the ops launch on the current HIP stream of their first tensor's device
// under a device guard (no sync, no host read), and a bad argument raises before anything is launched.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <cmath>

#include "../kernels/lda.h"
#include "tensor_access.h"

namespace {

using namespace minips_access;  // NOLINT: the accessors are this file's vocabulary
using OptTensor = c10::optional<at::Tensor>;
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

void check_blocks(int64_t blocks) {
  TORCH_CHECK(blocks >= 0 && blocks <= minips_k::kLdaMaxBlocks, "blocks is ", blocks, ", expected 0 <= blocks <= ",
              minips_k::kLdaMaxBlocks);
}

void check_K(int64_t K, const char* from) {
  TORCH_CHECK(K >= minips_k::kLdaMinK && K <= minips_k::kLdaMaxK, from, " says K = ", K, ", expected ",
              minips_k::kLdaMinK, " <= K <= ", minips_k::kLdaMaxK);
}

void check_priors(double alpha, double beta, double Vbeta) {
  TORCH_CHECK(alpha > 0.0 && alpha <= minips_k::kLdaMaxPrior, "alpha is ", alpha, ", expected 0 < alpha <= 64");
  TORCH_CHECK(beta > 0.0 && beta <= minips_k::kLdaMaxPrior, "beta is ", beta, ", expected 0 < beta <= 64");
  TORCH_CHECK(Vbeta > 0.0 && std::isfinite(Vbeta), "Vbeta is ", Vbeta, ", expected a positive finite V * beta");
}

int64_t ld_of(const at::Tensor& t) { return t.size(0) > 1 ? t.stride(0) : t.size(1); }

// the document side shared by lda_sample and lda_loglik: rowptr int64 [B + 1], inv int64 [n], rows fp32 [cap, >= K]
// row-major (padded or odd ld allowed), nk int64 [K]
struct Docs {
  int64_t B, n, cap, K;
  const int64_t *rowptr, *inv, *nk;
  const float* rows;
};

Docs docs_of(const at::Tensor& rowptr, const at::Tensor& inv, const at::Tensor& rows, const at::Tensor& nk) {
  Docs d;
  TORCH_CHECK(rowptr.dim() == 1 && rowptr.numel() >= 1, "rowptr must be a vector of B + 1 offsets");
  TORCH_CHECK(inv.dim() == 1, "inv must be a vector");
  TORCH_CHECK(nk.dim() == 1, "nk must be a vector");
  TORCH_CHECK(rows.dim() == 2, "rows must be a [cap, >= K] matrix");
  d.B = rowptr.numel() - 1, d.n = inv.numel(), d.cap = rows.size(0), d.K = nk.numel();
  check_K(d.K, "nk");
  TORCH_CHECK(d.n < (1ll << 31) && d.B < (1ll << 31) && d.cap < (1ll << 31), "n, B and cap must be below 2^31");
  TORCH_CHECK(rows.size(1) >= d.K, "rows has ", rows.size(1), " columns, nk says K = ", d.K);
  d.rowptr = dev<int64_t>(rowptr, "rowptr", d.B + 1);
  d.inv = dev<int64_t>(inv, "inv", d.n);
  d.rows = dev_rows<float>(rows, "rows", d.cap, d.K);
  d.nk = dev<int64_t>(nk, "nk", d.K);
  return d;
}

// gid int64 [B]; z_old int16 [n] (None: the initialisation, it == 0); z_new int16 [n]; dk int64 [K] (added to).
void lda_sample(const at::Tensor& rowptr, const at::Tensor& gid, const at::Tensor& inv, const OptTensor& z_old,
                const at::Tensor& rows, const at::Tensor& nk, double alpha, double beta, double Vbeta, int64_t seed,
                int64_t it, at::Tensor& z_new, at::Tensor& dk, int64_t blocks) {
  check_blocks(blocks);
  check_priors(alpha, beta, Vbeta);
  TORCH_CHECK(it >= 0, "it is ", it, ", expected a sweep number >= 0");
  TORCH_CHECK(present(z_old) == (it != 0), "it is ", it, present(z_old) ? " (the initialisation) but z_old is given"
                                                                         : " (a sweep) but z_old is missing");
  DeviceGuard gd(gpu_of(rows, "rows"));
  const Docs d = docs_of(rowptr, inv, rows, nk);
  TORCH_CHECK(gid.dim() == 1 && gid.numel() == d.B, "gid has shape ", gid.sizes(), ", expected [", d.B, "]");
  TORCH_CHECK(z_new.dim() == 1 && z_new.numel() == d.n, "z_new has shape ", z_new.sizes(), ", expected [", d.n, "]");
  TORCH_CHECK(dk.dim() == 1 && dk.numel() == d.K, "dk has shape ", dk.sizes(), ", expected [", d.K, "]");
  if (present(z_old))
    TORCH_CHECK(z_old->dim() == 1 && z_old->numel() == d.n, "z_old has shape ", z_old->sizes(), ", expected [", d.n,
                "]");
  const int64_t* gp = dev<int64_t>(gid, "gid", d.B);
  const int16_t* zo = dev_opt<int16_t>(z_old, "z_old", d.n);
  int16_t* zn = dev<int16_t>(z_new, "z_new", d.n);
  int64_t* dp = dev<int64_t>(dk, "dk", d.K);
  minips_k::lda_sample(d.rowptr, gp, d.inv, zo, d.rows, ld_of(rows), rows.size(1), d.cap, d.nk, (int)d.K, alpha, beta,
                       Vbeta, (uint64_t)seed, (uint64_t)it, d.B, d.n, zn, dp, (int)blocks, stream_of(rows));
}

// members / memrow int32 [n] (a plan's lookup CSR); z_old int16 [n] or None (+1 only); z_new int16 [n];
// delta fp32 [cap, align4(K)] contiguous.
void lda_delta(const at::Tensor& members, const at::Tensor& memrow, const OptTensor& z_old, const at::Tensor& z_new,
               int64_t K, at::Tensor& delta, int64_t blocks) {
  check_blocks(blocks);
  check_K(K, "the argument");
  const int64_t W = (K + 3) & ~(int64_t)3;
  TORCH_CHECK(members.dim() == 1 && memrow.dim() == 1 && z_new.dim() == 1, "members, memrow and z_new must be vectors");
  const int64_t n = z_new.numel();
  TORCH_CHECK(n < (1ll << 31), "n must be below 2^31");
  TORCH_CHECK(members.numel() == n && memrow.numel() == n, "members holds ", members.numel(), " and memrow ",
              memrow.numel(), " entries, z_new ", n);
  TORCH_CHECK(delta.dim() == 2 && delta.size(1) == W, "delta has shape ", delta.sizes(),
              ", expected [cap, align4(K) = ", W, "]");
  const int64_t cap = delta.size(0);
  TORCH_CHECK(cap < (1ll << 31), "cap must be below 2^31");
  if (present(z_old))
    TORCH_CHECK(z_old->dim() == 1 && z_old->numel() == n, "z_old has shape ", z_old->sizes(), ", expected [", n, "]");
  DeviceGuard gd(gpu_of(delta, "delta"));
  const int32_t* mp = dev<int32_t>(members, "members", n);
  const int32_t* rp = dev<int32_t>(memrow, "memrow", n);
  const int16_t* zo = dev_opt<int16_t>(z_old, "z_old", n);
  const int16_t* zn = dev<int16_t>(z_new, "z_new", n);
  float* dp = dev<float>(delta, "delta", cap * W);
  const int64_t pints = minips_k::lda_delta_part_ints(n, (int)W);
  at::Tensor part;
  if (pints > 0) part = at::empty({pints}, members.options());
  minips_k::lda_delta(mp, rp, zo, zn, n, (int)K, cap, dp, pints > 0 ? part.data_ptr<int32_t>() : nullptr,
                      (int)blocks, stream_of(delta));
}

// z int16 [n]: the current topics; acc int64 [2] (added to): the fixed-point sum and the token count.
void lda_loglik(const at::Tensor& rowptr, const at::Tensor& inv, const at::Tensor& z, const at::Tensor& rows,
                const at::Tensor& nk, double alpha, double beta, double Vbeta, at::Tensor& acc, int64_t blocks) {
  check_blocks(blocks);
  check_priors(alpha, beta, Vbeta);
  DeviceGuard gd(gpu_of(rows, "rows"));
  const Docs d = docs_of(rowptr, inv, rows, nk);
  TORCH_CHECK(z.dim() == 1 && z.numel() == d.n, "z has shape ", z.sizes(), ", expected [", d.n, "]");
  TORCH_CHECK(acc.dim() == 1 && acc.numel() == 2, "acc must hold two int64");
  const int16_t* zp = dev<int16_t>(z, "z", d.n);
  int64_t* ap = dev<int64_t>(acc, "acc", 2);
  minips_k::lda_loglik(d.rowptr, d.inv, zp, d.rows, ld_of(rows), rows.size(1), d.cap, d.nk, (int)d.K, alpha, beta,
                       Vbeta, d.B, d.n, ap, (int)blocks, stream_of(rows));
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "minips_amd LDA collapsed Gibbs kernels in exact fixed point (gfx950)";
  m.def("lda_sample", &lda_sample, py::arg("rowptr"), py::arg("gid"), py::arg("inv"), py::arg("z_old"),
        py::arg("rows"), py::arg("nk"), py::arg("alpha"), py::arg("beta"), py::arg("Vbeta"), py::arg("seed"),
        py::arg("it"), py::arg("z_new"), py::arg("dk"), py::arg("blocks"));
  m.def("lda_delta", &lda_delta, py::arg("members"), py::arg("memrow"), py::arg("z_old"), py::arg("z_new"),
        py::arg("K"), py::arg("delta"), py::arg("blocks"));
  m.def("lda_loglik", &lda_loglik, py::arg("rowptr"), py::arg("inv"), py::arg("z"), py::arg("rows"), py::arg("nk"),
        py::arg("alpha"), py::arg("beta"), py::arg("Vbeta"), py::arg("acc"), py::arg("blocks"));
  m.attr("MIN_K") = minips_k::kLdaMinK;
  m.attr("MAX_K") = minips_k::kLdaMaxK;
  m.attr("MAX_DOC_LEN") = minips_k::kLdaMaxDocLen;
  m.attr("WAVE_MAX") = minips_k::kLdaWaveMax;
  m.attr("CHUNK") = minips_k::kLdaChunk;
}
