// Torch-facing bindings of the gfx950 kernels (module minips_amd._kernels).
// Every device pointer handed to a launcher comes from a checked accessor of tensor_access.h
// (dev<T> / dev_rows<T> / dev_opt<T> / dev_rows_any / dev_bytes): device, dtype (from T), layout
// and the element count the kernel addresses are verified by the call that yields the pointer, so
// a bad argument raises a Python exception instead of faulting the GPU. What depends on
// device-resident values (key and index contents, device-side counts) cannot be checked on the
// host; those places say so. Ops launch on the current HIP stream of the tensor's device
// (graph-capture safe: no sync in here), under a device guard.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <tuple>

#include "../comm/rccl_comm.h"
#include "../kernels/kernels.h"
#include "../kernels/onesided.h"
#include "tensor_access.h"

namespace {

using minips_k::bf16_t;
using namespace minips_access;  // NOLINT: the accessors are this file's vocabulary
using OptTensor = c10::optional<at::Tensor>;
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

// Several outputs carved out of ONE caching-allocator block (256-byte aligned views): a planner
// call hands back ~10 tensors, and one allocation + views costs a fraction of ten allocations on
// the step's host path. The block lives while any of its views does.
std::vector<at::Tensor> carve(const at::TensorOptions& o,
                              const std::vector<std::pair<int64_t, at::ScalarType>>& parts) {
  std::vector<int64_t> offs;
  int64_t total = 0;
  for (const auto& p : parts) {
    offs.push_back(total);
    total += (p.first * (int64_t)c10::elementSize(p.second) + 255) & ~int64_t(255);
  }
  at::Tensor buf = at::empty({std::max<int64_t>(total, 256)}, o.dtype(at::kByte));
  std::vector<at::Tensor> out;
  out.reserve(parts.size());
  for (size_t i = 0; i < parts.size(); ++i)
    out.push_back(buf.narrow(0, offs[i], parts[i].first * (int64_t)c10::elementSize(parts[i].second))
                      .view(parts[i].second));
  return out;
}

// a device-side row count (nullable int64 scalar)
const int64_t* dev_count(const OptTensor& n_dev, const char* name = "n_dev") {
  return dev_opt<int64_t>(n_dev, name, 1);
}

// a row-major fp32 table shard [rows, >= cols] (the caller reads stride(0))
float* dev_table(const at::Tensor& table, int64_t cols = 0) { return dev_rows<float>(table, "table", 0, cols); }

// the requesters' segments of the received rows: segment p = rows [off[p], off[p+1])
minips_k::OwnerSegs owner_segs(const std::vector<int64_t>& splits, int64_t* total) {
  const int P = (int)splits.size();
  TORCH_CHECK(P >= 1 && P <= minips_k::kOwnerMaxP, "splits: 1..16 requesters");
  minips_k::OwnerSegs segs{};
  int64_t off = 0;
  for (int p = 0; p < P; ++p) {
    TORCH_CHECK(splits[p] >= 0, "splits: negative segment");
    segs.off[p] = off;
    off += splits[p];
  }
  segs.off[P] = off;
  *total = off;
  return segs;
}

// C = A . B with layout flags; see gemm.hip. Returns nothing (C preallocated).
// Batched mode (batch > 1): operands are flat buffers addressed with 2-level strides; every
// batch's extent is bounds-checked against the tensor sizes before launch.
// One validated GEMM launch: every pointer, dimension and epilogue argument of gemm_bf16_batched,
// so that a LaunchList can replay it without re-validating (the checks ran when it was prepared).
struct GemmLaunch {
  const bf16_t *A, *B;
  void* C;
  int M, N, K, lda, ldb, ldc;
  bool a_km, b_kn;
  int epi;
  const bf16_t *bias, *mask;
  int ldmask;
  float* colsum;
  float alpha;
  int split_k, batch, inner;
  int64_t st[6];
  float* slab;
  const int* perm;
  int seg, colsum_ld;
  int tile = 0;
  void launch(hipStream_t s) const {
    minips_k::gemm_bf16_batched(A, B, C, M, N, K, lda, ldb, ldc, a_km, b_kn, epi, bias, mask, ldmask, colsum, alpha,
                                split_k, batch, inner, st[0], st[1], st[2], st[3], st[4], st[5], s, slab, perm, seg,
                                colsum_ld, tile);
  }
};

// a GEMM tile hint: 0 (the launcher's choice), 128 (128x128), 200 (256x128) or 256 (256x256)
int check_tile(int64_t tile) {
  TORCH_CHECK(tile == 0 || tile == 128 || tile == 200 || tile == 256, "gemm tile hint: 0, 128, 200 or 256");
  return (int)tile;
}

// the operand shapes and alignment rules of the MFMA kernels, shared by gemm and gemm_slab
void check_gemm_dims(int64_t M, int64_t N, int64_t K, bool a_km, bool b_kn) {
  TORCH_CHECK(M >= 0 && N >= 0 && K >= 0 && M <= INT32_MAX && N <= INT32_MAX && K <= INT32_MAX, "M, N, K: int32");
  TORCH_CHECK(K % 8 == 0, "K must be a multiple of 8");
  if (a_km) TORCH_CHECK(M % 8 == 0, "KM layout needs M % 8 == 0");
  if (b_kn) TORCH_CHECK(N % 8 == 0, "KN layout needs N % 8 == 0");
}

// Validates a gemm() call and returns its launch; ``slab`` receives the split-K planes it needs
// (a caching-allocator block), if any.
GemmLaunch prepare_gemm(const at::Tensor& A, const at::Tensor& B, at::Tensor& C, int64_t M, int64_t N, int64_t K,
                        bool a_km, bool b_kn, int64_t epi, const OptTensor& bias, const OptTensor& mask,
                        const OptTensor& colsum, double alpha, int64_t split_k, int64_t batch, int64_t inner,
                        int64_t lda_, int64_t ldb_, int64_t ldc_, const std::vector<int64_t>& strides,
                        const OptTensor& perm, int64_t seg, at::Tensor& slab) {
  const bf16_t *a = dev_mat<bf16_t>(A, "A"), *b = dev_mat<bf16_t>(B, "B");
  const bool f32_out = epi == minips_k::kEpiStoreF32 || epi == minips_k::kEpiAtomicF32;
  void* c = f32_out ? (void*)dev_mat<float>(C, "C") : (void*)dev_mat<bf16_t>(C, "C");
  const bool permuted = epi == minips_k::kEpiPermRowsBf16;
  const int* perm_p = dev_opt<int>(perm, "perm");
  if (permuted) {
    // C is [M * N / seg, seg] rows in the permuted order; perm lists M * N / seg distinct rows of it
    // (the VALUES of perm are device-resident: a permutation of [0, M * N / seg) by contract)
    TORCH_CHECK(perm_p && seg > 0 && seg % 8 == 0 && N % seg == 0 && batch <= 1 && split_k <= 1,
                "permuted rows: perm, seg % 8 == 0, N % seg == 0, no batch / split-K");
    TORCH_CHECK(perm->numel() >= M * (N / seg) && C.is_contiguous() && C.numel() >= M * N,
                "permuted rows: perm [M*N/seg] and a contiguous C of >= M*N values");
  }
  check_gemm_dims(M, N, K, a_km, b_kn);
  const int64_t a_rows = a_km ? K : M, a_cols = a_km ? M : K;
  const int64_t b_rows = b_kn ? K : N, b_cols = b_kn ? N : K;
  int64_t lda, ldb, ldc;
  std::vector<int64_t> st(6, 0);
  if (batch <= 1) {
    TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && C.dim() == 2, "gemm operands must be 2-D");
    TORCH_CHECK(A.size(0) >= a_rows && A.size(1) >= a_cols, "A shape ", A.sizes(), " vs M,N,K=", M, ",", N, ",", K);
    TORCH_CHECK(B.size(0) >= b_rows && B.size(1) >= b_cols, "B shape ", B.sizes(), " vs M,N,K=", M, ",", N, ",", K);
    TORCH_CHECK(permuted || (C.size(0) >= M && C.size(1) >= N), "C shape ", C.sizes(), " vs M,N=", M, ",", N);
    lda = A.stride(0);
    ldb = B.stride(0);
    ldc = C.stride(0);
    batch = 1;
    inner = 1;
  } else {
    TORCH_CHECK(strides.size() == 6, "batched gemm needs 6 strides");
    st = strides;
    lda = lda_;
    ldb = ldb_;
    ldc = ldc_;
    TORCH_CHECK(inner >= 1 && batch % inner == 0, "batch must be a multiple of inner");
    auto extent = [&](int64_t rows, int64_t cols, int64_t ld, int64_t so, int64_t si) {
      return (batch / inner - 1) * so + (inner - 1) * si + (rows - 1) * ld + cols;
    };
    TORCH_CHECK(extent(a_rows, a_cols, lda, st[0], st[1]) <= A.numel(), "batched A out of bounds");
    TORCH_CHECK(extent(b_rows, b_cols, ldb, st[2], st[3]) <= B.numel(), "batched B out of bounds");
    TORCH_CHECK(extent(M, N, ldc, st[4], st[5]) <= C.numel(), "batched C out of bounds");
    TORCH_CHECK(!mask.has_value() && !colsum.has_value(), "batched gemm has no mask/colsum");
  }
  TORCH_CHECK(lda % 8 == 0 && ldb % 8 == 0, "leading dims must be multiples of 8 (16-byte rows)");
  for (int i = 0; i < 4; ++i) TORCH_CHECK(st[i] % 8 == 0, "operand batch strides must be multiples of 8");
  const bf16_t* bias_p = dev_opt<bf16_t>(bias, "bias", N);
  const bf16_t* mask_p = nullptr;
  int ldmask = 0;
  if (present(mask)) {
    mask_p = dev_rows<bf16_t>(*mask, "mask", M, N);
    TORCH_CHECK(mask->size(0) == M, "mask shape ", mask->sizes());
    ldmask = (int)mask->stride(0);
  }
  const bool needs_mask = epi == minips_k::kEpiReluMaskBf16 || epi == minips_k::kEpiBiasGeluAuxBf16 ||
                          epi == minips_k::kEpiGeluGradBf16 || epi == minips_k::kEpiBiasGeluDAuxBf16 ||
                          epi == minips_k::kEpiMulAuxBf16;
  if (needs_mask) TORCH_CHECK(mask_p, "this epilogue needs mask/aux");
  // a 1-D view may be strided (a column of a weight-gradient matrix: the folded-bias column)
  float* colsum_p = dev_opt_strided<float>(colsum, "colsum", N);
  const int colsum_ld = colsum_p ? (int)colsum->stride(0) : 1;
  if (epi == minips_k::kEpiStoreBf16 && split_k > 1)
    TORCH_CHECK(batch <= 1 && N % 4 == 0 && ldc % 4 == 0, "split-K bf16 store: no batch, N % 4 == 0, ldc % 4 == 0");
  // split-K slices land in fp32 slab planes and one reduce kernel adds them (deterministic, no atomics)
  if (split_k > 1 && batch <= 1 &&
      (epi == minips_k::kEpiAtomicF32 || epi == minips_k::kEpiStoreBf16) && N % 4 == 0)
    slab = at::empty({split_k * M * N}, A.options().dtype(at::kFloat));  // caching allocator, stream-ordered
  float* slab_p = slab.defined() ? slab.data_ptr<float>() : nullptr;
  GemmLaunch g{a, b, c, (int)M, (int)N, (int)K, (int)lda, (int)ldb, (int)ldc,
               a_km, b_kn, (int)epi, bias_p, mask_p, ldmask, colsum_p, (float)alpha, (int)split_k, (int)batch,
               (int)inner, {st[0], st[1], st[2], st[3], st[4], st[5]}, slab_p, perm_p, (int)seg, colsum_ld};
  return g;
}

void gemm(const at::Tensor& A, const at::Tensor& B, at::Tensor& C, int64_t M, int64_t N, int64_t K, bool a_km,
          bool b_kn, int64_t epi, const OptTensor& bias, const OptTensor& mask, const OptTensor& colsum, double alpha,
          int64_t split_k, int64_t batch, int64_t inner, int64_t lda_, int64_t ldb_, int64_t ldc_,
          std::vector<int64_t> strides, const OptTensor& perm, int64_t seg, int64_t tile) {
  DeviceGuard gd(gpu_of(A, "A"));
  at::Tensor slab;
  GemmLaunch g = prepare_gemm(A, B, C, M, N, K, a_km, b_kn, epi, bias, mask, colsum, alpha, split_k, batch, inner,
                              lda_, ldb_, ldc_, strides, perm, seg, slab);
  g.tile = check_tile(tile);
  g.launch(stream_of(A));
}

// split-K GEMM into slab planes without their reduction (the Adam kernel folds them)
struct GemmSlabLaunch {
  const bf16_t *A, *B;
  float* slab;
  int M, N, K, lda, ldb;
  bool a_km, b_kn;
  int split_k;
  int launch(hipStream_t s) const {
    return minips_k::gemm_slab(A, B, slab, M, N, K, lda, ldb, a_km, b_kn, split_k, s);
  }
};

// the operand rules of prepare_gemm (2-D mode) for contiguous operands; slab: [nsplit <= split_k][M][N]
GemmSlabLaunch prepare_gemm_slab(const at::Tensor& A, const at::Tensor& B, at::Tensor& slab, int64_t M, int64_t N,
                                 int64_t K, bool a_km, bool b_kn, int64_t split_k) {
  const bf16_t *a = dev<bf16_t>(A, "A"), *b = dev<bf16_t>(B, "B");
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2, "A, B: 2-D operands");
  check_gemm_dims(M, N, K, a_km, b_kn);
  TORCH_CHECK(N % 4 == 0, "gemm_slab: N % 4 == 0");
  TORCH_CHECK(A.size(0) >= (a_km ? K : M) && A.size(1) >= (a_km ? M : K), "A shape ", A.sizes(), " vs M,N,K=", M, ",",
              N, ",", K);
  TORCH_CHECK(B.size(0) >= (b_kn ? K : N) && B.size(1) >= (b_kn ? N : K), "B shape ", B.sizes(), " vs M,N,K=", M, ",",
              N, ",", K);
  const int64_t lda = A.stride(0), ldb = B.stride(0);
  TORCH_CHECK(lda % 8 == 0 && ldb % 8 == 0, "A, B: leading dims must be multiples of 8 (16-byte rows)");
  TORCH_CHECK(split_k <= INT32_MAX, "split_k: int32");
  float* p = dev<float>(slab, "slab", std::max<int64_t>(split_k, 1) * M * N);
  return GemmSlabLaunch{a, b, p, (int)M, (int)N, (int)K, (int)lda, (int)ldb, a_km, b_kn, (int)split_k};
}

// returns nsplit
int64_t gemm_slab(const at::Tensor& A, const at::Tensor& B, at::Tensor& slab, int64_t M, int64_t N, int64_t K,
                  bool a_km, bool b_kn, int64_t split_k) {
  const GemmSlabLaunch g = prepare_gemm_slab(A, B, slab, M, N, K, a_km, b_kn, split_k);
  DeviceGuard gd(gpu_of(A, "A"));
  return g.launch(stream_of(A));
}

// Bitmap planner of a bounded key space (keys, after the optional routing k * mult mod rn, in
// [0, num_rows)): same outputs as unique_bucketize -- (sorted unique keys [n] (first U valid),
// inverse [n], counts [P], U [1]) -- with no hash table. Keys outside the space are counted in oor.
std::vector<at::Tensor> bitmap_plan(const at::Tensor& keys, const at::Tensor& bounds, int64_t num_rows,
                                    int64_t route_mult, int64_t route_n, const OptTensor& oor) {
  const int64_t* kp = dev<int64_t>(keys, "keys");
  const int64_t* bp = dev<int64_t>(bounds, "bounds", 2);
  TORCH_CHECK(bounds.dim() == 1, "bounds must be [P+1]");
  TORCH_CHECK(num_rows > 0 && num_rows <= (1LL << 36), "bitmap_plan: 0 < num_rows <= 2^36");
  TORCH_CHECK(!route_mult || route_n == num_rows, "bitmap_plan: routing must map into [0, num_rows)");
  const int64_t n = keys.numel();
  const int P = (int)bounds.numel() - 1;
  auto opts = keys.options();
  auto ws = at::empty({minips_k::bitmap_plan_workspace_words(num_rows)}, opts);
  auto uniq = at::empty({std::max<int64_t>(n, 1)}, opts), inverse = at::empty({n}, opts);
  auto counts = at::empty({P + 1}, opts), U = at::empty({1}, opts);
  DeviceGuard g(gpu_of(keys, "keys"));
  minips_k::bitmap_plan(kp, n, num_rows, bp, P, (uint64_t)route_mult, (uint64_t)route_n, ws.data_ptr<int64_t>(),
                        uniq.data_ptr<int64_t>(), inverse.data_ptr<int64_t>(), counts.data_ptr<int64_t>(),
                        U.data_ptr<int64_t>(), stream_of(keys), dev_opt<int64_t>(oor, "oor", 1));
  return {uniq, inverse, counts.narrow(0, 0, P), U};
}

// Returns (unique keys grouped by owner [n] (first U valid), inverse [n], counts [P], U [1]).
std::vector<at::Tensor> unique_bucketize(const at::Tensor& keys, const at::Tensor& bounds, int64_t F,
                                         int64_t route_mult, int64_t route_n, int64_t extra_zero_ints,
                                         bool csr_counts) {
  const int64_t* kp = dev<int64_t>(keys, "keys");
  const int64_t* bp = dev<int64_t>(bounds, "bounds", 2);
  TORCH_CHECK(bounds.dim() == 1, "bounds must be [P+1]");
  const int64_t n = keys.numel();
  const int P = (int)bounds.numel() - 1;
  TORCH_CHECK(F >= 1 && n % F == 0, "unique_bucketize: numel must be a multiple of F");
  // capacity: the smallest power of two >= 1.6 n (every key fits: U <= n < cap), so even a batch
  // of all-distinct keys (DLRM / LR ids drawn uniformly from 10^8 rows: U ~ n) probes at load
  // <= 0.63 -- at next_pow2(n) such a batch ran at load ~0.8 and its linear-probing inserts took
  // 141 us for 426K keys (profiles/r2/dlrm_1gpu_kernels_before.txt). Criteo-shaped batches (U ~ n/5)
  // use the sort planner (plan.hip) instead.
  int64_t cap = 1024;
  while (cap * 5 < n * 8) cap <<= 1;
  if (cap <= n) cap <<= 1;
  auto opts = keys.options();
  // table_keys | counts[P] | total | shard counters [2*S*P] in one allocation: one zero memset
  const int64_t extra64 = (std::max<int64_t>(extra_zero_ints, 0) + 1) / 2;  // int32 count -> int64 words
  const int64_t shw = 2 * (int64_t)minips_k::ub_shards(P) * P;
  // csr_counts: the first n ints of the extra block receive the per-unique-key lookup counts (the
  // embedding-backward CSR's row sizes), from per-slot counters (cap int32) cleared by the memset
  TORCH_CHECK(!csr_counts || extra_zero_ints >= n, "csr_counts needs extra_zero_ints >= n");
  const int64_t scw = csr_counts ? cap / 2 : 0;
  auto zbuf = at::empty({cap + P + 1 + shw + scw + extra64}, opts);
  auto table_keys = zbuf.narrow(0, 0, cap), table_pos = at::empty({cap}, opts);
  auto slot = at::empty({n}, opts), flags = at::empty({n}, opts.dtype(at::kInt));
  auto counts = zbuf.narrow(0, cap, P + 1), cursor = zbuf.narrow(0, cap + P + 1, shw);
  auto out_keys = at::empty({n}, opts), inverse = at::empty({n}, opts);
  at::Tensor extra;  // zeroed int32 workspace after the counters, when asked for
  if (extra64) extra = zbuf.narrow(0, cap + P + 1 + shw + scw, extra64).view(at::kInt);
  DeviceGuard g(gpu_of(keys, "keys"));
  minips_k::unique_bucketize(kp, n, (int)F, bp, P, table_keys.data_ptr<int64_t>(), table_pos.data_ptr<int64_t>(), cap,
                             slot.data_ptr<int64_t>(), flags.data_ptr<int32_t>(), counts.data_ptr<int64_t>(),
                             cursor.data_ptr<int64_t>(), out_keys.data_ptr<int64_t>(), inverse.data_ptr<int64_t>(),
                             stream_of(keys), (uint64_t)route_mult, (uint64_t)route_n, extra64 * 8,
                             csr_counts && extra64 ? extra.data_ptr<int>() : nullptr);
  std::vector<at::Tensor> out{out_keys, inverse, counts.narrow(0, 0, P), counts.narrow(0, P, 1)};
  if (extra64) out.push_back(extra);
  return out;
}

// Table ops below: the rows addressed are keys[i] - base, key VALUES live on the device, so that
// they fall inside the table cannot be checked here (the planner bounds them by the shard ranges).
void gather_rows(const at::Tensor& table, const at::Tensor& keys, int64_t base, at::Tensor& out,
                 const OptTensor& n_dev) {
  const int64_t* kp = dev<int64_t>(keys, "keys");
  const int64_t n = keys.numel();
  TORCH_CHECK(out.dim() == 2 && out.size(0) >= n, "out shape ", out.sizes());
  const int D = (int)out.size(1);
  TORCH_CHECK(table.dim() == 2 && D <= table.size(1), "out row wider than table row");
  DeviceGuard g(gpu_of(keys, "keys"));
  if (table.scalar_type() == at::kDouble) {  // reference-precision tables (f64.hip)
    TORCH_CHECK(D == table.size(1), "fp64 gather: whole rows");
    minips_k::gather_rows_f64(dev<double>(table, "table"), D, kp, base, n, dev_count(n_dev),
                              dev<double>(out, "out", n * D), stream_of(keys));
    return;
  }
  bool out_bf;
  void* op = dev_rows_any(out, "out", &out_bf, n, D);
  if (table.scalar_type() == at::kBFloat16) {  // bf16 rows (bf16rows.hip)
    TORCH_CHECK(D == table.size(1), "bf16 table gather: whole rows");
    minips_k::gather_rows_bf16tab(dev_rows<bf16_t>(table, "table", 0, D), table.stride(0), kp, n, base, D, op, out_bf,
                                  stream_of(keys), dev_count(n_dev));
    return;
  }
  minips_k::gather_rows(dev_table(table, D), table.stride(0), kp, n, base, D, op, out_bf, stream_of(keys),
                        dev_count(n_dev));
}

// fp32 gradient rows into bf16 table rows (stochastic rounding): opt 0 row-wise Adagrad, 1 w += scale*g
void sparse_apply_bf16(int64_t opt, at::Tensor& table, const OptTensor& state, const OptTensor& state2, int64_t D1,
                       const at::Tensor& keys, int64_t base, const at::Tensor& grads, double lr, double eps,
                       double scale, int64_t step, int64_t seed, const OptTensor& n_dev) {
  bf16_t* tp = dev_rows<bf16_t>(table, "table");
  const int64_t n = keys.numel();
  const int D = (int)table.size(1);
  TORCH_CHECK(grads.dim() == 2 && grads.size(0) >= n && grads.size(1) == D, "grads [>= n, D]");
  // one accumulator per table row for the row-wise Adagrad (opt 0)
  float* st = dev_opt<float>(state, "state", opt == 0 ? table.size(0) : 0);
  float* st2 = dev_opt<float>(state2, "state2", opt == 0 ? table.size(0) : 0);
  TORCH_CHECK(opt != 0 || st, "state: row-wise Adagrad needs its state");
  DeviceGuard g(gpu_of(keys, "keys"));
  minips_k::sparse_apply_bf16tab((int)opt, tp, table.stride(0), st, st2, (int)D1, dev<int64_t>(keys, "keys"), n, base,
                                 D, dev<float>(grads, "grads", n * D), (float)lr, (float)eps, (float)scale,
                                 (uint32_t)step, (uint32_t)seed, stream_of(keys), dev_count(n_dev));
}

// inv VALUES (rows of ``rows``) are device-resident: not checked here
void lookup_rows(const at::Tensor& rows, const at::Tensor& inv, int64_t F, int64_t D, at::Tensor& out) {
  const bf16_t* rp = dev<bf16_t>(rows, "rows");
  bf16_t* op = dev_rows<bf16_t>(out, "out", 0, F * D);
  const int64_t B = out.size(0);
  TORCH_CHECK(rows.dim() == 2 && inv.numel() == B * F && rows.size(1) >= D, "lookup_rows shapes: rows / inv");
  DeviceGuard g(gpu_of(rows, "rows"));
  minips_k::lookup_rows(rp, (int)rows.size(1), dev<int64_t>(inv, "inv", B * F), B, (int)F, (int)D, op,
                        (int)out.stride(0), stream_of(rows));
}

// idx VALUES (rows of acc) are device-resident: not checked here
void scatter_add_rows(const at::Tensor& src, const at::Tensor& idx, at::Tensor& acc) {
  TORCH_CHECK(src.dim() == 2 && acc.dim() == 2 && src.size(1) == acc.size(1), "src / acc: row widths differ");
  const int64_t n = src.size(0);
  const int D = (int)src.size(1);
  TORCH_CHECK(idx.numel() == n, "idx/src length mismatch");
  const int64_t* ip = dev<int64_t>(idx, "idx", n);
  DeviceGuard g(gpu_of(src, "src"));
  if (src.scalar_type() == at::kDouble) {
    minips_k::scatter_add_rows_f64(dev<double>(src, "src"), ip, n, D, dev<double>(acc, "acc"), stream_of(src));
    return;
  }
  float* ap = dev<float>(acc, "acc");
  if (src.scalar_type() == at::kFloat)
    minips_k::scatter_add_rows(dev<float>(src, "src"), n, D, ip, ap, stream_of(src));
  else  // (dev<bf16_t> rejects every other dtype: src must be fp32, bf16 or fp64)
    minips_k::scatter_add_rows_bf16(dev<bf16_t>(src, "src"), n, D, ip, ap, stream_of(src));
}

// slots [cap * P] int32 of the owned unique rows (see kernels.h owner_slots); own_inv VALUES
// (< cap) are device-resident: not checked here
at::Tensor owner_slots(const at::Tensor& own_inv, std::vector<int64_t> splits, int64_t cap) {
  int64_t total = 0;
  const minips_k::OwnerSegs segs = owner_segs(splits, &total);
  const int P = (int)splits.size();
  TORCH_CHECK(total == own_inv.numel(), "owner_slots: splits must sum to the received rows");
  const int64_t* ip = dev<int64_t>(own_inv, "own_inv", total);
  at::Tensor slots = at::empty({std::max<int64_t>(cap, 1) * P}, own_inv.options().dtype(at::kInt));
  DeviceGuard g(gpu_of(own_inv, "own_inv"));
  minips_k::owner_slots(ip, total, segs, P, slots.data_ptr<int>(), std::max<int64_t>(cap, 1), stream_of(own_inv));
  return slots;
}

// received gradient rows [M, D <= table width], fp32 or bf16
const void* dev_recv(const at::Tensor& recv, const at::Tensor& table, bool* bf16, int64_t rows) {
  const void* p = dev_rows_any(recv, "recv", bf16, rows, 0);
  TORCH_CHECK(recv.size(1) <= table.size(1), "recv [M, D]: rows wider than the table's");
  return p;
}

// slots VALUES (rows of recv, -1 = none) are device-resident: not checked here
void owner_rows_adagrad(at::Tensor& table, at::Tensor& state, const OptTensor& state2, int64_t D1,
                        const at::Tensor& keys, int64_t n, const OptTensor& n_dev, int64_t base,
                        const at::Tensor& recv, int64_t P, const at::Tensor& slots, double lr, double eps) {
  float* tp = dev_table(table);
  bool recv_bf;
  const void* rp = dev_recv(recv, table, &recv_bf, 0);
  TORCH_CHECK(n >= 0 && P >= 1, "owner_rows_adagrad: n >= 0, P >= 1");
  DeviceGuard g(gpu_of(table, "table"));
  minips_k::owner_rows_adagrad(tp, table.stride(0), dev<float>(state, "state"), dev_opt<float>(state2, "state2"),
                               (int)D1, dev<int64_t>(keys, "keys", n), n, dev_count(n_dev), base, (int)recv.size(1), rp,
                               recv_bf, (int)P, dev<int>(slots, "slots", n * P), (float)lr, (float)eps,
                               stream_of(table));
}

// direct-addressed owner apply of one push (kernels.h owner_push_adagrad); rs: int32 [rows_local * P * 2]
void owner_push_adagrad(at::Tensor& table, at::Tensor& state, const OptTensor& state2, int64_t D1,
                        const at::Tensor& keys, int64_t base, const at::Tensor& recv, std::vector<int64_t> splits,
                        at::Tensor& rs, int64_t stamp, double lr, double eps) {
  float* tp = dev_table(table);
  int64_t total = 0;
  const minips_k::OwnerSegs segs = owner_segs(splits, &total);
  const int P = (int)splits.size();
  TORCH_CHECK(total == keys.numel(), "owner_push_adagrad: splits must sum to the received keys");
  TORCH_CHECK(total < (int64_t)INT32_MAX, "owner_push_adagrad: < 2^31 received rows");
  bool recv_bf;
  const void* rp = dev_recv(recv, table, &recv_bf, total);
  DeviceGuard g(gpu_of(table, "table"));
  minips_k::owner_push_adagrad(tp, table.stride(0), dev<float>(state, "state"), dev_opt<float>(state2, "state2"),
                               (int)D1, dev<int64_t>(keys, "keys", total), total, base, table.size(0),
                               (int)recv.size(1), rp, recv_bf, segs, P, dev<int>(rs, "rs", table.size(0) * P * 2),
                               (int)stamp, (float)lr, (float)eps, stream_of(table));
}

void sparse_rowwise_adagrad(at::Tensor& table, at::Tensor& state, const OptTensor& state2, int64_t D1,
                            const at::Tensor& keys, int64_t base, const at::Tensor& grads, double lr, double eps,
                            const OptTensor& n_dev, bool zero_g) {
  float* tp = dev_table(table);
  const int64_t n = keys.numel();
  TORCH_CHECK(grads.dim() == 2 && grads.size(0) == n && grads.size(1) <= table.size(1), "grads shape");
  DeviceGuard g(gpu_of(table, "table"));
  minips_k::sparse_rowwise_adagrad(tp, table.stride(0), dev<float>(state, "state"), dev_opt<float>(state2, "state2"),
                                   (int)D1, dev<int64_t>(keys, "keys"), n, base, (int)grads.size(1),
                                   dev<float>(grads, "grads", n * grads.size(1)), (float)lr, (float)eps,
                                   stream_of(table), dev_count(n_dev), zero_g);
}

void sparse_sgd(at::Tensor& table, const at::Tensor& keys, int64_t base, const at::Tensor& grads, double scale,
                const OptTensor& n_dev) {
  const int64_t* kp = dev<int64_t>(keys, "keys");
  const int64_t n = keys.numel();
  TORCH_CHECK(table.dim() == 2 && grads.dim() == 2 && grads.size(0) == n && grads.size(1) <= table.size(1),
              "grads shape");
  const int D = (int)grads.size(1);
  DeviceGuard g(gpu_of(table, "table"));
  if (table.scalar_type() == at::kDouble) {
    TORCH_CHECK(D == table.size(1), "fp64 apply: whole rows");
    minips_k::sparse_add_f64(dev<double>(table, "table"), D, kp, base, dev<double>(grads, "grads", n * D), n, scale,
                             dev_count(n_dev), stream_of(table));
    return;
  }
  minips_k::sparse_sgd(dev_table(table, D), table.stride(0), kp, n, base, D, dev<float>(grads, "grads", n * D),
                       (float)scale, stream_of(table), dev_count(n_dev));
}

// offsets VALUES (ranges of idx) and idx VALUES (rows) are device-resident: not checked here
void embedding_bag_fwd(const at::Tensor& rows, const at::Tensor& idx, const at::Tensor& offsets, bool mean,
                       at::Tensor& out) {
  const float* rp = dev<float>(rows, "rows");
  const int64_t* fp = dev<int64_t>(offsets, "offsets", 1);
  const int64_t B = offsets.numel() - 1;
  TORCH_CHECK(rows.dim() == 2 && out.dim() == 2 && out.size(0) == B && out.size(1) == rows.size(1), "out shape");
  DeviceGuard g(gpu_of(rows, "rows"));
  minips_k::embedding_bag_fwd(rp, dev<int64_t>(idx, "idx"), fp, B, (int)rows.size(1), mean,
                              dev<float>(out, "out", B * rows.size(1)), stream_of(rows));
}

void embedding_bag_bwd(const at::Tensor& grad_out, const at::Tensor& idx, const at::Tensor& offsets, bool mean,
                       at::Tensor& grad_rows) {
  const float* gp = dev<float>(grad_out, "grad_out");
  float* rp = dev<float>(grad_rows, "grad_rows");
  TORCH_CHECK(grad_out.dim() == 2 && grad_rows.dim() == 2 && grad_out.size(1) == grad_rows.size(1), "width mismatch");
  const int64_t B = grad_out.size(0);
  DeviceGuard g(gpu_of(grad_out, "grad_out"));
  minips_k::embedding_bag_bwd(gp, dev<int64_t>(idx, "idx"), dev<int64_t>(offsets, "offsets", B + 1), B,
                              (int)grad_out.size(1), mean, rp, stream_of(grad_out));
}

// inv VALUES (rows of ``rows``) are device-resident: not checked here
void wd_assemble(const at::Tensor& dense, const at::Tensor& rows, const at::Tensor& inv, int64_t F, int64_t D,
                 at::Tensor& X, at::Tensor& wide_logit, int64_t ones_col, const OptTensor& zero) {
  float* z = dev_opt<float>(zero, "zero", 1);
  bf16_t* xp = dev<bf16_t>(X, "X");
  TORCH_CHECK(X.dim() == 2 && dense.dim() == 2 && rows.dim() == 2 && F >= 0 && D >= 0, "X, dense, rows: 2-D");
  const int64_t B = X.size(0);
  TORCH_CHECK(inv.numel() == B * F, "inv must be [B*F]");
  TORCH_CHECK(dense.size(0) == B, "dense rows");
  TORCH_CHECK(rows.size(1) > D, "rows must hold D deep values + the wide weight");
  DeviceGuard g(gpu_of(X, "X"));
  minips_k::wd_assemble(dev<float>(dense, "dense"), (int)dense.size(1), dev<bf16_t>(rows, "rows"), (int)rows.size(1),
                        dev<int64_t>(inv, "inv", B * F), B, (int)F, (int)D, xp, (int)X.size(1),
                        dev<float>(wide_logit, "wide_logit", B), (int)ones_col, stream_of(X), z);
}

// wd_assemble reading the fp32 table shard directly: row of lookup (b, f) = tab[uniq[inv] - base]
// (uniq / inv / rowidx VALUES are device-resident: not checked here)
void wd_assemble_tab(const at::Tensor& dense, const at::Tensor& tab, const at::Tensor& uniq, int64_t base,
                     const at::Tensor& inv, int64_t F, int64_t D, at::Tensor& X, at::Tensor& wide_logit,
                     int64_t ones_col, const OptTensor& zero, const OptTensor& rowidx) {
  float* z = dev_opt<float>(zero, "zero", 1);
  bf16_t* xp = dev<bf16_t>(X, "X");
  const float* tp = dev<float>(tab, "tab");
  TORCH_CHECK(X.dim() == 2 && dense.dim() == 2 && F >= 0 && D >= 0, "X, dense: 2-D");
  TORCH_CHECK(tab.dim() == 2 && tab.stride(1) == 1, "tab must be a row-major [rows, W] matrix");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(tp) % 16 == 0, "tab must be 16-byte aligned");
  const int64_t B = X.size(0);
  TORCH_CHECK(inv.numel() == B * F, "inv must be [B*F]");
  TORCH_CHECK(dense.size(0) == B, "dense rows");
  TORCH_CHECK(tab.size(1) > D, "tab rows must hold D deep values + the wide weight");
  const int32_t* ri = dev_opt<int32_t>(rowidx, "rowidx", B * F);
  TORCH_CHECK(!ri || rowidx->numel() == B * F, "rowidx must be [B*F]");
  DeviceGuard g(gpu_of(X, "X"));
  minips_k::wd_assemble_tab(dev<float>(dense, "dense"), (int)dense.size(1), tp, tab.stride(0),
                            dev<int64_t>(uniq, "uniq"), base, dev<int64_t>(inv, "inv", B * F), B, (int)F, (int)D, xp,
                            (int)X.size(1), dev<float>(wide_logit, "wide_logit", B), (int)ones_col, stream_of(X), z,
                            ri);
}

void wd_head(const at::Tensor& H, const at::Tensor& w, const at::Tensor& b0, const at::Tensor& wide_logit,
             const at::Tensor& labels, at::Tensor& dH, at::Tensor& dw, at::Tensor& db, at::Tensor& dwide,
             at::Tensor& loss_sum, const OptTensor& dH_colsum, double grad_scale, bool defer_fold) {
  const bf16_t* hp = dev<bf16_t>(H, "H");
  TORCH_CHECK(H.dim() == 2, "H: [B, Hd]");
  const int64_t B = H.size(0), Hd = H.size(1);
  TORCH_CHECK(dH.sizes() == H.sizes(), "dH shape");
  TORCH_CHECK(w.numel() == Hd && dw.numel() == Hd, "w/dw length");
  DeviceGuard g(gpu_of(H, "H"));
  minips_k::wd_head(hp, B, (int)Hd, dev<bf16_t>(w, "w", Hd), dev<bf16_t>(b0, "b0", 1),
                    dev<float>(wide_logit, "wide_logit", B), dev<float>(labels, "labels", B),
                    dev<bf16_t>(dH, "dH", B * Hd), dev<float>(dw, "dw", Hd), dev<float>(db, "db", 1),
                    dev<float>(dwide, "dwide", B), dev<float>(loss_sum, "loss_sum", 1),
                    dev_opt<float>(dH_colsum, "dH_colsum", Hd), (float)grad_scale, stream_of(H), defer_fold);
}

struct HeadFoldLaunch {
  int64_t B;
  int Hd;
  float *dw, *db, *loss, *colsum;
  void launch(hipStream_t s) const { minips_k::wd_head_fold(B, Hd, dw, db, loss, colsum, s); }
};

HeadFoldLaunch prepare_head_fold(int64_t B, int64_t Hd, at::Tensor& dw, at::Tensor& db, at::Tensor& loss_sum,
                                 const OptTensor& dH_colsum) {
  TORCH_CHECK(dw.numel() == Hd, "wd_head_fold: dw [Hd]");
  return HeadFoldLaunch{B, (int)Hd, dev<float>(dw, "dw", Hd), dev<float>(db, "db", 1),
                        dev<float>(loss_sum, "loss_sum", 1), dev_opt<float>(dH_colsum, "dH_colsum", Hd)};
}

// the totals of the last wd_head(defer_fold=True) of this device (same B, Hd), on dw's stream
void wd_head_fold(int64_t B, int64_t Hd, at::Tensor& dw, at::Tensor& db, at::Tensor& loss_sum,
                  const OptTensor& dH_colsum) {
  const HeadFoldLaunch f = prepare_head_fold(B, Hd, dw, db, loss_sum, dH_colsum);
  DeviceGuard g(gpu_of(dw, "dw"));
  f.launch(stream_of(dw));
}

// Lookup CSR grouped by unique row (members/memrow int32 [B*F]) for U (upper-bound) rows.
// (inv VALUES, < U, are device-resident: not checked here)
std::vector<at::Tensor> emb_build_csr(const at::Tensor& inv, int64_t F, int64_t U, const OptTensor& zeroed,
                                      bool counts_ready) {
  const int64_t* ip = dev<int64_t>(inv, "inv");
  const int64_t n = inv.numel();
  TORCH_CHECK(F >= 1 && n % F == 0 && U >= 1 && U < (1ll << 31) && n < (1ll << 31), "emb_build_csr shapes");
  auto io = inv.options().dtype(at::kInt);
  int* zc = dev_opt<int>(zeroed, "zeroed", 2 * U);  // (already zero)
  at::Tensor ws = at::empty({(zc ? 0 : 2 * U) + U + 1 + U / 1024 + 1}, io);
  at::Tensor members = at::empty({n}, io), memrow = at::empty({n}, io);
  DeviceGuard g(gpu_of(inv, "inv"));
  minips_k::emb_build_csr(ip, n / F, (int)F, (int)U, ws.data_ptr<int>(), members.data_ptr<int>(),
                          memrow.data_ptr<int>(), stream_of(inv), zc, counts_ready && zc);
  return {members, memrow};
}

// inv / members / memrow VALUES (rows of grad_rows, lookups) are device-resident: not checked here
void wd_emb_backward(const at::Tensor& dX, const OptTensor& dwide, const at::Tensor& inv, int64_t F, int64_t D,
                     at::Tensor& grad_rows, int64_t x_off, const OptTensor& members, const OptTensor& memrow,
                     bool sorted_rows) {
  TORCH_CHECK(F >= 1 && D >= 1 && x_off >= 0, "wd_emb_backward: F, D >= 1, x_off >= 0");
  bool bf0, out_bf;
  const void* xp = dev_rows_any(dX, "dX", &bf0);
  if (sorted_rows) {  // dX [B*F, D] in the CSR's member order (kEpiPermRowsBf16 dgrad output)
    TORCH_CHECK(present(members) && x_off == 0 && dX.size(1) == D && dX.size(0) == inv.numel() &&
                    inv.numel() % F == 0, "sorted rows: dX [B*F, D] + the CSR");
  }
  const int64_t B = sorted_rows ? inv.numel() / F : dX.size(0);
  TORCH_CHECK(inv.numel() == B * F && (sorted_rows || dX.size(1) >= x_off + F * D), "dX / inv shapes");
  const int64_t* ip = dev<int64_t>(inv, "inv", B * F);
  const float* dw = dev_opt<float>(dwide, "dwide", B);
  void* gp = dev_rows_any(grad_rows, "grad_rows", &out_bf, 0, D + (dw ? 1 : 0));
  // pointer arithmetic on the checked dX: the embedding columns start at x_off (<= the row width, above)
  const void* base0 = bf0 ? (const void*)((const bf16_t*)xp + x_off) : (const void*)((const float*)xp + x_off);
  DeviceGuard g(gpu_of(dX, "dX"));
  if ((D == 16 || D == 32 || D == 64) && grad_rows.size(0) < (1ll << 31) && B * F < (1ll << 31) && x_off % 4 == 0 &&
      dX.stride(0) % 4 == 0) {
    // segment-sum path: writes rows [0, U) of grad_rows exactly once (deterministic)
    const int64_t U = grad_rows.size(0);
    at::Tensor part = at::empty({minips_k::emb_seg_part_floats(B * F, D)}, dX.options().dtype(at::kFloat));
    if (present(members)) {  // CSR prebuilt at planning time
      TORCH_CHECK(present(memrow) && members->numel() == B * F && memrow->numel() == B * F,
                  "members/memrow: int32 [B*F]");
      minips_k::emb_backward_csr(base0, bf0, (int)dX.stride(0), dw, B, (int)F, (int)D,
                                 dev<int>(*members, "members", B * F), dev<int>(*memrow, "memrow", B * F), gp, out_bf,
                                 (int)grad_rows.stride(0), part.data_ptr<float>(), stream_of(dX), sorted_rows);
      return;
    }
    at::Tensor ws = at::empty({3 * U + 1 + 2 * B * F + U / 1024 + 1}, inv.options().dtype(at::kInt));
    minips_k::emb_backward_segment(base0, bf0, (int)dX.stride(0), dw, ip, B, (int)F, (int)D, gp, out_bf,
                                   (int)grad_rows.stride(0), (int)U, ws.data_ptr<int>(), part.data_ptr<float>(),
                                   stream_of(dX));
    return;
  }
  TORCH_CHECK(!out_bf, "bf16 gradient rows need the segment-sum path (D 16 / 32 / 64, 4-aligned strides)");
  if (bf0)
    minips_k::wd_emb_backward_bf16((const bf16_t*)base0, (int)dX.stride(0), dw, ip, B, (int)F, (int)D, (float*)gp,
                                   (int)grad_rows.size(1), stream_of(dX));
  else
    minips_k::wd_emb_backward((const float*)base0, (int)dX.stride(0), dw, ip, B, (int)F, (int)D, (float*)gp,
                              (int)grad_rows.size(1), stream_of(dX));
}

// Sort-based planning of a [B, F] batch with disjoint column key ranges (see kernels.h).
// Returns (uniq, inv, counts [1], U_dev [1], members, memrow).
std::vector<at::Tensor> plan_sorted(const at::Tensor& keys, const at::Tensor& col_base, const at::Tensor& col_bits,
                                    std::vector<int64_t> col_bits_host, int64_t route_mult, int64_t route_n,
                                    const at::Tensor& bounds, bool with_positions) {
  const int64_t* bp = dev<int64_t>(bounds, "bounds", 2);
  const int64_t P = bounds.numel() - 1;
  TORCH_CHECK(P >= 1 && P <= 16, "plan_sorted: 1..16 owners");
  const int64_t* kp = dev<int64_t>(keys, "keys");
  TORCH_CHECK(keys.dim() == 2, "keys: [B, F]");
  const int64_t B = keys.size(0), F = keys.size(1);
  TORCH_CHECK(B >= 1 && B <= 16384 && F >= 1 && F <= 64, "plan_sorted: 1 <= B <= 16384, 1 <= F <= 64");
  TORCH_CHECK(col_base.numel() == F && col_bits.numel() == F && (int64_t)col_bits_host.size() == F,
              "col_base / col_bits / col_bits_host: one base / bit count per column");
  // the host copy of the device bit counts is what is validated (the kernel trusts the device one)
  const int obits = P > 1 ? minips_k::plan_owner_bits((int)P) : 0;
  for (int64_t b : col_bits_host)
    TORCH_CHECK(b >= 1 && b + obits <= 32, "col_bits_host: 1..32, owner bits included (plan_sorted_ok)");
  const int64_t n = B * F;
  // one owner: each row's lookup range in member order (the row-parallel embedding backward);
  // one owner, routed keys below 2^31: each lookup's table row (the input assembly's index)
  const bool want_rs = P == 1, want_ri = P == 1 && route_mult && route_n > 0 && route_n <= INT32_MAX;
  auto parts = carve(keys.options(), {{minips_k::plan_sorted_ws_ints(n, (int)F, (int)P), at::kInt},
                                      {n, at::kLong}, {n, at::kLong}, {n, at::kLong}, {n, at::kInt}, {n, at::kInt},
                                      {P + 1, at::kLong}, {with_positions ? n : 0, at::kInt},
                                      {want_rs ? n + 1 : 0, at::kInt}, {want_ri ? n : 0, at::kInt}});
  auto &ws = parts[0], &ukey = parts[1], &uniq = parts[2], &inv = parts[3], &members = parts[4], &memrow = parts[5],
       &counts = parts[6];
  at::Tensor pos = with_positions ? parts[7] : at::Tensor();
  at::Tensor rowstart = want_rs ? parts[8] : at::Tensor();
  at::Tensor rowidx = want_ri ? parts[9] : at::Tensor();
  DeviceGuard g(gpu_of(keys, "keys"));
  minips_k::plan_sorted(kp, (int)B, (int)F, dev<int64_t>(col_base, "col_base", F),
                        dev<int32_t>(col_bits, "col_bits", F), (uint64_t)route_mult, (uint64_t)route_n, bp, (int)P,
                        ws.data_ptr<int32_t>(), ukey.data_ptr<int64_t>(), uniq.data_ptr<int64_t>(),
                        inv.data_ptr<int64_t>(), members.data_ptr<int32_t>(), memrow.data_ptr<int32_t>(),
                        counts.data_ptr<int64_t>(), stream_of(keys), with_positions ? pos.data_ptr<int32_t>() : nullptr,
                        rowstart.defined() ? rowstart.data_ptr<int32_t>() : nullptr,
                        rowidx.defined() ? rowidx.data_ptr<int32_t>() : nullptr);
  // (members, memrow, positions or None, rowstart, rowidx or None) with one owner
  if (rowstart.defined())
    return {uniq, inv, counts.narrow(0, 0, P), counts.narrow(0, P, 1), members, memrow, pos, rowstart, rowidx};
  if (with_positions) return {uniq, inv, counts.narrow(0, 0, P), counts.narrow(0, P, 1), members, memrow, pos};
  return {uniq, inv, counts.narrow(0, 0, P), counts.narrow(0, P, 1), members, memrow};
}

// A dedicated HIP stream (hipStreamCreateWithPriority), returned as an integer handle for
// torch.cuda.ExternalStream. torch.cuda.Stream() hands out streams round-robin from a pool of 32 per
// priority, so past 32 of them two "independent" streams silently alias (and a table's clock work
// serialises behind another's planning); tables and the planning stream take their own instead
// (never destroyed: the Python side reuses a dead owner's stream, see ps/comm.py).
int64_t new_stream(int64_t device, int64_t priority) {
  DeviceGuard g(c10::Device(c10::DeviceType::CUDA, (c10::DeviceIndex)device));
  hipStream_t st = nullptr;
  const hipError_t e = hipStreamCreateWithPriority(&st, hipStreamNonBlocking, (int)priority);
  TORCH_CHECK(e == hipSuccess, "hipStreamCreateWithPriority: ", hipGetErrorString(e));
  return reinterpret_cast<int64_t>(st);
}

struct ColsumLaunch {
  const bf16_t* x;
  int64_t M;
  int N, ld;
  float *out, *slab;
  void launch(hipStream_t s) const { minips_k::colsum_bf16(x, M, N, ld, out, slab, s); }
};

ColsumLaunch prepare_colsum(const at::Tensor& x, at::Tensor& out, at::Tensor& slab) {
  const bf16_t* xp = dev_rows<bf16_t>(x, "x");
  float* op = dev<float>(out, "out", x.size(1));
  TORCH_CHECK(x.size(1) % 8 == 0 && x.stride(0) % 8 == 0, "colsum: x's N and row stride multiples of 8");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(xp) % 16 == 0, "colsum: x must be 16-byte aligned");
  // the blocks' partial rows: a caching-allocator block on the stream (reused, no fill)
  const int64_t strips = (x.size(1) + 63) / 64;
  slab = at::empty({minips_k::colsum_chunks(x.size(0), (int)x.size(1)) * strips * 64}, out.options().dtype(at::kFloat));
  return ColsumLaunch{xp, x.size(0), (int)x.size(1), (int)x.stride(0), op, slab.data_ptr<float>()};
}

void colsum_bf16(const at::Tensor& x, at::Tensor& out) {
  DeviceGuard g(gpu_of(x, "x"));
  at::Tensor slab;
  prepare_colsum(x, out, slab).launch(stream_of(x));
}

void adam_apply(at::Tensor& w, at::Tensor& m, at::Tensor& v, const at::Tensor& g, double lr, double beta1,
                double beta2, double eps, double weight_decay, int64_t step, double grad_scale,
                const OptTensor& w_bf16, const OptTensor& step_dev, bool zero_g, const SlabList& slabs) {
  const int64_t n = w.numel();
  TORCH_CHECK(n == m.numel() && n == v.numel() && n == g.numel(), "adam sizes differ: w, m, v, g");
  TORCH_CHECK(!present(w_bf16) || w_bf16->numel() == n, "w_bf16 size");
  const minips_k::AdamSlabs sl = parse_slabs(slabs, n, "adam_apply");
  DeviceGuard gd(gpu_of(w, "w"));
  minips_k::adam_apply(dev<float>(w, "w"), dev<float>(m, "m"), dev<float>(v, "v"), dev<float>(g, "g"), n, (float)lr,
                       (float)beta1, (float)beta2, (float)eps, (float)weight_decay, (int)step, (float)grad_scale,
                       dev_opt<bf16_t>(w_bf16, "w_bf16", n), stream_of(w), dev_opt<int>(step_dev, "step_dev", 1),
                       zero_g, nullptr, sl.n ? &sl : nullptr);
}

// several ranks: the dense clock's reduce-scatter input = g + its split-K slab planes, g cleared
void slab_pack(at::Tensor& g, at::Tensor& out, const SlabList& slabs) {
  TORCH_CHECK(out.numel() == g.numel(), "slab_pack: out and g sizes differ");
  const minips_k::AdamSlabs sl = parse_slabs(slabs, g.numel(), "slab_pack");
  DeviceGuard gd(gpu_of(g, "g"));
  minips_k::slab_pack(dev<float>(g, "g"), dev<float>(out, "out"), g.numel(), sl.n ? &sl : nullptr, stream_of(g));
}

void emu_sum_slices(const at::Tensor& in, at::Tensor& out, int64_t P) {
  TORCH_CHECK(P >= 1 && in.numel() == out.numel() * P, "emu_sum_slices: in = P x out");
  DeviceGuard gd(gpu_of(in, "in"));
  minips_k::emu_sum_slices(dev<float>(in, "in"), dev<float>(out, "out"), out.numel(), (int)P, stream_of(in));
}

void emu_rebase(at::Tensor& keys, int64_t step, int64_t P, int64_t base) {
  int64_t* kp = dev<int64_t>(keys, "keys");
  DeviceGuard gd(gpu_of(keys, "keys"));
  minips_k::emu_rebase(kp, keys.numel(), step, (int)P, base, stream_of(keys));
}

void sgd_apply(at::Tensor& w, const at::Tensor& g, double lr, double grad_scale, const OptTensor& w_bf16) {
  const int64_t n = w.numel();
  TORCH_CHECK(n == g.numel(), "sizes differ: w, g");
  DeviceGuard gd(gpu_of(w, "w"));
  minips_k::sgd_apply(dev<float>(w, "w"), dev<float>(g, "g"), n, (float)lr, (float)grad_scale,
                      dev_opt<bf16_t>(w_bf16, "w_bf16", n), stream_of(w));
}

void adagrad_apply(at::Tensor& w, at::Tensor& acc, const at::Tensor& g, double lr, double eps, double grad_scale,
                   const OptTensor& w_bf16) {
  const int64_t n = w.numel();
  TORCH_CHECK(n == g.numel() && n == acc.numel(), "sizes differ: w, acc, g");
  DeviceGuard gd(gpu_of(w, "w"));
  minips_k::adagrad_apply(dev<float>(w, "w"), dev<float>(acc, "acc"), dev<float>(g, "g"), n, (float)lr, (float)eps,
                          (float)grad_scale, dev_opt<bf16_t>(w_bf16, "w_bf16", n), stream_of(w));
}

void cast_f32_bf16(const at::Tensor& x, at::Tensor& y) {
  TORCH_CHECK(x.numel() == y.numel(), "sizes differ: x, y");
  DeviceGuard gd(gpu_of(x, "x"));
  minips_k::cast_f32_bf16(dev<float>(x, "x"), dev<bf16_t>(y, "y"), x.numel(), stream_of(x));
}

// rowptr VALUES (ranges of cols / vals) and cols VALUES (positions in w) are device-resident: not checked here
void lr_sparse_step(const at::Tensor& rowptr, const at::Tensor& cols, const at::Tensor& vals,
                    const at::Tensor& labels, const at::Tensor& w, double alpha, const OptTensor& delta,
                    const OptTensor& correct) {
  const int64_t B = labels.numel();
  TORCH_CHECK(rowptr.numel() == B + 1, "rowptr must be [B+1]");
  TORCH_CHECK(!present(delta) || delta->numel() == w.numel(), "delta must match w");
  const int64_t *rp = dev<int64_t>(rowptr, "rowptr"), *cp = dev<int64_t>(cols, "cols");
  const float *vp = dev<float>(vals, "vals", cols.numel()), *lp = dev<float>(labels, "labels");
  float* c = dev_opt<float>(correct, "correct", 1);
  DeviceGuard gd(gpu_of(w, "w"));
  if (w.scalar_type() == at::kDouble)  // reference-precision LR (double tables)
    minips_k::lr_sparse_step_f64(rp, cp, vp, lp, B, dev<double>(w, "w"), alpha, dev_opt<double>(delta, "delta"), c,
                                 stream_of(w));
  else
    minips_k::lr_sparse_step(rp, cp, vp, lp, B, dev<float>(w, "w"), (float)alpha, dev_opt<float>(delta, "delta"), c,
                             stream_of(w));
}

void kmeans_assign(const at::Tensor& X, const at::Tensor& C, at::Tensor& assign, const OptTensor& dist) {
  TORCH_CHECK(X.dim() == 2 && C.dim() == 2 && X.size(1) == C.size(1) && assign.numel() == X.size(0),
              "kmeans shapes: X, C, assign");
  const int64_t n = X.size(0);
  DeviceGuard gd(gpu_of(X, "X"));
  minips_k::kmeans_assign(dev<float>(X, "X"), n, (int)X.size(1), dev<float>(C, "C"), (int)C.size(0),
                          dev<int32_t>(assign, "assign", n), dev_opt<float>(dist, "dist", n), stream_of(X));
}

void kmeans_split3(const at::Tensor& src, at::Tensor& out, int64_t order, at::Tensor& norms) {
  TORCH_CHECK(src.dim() == 2 && out.dim() == 2 && out.size(0) == src.size(0) && out.size(1) >= 3 * src.size(1),
              "kmeans_split3 shapes: src, out");
  DeviceGuard g(gpu_of(src, "src"));
  minips_k::kmeans_split3(dev<float>(src, "src"), src.size(0), (int)src.size(1), dev<bf16_t>(out, "out"),
                          (int)out.size(1), (int)order, dev<float>(norms, "norms", src.size(0)), stream_of(src));
}

void kmeans_argmin(const at::Tensor& S, const at::Tensor& cn, const at::Tensor& xn, at::Tensor& assign,
                   const OptTensor& dist) {
  TORCH_CHECK(S.dim() == 2, "S: [n, k]");
  const int64_t n = S.size(0), k = S.size(1);
  DeviceGuard g(gpu_of(S, "S"));
  minips_k::kmeans_argmin(dev<float>(S, "S"), n, (int)k, dev<float>(cn, "cn", k), dev<float>(xn, "xn", n),
                          dev<int32_t>(assign, "assign", n), dev_opt<float>(dist, "dist", n), stream_of(S));
}

void criteo_synth(int64_t seed, int64_t step, const OptTensor& step_dev, const at::Tensor& cards,
                  const at::Tensor& offsets, const at::Tensor& w, at::Tensor& dense, at::Tensor& keys,
                  at::Tensor& labels) {
  const int64_t B = labels.numel();
  const int F = (int)cards.numel();
  TORCH_CHECK(dense.dim() == 2 && keys.numel() == B * F && dense.size(0) == B && w.numel() == dense.size(1),
              "criteo_synth shapes: keys, dense, w");
  const int nd = (int)dense.size(1);
  DeviceGuard g(gpu_of(keys, "keys"));
  minips_k::criteo_synth((uint64_t)seed, (uint64_t)step, dev_count(step_dev, "step_dev"), B, F,
                         dev<int64_t>(cards, "cards"), dev<int64_t>(offsets, "offsets", F), nd, dev<float>(w, "w", nd),
                         dev<float>(dense, "dense", B * nd), dev<int64_t>(keys, "keys", B * F),
                         dev<float>(labels, "labels"), stream_of(keys));
}

// dst[i].copy_(src[i]) for every pair, in one launch on dst[0]'s current stream (same byte sizes,
// contiguous, one device; at most 16 pairs per launch)
void multi_copy(const std::vector<at::Tensor>& dst, const std::vector<at::Tensor>& src) {
  TORCH_CHECK(dst.size() == src.size() && !dst.empty(), "multi_copy: matching non-empty lists");
  DeviceGuard g(gpu_of(dst[0], "dst"));
  for (size_t base = 0; base < dst.size(); base += minips_k::kMultiCopyMax) {
    minips_k::MultiCopyArgs a{};
    a.n = (int)std::min<size_t>(minips_k::kMultiCopyMax, dst.size() - base);
    a.start[0] = 0;
    for (int t = 0; t < a.n; ++t) {
      const at::Tensor& d = dst[base + t];
      const at::Tensor& s = src[base + t];
      const int64_t nb = d.numel() * d.element_size();
      TORCH_CHECK(nb == s.numel() * s.element_size(), "multi_copy: dst / src byte sizes differ");
      a.dst[t] = dev_bytes(d, "dst", nb);
      a.src[t] = dev_bytes(s, "src", nb);
      TORCH_CHECK(d.get_device() == dst[0].get_device() && s.get_device() == dst[0].get_device(),
                  "multi_copy: dst / src on one GPU");
      const bool al = (reinterpret_cast<uintptr_t>(a.dst[t]) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(a.src[t]) & 15) == 0;
      a.n16[t] = al ? nb / 16 : 0;
      a.tail[t] = nb - a.n16[t] * 16;
      a.start[t + 1] = a.start[t] + a.n16[t] + a.tail[t];
    }
    minips_k::multi_copy(a, stream_of(dst[base]));
  }
}

// out: int64 [2] on the GPU; launched on `stream` (a torch stream handle; 0 = out's current stream)
void clock_probe(at::Tensor& out, int64_t spin_ticks, int64_t stream) {
  int64_t* op = dev<int64_t>(out, "out", 2);
  DeviceGuard g(gpu_of(out, "out"));
  minips_k::clock_probe(op, (int)spin_ticks, stream ? reinterpret_cast<hipStream_t>(stream) : stream_of(out));
}

void uniform_synth(int64_t seed, int64_t step, int64_t rows, at::Tensor& dense, at::Tensor& keys, at::Tensor& labels) {
  TORCH_CHECK(keys.dim() == 2 && dense.dim() == 2 && keys.size(0) == labels.numel() && dense.size(0) == labels.numel(),
              "uniform_synth shapes: keys [B, F], dense [B, n], labels [B]");
  DeviceGuard g(gpu_of(keys, "keys"));
  minips_k::uniform_synth((uint64_t)seed, (uint64_t)step, keys.size(0), (int)keys.size(1), (uint64_t)rows,
                          (int)dense.size(1), dev<float>(dense, "dense"), dev<int64_t>(keys, "keys"),
                          dev<float>(labels, "labels"), stream_of(keys));
}

// a layernorm activation: bf16 [M, >= C] rows with a leading dim % 4 == 0
bf16_t* ln_rows(const at::Tensor& t, int64_t M, int64_t C, const char* n) {
  bf16_t* p = dev_rows<bf16_t>(t, n, M, C);
  TORCH_CHECK(t.size(0) == M && t.stride(0) % 4 == 0, n, " must have ", M, " rows and a leading dim % 4 == 0");
  return p;
}

void layernorm_fwd(const at::Tensor& x, int64_t C, const at::Tensor& gamma, const at::Tensor& beta, double eps,
                   at::Tensor& y, at::Tensor& mean, at::Tensor& rstd) {
  TORCH_CHECK(C % 4 == 0 && C >= 0 && C <= 1024, "layernorm: C % 4 == 0 and C <= 1024");
  TORCH_CHECK(x.dim() == 2, "x must be a row-major matrix");
  const int64_t M = x.size(0);
  TORCH_CHECK(mean.numel() == M && rstd.numel() == M, "layernorm rows: mean, rstd");
  DeviceGuard g(gpu_of(x, "x"));
  minips_k::layernorm_fwd(ln_rows(x, M, C, "x"), (int)x.stride(0), M, (int)C, dev<bf16_t>(gamma, "gamma", C),
                          dev<bf16_t>(beta, "beta", C), (float)eps, ln_rows(y, M, C, "y"), (int)y.stride(0),
                          dev<float>(mean, "mean", M), dev<float>(rstd, "rstd", M), stream_of(x));
}

void layernorm_bwd(const at::Tensor& x, const at::Tensor& dy, int64_t C, const at::Tensor& gamma,
                   const at::Tensor& mean, const at::Tensor& rstd, at::Tensor& dx, at::Tensor& dgamma,
                   at::Tensor& dbeta, bool accumulate) {
  TORCH_CHECK(C % 4 == 0 && C >= 0 && C <= 1024, "layernorm: C % 4 == 0 and C <= 1024");
  TORCH_CHECK(x.dim() == 2, "x must be a row-major matrix");
  const int64_t M = x.size(0);
  TORCH_CHECK(mean.numel() == M && rstd.numel() == M, "layernorm_bwd rows: mean, rstd");
  const bf16_t *xp = ln_rows(x, M, C, "x"), *dyp = ln_rows(dy, M, C, "dy");
  bf16_t* dxp = ln_rows(dx, M, C, "dx");
  DeviceGuard g(gpu_of(x, "x"));
  at::Tensor partial = at::empty({(int64_t)minips_k::layernorm_bwd_blocks(M) * 2 * C}, x.options().dtype(at::kFloat));
  minips_k::layernorm_bwd(xp, (int)x.stride(0), dyp, (int)dy.stride(0), M, (int)C, dev<bf16_t>(gamma, "gamma", C),
                          dev<float>(mean, "mean", M), dev<float>(rstd, "rstd", M), dxp, (int)dx.stride(0),
                          dev<float>(dgamma, "dgamma", C), dev<float>(dbeta, "dbeta", C), partial.data_ptr<float>(),
                          accumulate, stream_of(x));
}

// labels VALUES (< V) are device-resident: not checked here
void softmax_xent(at::Tensor& logits, int64_t V, const at::Tensor& labels, double scale, at::Tensor& loss_sum,
                  const OptTensor& correct) {
  bf16_t* lp = dev<bf16_t>(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && V >= 0 && logits.size(1) >= V && labels.numel() == logits.size(0),
              "softmax_xent shapes: logits, labels");
  DeviceGuard g(gpu_of(logits, "logits"));
  minips_k::softmax_xent(lp, (int)logits.size(1), logits.size(0), (int)V, dev<int64_t>(labels, "labels"), (float)scale,
                         dev<float>(loss_sum, "loss_sum", 1), dev_opt<float>(correct, "correct", 1),
                         stream_of(logits));
}

void causal_softmax_fwd(const at::Tensor& S, int64_t T, at::Tensor& P) {
  TORCH_CHECK(T >= 1 && S.numel() == P.numel() && S.numel() % (T * T) == 0, "causal_softmax shapes: S, P");
  DeviceGuard g(gpu_of(S, "S"));
  minips_k::causal_softmax_fwd(dev<float>(S, "S"), S.numel() / T, (int)T, dev<bf16_t>(P, "P"), stream_of(S));
}

void causal_softmax_bwd(const at::Tensor& P, const at::Tensor& dP, int64_t T, double scale, at::Tensor& dS) {
  TORCH_CHECK(T >= 1 && P.numel() == dP.numel() && P.numel() == dS.numel() && P.numel() % (T * T) == 0,
              "causal_softmax shapes: P, dP, dS");
  DeviceGuard g(gpu_of(P, "P"));
  minips_k::causal_softmax_bwd(dev<bf16_t>(P, "P"), dev<float>(dP, "dP"), P.numel() / T, (int)T, (float)scale,
                               dev<bf16_t>(dS, "dS"), stream_of(P));
}

void gelu_bwd(const at::Tensor& dh, const at::Tensor& u, at::Tensor& du) {
  const int64_t n = u.numel();
  TORCH_CHECK(dh.numel() == n && du.numel() == n, "gelu_bwd sizes: dh, u, du");
  const bf16_t* up = dev<bf16_t>(u, "u");
  DeviceGuard g(gpu_of(u, "u"));
  minips_k::gelu_bwd(dev<bf16_t>(dh, "dh"), up, n, dev<bf16_t>(du, "du"), stream_of(u));
}

void add_bf16(const at::Tensor& a, const at::Tensor& b, at::Tensor& out) {
  const int64_t n = a.numel();
  TORCH_CHECK(b.numel() == n && out.numel() == n, "add sizes: a, b, out");
  const bf16_t* ap = dev<bf16_t>(a, "a");
  DeviceGuard g(gpu_of(a, "a"));
  minips_k::add_bf16(ap, dev<bf16_t>(b, "b"), n, dev<bf16_t>(out, "out"), stream_of(a));
}

// an attention activation: bf16 [rows, >= cols] with a leading dim % 8 == 0
bf16_t* attn_rows(const at::Tensor& t, int64_t rows, int64_t cols, const char* n) {
  bf16_t* p = dev_rows<bf16_t>(t, n, rows, cols);
  TORCH_CHECK(t.size(0) == rows && t.stride(0) % 8 == 0, n, " must have ", rows, " rows and a leading dim % 8 == 0");
  return p;
}

void attn_fwd(const at::Tensor& qkv, int64_t B, int64_t T, int64_t H, double scale, at::Tensor& O, at::Tensor& lse) {
  TORCH_CHECK(B >= 0 && T >= 0 && H >= 1, "attn: B, T >= 0, H >= 1");
  const int64_t d = H * 64;
  const bf16_t* qp = attn_rows(qkv, B * T, 3 * d, "qkv");
  DeviceGuard g(gpu_of(qkv, "qkv"));
  minips_k::attn_fwd(qp, (int)qkv.stride(0), (int)B, (int)T, (int)H, (int)d, (float)scale, attn_rows(O, B * T, d, "O"),
                     (int)O.stride(0), dev<float>(lse, "lse", B * H * T), stream_of(qkv));
}

void attn_bwd(const at::Tensor& qkv, const at::Tensor& O, const at::Tensor& dO, const at::Tensor& lse,
              at::Tensor& delta, int64_t B, int64_t T, int64_t H, double scale, at::Tensor& dqkv) {
  TORCH_CHECK(B >= 0 && T >= 0 && H >= 1, "attn: B, T >= 0, H >= 1");
  const int64_t d = H * 64;
  const bf16_t* qp = attn_rows(qkv, B * T, 3 * d, "qkv");
  DeviceGuard g(gpu_of(qkv, "qkv"));
  minips_k::attn_bwd(qp, (int)qkv.stride(0), attn_rows(O, B * T, d, "O"), (int)O.stride(0),
                     attn_rows(dO, B * T, d, "dO"), (int)dO.stride(0), dev<float>(lse, "lse", B * H * T),
                     dev<float>(delta, "delta", B * H * T), (int)B, (int)T, (int)H, (int)d, (float)scale,
                     attn_rows(dqkv, B * T, 3 * d, "dqkv"), (int)dqkv.stride(0), stream_of(qkv));
}

// hash keys: the kernels take them as unsigned 64-bit words (EMPTY = ~0), cast from a checked int64_t*
unsigned long long* dev_hash_keys(const at::Tensor& t, const char* name) {
  return reinterpret_cast<unsigned long long*>(dev<int64_t>(t, name));
}

void hash_slots(at::Tensor& tab_keys, const at::Tensor& q, at::Tensor& slots, at::Tensor& vals, double init_scale,
                int64_t seed, at::Tensor& counters, const OptTensor& n_dev) {
  const int64_t cap = tab_keys.numel();
  TORCH_CHECK(vals.dim() == 2 && vals.size(0) == cap, "vals [cap, W]");
  DeviceGuard g(gpu_of(q, "q"));
  minips_k::hash_slots(dev_hash_keys(tab_keys, "tab_keys"), cap, dev<int64_t>(q, "q"), q.numel(),
                       dev<int64_t>(slots, "slots", q.numel()), dev<float>(vals, "vals"), (int)vals.size(1),
                       (float)init_scale, (uint64_t)seed, dev<int>(counters, "counters", 2), stream_of(q),
                       dev_count(n_dev));
}

void hash_rehash(const at::Tensor& old_keys, const at::Tensor& old_vals, const OptTensor& old_state,
                 at::Tensor& new_keys, at::Tensor& new_vals, const OptTensor& new_state, at::Tensor& counters) {
  const int64_t old_cap = old_keys.numel(), new_cap = new_keys.numel();
  TORCH_CHECK(old_vals.dim() == 2 && new_vals.dim() == 2 && old_vals.size(0) == old_cap &&
                  new_vals.size(0) == new_cap && old_vals.size(1) == new_vals.size(1),
              "rehash shapes: old_vals [old cap, W], new_vals [new cap, W]");
  TORCH_CHECK(old_state.has_value() == new_state.has_value(), "state on both sides or neither");
  const unsigned long long* ok = dev_hash_keys(old_keys, "old_keys");
  DeviceGuard g(gpu_of(old_keys, "old_keys"));
  minips_k::hash_rehash(ok, dev<float>(old_vals, "old_vals"), dev_opt<float>(old_state, "old_state", old_cap), old_cap,
                        dev_hash_keys(new_keys, "new_keys"), dev<float>(new_vals, "new_vals"),
                        dev_opt<float>(new_state, "new_state", new_cap), new_cap, (int)new_vals.size(1),
                        dev<int>(counters, "counters", 1), stream_of(old_keys));
}

// tok VALUES (rows of wte / dwte) are device-resident: not checked here
void embed_fwd(const at::Tensor& wte, const at::Tensor& wpe, const at::Tensor& tok, int64_t T, at::Tensor& out) {
  const bf16_t* ep = dev<bf16_t>(wte, "wte");
  TORCH_CHECK(wte.dim() == 2 && wpe.dim() == 2 && out.dim() == 2, "wte, wpe, out: 2-D");
  const int64_t C = wte.size(1), M = tok.numel();
  TORCH_CHECK(C % 8 == 0 && wpe.size(1) == C && T >= 1 && wpe.size(0) >= T && out.size(0) == M && out.size(1) >= C &&
                  out.stride(0) % 8 == 0,
              "embed_fwd shapes: wpe, out");
  DeviceGuard g(gpu_of(wte, "wte"));
  minips_k::embed_fwd(ep, dev<bf16_t>(wpe, "wpe", T * C), dev<int64_t>(tok, "tok"), M, (int)T, (int)C,
                      dev<bf16_t>(out, "out"), (int)out.stride(0), stream_of(wte));
}

void embed_bwd(const at::Tensor& dx, const at::Tensor& tok, int64_t T, at::Tensor& dwte, at::Tensor& dwpe) {
  const bf16_t* xp = dev<bf16_t>(dx, "dx");
  TORCH_CHECK(dwte.dim() == 2 && dwpe.dim() == 2 && dx.dim() == 2, "dx, dwte, dwpe: 2-D");
  const int64_t C = dwte.size(1), M = tok.numel();
  TORCH_CHECK(C % 2 == 0 && dwpe.size(1) == C && T >= 1 && dwpe.size(0) >= T && dx.size(0) == M && dx.size(1) >= C &&
                  dx.stride(0) % 2 == 0,
              "embed_bwd shapes: dx, dwpe");
  DeviceGuard g(gpu_of(dx, "dx"));
  minips_k::embed_bwd(xp, (int)dx.stride(0), dev<int64_t>(tok, "tok"), M, (int)T, (int)C, dev<float>(dwte, "dwte"),
                      dev<float>(dwpe, "dwpe", T * C), stream_of(dx));
}

void dlrm_interact_fwd(const at::Tensor& V, int64_t NV, int64_t D, int64_t dense_idx, at::Tensor& out) {
  TORCH_CHECK(NV >= 1 && D >= 1 && dense_idx >= 0 && dense_idx < NV, "dense_idx / NV / D");
  const int64_t B = V.numel() / (NV * D);
  TORCH_CHECK(out.dim() == 2 && out.size(0) == B && out.size(1) >= D + NV * (NV - 1) / 2, "interaction out shape");
  DeviceGuard g(gpu_of(V, "V"));
  minips_k::dlrm_interact_fwd(dev<bf16_t>(V, "V"), B, (int)NV, (int)D, (int)dense_idx, dev<bf16_t>(out, "out"),
                              (int)out.size(1), stream_of(V));
}

void dlrm_interact_bwd(const at::Tensor& V, int64_t NV, int64_t D, int64_t dense_idx, const at::Tensor& dout,
                       at::Tensor& dV, at::Tensor& d_dense) {
  TORCH_CHECK(NV >= 1 && D >= 1 && dense_idx >= 0 && dense_idx < NV, "dense_idx / NV / D");
  const int64_t B = V.numel() / (NV * D);
  TORCH_CHECK(dV.numel() == V.numel() && dout.dim() == 2 && dout.size(0) == B &&
                  dout.size(1) >= D + NV * (NV - 1) / 2 && d_dense.numel() == B * D,
              "interaction bwd shapes: dV, dout, d_dense");
  const bf16_t *vp = dev<bf16_t>(V, "V"), *op = dev<bf16_t>(dout, "dout");
  bf16_t* dd = dev<bf16_t>(d_dense, "d_dense");
  DeviceGuard g(gpu_of(V, "V"));
  if (dV.scalar_type() == at::kBFloat16)
    minips_k::dlrm_interact_bwd_bf16(vp, B, (int)NV, (int)D, (int)dense_idx, op, (int)dout.size(1),
                                     dev<bf16_t>(dV, "dV"), dd, stream_of(V));
  else
    minips_k::dlrm_interact_bwd(vp, B, (int)NV, (int)D, (int)dense_idx, op, (int)dout.size(1), dev<float>(dV, "dV"),
                                dd, stream_of(V));
}

// --- one-sided shards over xGMI (minips_amd/ps/onesided.py) -------------------------------------
// A hipMalloc'd, zero-filled buffer exported for IPC: (uint8 tensor owning it, 64-byte handle).
// kind: 0 coarse-grained (hipMalloc), 1 fine-grained (shards / pull copies / control lines: coherent
// for peer reads and system-scope atomics), 2 uncached (inboxes: written by peers, read once by the
// owner). The memory model of these buffers is written down in csrc/kernels/onesided.hip.
std::tuple<at::Tensor, py::bytes> ipc_alloc(int64_t nbytes, int64_t device, int64_t kind) {
  TORCH_CHECK(nbytes > 0, "ipc_alloc: nbytes must be > 0");
  DeviceGuard g(at::Device(at::kCUDA, (c10::DeviceIndex)device));
  void* p = nullptr;
  if (kind == 0) {
    TORCH_CHECK(hipMalloc(&p, (size_t)nbytes) == hipSuccess, "ipc_alloc: hipMalloc of ", nbytes, " bytes failed");
  } else {
    TORCH_CHECK(hipExtMallocWithFlags(&p, (size_t)nbytes,
                                      kind == 1 ? hipDeviceMallocFinegrained : hipDeviceMallocUncached) == hipSuccess,
                "ipc_alloc: hipExtMallocWithFlags(", kind == 1 ? "fine-grained" : "uncached", ") of ", nbytes,
                " bytes failed");
  }
  TORCH_CHECK(hipMemset(p, 0, (size_t)nbytes) == hipSuccess, "ipc_alloc: hipMemset failed");
  hipIpcMemHandle_t h;
  TORCH_CHECK(hipIpcGetMemHandle(&h, p) == hipSuccess, "ipc_alloc: hipIpcGetMemHandle failed");
  auto t = torch::from_blob(p, {nbytes}, [](void* q) { (void)hipFree(q); },
                            at::TensorOptions().dtype(at::kByte).device(at::kCUDA, (c10::DeviceIndex)device));
  return {t, py::bytes(reinterpret_cast<const char*>(&h), sizeof(h))};
}

// Maps a peer's exported buffer into this process (peer access enabled lazily); the tensor owns
// the mapping (closed when it is freed).
at::Tensor ipc_open(py::bytes handle, int64_t nbytes, int64_t device) {
  const std::string hs = handle;
  TORCH_CHECK(hs.size() == sizeof(hipIpcMemHandle_t), "ipc_open: bad handle size ", hs.size());
  hipIpcMemHandle_t h;
  std::memcpy(&h, hs.data(), sizeof(h));
  DeviceGuard g(at::Device(at::kCUDA, (c10::DeviceIndex)device));
  void* p = nullptr;
  TORCH_CHECK(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess) == hipSuccess,
              "ipc_open: hipIpcOpenMemHandle failed");
  return torch::from_blob(p, {nbytes}, [](void* q) { (void)hipIpcCloseMemHandle(q); },
                          at::TensorOptions().dtype(at::kByte).device(at::kCUDA, (c10::DeviceIndex)device));
}

// The tensors of device ADDRESSES below (inbox, bases, hkeys, hvals, srcs, locks: one int64 per
// owner) are checked as tensors; what the addresses point to is the Python side's contract.
const int64_t* dev_owners(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.numel() >= 1 && t.numel() <= minips_k::kPsMaxWorld, name, " must list 1..16 owners");
  return dev<int64_t>(t, name);
}

// Requester -> owners push of one clock (onesided.hip): uniq/counts/U_dev of the plan, fp32
// gradient rows [>= n, W], inbox = [P] int64 addresses of every owner's inbox as mapped here.
void ps_push_rows(const at::Tensor& uniq, const at::Tensor& counts, const OptTensor& U_dev, int64_t n,
                  const at::Tensor& g, const at::Tensor& inbox, int64_t slot_off, int64_t cap) {
  const int64_t* ip = dev_owners(inbox, "inbox");
  const int64_t P = inbox.numel();
  TORCH_CHECK(n >= 0 && g.dim() == 2 && g.size(0) >= n, "push: g shorter than n rows");
  TORCH_CHECK(n <= cap && slot_off >= 0, "push: n exceeds the inbox slot capacity");
  DeviceGuard guard(gpu_of(g, "g"));
  minips_k::ps_push_rows(dev<int64_t>(uniq, "uniq", n), dev<int64_t>(counts, "counts", P), dev_count(U_dev, "U_dev"), n,
                         dev<float>(g, "g", n * g.size(1)), (int)g.size(1), ip, (int)P, slot_off, cap, stream_of(g));
}

void ps_push_dense(at::Tensor& grad, const at::Tensor& inbox, int64_t data_off, int64_t S, const SlabList& slabs) {
  const int64_t* ip = dev_owners(inbox, "inbox");
  const int64_t P = inbox.numel();
  TORCH_CHECK(S >= 0 && data_off >= 0, "ps_push_dense: S, data_off >= 0");
  // (slab regions as adam_apply's, inside the P * S floats pushed)
  const minips_k::AdamSlabs sl = parse_slabs(slabs, P * S, "ps_push_dense");
  DeviceGuard g(gpu_of(grad, "grad"));
  minips_k::ps_push_dense(dev<float>(grad, "grad", P * S), ip, (int)P, data_off, S, stream_of(grad),
                          sl.n ? &sl : nullptr);
}

void ps_set_headers(const at::Tensor& inbox, int64_t slot_off, int64_t value) {
  const int64_t* ip = dev_owners(inbox, "inbox");
  DeviceGuard guard(gpu_of(inbox, "inbox"));
  minips_k::ps_set_headers(ip, (int)inbox.numel(), slot_off, value, stream_of(inbox));
}

// the gather of fp32 (bf16tab = false) or bf16 table rows from every owner's shard
template <bool bf16tab>
void ps_gather_rows(const at::Tensor& bases, const at::Tensor& bounds, const at::Tensor& keys, const OptTensor& n_dev,
                    int64_t W, at::Tensor& out) {
  const int64_t* bp = dev_owners(bases, "bases");
  const int64_t P = bases.numel(), n = keys.numel();
  TORCH_CHECK(bounds.numel() == P + 1, "bounds must have P+1 entries");
  TORCH_CHECK(out.dim() == 2 && out.size(1) == W, "out must be [>= n, W]");
  bool bf;
  void* op = dev_rows_any(out, "out", &bf, n, W);
  DeviceGuard guard(gpu_of(keys, "keys"));
  (bf16tab ? minips_k::ps_gather_rows_bf16tab : minips_k::ps_gather_rows)(
      bp, dev<int64_t>(bounds, "bounds"), (int)P, dev<int64_t>(keys, "keys"), n, dev_count(n_dev), (int)W, op, bf,
      stream_of(keys));
}

void ps_hash_gather(const at::Tensor& hkeys, const at::Tensor& hvals, const at::Tensor& bounds, int64_t cap,
                    const at::Tensor& keys, const OptTensor& n_dev, int64_t W, at::Tensor& out) {
  const int64_t P = hkeys.numel(), n = keys.numel();
  TORCH_CHECK(P == hvals.numel() && bounds.numel() == P + 1, "P owners (hkeys, hvals), P+1 bounds");
  TORCH_CHECK(out.dim() == 2 && out.size(1) == W, "out must be [>= n, W]");
  bool bf;
  void* op = dev_rows_any(out, "out", &bf, n, W);
  DeviceGuard guard(gpu_of(keys, "keys"));
  minips_k::ps_hash_gather(dev_owners(hkeys, "hkeys"), dev_owners(hvals, "hvals"), dev<int64_t>(bounds, "bounds"),
                           (int)P, cap, dev<int64_t>(keys, "keys"), n, dev_count(n_dev), (int)W, op, bf,
                           stream_of(keys));
}

// dst[o * shard_bytes, ...) = srcs[o][0, shard_bytes) for the listed owners (one kernel)
void ps_pull(const at::Tensor& srcs, const std::vector<int64_t>& owners, int64_t shard_bytes, at::Tensor& dst) {
  const int64_t* sp = dev<int64_t>(srcs, "srcs");
  TORCH_CHECK(owners.size() <= (size_t)minips_k::kPsMaxWorld, "<= 16 owners");
  TORCH_CHECK(shard_bytes >= 0, "shard_bytes >= 0");
  uint64_t packed = 0;
  for (size_t i = 0; i < owners.size(); ++i) {
    TORCH_CHECK(owners[i] >= 0 && owners[i] < srcs.numel(), "owners: id out of range");
    packed |= (uint64_t)owners[i] << (4 * i);
  }
  DeviceGuard guard(gpu_of(dst, "dst"));
  minips_k::ps_pull(sp, packed, (int)owners.size(), shard_bytes, dev_bytes(dst, "dst", srcs.numel() * shard_bytes),
                    stream_of(dst));
}

// Reader side of the per-owner locks: `locks` [P] int64 device addresses of the owners' lock words,
// `held` / `err` raw device addresses (a slot of the reader's held ring, the rank's error word).
void ps_read_lock(const at::Tensor& locks, int64_t held, int64_t err) {
  const int64_t* lp = dev<int64_t>(locks, "locks");
  DeviceGuard guard(gpu_of(locks, "locks"));
  minips_k::ps_read_lock(lp, (int)locks.numel(), reinterpret_cast<uint32_t*>(held), reinterpret_cast<uint32_t*>(err),
                         stream_of(locks));
}

void ps_read_unlock(const at::Tensor& locks, int64_t held) {
  const int64_t* lp = dev<int64_t>(locks, "locks");
  DeviceGuard guard(gpu_of(locks, "locks"));
  minips_k::ps_read_unlock(lp, (int)locks.numel(), reinterpret_cast<uint32_t*>(held), stream_of(locks));
}

// A host-resident, device-mapped 32-bit word (hipHostMalloc, coherent): the rank's error word of the
// one-sided protocol (a device spin that timed out sets a bit; the host reads it with no sync).
class HostWord {
 public:
  HostWord() {
    TORCH_CHECK(hipHostMalloc(reinterpret_cast<void**>(&h_), 64, hipHostMallocMapped | hipHostMallocCoherent) ==
                    hipSuccess,
                "HostWord: hipHostMalloc");
    *h_ = 0;
    TORCH_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_), h_, 0) == hipSuccess, "HostWord: device ptr");
  }
  ~HostWord() { (void)hipHostFree(h_); }
  int64_t value() const { return (int64_t)__atomic_load_n(h_, __ATOMIC_ACQUIRE); }
  void clear() { __atomic_store_n(h_, 0u, __ATOMIC_RELEASE); }
  int64_t device_ptr() const { return reinterpret_cast<int64_t>(d_); }

 private:
  uint32_t* h_ = nullptr;
  uint32_t* d_ = nullptr;
};

// A same-device stream-ordering event: no timing, no system-scope fence (hipEventDisableSystemFence).
// The fork / join events of a step order streams of ONE device, which needs agent scope only; the
// default event's system-scope release on every record cost the W&D step's main queue 7-9 us per
// fork (rocprofv3 timeline, profiles/r4).
class FastEvent {
 public:
  FastEvent() {
    TORCH_CHECK(hipEventCreateWithFlags(&ev_, hipEventDisableTiming | hipEventDisableSystemFence) == hipSuccess,
                "FastEvent: hipEventCreateWithFlags");
  }
  ~FastEvent() {
    if (ev_) (void)hipEventDestroy(ev_);
  }
  void record(int64_t stream) {
    TORCH_CHECK(hipEventRecord(ev_, reinterpret_cast<hipStream_t>(stream)) == hipSuccess, "FastEvent: record");
  }
  void wait(int64_t stream) {
    TORCH_CHECK(hipStreamWaitEvent(reinterpret_cast<hipStream_t>(stream), ev_, 0) == hipSuccess, "FastEvent: wait");
  }
  bool query() { return hipEventQuery(ev_) == hipSuccess; }
  void synchronize() { TORCH_CHECK(hipEventSynchronize(ev_) == hipSuccess, "FastEvent: synchronize"); }

 private:
  hipEvent_t ev_ = nullptr;
};

// A recorded launch sequence over two streams (0: the step's compute stream, 1: its side stream),
// replayed from C++ with no per-launch validation, argument conversion or Python dispatch. The
// recording IS the first execution: every op below launches on the current stream (which must be
// one of the list's two) and appends its validated launch; fork() orders the two streams with an
// event the list owns. run() replays the whole sequence onto the streams it is given. The list
// holds every tensor a launch addresses (operands and its own split-K planes), so no recorded
// address can be freed and handed to another buffer while the list lives; callers key lists by
// the buffers they address and record again when those change. Replaces ~25 binding calls of the
// W&D dense forward / backward per step (ops.gemm's argument conversion is 4-6 us of host each).
class LaunchList {
 public:
  LaunchList(int64_t main, int64_t side)
      : rec_{reinterpret_cast<hipStream_t>(main), reinterpret_cast<hipStream_t>(side)} {}
  ~LaunchList() {
    for (hipEvent_t e : events_) (void)hipEventDestroy(e);
  }
  LaunchList(const LaunchList&) = delete;
  LaunchList& operator=(const LaunchList&) = delete;

  void gemm(const at::Tensor& A, const at::Tensor& B, at::Tensor& C, int64_t M, int64_t N, int64_t K, bool a_km,
            bool b_kn, int64_t epi, const OptTensor& bias, const OptTensor& mask, const OptTensor& colsum, double alpha,
            int64_t split_k, const OptTensor& perm, int64_t seg, int64_t tile) {
    DeviceGuard gd(gpu_of(A, "A"));
    at::Tensor slab;
    GemmLaunch g = prepare_gemm(A, B, C, M, N, K, a_km, b_kn, epi, bias, mask, colsum, alpha, split_k, 1, 1, 0, 0, 0,
                                {}, perm, seg, slab);
    g.tile = check_tile(tile);
    const int k = slot(A);
    g.launch(rec_[k]);
    for (const auto* t : {&bias, &mask, &colsum, &perm})
      if (present(*t)) keep_.push_back(**t);
    hold({A, B, C, slab});
    ops_.push_back([g, k](const hipStream_t* s) { g.launch(s[k]); });
  }

  int64_t gemm_slab(const at::Tensor& A, const at::Tensor& B, at::Tensor& slab, int64_t M, int64_t N, int64_t K,
                    bool a_km, bool b_kn, int64_t split_k) {
    const GemmSlabLaunch g = prepare_gemm_slab(A, B, slab, M, N, K, a_km, b_kn, split_k);
    DeviceGuard gd(gpu_of(A, "A"));
    const int k = slot(A);
    const int nsplit = g.launch(rec_[k]);
    hold({A, B, slab});
    ops_.push_back([g, k](const hipStream_t* s) { (void)g.launch(s[k]); });
    return nsplit;
  }

  void colsum_bf16(const at::Tensor& x, at::Tensor& out) {
    DeviceGuard gd(gpu_of(x, "x"));
    at::Tensor slab;
    const ColsumLaunch c = prepare_colsum(x, out, slab);
    const int k = slot(x);
    c.launch(rec_[k]);
    hold({x, out, slab});
    ops_.push_back([c, k](const hipStream_t* s) { c.launch(s[k]); });
  }

  void wd_head_fold(int64_t B, int64_t Hd, at::Tensor& dw, at::Tensor& db, at::Tensor& loss_sum,
                    const OptTensor& dH_colsum) {
    const HeadFoldLaunch f = prepare_head_fold(B, Hd, dw, db, loss_sum, dH_colsum);
    DeviceGuard gd(gpu_of(dw, "dw"));
    const int k = slot(dw);
    f.launch(rec_[k]);
    hold({dw, db, loss_sum});
    if (dH_colsum.has_value()) hold({*dH_colsum});
    ops_.push_back([f, k](const hipStream_t* s) { f.launch(s[k]); });
  }

  // stream ``dst`` waits for the work issued so far on stream ``src`` (raw stream handles of the
  // recording: the list's two streams)
  void fork(int64_t src, int64_t dst) {
    const int a = slot_raw(reinterpret_cast<hipStream_t>(src)), b = slot_raw(reinterpret_cast<hipStream_t>(dst));
    TORCH_CHECK(a != b, "LaunchList.fork: one stream");
    hipEvent_t ev = nullptr;
    TORCH_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming | hipEventDisableSystemFence) == hipSuccess,
                "LaunchList: hipEventCreateWithFlags");
    events_.push_back(ev);
    auto op = [ev, a, b](const hipStream_t* s) {
      TORCH_CHECK(hipEventRecord(ev, s[a]) == hipSuccess, "LaunchList: event record");
      TORCH_CHECK(hipStreamWaitEvent(s[b], ev, 0) == hipSuccess, "LaunchList: stream wait");
    };
    op(rec_);
    ops_.push_back(op);
  }

  void run(int64_t main, int64_t side) {
    const hipStream_t s[2] = {reinterpret_cast<hipStream_t>(main), reinterpret_cast<hipStream_t>(side)};
    for (const auto& op : ops_) op(s);
  }

  int64_t size() const { return (int64_t)ops_.size(); }

 private:
  int slot_raw(hipStream_t st) const {
    for (int i = 0; i < 2; ++i)
      if (st == rec_[i]) return i;
    TORCH_CHECK(false, "LaunchList: an op on a stream that is neither the list's compute nor its side stream");
    return 0;
  }
  int slot(const at::Tensor& t) const { return slot_raw(stream_of(t)); }
  void hold(std::initializer_list<at::Tensor> ts) {
    for (const auto& t : ts)
      if (t.defined()) keep_.push_back(t);
  }

  hipStream_t rec_[2];
  std::vector<std::function<void(const hipStream_t*)>> ops_;
  std::vector<at::Tensor> keep_;
  std::vector<hipEvent_t> events_;
};

// pos[members[m]] = m: where the dgrad's permuted-rows epilogue puts each lookup's gradient row.
// (members VALUES, a permutation of [0, n), are device-resident: not checked here)
at::Tensor emb_csr_positions(const at::Tensor& members) {
  const int* mp = dev<int>(members, "members");
  at::Tensor pos = at::empty_like(members);
  DeviceGuard g(gpu_of(members, "members"));
  minips_k::emb_csr_positions(mp, members.numel(), pos.data_ptr<int>(), stream_of(members));
  return pos;
}

// The rank's native RCCL data plane (csrc/comm/rccl_comm.h) over torch tensors: each call is one
// enqueue on the tensors' current HIP stream (minips_amd/ps/comm.py Comm uses it for every
// collective of the step when the backend is RCCL).
int rccl_dtype(const at::Tensor& t) {
  switch (t.scalar_type()) {
    case at::kChar: case at::kByte: case at::kBool: return minips::RcclComm::kI8;
    case at::kInt: return minips::RcclComm::kI32;
    case at::kLong: return minips::RcclComm::kI64;
    case at::kHalf: return minips::RcclComm::kF16;
    case at::kBFloat16: return minips::RcclComm::kBF16;
    case at::kFloat: return minips::RcclComm::kF32;
    case at::kDouble: return minips::RcclComm::kF64;
    default: TORCH_CHECK(false, "rccl: dtype ", t.scalar_type());
  }
  return 0;
}

class PyRccl {
 public:
  // (id: the 128 raw bytes of the unique id; pybind converts Python bytes to std::string before
  // the GIL is released around the communicator's rendezvous)
  PyRccl(const std::string& lib, const std::string& id, int64_t world, int64_t rank, int64_t device, double timeout_s,
         bool teardown)
      : c_(lib, id, (int)world, (int)rank, (int)device, timeout_s, teardown) {}
  // out / inp: row-major [rows, ...] (a row = one element of a 1-D tensor); splits in rows
  void all_to_all_v(const at::Tensor& out, const at::Tensor& inp, const std::vector<int64_t>& recv,
                    const std::vector<int64_t>& send) {
    TORCH_CHECK(out.scalar_type() == inp.scalar_type(), "rccl all_to_all_v: dtypes differ");
    const int64_t row = inp.dim() > 1 ? inp[0].numel() * inp.element_size() : inp.element_size();
    int64_t ns = 0, nr = 0;
    for (int64_t v : send) ns += v;
    for (int64_t v : recv) nr += v;
    void *ip = dev_bytes(inp, "inp", ns * row), *op = dev_bytes(out, "out", nr * row);
    const hipStream_t s = stream_of(inp);
    py::gil_scoped_release rel;
    c_.AllToAllV(ip, send, op, recv, row, s);
  }
  void all_to_all(const at::Tensor& out, const at::Tensor& inp) {
    const int64_t nb = inp.numel() * inp.element_size();
    TORCH_CHECK(nb % c_.world() == 0 && out.numel() * out.element_size() == nb, "rccl all_to_all: equal blocks");
    void *ip = dev_bytes(inp, "inp", nb), *op = dev_bytes(out, "out", nb);
    const hipStream_t s = stream_of(inp);
    py::gil_scoped_release rel;
    c_.AllToAll(ip, op, nb / c_.world(), s);
  }
  void reduce_scatter(const at::Tensor& out, const at::Tensor& inp) {
    TORCH_CHECK(inp.numel() == out.numel() * c_.world() && inp.scalar_type() == out.scalar_type(),
                "rccl reduce_scatter: inp = world x out");
    void *ip = dev_bytes(inp, "inp"), *op = dev_bytes(out, "out");
    const hipStream_t s = stream_of(inp);
    py::gil_scoped_release rel;
    c_.ReduceScatter(ip, op, out.numel(), rccl_dtype(out), s);
  }
  void all_gather(const at::Tensor& out, const at::Tensor& inp) {
    TORCH_CHECK(out.numel() == inp.numel() * c_.world() && inp.scalar_type() == out.scalar_type(),
                "rccl all_gather: out = world x inp");
    void *ip = dev_bytes(inp, "inp"), *op = dev_bytes(out, "out");
    const hipStream_t s = stream_of(inp);
    py::gil_scoped_release rel;
    c_.AllGather(ip, op, inp.numel(), rccl_dtype(inp), s);
  }
  void all_reduce(const at::Tensor& t, int64_t op) {
    void* p = dev_bytes(t, "t");
    const hipStream_t s = stream_of(t);
    py::gil_scoped_release rel;
    c_.AllReduce(p, p, t.numel(), rccl_dtype(t), (int)op, s);
  }
  std::string async_error() { return c_.AsyncError(); }
  void abort(const std::string& why) { c_.Abort(why); }
  bool aborted() const { return c_.aborted(); }

 private:
  minips::RcclComm c_;
};

// The owner side of the asynchronous PS on a GPU rank: minips::AsyncServer (the server thread,
// csrc/runtime/async_server.h) driving a HipApplier (the optimizer kernels on the owner's own
// stream). Table buffers are passed as raw device addresses; the Python table keeps them alive
// and stops the server before freeing them.
class GpuAsyncServer {
 public:
  GpuAsyncServer(const std::string& board, int64_t world, int64_t rank, int64_t tables, int64_t device)
      : device_((int)device), applier_((int)device, (int)tables),
        server_(board, (int)world, (int)rank, (int)tables, &applier_) {
    pub_ = std::thread([this] { PublishLoop(); });
  }
  ~GpuAsyncServer() {
    {
      std::lock_guard<std::mutex> lk(pmu_);
      pstop_ = true;
    }
    pcv_.notify_all();
    if (pub_.joinable()) pub_.join();
    server_.Stop();
  }

  // Requester side: publish sent[t] = c once the work issued so far on the tensor's current
  // stream (the clock's pushes) has completed -- an event waited for by a native thread, so no
  // Python thread (and no GIL hand-off) sits between the GPU and the board.
  void publish_after(int64_t t, int64_t c, const at::Tensor& on) {
    DeviceGuard guard(gpu_of(on, "on"));
    hipEvent_t e;
    TORCH_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess, "publish_after: event");
    TORCH_CHECK(hipEventRecord(e, stream_of(on)) == hipSuccess, "publish_after: record");
    {
      std::lock_guard<std::mutex> lk(pmu_);
      pq_.push_back({e, (int)t, c});
      ++queued_;
    }
    pcv_.notify_one();
  }
  int64_t published() const { return published_.load(); }
  int64_t queued() {
    std::lock_guard<std::mutex> lk(pmu_);
    return queued_;
  }

  void set_error_word(int64_t err) { applier_.SetErrorWord(reinterpret_cast<uint32_t*>(err)); }

  void add_sparse(int64_t t, int64_t opt, int64_t table, int64_t ld, int64_t W, int64_t state, int64_t state2,
                  int64_t D1, int64_t base, double lr, double eps, int64_t cap, int64_t inbox, int64_t slot_bytes,
                  int64_t depth, int64_t bf16, int64_t seed, int64_t hash_cap, int64_t hkeys, int64_t lock, int64_t rs,
                  bool coalesce) {
    TORCH_CHECK(cap % 2 == 0 && slot_bytes % 256 == 0 && depth >= 1, "sparse inbox layout");
    TORCH_CHECK(slot_bytes >= minips_k::kPsSlotHeader + cap * (8 + 4 * W), "sparse inbox slot too small");
    TORCH_CHECK(opt == minips_k::kPsAdd || opt == minips_k::kPsSgd || opt == minips_k::kPsRowwiseAdagrad,
                "sparse optimizer ", opt);
    TORCH_CHECK(opt != minips_k::kPsRowwiseAdagrad || state != 0, "row-wise Adagrad needs its state");
    minips_k::PsSparseDesc d;
    d.opt = (int)opt;
    d.table = reinterpret_cast<float*>(table);
    d.ld = ld;
    d.W = (int)W;
    d.state = reinterpret_cast<float*>(state);
    d.state2 = reinterpret_cast<float*>(state2);
    d.D1 = (int)D1;
    d.base = base;
    d.lr = (float)lr;
    d.eps = (float)eps;
    d.cap = cap;
    d.inbox = reinterpret_cast<char*>(inbox);
    d.slot_bytes = slot_bytes;
    d.depth = (int)depth;
    d.bf16 = (int)bf16;
    d.seed = (uint32_t)seed;
    d.hash_cap = hash_cap;
    d.hkeys = reinterpret_cast<unsigned long long*>(hkeys);
    d.lock = reinterpret_cast<uint32_t*>(lock);
    d.flush = lock ? reinterpret_cast<uint32_t*>(lock) + 1 : nullptr;
    TORCH_CHECK(!bf16 || (W == 16 || W == 32 || W == 64), "bf16 rows hold 16, 32 or 64 values");
    TORCH_CHECK(hash_cap == 0 || ((hash_cap & (hash_cap - 1)) == 0 && hkeys), "hash capacity: a power of two");
    d.rs = reinterpret_cast<void*>(rs);
    TORCH_CHECK(!coalesce || opt != minips_k::kPsRowwiseAdagrad || hash_cap != 0 || rs != 0,
                "clock-coalesced row-wise Adagrad needs its (stamp, index) table");
    TORCH_CHECK(cap < (int64_t)INT32_MAX, "sparse inbox capacity");
    TORCH_CHECK(rs == 0 || (W % 4 == 0 && W <= 64), "clock-coalesced sparse rows: W % 4 == 0, W <= 64");
    applier_.SetSparse((int)t, d);
    server_.SetCoalesce((int)t, coalesce);
    server_.Enable((int)t);
  }

  void add_dense(int64_t t, int64_t opt, int64_t w, int64_t m, int64_t v, int64_t wb, int64_t n, double lr, double b1,
                 double b2, double eps, double wd, int64_t step, int64_t inbox, int64_t slot_bytes, int64_t depth,
                 int64_t lock, int64_t sum, int64_t sum_active, bool coalesce) {
    TORCH_CHECK(slot_bytes % 256 == 0 && depth >= 1 && n % 4 == 0, "dense inbox layout");
    TORCH_CHECK(slot_bytes >= minips_k::kPsSlotHeader + 4 * n, "dense inbox slot too small");
    TORCH_CHECK(opt != minips_k::kPsRowwiseAdagrad, "dense optimizer ", opt);
    TORCH_CHECK((opt != minips_k::kPsAdam || (m && v)) && (opt != minips_k::kPsAdagrad || m), "optimizer state");
    minips_k::PsDenseDesc d;
    d.opt = (int)opt;
    d.w = reinterpret_cast<float*>(w);
    d.m = reinterpret_cast<float*>(m);
    d.v = reinterpret_cast<float*>(v);
    d.wb = reinterpret_cast<bf16_t*>(wb);
    d.n = n;
    d.lr = (float)lr;
    d.b1 = (float)b1;
    d.b2 = (float)b2;
    d.eps = (float)eps;
    d.wd = (float)wd;
    d.step = step;
    d.inbox = reinterpret_cast<char*>(inbox);
    d.slot_bytes = slot_bytes;
    d.depth = (int)depth;
    d.lock = reinterpret_cast<uint32_t*>(lock);
    d.flush = lock ? reinterpret_cast<uint32_t*>(lock) + 1 : nullptr;
    d.sum = reinterpret_cast<float*>(sum);
    d.sum_active = reinterpret_cast<int64_t*>(sum_active);
    TORCH_CHECK(!coalesce || opt == minips_k::kPsAdd || opt == minips_k::kPsSgd || (sum && sum_active),
                "clock-coalesced Adam / Adagrad needs the sum buffer");
    applier_.SetDense((int)t, d);
    server_.SetCoalesce((int)t, coalesce);
    server_.Enable((int)t);
  }

  int64_t step(int64_t t) const { return applier_.Step((int)t); }
  void set_step(int64_t t, int64_t s) { applier_.SetStep((int)t, s); }
  void start() { server_.Start(); }
  void stop() { server_.Stop(); }
  void pause() { server_.Pause(); }
  void resume() { server_.Resume(); }
  bool running() const { return server_.Running(); }
  std::string error() const { return server_.Error(); }
  void set_log(bool on) { server_.SetLog(on); }
  std::vector<int64_t> take_log() { return server_.TakeLog(); }
  int64_t applied() const { return server_.Applied(); }
  int64_t batches() const { return server_.Batches(); }
  std::string publish_error() {
    std::lock_guard<std::mutex> lk(pmu_);
    return perr_;
  }

 private:
  struct Pub {
    hipEvent_t e;
    int t;
    int64_t c;
  };
  void PublishLoop() {
    (void)hipSetDevice(device_);
    for (;;) {
      Pub p;
      {
        std::unique_lock<std::mutex> lk(pmu_);
        pcv_.wait(lk, [&] { return pstop_ || !pq_.empty(); });
        if (pq_.empty()) return;  // stop requested and nothing left
        p = pq_.front();
        pq_.pop_front();
      }
      const hipError_t err = hipEventSynchronize(p.e);
      (void)hipEventDestroy(p.e);
      {
        std::lock_guard<std::mutex> lk(pmu_);
        if (err != hipSuccess && perr_.empty()) perr_ = std::string("publish: ") + hipGetErrorString(err);
        // never publish a clock whose pushes did not complete, nor any later one
        if (!perr_.empty()) continue;
      }
      server_.board().PublishSent(p.t, p.c);
      published_.fetch_add(1);
    }
  }

  int device_;
  minips_k::HipApplier applier_;
  minips::AsyncServer server_;
  std::thread pub_;
  std::mutex pmu_;
  std::condition_variable pcv_;
  std::deque<Pub> pq_;
  bool pstop_ = false;
  int64_t queued_ = 0;
  std::atomic<int64_t> published_{0};
  std::string perr_;
};

// rowptr VALUES (ranges of cols / vals), cols VALUES (< d) and assign VALUES (< k) are
// device-resident: not checked here
void kmeans_assign_csr(const at::Tensor& rowptr, const at::Tensor& cols, const at::Tensor& vals, const at::Tensor& C,
                       at::Tensor& cnorm, at::Tensor& assign, const OptTensor& dist) {
  const int64_t* rp = dev<int64_t>(rowptr, "rowptr", 1);
  const int64_t n = rowptr.numel() - 1;
  TORCH_CHECK(C.dim() == 2 && cnorm.numel() == C.size(0) && assign.numel() == n && cols.numel() == vals.numel(),
              "kmeans_csr shapes: C, cnorm, assign, cols / vals");
  TORCH_CHECK(!present(dist) || dist->numel() == n, "dist must be [n]");
  DeviceGuard g(gpu_of(C, "C"));
  minips_k::kmeans_assign_csr(rp, dev<int64_t>(cols, "cols"), dev<float>(vals, "vals"), n, dev<float>(C, "C"),
                              (int)C.size(0), C.size(1), dev<float>(cnorm, "cnorm"), dev<int32_t>(assign, "assign"),
                              dev_opt<float>(dist, "dist", n), stream_of(C));
}

void kmeans_csr_accum(const at::Tensor& rowptr, const at::Tensor& cols, const at::Tensor& vals,
                      const at::Tensor& assign, at::Tensor& sums) {
  const int64_t* rp = dev<int64_t>(rowptr, "rowptr", 1);
  const int64_t n = rowptr.numel() - 1;
  TORCH_CHECK(sums.dim() == 2 && assign.numel() == n, "kmeans_csr_accum shapes: sums, assign");
  DeviceGuard g(gpu_of(sums, "sums"));
  minips_k::kmeans_csr_accum(rp, dev<int64_t>(cols, "cols"), dev<float>(vals, "vals", cols.numel()), n,
                             dev<int32_t>(assign, "assign"), sums.size(1), dev<float>(sums, "sums"), stream_of(sums));
}

}  // namespace


PYBIND11_MODULE(_kernels, m) {
  m.doc() = "minips_amd gfx950 HIP kernels";
  m.attr("EPI_STORE_F32") = (int)minips_k::kEpiStoreF32;
  m.attr("EPI_ATOMIC_F32") = (int)minips_k::kEpiAtomicF32;
  m.attr("EPI_BIAS_RELU_BF16") = (int)minips_k::kEpiBiasReluBf16;
  m.attr("EPI_BIAS_BF16") = (int)minips_k::kEpiBiasBf16;
  m.attr("EPI_STORE_BF16") = (int)minips_k::kEpiStoreBf16;
  m.attr("EPI_RELU_MASK_BF16") = (int)minips_k::kEpiReluMaskBf16;
  m.attr("EPI_BIAS_GELU_BF16") = (int)minips_k::kEpiBiasGeluBf16;
  m.attr("EPI_BIAS_GELU_AUX_BF16") = (int)minips_k::kEpiBiasGeluAuxBf16;
  m.attr("EPI_GELU_GRAD_BF16") = (int)minips_k::kEpiGeluGradBf16;
  m.def("gemm", &gemm, py::arg("A"), py::arg("B"), py::arg("C"), py::arg("M"), py::arg("N"), py::arg("K"),
        py::arg("a_km"), py::arg("b_kn"), py::arg("epi"), py::arg("bias"), py::arg("mask"), py::arg("colsum"),
        py::arg("alpha") = 1.0, py::arg("split_k") = 1, py::arg("batch") = 1, py::arg("inner") = 1,
        py::arg("lda") = 0, py::arg("ldb") = 0, py::arg("ldc") = 0, py::arg("strides") = std::vector<int64_t>(),
        py::arg("perm") = py::none(), py::arg("seg") = 0, py::arg("tile") = 0);
  m.def("layernorm_fwd", &layernorm_fwd);
  m.def("layernorm_bwd", &layernorm_bwd);
  m.def("softmax_xent", &softmax_xent);
  m.def("new_stream", &new_stream);
  m.def("causal_softmax_fwd", &causal_softmax_fwd);
  m.def("causal_softmax_bwd", &causal_softmax_bwd);
  m.def("gelu_bwd", &gelu_bwd);
  m.def("add_bf16", &add_bf16);
  m.def("dlrm_interact_fwd", &dlrm_interact_fwd);
  m.def("dlrm_interact_bwd", &dlrm_interact_bwd);
  m.def("unique_bucketize", &unique_bucketize, py::arg("keys"), py::arg("bounds"), py::arg("F") = 1,
        py::arg("route_mult") = 0, py::arg("route_n") = 0, py::arg("extra_zero_ints") = 0,
        py::arg("csr_counts") = false);
  m.def("gather_rows", &gather_rows, py::arg("table"), py::arg("keys"), py::arg("base"), py::arg("out"),
        py::arg("n_dev") = py::none());
  m.def("scatter_add_rows", &scatter_add_rows);
  m.def("lookup_rows", &lookup_rows);
  m.def("embed_fwd", &embed_fwd);
  m.def("hash_slots", &hash_slots, py::arg("tab_keys"), py::arg("q"), py::arg("slots"), py::arg("vals"),
        py::arg("init_scale"), py::arg("seed"), py::arg("counters"), py::arg("n_dev") = py::none());
  m.def("hash_rehash", &hash_rehash);
  m.def("attn_fwd", &attn_fwd);
  m.def("attn_bwd", &attn_bwd);
  m.def("embed_bwd", &embed_bwd);
  m.def("sparse_rowwise_adagrad", &sparse_rowwise_adagrad, py::arg("table"), py::arg("state"), py::arg("state2"),
        py::arg("D1"), py::arg("keys"), py::arg("base"), py::arg("grads"), py::arg("lr"), py::arg("eps"),
        py::arg("n_dev") = py::none(), py::arg("zero_g") = false);
  m.def("sparse_sgd", &sparse_sgd, py::arg("table"), py::arg("keys"), py::arg("base"), py::arg("grads"),
        py::arg("scale"), py::arg("n_dev") = py::none());
  m.def("embedding_bag_fwd", &embedding_bag_fwd);
  m.def("embedding_bag_bwd", &embedding_bag_bwd);
  m.def("wd_assemble", &wd_assemble, py::arg("dense"), py::arg("rows"), py::arg("inv"), py::arg("F"),
        py::arg("D"), py::arg("X"), py::arg("wide_logit"), py::arg("ones_col") = -1, py::arg("zero") = py::none());
  m.def("wd_head", &wd_head, py::arg("H"), py::arg("w"), py::arg("b0"), py::arg("wide_logit"), py::arg("labels"),
        py::arg("dH"), py::arg("dw"), py::arg("db"), py::arg("dwide"), py::arg("loss_sum"), py::arg("dH_colsum"),
        py::arg("grad_scale"), py::arg("defer_fold") = false);
  m.def("wd_head_fold", &wd_head_fold);
  m.def("wd_assemble_tab", &wd_assemble_tab);
  m.def("owner_slots", &owner_slots, py::arg("own_inv"), py::arg("splits"), py::arg("cap"));
  m.def("owner_rows_adagrad", &owner_rows_adagrad, py::arg("table"), py::arg("state"), py::arg("state2"),
        py::arg("D1"), py::arg("keys"), py::arg("n"), py::arg("n_dev"), py::arg("base"), py::arg("recv"),
        py::arg("P"), py::arg("slots"), py::arg("lr"), py::arg("eps"));
  m.def("owner_push_adagrad", &owner_push_adagrad, py::arg("table"), py::arg("state"), py::arg("state2"),
        py::arg("D1"), py::arg("keys"), py::arg("base"), py::arg("recv"), py::arg("splits"), py::arg("rs"),
        py::arg("stamp"), py::arg("lr"), py::arg("eps"));
  m.def("wd_emb_backward", &wd_emb_backward, py::arg("dX"), py::arg("dwide"), py::arg("inv"), py::arg("F"),
        py::arg("D"), py::arg("grad_rows"), py::arg("x_off") = 0, py::arg("members") = py::none(),
        py::arg("memrow") = py::none(), py::arg("sorted_rows") = false);
  m.def("colsum_bf16", &colsum_bf16);
  m.def("plan_sorted", &plan_sorted, py::arg("keys"), py::arg("col_base"), py::arg("col_bits"),
        py::arg("col_bits_host"), py::arg("route_mult"), py::arg("route_n"), py::arg("bounds"),
        py::arg("with_positions") = false);
  m.def("emb_build_csr", &emb_build_csr, py::arg("inv"), py::arg("F"), py::arg("U"), py::arg("zeroed") = py::none(),
        py::arg("counts_ready") = false);
  m.def("adam_apply", &adam_apply, py::arg("w"), py::arg("m"), py::arg("v"), py::arg("g"), py::arg("lr"),
        py::arg("beta1"), py::arg("beta2"), py::arg("eps"), py::arg("weight_decay"), py::arg("step"),
        py::arg("grad_scale"), py::arg("w_bf16"), py::arg("step_dev") = py::none(), py::arg("zero_g") = false,
        py::arg("slabs") = SlabList());
  m.def("gemm_slab", &gemm_slab);
  m.def("sgd_apply", &sgd_apply);
  m.def("adagrad_apply", &adagrad_apply);
  m.def("cast_f32_bf16", &cast_f32_bf16);
  m.def("lr_sparse_step", &lr_sparse_step);
  m.def("kmeans_assign", &kmeans_assign);
  m.def("kmeans_split3", &kmeans_split3);
  m.def("kmeans_argmin", &kmeans_argmin);
  m.def("criteo_synth", &criteo_synth);
  m.def("multi_copy", &multi_copy);
  m.def("slab_pack", &slab_pack);
  m.def("emu_sum_slices", &emu_sum_slices);
  m.def("emu_rebase", &emu_rebase);
  m.def("wire_spin", [](int64_t ticks, int64_t blocks, int64_t stream) {
    minips_k::wire_spin((int)ticks, (int)blocks,
                       stream ? reinterpret_cast<hipStream_t>(stream)
                              : c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream());
  });
  m.def("clock_probe", &clock_probe, py::arg("out"), py::arg("spin_ticks") = 2000, py::arg("stream") = 0);
  m.def("bitmap_plan", &bitmap_plan, py::arg("keys"), py::arg("bounds"), py::arg("num_rows"), py::arg("route_mult"),
        py::arg("route_n"), py::arg("oor") = py::none());
  m.def("uniform_synth", &uniform_synth);
  m.def("ipc_alloc", &ipc_alloc, py::arg("nbytes"), py::arg("device"), py::arg("kind") = 0);
  m.def("kmeans_assign_csr", &kmeans_assign_csr);
  m.def("kmeans_csr_accum", &kmeans_csr_accum);
  m.def("ipc_open", &ipc_open);
  m.def("ps_push_rows", &ps_push_rows, py::arg("uniq"), py::arg("counts"), py::arg("U_dev"), py::arg("n"),
        py::arg("g"), py::arg("inbox"), py::arg("slot_off"), py::arg("cap"));
  m.def("ps_set_headers", &ps_set_headers);
  m.def("ps_push_dense", &ps_push_dense, py::arg("grad"), py::arg("inbox"), py::arg("data_off"), py::arg("S"),
        py::arg("slabs") = SlabList());
  m.def("ps_gather_rows_bf16tab", &ps_gather_rows<true>, py::arg("bases"), py::arg("bounds"), py::arg("keys"),
        py::arg("n_dev"), py::arg("W"), py::arg("out"));
  m.def("ps_hash_gather", &ps_hash_gather, py::arg("hkeys"), py::arg("hvals"), py::arg("bounds"), py::arg("cap"),
        py::arg("keys"), py::arg("n_dev"), py::arg("W"), py::arg("out"));
  m.def("ps_pull", &ps_pull);
  m.def("ps_set_fences", [](bool on) { minips_k::ps_set_fences(on); });
  m.def("ps_read_lock", &ps_read_lock);
  m.def("ps_read_unlock", &ps_read_unlock);
  m.attr("PS_CTRL_BYTES") = minips_k::kPsCtrlBytes;
  m.attr("PS_CTRL_LINE") = minips_k::kPsCtrlLine;
  m.attr("PS_HELD_SLOTS") = minips_k::kPsHeldSlots;
  m.def("rccl_unique_id", [](const std::string& lib) { return py::bytes(minips::RcclComm::UniqueId(lib)); });
  py::class_<PyRccl>(m, "Rccl")
      .def(py::init<const std::string&, const std::string&, int64_t, int64_t, int64_t, double, bool>(),
           py::arg("lib"), py::arg("unique_id"), py::arg("world"), py::arg("rank"), py::arg("device"),
           py::arg("timeout_s") = 60.0, py::arg("teardown") = false, py::call_guard<py::gil_scoped_release>())
      .def("all_to_all_v", &PyRccl::all_to_all_v)
      .def("all_to_all", &PyRccl::all_to_all)
      .def("reduce_scatter", &PyRccl::reduce_scatter)
      .def("all_gather", &PyRccl::all_gather)
      .def("all_reduce", &PyRccl::all_reduce)
      .def("async_error", &PyRccl::async_error)
      .def("abort", &PyRccl::abort, py::arg("why") = "aborted by the caller",
           py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("aborted", &PyRccl::aborted);
  py::class_<LaunchList>(m, "LaunchList")
      .def(py::init<int64_t, int64_t>())
      .def("gemm", &LaunchList::gemm)
      .def("gemm_slab", &LaunchList::gemm_slab)
      .def("colsum_bf16", &LaunchList::colsum_bf16)
      .def("wd_head_fold", &LaunchList::wd_head_fold)
      .def("fork", &LaunchList::fork)
      .def("run", &LaunchList::run)
      .def("size", &LaunchList::size);
  py::class_<FastEvent>(m, "FastEvent")
      .def(py::init<>())
      .def("record", &FastEvent::record)
      .def("wait", &FastEvent::wait)
      .def("query", &FastEvent::query)
      .def("synchronize", &FastEvent::synchronize);
  py::class_<HostWord>(m, "HostWord")
      .def(py::init<>())
      .def_property_readonly("value", &HostWord::value)
      .def("clear", &HostWord::clear)
      .def_property_readonly("device_ptr", &HostWord::device_ptr);
  m.def("emb_csr_positions", &emb_csr_positions);
  m.def("sparse_apply_bf16", &sparse_apply_bf16);
  m.attr("EPI_PERM_ROWS_BF16") = (int)minips_k::kEpiPermRowsBf16;
  m.def("ps_gather_rows", &ps_gather_rows<false>, py::arg("bases"), py::arg("bounds"), py::arg("keys"),
        py::arg("n_dev"), py::arg("W"), py::arg("out"));
  m.attr("PS_ADD") = (int)minips_k::kPsAdd;
  m.attr("PS_SGD") = (int)minips_k::kPsSgd;
  m.attr("PS_ROWWISE_ADAGRAD") = (int)minips_k::kPsRowwiseAdagrad;
  m.attr("PS_ADAGRAD") = (int)minips_k::kPsAdagrad;
  m.attr("PS_ADAM") = (int)minips_k::kPsAdam;
  py::class_<GpuAsyncServer>(m, "AsyncServer")
      .def(py::init<const std::string&, int64_t, int64_t, int64_t, int64_t>(), py::arg("board"), py::arg("world"),
           py::arg("rank"), py::arg("tables"), py::arg("device"))
      .def("add_sparse", &GpuAsyncServer::add_sparse, py::arg("t"), py::arg("opt"), py::arg("table"), py::arg("ld"),
           py::arg("W"), py::arg("state"), py::arg("state2"), py::arg("D1"), py::arg("base"), py::arg("lr"),
           py::arg("eps"), py::arg("cap"), py::arg("inbox"), py::arg("slot_bytes"), py::arg("depth"), py::arg("bf16"),
           py::arg("seed"), py::arg("hash_cap"), py::arg("hkeys"), py::arg("lock"), py::arg("rs") = 0,
           py::arg("coalesce") = false)
      .def("set_error_word", &GpuAsyncServer::set_error_word)
      .def("publish_after", &GpuAsyncServer::publish_after)
      .def_property_readonly("published", &GpuAsyncServer::published)
      .def_property_readonly("queued", &GpuAsyncServer::queued)
      .def("publish_error", &GpuAsyncServer::publish_error)
      .def("add_dense", &GpuAsyncServer::add_dense, py::arg("t"), py::arg("opt"), py::arg("w"), py::arg("m"),
           py::arg("v"), py::arg("wb"), py::arg("n"), py::arg("lr"), py::arg("b1"), py::arg("b2"), py::arg("eps"),
           py::arg("wd"), py::arg("step"), py::arg("inbox"), py::arg("slot_bytes"), py::arg("depth"), py::arg("lock"),
           py::arg("sum") = 0, py::arg("sum_active") = 0, py::arg("coalesce") = false)
      .def("step", &GpuAsyncServer::step)
      .def("set_step", &GpuAsyncServer::set_step)
      .def("start", &GpuAsyncServer::start)
      .def("stop", &GpuAsyncServer::stop, py::call_guard<py::gil_scoped_release>())
      .def("pause", &GpuAsyncServer::pause, py::call_guard<py::gil_scoped_release>())
      .def("resume", &GpuAsyncServer::resume)
      .def("running", &GpuAsyncServer::running)
      .def("error", &GpuAsyncServer::error)
      .def("set_log", &GpuAsyncServer::set_log)
      .def("take_log", &GpuAsyncServer::take_log)
      .def_property_readonly("applied", &GpuAsyncServer::applied)
      .def_property_readonly("batches", &GpuAsyncServer::batches);
}
