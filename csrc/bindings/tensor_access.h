// Checked typed accessors: the ONLY way a binding in ops_py.cpp turns a torch tensor into a device
// pointer. The cast and its checks are one call, so no op can take a pointer it did not validate:
//   dev<T>(t, "name", n)              GPU tensor of T's dtype, contiguous, >= n elements
//   dev_rows<T>(t, "name", rows, cols) GPU 2-D tensor of T's dtype with unit column stride (a row-major matrix
//                                     whose leading dimension, stride(0), may be padded), >= rows x cols
//   dev_mat<T>(t, "name", n)          a GEMM operand: dev_rows' layout if 2-D, else contiguous (flat batched buffers)
//   dev_opt<T>(opt, "name", n)        nullptr when absent / undefined, otherwise dev<T>
//   dev_opt_strided<T>(opt, "name", n) the same for a 1-D view of any positive stride (the caller reads stride(0))
//   dev_rows_any(t, "name", &bf16, rows, cols)  contiguous fp32 or bf16 rows; says which it found
//   dev_bytes(t, "name", nbytes)      any dtype (copies and collectives): GPU, contiguous, >= nbytes
//   parse_slabs(list, n, "op")        the split-K slab list of a dense-clock op -> AdamSlabs inside n elements
// stream_of(t) is the current HIP stream of t's device, aligned16(t, "name") the 16-byte check of float4 kernels.
// The element counts are what the kernel will address, stated where the pointer is taken. The dtype
// follows from T (dtype_of), never from a second argument that could disagree with the cast.
#pragma once

#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <tuple>
#include <vector>

#include "../kernels/kernels.h"

namespace minips_access {

using minips_k::bf16_t;

template <typename T>
struct dtype_of;
template <> struct dtype_of<float> { static constexpr at::ScalarType value = at::kFloat; };
template <> struct dtype_of<double> { static constexpr at::ScalarType value = at::kDouble; };
template <> struct dtype_of<bf16_t> { static constexpr at::ScalarType value = at::kBFloat16; };
template <> struct dtype_of<int64_t> { static constexpr at::ScalarType value = at::kLong; };
template <> struct dtype_of<int32_t> { static constexpr at::ScalarType value = at::kInt; };
template <> struct dtype_of<uint8_t> { static constexpr at::ScalarType value = at::kByte; };
template <> struct dtype_of<int16_t> { static constexpr at::ScalarType value = at::kShort; };

inline bool present(const c10::optional<at::Tensor>& t) { return t.has_value() && t->defined(); }

// the device of an op's guard: checked here because the guard is set before the launch arguments are built
inline c10::Device gpu_of(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  return t.device();
}

inline void check_dev_dtype(const at::Tensor& t, at::ScalarType dt, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == dt, name, " has dtype ", t.scalar_type(), ", expected ", dt);
}

inline void check_numel(const at::Tensor& t, int64_t n, const char* name) {
  TORCH_CHECK(n >= 0 && t.numel() >= n, name, " holds ", t.numel(), " elements, the kernel addresses ", n);
}

inline void check_rows(const at::Tensor& t, int64_t rows, int64_t cols, const char* name) {
  TORCH_CHECK(t.dim() == 2 && t.stride(1) == 1 && (t.size(0) <= 1 || t.stride(0) >= t.size(1)), name,
              " must be a row-major matrix (unit column stride)");
  TORCH_CHECK(rows >= 0 && cols >= 0 && t.size(0) >= rows && t.size(1) >= cols, name, " has shape ", t.sizes(),
              ", the kernel addresses [", rows, ", ", cols, "]");
}

template <typename T>
T* dev(const at::Tensor& t, const char* name, int64_t n = 0) {
  check_dev_dtype(t, dtype_of<T>::value, name);
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  check_numel(t, n, name);
  return static_cast<T*>(t.data_ptr());
}

template <typename T>
T* dev_rows(const at::Tensor& t, const char* name, int64_t rows = 0, int64_t cols = 0) {
  check_dev_dtype(t, dtype_of<T>::value, name);
  check_rows(t, rows, cols, name);
  return static_cast<T*>(t.data_ptr());
}

// a GEMM operand: a 2-D operand may be a column-sliced view (rows contiguous, ld = stride(0)), the flat
// buffer of a batched GEMM is contiguous; n = the elements the (batched) GEMM addresses in a flat buffer
template <typename T>
T* dev_mat(const at::Tensor& t, const char* name, int64_t n = 0) {
  check_dev_dtype(t, dtype_of<T>::value, name);
  TORCH_CHECK(t.dim() == 2 ? t.stride(1) == 1 : t.is_contiguous(), name, " rows must be contiguous");
  check_numel(t, n, name);
  return static_cast<T*>(t.data_ptr());
}

template <typename T>
T* dev_opt(const c10::optional<at::Tensor>& t, const char* name, int64_t n = 0) {
  return present(t) ? dev<T>(*t, name, n) : nullptr;
}

template <typename T>
T* dev_opt_strided(const c10::optional<at::Tensor>& t, const char* name, int64_t n = 0) {
  if (!present(t)) return nullptr;
  check_dev_dtype(*t, dtype_of<T>::value, name);
  TORCH_CHECK(t->dim() == 1 && t->stride(0) >= 1, name, " must be 1-D with a positive stride");
  check_numel(*t, n, name);
  return static_cast<T*>(t->data_ptr());
}

inline void* dev_rows_any(const at::Tensor& t, const char* name, bool* bf16, int64_t rows = 0, int64_t cols = 0) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  *bf16 = t.scalar_type() == at::kBFloat16;
  TORCH_CHECK(*bf16 || t.scalar_type() == at::kFloat, name, " has dtype ", t.scalar_type(), ", expected fp32 or bf16");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  check_rows(t, rows, cols, name);
  return t.data_ptr();
}

inline void* dev_bytes(const at::Tensor& t, const char* name, int64_t nbytes = 0) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(nbytes >= 0 && t.numel() * (int64_t)t.element_size() >= nbytes, name, " holds ",
              t.numel() * (int64_t)t.element_size(), " bytes, the kernel addresses ", nbytes);
  return t.data_ptr();
}

inline hipStream_t stream_of(const at::Tensor& t) {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}

inline void aligned16(const at::Tensor& t, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
}

// (slab [nsplit * plane] fp32, nsplit, plane, offset of its region in the gradient): split-K planes left
// unreduced by gemm_slab; each region's length is its plane and lies inside [0, region_len). Every message
// names `slabs`, the argument (the validation tables look for it).
using SlabList = std::vector<std::tuple<at::Tensor, int64_t, int64_t, int64_t>>;
inline minips_k::AdamSlabs parse_slabs(const SlabList& slabs, int64_t region_len, const char* what) {
  minips_k::AdamSlabs sl;
  TORCH_CHECK(slabs.size() <= 4, what, ": slabs: at most 4 slab regions");
  for (const auto& t : slabs) {
    const int64_t ns = std::get<1>(t), plane = std::get<2>(t), off = std::get<3>(t);
    TORCH_CHECK(ns >= 1 && ns <= (1 << 20) && plane >= 0 && off >= 0 && off + plane <= region_len, what,
                ": slabs: region bounds (nsplit ", ns, ", plane ", plane, ", offset ", off,
                ") outside a gradient of ", region_len, " elements");
    TORCH_CHECK(plane % 4 == 0 && off % 4 == 0, what, ": slabs: plane ", plane, " and offset ", off,
                " must be multiples of 4");
    sl.p[sl.n] = dev<float>(std::get<0>(t), "slabs plane", ns * plane);
    aligned16(std::get<0>(t), "slabs plane");
    sl.nsplit[sl.n] = (int)ns;
    sl.plane[sl.n] = plane;
    sl.len[sl.n] = plane;
    sl.off[sl.n] = off;
    ++sl.n;
  }
  return sl;
}

}  // namespace minips_access
