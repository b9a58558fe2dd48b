// The FTRL-Proximal coordinate rule as device code (ftrl.h states it), shared by the kernels that apply it:
// ftrl.hip (every column of a row) and wideftrl.hip (the wide columns of a split row). Every operation is
// rounded on its own -- the contraction pragma travels with the function -- so each kernel that inlines it
// computes the bits of ops.sparse_ftrl's CPU reference.
#pragma once

#include <hip/hip_runtime.h>

namespace minips_k {

struct FtrlHyper {
  float alpha, beta, l1, l2;
};

// one coordinate of the rule: every operation is rounded on its own (the CPU reference's sequence)
__device__ __forceinline__ void ftrl_coord(float& w, float& z, float& n, float g, const FtrlHyper h) {
#pragma clang fp contract(off)
  const float g2 = g * g;
  const float n1 = n + g2;
  const float s1 = sqrtf(n1), s0 = sqrtf(n);
  const float den = h.alpha * (s1 + s0);
  const float sigma = den > 0.f ? g2 / den : 0.f;
  const float z1 = z + (g - sigma * w);
  const float shrunk = z1 - copysignf(h.l1, z1);
  const float scale = (h.beta + s1) / h.alpha + h.l2;
  w = fabsf(z1) <= h.l1 ? 0.f : -shrunk / scale;
  z = z1;
  n = n1;
}

__device__ __forceinline__ void ftrl_coord4(float4& w, float4& z, float4& n, const float4 g, const FtrlHyper h) {
  ftrl_coord(w.x, z.x, n.x, g.x, h);
  ftrl_coord(w.y, z.y, n.y, g.y, h);
  ftrl_coord(w.z, z.z, n.z, g.z, h);
  ftrl_coord(w.w, z.w, n.w, g.w, h);
}

}  // namespace minips_k
