// The dense clock's shared device code: the fold of split-K weight-gradient planes (AdamSlabs) into a
// gradient float4, and the Adam update of one element and of one float4. Every kernel of the dense clock
// takes them from here (optim.hip, gradclip.hip, onesided.hip), so their agreement is structural.
#pragma once

#include "common.h"
#include "kernels.h"

namespace minips_k {

// G = elements [4i, 4i + 4) of the gradient, plus the planes of every region that covers them.
// Two summation orders are shipped behaviour, and each kernel names its own:
//   kGroup4 = true   planes in groups of four as (a0+a1)+(a2+a3), then the remainder one by one:
//                    adam_kernel, adam_clip_kernel, grad_sumsq_kernel (what an Adam consumes)
//   kGroup4 = false  planes one by one: slab_pack_kernel, ps_push_dense_kernel (what a reduce-scatter
//                    or a push ships)
// The two round differently from nsplit >= 4 (equal below: no full group). Changing either order is a
// numerics change.
template <bool kGroup4>
__device__ __forceinline__ float4 slab_fold(float4 G, int64_t i, const AdamSlabs& sl) {
  for (int k = 0; k < sl.n; ++k) {
    const int64_t e = 4 * i - sl.off[k];
    if (e < 0 || e >= sl.len[k]) continue;
    const float* p = sl.p[k] + e;
    int z = 0;
    if constexpr (kGroup4) {
      for (; z + 3 < sl.nsplit[k]; z += 4) {
        const float4 a0 = *reinterpret_cast<const float4*>(p + z * sl.plane[k]);
        const float4 a1 = *reinterpret_cast<const float4*>(p + (z + 1) * sl.plane[k]);
        const float4 a2 = *reinterpret_cast<const float4*>(p + (z + 2) * sl.plane[k]);
        const float4 a3 = *reinterpret_cast<const float4*>(p + (z + 3) * sl.plane[k]);
        G.x += (a0.x + a1.x) + (a2.x + a3.x);
        G.y += (a0.y + a1.y) + (a2.y + a3.y);
        G.z += (a0.z + a1.z) + (a2.z + a3.z);
        G.w += (a0.w + a1.w) + (a2.w + a3.w);
      }
    }
    for (; z < sl.nsplit[k]; ++z) {
      const float4 a = *reinterpret_cast<const float4*>(p + z * sl.plane[k]);
      G.x += a.x;
      G.y += a.y;
      G.z += a.z;
      G.w += a.w;
    }
  }
  return G;
}

// Adam(W) on one element: m, v and w of gradient g * gscale. The rounding is spelled out -- contraction off,
// the fused multiply-adds written as fmaf -- because left to the compiler the choice of which product of
// b2 * v + (1 - b2) * gg * gg is fused changed with the inlining context, and with it the result's last bits.
// These are the fusions of the kernels as shipped: every Adam of the dense clock rounds alike.
__device__ __forceinline__ void adam_update1(float& w, float& m, float& v, float g, float lr, float b1, float b2,
                                             float eps, float wd, float bc1, float bc2, float gscale) {
#pragma clang fp contract(off)
  const float gg = g * gscale;
  m = fmaf(b1, m, (1.f - b1) * gg);
  v = fmaf(gg, (1.f - b2) * gg, b2 * v);
  const float mh = m / bc1, vh = v / bc2;
  w = fmaf(-lr, fmaf(wd, w, mh / (sqrtf(vh) + eps)), w);
}

// Adam(W) on elements [4i, 4i + 4): one pass over w / m / v / g with the split-K planes folded into the
// gradient (no separate reduce pass: this is the kernel that reads the gradient anyway), the bf16 copy
// of the new weights (wb nullable) and, on zero_g, the cleared accumulator of the next clock.
__device__ __forceinline__ void adam_update4(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                             float* __restrict__ g, int64_t i, const AdamSlabs& sl, float lr,
                                             float b1, float b2, float eps, float wd, float bc1, float bc2,
                                             float gscale, bf16_t* __restrict__ wb, bool zero_g) {
  float4 W = reinterpret_cast<float4*>(w)[i], M = reinterpret_cast<float4*>(m)[i];
  float4 V = reinterpret_cast<float4*>(v)[i];
  const float4 G = reinterpret_cast<const float4*>(g)[i];
  const float4 Gs = slab_fold<true>(G, i, sl);
  adam_update1(W.x, M.x, V.x, Gs.x, lr, b1, b2, eps, wd, bc1, bc2, gscale);
  adam_update1(W.y, M.y, V.y, Gs.y, lr, b1, b2, eps, wd, bc1, bc2, gscale);
  adam_update1(W.z, M.z, V.z, Gs.z, lr, b1, b2, eps, wd, bc1, bc2, gscale);
  adam_update1(W.w, M.w, V.w, Gs.w, lr, b1, b2, eps, wd, bc1, bc2, gscale);
  reinterpret_cast<float4*>(w)[i] = W;
  reinterpret_cast<float4*>(m)[i] = M;
  reinterpret_cast<float4*>(v)[i] = V;
  if (wb) reinterpret_cast<uint2*>(wb)[i] = make_uint2(pack_bf2(W.x, W.y), pack_bf2(W.z, W.w));
  if (zero_g) reinterpret_cast<float4*>(g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

}  // namespace minips_k
