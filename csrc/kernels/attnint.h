// AutoInt's interacting layers (Song et al., CIKM 2019) on the Wide & Deep step (attnint.hip; binding in
// csrc/bindings/attn_py.cpp, module minips_amd._aink): T layers of multi-head self-attention with a residual over the
// F field embeddings of a sample, the last layer's output entering the wide logit through one vector.
//
// THE RULE (identical in the kernels and in the CPU references of minips_amd/ops).
//   shapes      m = F fields, 1 <= m <= 32; D = emb_dim, D % 8 == 0, 8 <= D <= 64; 1 <= T <= 3 layers; H heads of size
//               d in {16, 32}, A = H d in {16, 32, 48, 64}; Din_1 = D, Din_l = A for l > 1.
//               E^0_b[j, :] = X[b, j D : j D + D] (bf16; the dense-feature columns take no part).
//   parameters  W^l bf16 [Din_l, 4 A], columns Q | K | V | R (no biases), w_out bf16 [m A].
//   buffers     EK bf16 [B, T, m, A]: E^l_b = EK[b, l - 1]; dEK likewise (dE^l for l < T; slot T - 1 is unused).
//   forward     [Q | K | V] = bf16_rne(E^{l-1} W_QKV): fp32 MFMA accumulation over ascending steps of 32 (inside a step
//               the instruction's own order), one rounding. R = E^{l-1} W_R likewise, kept in fp32.
//               per head h: s_ij = <Q_h[i], K_h[j]> in fp32 (one MFMA step; no 1 / sqrt(d)); only i, j < m exist
//               p_ij = exp(s_ij - max_j s_ij), l_i = sum_{j < m} p_ij, P = bf16_rne(p / l_i). The lane-level order of
//               l_i: a lane adds its j = 4 g + r (g = lane / 16, r = 0 .. 3) and then 16 + 4 g + r in ascending
//               order, the four g are folded by __shfl_xor 16, then 32.
//               E^l = bf16_rne(max(R + P V_h, 0)): the fp32 accumulator starts from R and takes P V_h as one MFMA step.
//               after layer T: wide[b] += sum_o float(w_out[o]) float(E^T_b[o]) over o = i A + a: lane l adds o = l,
//               l + 64, ... in ascending order, the 64 lanes are folded by __shfl_xor 32, 16, 8, 4, 2, 1.
//   backward    only EK is kept: Q, K, V, P are recomputed from E^{l-1} with the forward's roundings.
//               dE^T = bf16_rne(dwide[b] float(w_out)), formed on the fly. For l = T .. 1:
//               dY = dE^l where E^l > 0, else 0;  dV_h = P^T dY_h;  dP = dY_h V_h^T;
//               dS = P o (dP - rowsum(dP o P)) (rowsum in the order of l_i);  dQ_h = dS K_h;  dK_h = dS^T Q_h
//               (dS, dQ, dK, dV rounded to bf16: they are MFMA operands)
//               dE^{l-1} = [dQ | dK | dV | dY] W^{l T} in fp32: each part's share is one MFMA step per head in
//               ascending head order, the shares are added as ((Q + K) + V) + Y; stored bf16 in dEK for l > 1; for
//               l = 1 row r = perm[b F + i] (b F + i without perm) of dX [B F, D] becomes
//               bf16_rne(float(dX[r, c]) + dE^0[i, c]); a perm entry outside [0, B F) is skipped.
//   weights     dW^l = sum_b E^{l-1 T}_b [dQ | dK | dV | dY]_b, dw_out = sum_b dwide[b] E^T_b. Per-chunk partials over
//               attn_chunk(B) consecutive samples, added in ascending order (one MFMA step each for dW^l); dw_out's
//               partial likewise. Partials are folded in chunk order and ADDED into the gradient
//               block in fp32.
//   No float atomics; every output is a function of the inputs alone (same bits for every grid size and run).
//
// KERNELS (wave64, 256 threads = 4 waves; fp32 accumulators; scratch 0 in every instantiation; registers and waves
// per SIMD are the compiler's, profiles/autoint/resources.txt).
//   The mapping rests on one fact about v_mfma_f32_16x16x32_bf16: the accumulator tile of M N^T leaves lane (g, c) with
//   rows 4 g .. 4 g + 3 of column c -- which is, after one bf16 pack of two such tiles, exactly the operand fragment
//   "row c, contraction indices {4 g + r, 16 + 4 g + r}" of the transposed matrix; the order of the contraction index
//   is free as long as both operands agree. So every product's output is the next product's operand in registers, and
//   a matrix that is needed in both orientations (P, dS, the gradients) is produced twice with the operands swapped
//   instead of being transposed through LDS. Q, K, V, S, P and every gradient exist only in VGPRs.
//   attn_fwd<KS, HD>     one wave per sample. KS = ceil(Din / 32) projection steps, HD = d / 16. LDS: W^l transposed,
//                        [4 A][32 KS + 8] bf16 (k >= Din zero; at most 36,864 B), staged element by element once
//                        per workgroup -- no alignment is asked of W or X -- and resident for the workgroup's life.
//                        E^{l-1}'s fragments come straight from global memory (16-byte loads when aligned,
//                        element-wise otherwise). Pad rows and columns (>= m) are masked out of the softmax and
//                        write nothing. Layers are separate launches.
//   attn_bwd<KS, H, HD>  same residency; the four waves of a workgroup carry ONE sample together, wave w owning part w
//                        of [dQ | dK | dV | dY]: it recomputes what its part needs (Q and K for the softmax
//                        statistics, V and dY for dS in parts 0 and 1; the Y wave only loads), forms the part in both
//                        orientations, and keeps the part's A / 16 x 2 KS tiles of dW^l (64 registers at A = Din = 64)
//                        in its accumulators across the chunk's samples: no fold over waves, the chunk's partial is
//                        stored once. dE^{l-1}'s W fragments are gathered from the transposed copy (2-byte LDS reads);
//                        the four shares of dE^{l-1} meet in LDS, lane by lane, behind three barriers per sample (two
//                        samples deep: + 4,096 KS x 2 bytes, at most 53,248 B in all). A workgroup owns whole chunks: a
//                        grid changes how many chunks a workgroup takes, never the order inside one. Every
//                        instantiation takes the full 512 registers of a lane (1 wave per SIMD).
//   attn_out / attn_wout / attn_fold   the wide term, the per-chunk dw_out sums, the in-order fold into G.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace minips_k {

constexpr int kAttnMaxBlocks = 65535;
constexpr int kAttnMaxT = 3;
constexpr int kAttnMaxM = 32;
constexpr int kAttnMaxD = 64;
constexpr int kAttnMaxA = 64;
constexpr int kAttnChunk = 32;       // samples per partial of the batch sums up to kAttnChunk * kAttnMaxChunks samples
constexpr int kAttnMaxChunks = 512;  // the workspace never exceeds 512 copies of a layer's weights (32 MB of fp32)

inline int64_t attn_chunk(int64_t B) {
  if (B <= (int64_t)kAttnChunk * kAttnMaxChunks) return kAttnChunk;
  return ((B + kAttnMaxChunks - 1) / kAttnMaxChunks + 3) / 4 * 4;
}
inline int64_t attn_nchunks(int64_t B) { return (B + attn_chunk(B) - 1) / attn_chunk(B); }

// One layer of the stack: l in [1, T].
struct AttnLayer {
  int m, D, T, H, d, l;
  int A() const { return H * d; }
  int Din() const { return l == 1 ? D : H * d; }
};

// X bf16 [B, ldx] (columns < m D are read, layer 1 only), W bf16 [Din, 4 A], EK bf16 [B, T, m, A] 16-byte aligned
// (slot l - 2 read for l > 1, slot l - 1 written). blocks > 0 forces the grid. B == 0 launches nothing.
void wd_attn_layer_forward(const uint16_t* X, int64_t ldx, int64_t B, const AttnLayer& L, const uint16_t* W,
                           uint16_t* EK, int blocks, hipStream_t stream);

// wide fp32 [B] += <w_out, E^T_b>; w_out bf16 [m A].
void wd_attn_output(const uint16_t* EK, int64_t B, const AttnLayer& L, const uint16_t* w_out, float* wide, int blocks,
                    hipStream_t stream);

// One layer of the backward. dEK bf16 like EK (slot l - 1 read unless l == T, slot l - 2 written unless l == 1), perm
// nullable int32 [B F], dX bf16 [B F, D] 8-byte aligned (updated by l == 1 only), part fp32 [attn_nchunks(B), Din, 4 A]
// 16-byte aligned (written: the chunks' partial dW^l).
void wd_attn_layer_backward(const uint16_t* X, int64_t ldx, int64_t B, const AttnLayer& L, const uint16_t* W,
                            const uint16_t* EK, uint16_t* dEK, const uint16_t* w_out, const float* dwide,
                            const int32_t* perm, uint16_t* dX, float* part, int blocks, hipStream_t stream);

// part fp32 [attn_nchunks(B), m A] (written): the per-chunk sums of dwide[b] E^T_b.
void wd_attn_wout_partial(const uint16_t* EK, int64_t B, const AttnLayer& L, const float* dwide, float* part,
                          hipStream_t stream);

// G[i] += sum over chunks (ascending) of part[chunk, i], i < n.
void wd_attn_fold(const float* part, int64_t nchunks, int64_t n, float* G, hipStream_t stream);

}  // namespace minips_k
