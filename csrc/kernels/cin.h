// xDeepFM's Compressed Interaction Network (CIN, Lian et al., 2018) on the Wide & Deep step (cin.hip; binding in
// csrc/bindings/cin_py.cpp, module minips_amd._cink): T layers of explicit vector-wise feature crosses over the F
// field embeddings of the assembled input, every feature map sum-pooled into the wide logit through one vector.
//
// THE RULE (identical in the kernels and in the CPU references of minips_amd/ops).
//   shapes      m = F fields, D = emb_dim, X^0_b[j, c] = X[b, j D + c] (bf16; the dense-feature columns take no part).
//               H_0 = m, 1 <= T <= 3, H_k % 16 == 0, 16 <= H_k <= 128, 1 <= m <= 64, D % 8 == 0, 8 <= D <= 64,
//               mp = align8(m), Hs = H_1 + ... + H_T, o_k = H_1 + ... + H_{k-1}.
//   parameters  W^k bf16 [H_k, H_{k-1}, mp] (columns j >= m are zero and get a zero gradient), w_out bf16 [Hs].
//   buffers     XK bf16 [B, Hs, D]: X^k_b = XK[b, o_k : o_k + H_k, :]; dXK likewise (dX^k for k < T); p fp32 [B, Hs].
//   forward     z = bf16_rne(float(a) float(b)) for a = X^{k-1}[i, c], b = X^0[j, c] (the fp32 product is exact)
//               acc[h, c] = sum_{i, j < m} W^k[h, i, j] z_{ij, c}: fp32, v_mfma_f32_16x16x32_bf16 over the flattened
//               index i mp + j in ascending steps of 32 (inside a step the instruction's own order)
//               X^k = bf16_rne(acc);  p_b[o_k + h] = sum_c float(X^k_b[h, c]) in ascending c on the stored values
//               wide[b] += sum_o float(w_out[o]) p_b[o]: lane l adds o = l, l + 64, ... in ascending order, the 64
//               lanes are folded by __shfl_xor with offsets 32, 16, 8, 4, 2, 1
//   backward    dz = dwide[b]; the output roundings are the identity. For k = T .. 1:
//               dX^T[h, c] = bf16_rne(dz float(w_out[o_T + h])) -- formed on the fly; rounded because it is an MFMA
//               operand (the one rounding the rule adds to the mathematical backward); dX^k for k < T is stored bf16
//               dZ[(i, j), c] = sum_h W^k[h, i, j] dX^k[h, c]: fp32 MFMA over ascending h in steps of 32
//               dX^{k-1}[i, c] = bf16_rne(sum_j dZ[(i, j), c] X^0[j, c] + dz w_out[o_{k-1} + i])   (k > 1)
//               g0[j, c] += sum_i dZ[(i, j), c] X^{k-1}[i, c]; at k = 1 the first sum goes to g0[i, c] as well
//               (the lane-level order of these fp32 sums is the mapping's, below)
//               embedding gradient, once, by the k = 1 kernel: row r = perm[b F + j] (b F + j without perm) of dX
//               [B F, D] becomes bf16_rne(float(dX[r, c]) + g0[j, c]); a perm entry outside [0, B F) is skipped
//   weights     dW^k[h, i, j] = sum_b sum_c dX^k_b[h, c] z_b[(i, j), c] (z regenerated, rounded as in the forward),
//               dw_out[o] = sum_b dz_b p_b[o]. Both as per-chunk partials over cin_chunk(B) consecutive samples
//               (a function of B alone), folded in chunk order and ADDED into the gradient block in fp32.
//   No float atomics; every output is a function of the inputs alone (same bits for every grid size and run).
//
// KERNELS (wave64, 256 threads = 4 waves, one per SIMD; fp32 accumulators; scratch 0 in every instantiation). LDS is
// dynamic; a launch asks for at most 64 KB (kLdsBudget) and takes the largest NT that fits. Registers and waves per
// SIMD below are the compiler's (profiles/cin/resources.txt); a workgroup per CU needs one wave per SIMD.
//   cin_fwd<HT, NT>  HT in {2, 4, 8} >= H_k / 16 row tiles, NT in {4, 2, 1} 16-column tiles per wave: a workgroup owns
//                    NC = 64 NT columns (b, c) -- NC / D whole samples -- as the GEMM's N, a wave 16 NT of them against
//                    all row tiles. X^0 of the tile is resident in LDS transposed ([column][j], 16-byte reads of 8
//                    consecutive j), X^{k-1} as [i][column]. W^k streams in 32-deep K slices through two LDS buffers
//                    [H][32 + 8]; the next slice's global loads are in flight during the MFMAs. The flattened K index
//                    is i mp + j, so a lane's 8 k share one i: the lane forms its B operand from one 16-byte LDS read
//                    of X^0, one bf16 of X^{k-1} and 8 multiplies, and reuses it for every row tile. Z exists only in
//                    VGPRs. Staging is element-wise (no alignment asked of X); W is staged with 16-byte loads when it
//                    is 16-byte aligned, element by element otherwise (the slow form: nothing inside the rule is
//                    refused). LDS 2 (80 H + NC (mp + 8) + NC H_{k-1}) bytes:
//                      m = 26, H = 64:   layer 1 <4,4> 44,032 B, layer 2 (H_1 = 64) <4,4> 63,488 B; 194 VGPR + 64
//                                        AGPR, 1 wave per SIMD: 1 workgroup per CU
//                      m = 26, H = 128:  layer 1 <8,4> 54,272 B (256 + 152, 1 per CU); layer 2 (H_1 = 128) does not fit
//                                        at NT = 4 (106,496 B) and runs <8,2> 63,488 B (203 + 68, 1 per CU)
//                      m = 64, H = 128, H_{k-1} = 128: <8,1> 46,080 B (157 + 32, 2 waves per SIMD, 2 per CU)
//                      H <= 32: <2,4> 146 + 32 registers, 2 per CU while the LDS allows
//   cin_out          one wave per sample: lane l sums the rows l, l + 64, ... of XK[b] (16-byte loads), stores p and
//                    folds the wide term. 29 VGPR, no LDS.
//   cin_bwd<MQ, NT>  W^k transposed: the M index is (i, jj) with jj < MQ = the power of two >= mp (8 .. 64; rows
//                    jj >= mp are zero), 32 rows per step, staged transposed ([row][h]) through two LDS buffers. NT in
//                    {2, 1}: a workgroup owns NC = 64 NT columns, a wave 16 NT; the lane keeps dX^k of its columns as
//                    the B operands (NT x 4 fragments, h padded to 32), its X^0 values and its g0 sums in registers for
//                    the whole sweep: with MQ a power of two a lane's accumulator rows meet the same jj in every
//                    period of max(1, MQ / 32) steps. A dZ tile is contracted at once: dZ X^0 summed over the rows of
//                    one i in the lane (q, then tile, then step ascending), then over the lanes by __shfl_xor 16 (and
//                    32 when MQ >= 16); dZ is never stored. g0 of a column = (the lane's sums over i ascending [+ the
//                    other tile, + the lane 32 away when MQ <= 16 / 8]) + the k = 1 dX^0 term + what the layers above
//                    left in the fp32 workspace g0 [B, m, D] (written by k = T, read by k = 1; unused when T = 1).
//                    LDS 2 (64 (Hpad + 8) + NC H_{k-1}) bytes, + 4 m NC at k = 1 (dX^0's share of g0):
//                      m = 26, H = 64:   <32,2> layer 1 29,184 B, layer 2 25,600 B; 256 VGPR + 35 AGPR, 1 per CU
//                      m = 26, H = 128:  <32,2> layer 1 37,376 B, layer 2 (H_1 = 128) 50,176 B
//                      m = 64, H = 128:  layer 1 does not fit at NT = 2 (66,560 B) and runs <64,1> 41,984 B (256 + 50,
//                                        1 per CU); layer 2 <64,2> 50,176 B (256 + 142, 1 per CU)
//   cin_wgrad<HT>    grid (K / 128 tiles, chunk): a wave owns 32 flattened (i, j) columns against all row tiles and
//                    reduces over the chunk's flattened (b, c) in steps of 32, both operands straight from global
//                    memory (16-byte loads; z formed in registers). No LDS; <4> 89 + 32 registers, 4 waves per SIMD,
//                    <8> 129 + 64, 2. Partials [nchunks, H, K] fp32; cin_chunk(B) is 256 up to B = 16384 and
//                    ceil(B / 64) rounded to 8 above, so the workspace never exceeds 64 copies of the layer's weights.
//   cin_wout / cin_fold   per-chunk dz p sums; one thread per parameter adds the chunks in order into G.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace minips_k {

constexpr int kCinMaxBlocks = 65535;
constexpr int kCinMaxT = 3;
constexpr int kCinMaxH = 128;
constexpr int kCinMaxM = 64;
constexpr int kCinMaxD = 64;
constexpr int kCinChunk = 256;      // samples per partial of the batch sums up to kCinChunk * kCinMaxChunks samples
constexpr int kCinMaxChunks = 64;

inline int cin_mp(int m) { return (m + 7) / 8 * 8; }
inline int64_t cin_chunk(int64_t B) {
  if (B <= (int64_t)kCinChunk * kCinMaxChunks) return kCinChunk;
  return ((B + kCinMaxChunks - 1) / kCinMaxChunks + 7) / 8 * 8;
}
inline int64_t cin_nchunks(int64_t B) { return (B + cin_chunk(B) - 1) / cin_chunk(B); }

// The shapes of one layer inside the stacked buffers. off / off_prev are o_k / o_{k-1} (rows of XK), Hs the rows of a
// sample; Hp = H_{k-1} (m at k = 1, where X^{k-1} is read from X and off_prev is unused).
struct CinLayer {
  int m, D, Hp, H, off_prev, off, Hs;
  bool first;  // k == 1
  bool last;   // k == T
};

// X bf16 [B, ldx] (columns < m D are read), W bf16 [H, Hp, mp], XK bf16 [B, Hs, D] 16-byte aligned (layer k - 1 read,
// layer k written). blocks > 0 forces the grid. B == 0 launches nothing.
void wd_cin_layer_forward(const uint16_t* X, int64_t ldx, int64_t B, const CinLayer& L, const uint16_t* W,
                          uint16_t* XK, int blocks, hipStream_t stream);

// XK as above, w_out bf16 [Hs], wide fp32 [B] (updated), p fp32 [B, Hs] (written).
void wd_cin_output(const uint16_t* XK, int64_t B, int Hs, int D, const uint16_t* w_out, float* wide, float* p,
                   int blocks, hipStream_t stream);

// One layer of the backward. dXK bf16 [B, Hs, D] (layer k read unless last, layer k - 1 written unless first), g0 fp32
// [B, m, D] (written by the last layer, updated between, read by the first; may be null when the layer is both),
// perm nullable int32 [B F], dX bf16 [B F, D] (updated by the first layer only).
void wd_cin_layer_backward(const uint16_t* X, int64_t ldx, int64_t B, const CinLayer& L, const uint16_t* W,
                           const uint16_t* XK, uint16_t* dXK, const uint16_t* w_out, const float* dwide, float* g0,
                           const int32_t* perm, uint16_t* dX, int blocks, hipStream_t stream);

// part fp32 [cin_nchunks(B), H, Hp mp] (written).
void wd_cin_layer_wgrad(const uint16_t* X, int64_t ldx, int64_t B, const CinLayer& L, const uint16_t* XK,
                        const uint16_t* dXK, const uint16_t* w_out, const float* dwide, float* part,
                        hipStream_t stream);

// part fp32 [cin_nchunks(B), Hs] (written): the per-chunk sums of dwide[b] p[b, :].
void wd_cin_wout_partial(const float* dwide, const float* p, int64_t B, int Hs, float* part, hipStream_t stream);

// G[i] += sum over chunks (ascending) of part[chunk, i], i < n.
void wd_cin_fold(const float* part, int64_t nchunks, int64_t n, float* G, hipStream_t stream);

}  // namespace minips_k
