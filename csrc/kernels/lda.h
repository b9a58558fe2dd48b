// Latent Dirichlet Allocation by delayed-update collapsed Gibbs sampling (AD-LDA) in exact fixed point (lda.hip;
// binding in csrc/bindings/lda_py.cpp, module minips_amd._ldak). Everything that is accumulated is an integer; the
// only floating point is a handful of fp64 operations per (token, topic), each correctly rounded on its own and
// truncated to an integer before anything is summed. So topics, count deltas and totals are the same bits for
// every launch shape, path, batch split and rank count, and on the CPU reference (minips_amd/ops).
//
// State     K topics, 2 <= K <= 1024; alpha, beta in (0, 64]; a token's topic z is an int16. nwk[w][k] (tokens of
//           word w with topic k) lives in fp32 rows of W = align4(K) columns (exact: every value is an integer
//           below 2^24; pad columns 0), pulled for a clock as rows [cap, ld], token t reading rows[inv[t]].
//           nk int64 [K] are the topic totals. A document has at most 4096 tokens and a global id g < 2^51;
//           position j is the token's index inside its document. ndk, the document's own topic counts, are
//           rebuilt from its z whenever it is visited.
// Random    mix(x): x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31
//           (mod 2^64). r(it, g, j) = mix(mix(seed + it * 0x9E3779B97F4A7C15) ^ (g * 4096 + j)). A draw below T
//           is mulhi_u64(r, T). it is the sweep number; it = 0 is the initialisation.
// Live      a token is live when 0 <= inv < cap and (in a sweep) 0 <= z_old < K. A token that is not live does
//           not exist for the rule: it keeps its topic (-1 at the initialisation), is not counted in ndk and
//           adds nothing to dk, delta or the log likelihood.
// sample    against one snapshot (rows and nk, fixed for the clock), documents independent, a document's live
//           tokens in position order, ndk = bincount(z_old of its live tokens). For token j, word row u, old
//           topic ko:
//             ndk[ko] -= 1;
//             for k < K, in fp64, one operation at a time, contraction off, IEEE division, e = [k == ko]:
//               a = (double)ndk[k] + alpha;
//               b = max((double)rows[u][k] - e, 0) + beta;
//               c = 1.0 / ((double)max(nk[k] - e, 0) + Vbeta);          Vbeta = V * beta, formed by the caller
//               x = (a * b) * c;   wt[k] = (uint64)trunc(x * 2^40) + 1;
//             T = sum_k wt[k] (uint64); target = mulhi_u64(r(it, g, j), T);
//             kn = the smallest k whose prefix sum wt[0] + .. + wt[k] exceeds target;
//             z_new[j] = kn; ndk[kn] += 1; if kn != ko: dk[ko] -= 1, dk[kn] += 1.
//           With nwk <= nk and V >= 1, b c <= 1, so x < 4096 + 64, wt <= 2^53 (every conversion exact) and
//           T < 2^63. Initialisation (it = 0, z_old null): kn = mulhi_u64(r(0, g, j), K), dk[kn] += 1.
// delta     per unique pulled row u with member tokens (a plan's lookup CSR: members / memrow, memrow sorted):
//           delta[u][k] = #{members with z_new == k} - #{members with z_old == k} for k < K, 0 for the pad
//           columns K <= k < W: the whole row of W floats is written once, explicit zeros included. A topic
//           outside [0, K) counts nowhere (z_old null: the initialisation, +1 only). Rows without members are
//           not touched.
// loglik    per live token, in fp64: l = log(sum_k ((ndk[k] + alpha) / (L + K alpha)) * ((rows[u][k] + beta) /
//           (nk[k] + Vbeta))), ndk the document's counts over its live tokens and L their number, k ascending.
//           acc int64 [2] += (sum of llrint(-l 2^24), live tokens). The order of the fp64 sum and `log` may
//           differ between implementations: at most one unit per token.
//
// Mapping (wave64, 256-thread workgroups).
//   sample  one wave per document. ndk is counted in the wave's LDS slice and then held in registers: lane l owns
//           the topics [l R, l R + R), R = pow2ceil(ceil(K / 64)) <= 16, so its row loads are contiguous -- one
//           float4 per four topics when R >= 4, rows is 16-byte aligned, ld % 4 == 0 and a row is addressable to
//           align4(K), else scalar loads (never refused). 1 / (nk + Vbeta) is formed once per wave and topic and
//           again only for k == ko (the same operation, the same bits). Tokens go in chunks of 64: inv and z_old
//           are loaded coalesced and broadcast by __shfl, the next token's row is in flight while this one's
//           weights are formed. The uint64 prefix goes by __shfl_up, the winner lane by __ballot, z_new is stored
//           a chunk at a time. dk goes to an int32 LDS histogram per workgroup (|sum| <= n < 2^31) flushed by
//           64-bit global integer atomics, zero entries skipped. blocks > 0 forces the grid.
//   delta   by the member count M of a row (found by binary search in memrow):
//             M <= kLdaWaveMax (2048)   one wave: int32 LDS histogram of W entries, members strided over the
//                                       lanes, then W coalesced stores;
//             M >  kLdaWaveMax          workgroups, by the chunk rule of member_rows.h: int32 partials per
//                                       kLdaChunk (1024) members, added in int64.
//           Integer sums: no order can change a bit. No global atomics.
//   loglik  one wave per document, lanes own topics as in sample, a __shfl_xor fold of the fp64 partial sums,
//           the wave's int64 sums by two global integer atomics.
// Every index read from a tensor is checked on the device and skipped, never trusted. Empty inputs launch nothing.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace minips_k {

constexpr int kLdaMaxBlocks = 65535;
constexpr int kLdaMinK = 2;
constexpr int kLdaMaxK = 1024;
constexpr int kLdaMaxDocLen = 4096;
constexpr double kLdaMaxPrior = 64.0;   // alpha and beta lie in (0, 64]
constexpr int kLdaWeightBits = 40;      // wt = trunc(x 2^40) + 1
constexpr int kLdaLoglikBits = 24;      // the log likelihood counts units of 2^-24
constexpr int kLdaWaveMax = 2048;       // members of a row one wave counts; more go to the chunked workgroups
constexpr int kLdaChunk = 1024;         // members per workgroup of the chunked path (kLdaWaveMax >= 2 kLdaChunk)

// mix and mulhi_u64 of the rule (the negative sampler of sgns.h draws with them too)
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

__device__ __forceinline__ uint64_t mulhi_u64(uint64_t a, uint64_t b) { return __umul64hi(a, b); }

// int32 partials the chunked path of lda_delta needs for n members and rows of W columns (0: none)
int64_t lda_delta_part_ints(int64_t n, int W);

// rowptr [B + 1] over n tokens, gid [B], inv [n], z_old [n] (nullptr: the initialisation), rows [cap, ld] with
// `width` addressable columns per row (K <= width <= ld; the float4 loads need width >= align4(K)), nk [K]; z_new
// [n], dk [K] (added to).
void lda_sample(const int64_t* rowptr, const int64_t* gid, const int64_t* inv, const int16_t* z_old,
                const float* rows, int64_t ld, int64_t width, int64_t cap, const int64_t* nk, int K, double alpha,
                double beta, double Vbeta, uint64_t seed, uint64_t it, int64_t B, int64_t n, int16_t* z_new,
                int64_t* dk, int blocks, hipStream_t stream);

// members / memrow [n] (memrow sorted; the unique count memrow[n - 1] + 1 is read on the device), z_old [n]
// (nullptr: +1 only), z_new [n]; delta [cap, W], W = align4(K), contiguous; part: lda_delta_part_ints(n, W) ints.
void lda_delta(const int32_t* members, const int32_t* memrow, const int16_t* z_old, const int16_t* z_new, int64_t n,
               int K, int64_t cap, float* delta, int32_t* part, int blocks, hipStream_t stream);

// the inputs of lda_sample with the current topics z [n]; acc int64 [2] (added to).
void lda_loglik(const int64_t* rowptr, const int64_t* inv, const int16_t* z, const float* rows, int64_t ld,
                int64_t width, int64_t cap, const int64_t* nk, int K, double alpha, double beta, double Vbeta,
                int64_t B, int64_t n, int64_t* acc, int blocks, hipStream_t stream);

}  // namespace minips_k
