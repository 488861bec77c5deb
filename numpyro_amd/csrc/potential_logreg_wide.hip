// Logistic-regression potential + gradient for 65 <= D <= 1024 features:
// coefs ~ N(0, 1)^D, obs ~ Bernoulli(logits = X @ coefs).
//
//   U(b)  = sum_n [max(l_n, 0) + log1p(exp(-|l_n|)) - y_n l_n] + sum_d [b_d^2 / 2 + log(2 pi) / 2]
//   dU/db = X^T (sigmoid(l) - y) + b,      l = X b
//
// k_logreg_wide: the D-blocked sibling of k_logreg_x3 (potential_logreg.hip).  That kernel keeps a
// wave's whole coefficient tile (0.75 D VGPRs), all its gradient accumulators (D / 2 VGPRs) and the
// whole 32-row X tile (384 D bytes of LDS) resident, which ends at D = 64.  Here a workgroup's waves
// are a grid of CT chain tiles x DS feature slices, both functions of D alone (lw_class):
//
//   wave (j, i) owns chain tile j (32 chains) and the features [i DW, (i + 1) DW), DW = 32 DTS,
//   DTS = 3 or 4 (1 or 2 below 65 features); it holds only its slice's coefficient fragments (0.75 DW VGPRs) and its slice's
//   gradient accumulators (DW / 2 VGPRs).
//
// Per 32-row tile
//   1. GEMM1, sliced: wave (j, i) computes the partial logits of its slice, L_i = X[:, slice i] .
//      Z[slice i, tile j] (split-bf16, six products per 16-deep k-block, nmx_split_bf16.h), and
//      writes its 16 accumulator registers to its 4 KiB exchange slot in LDS;
//   2. after the workgroup barrier every wave of chain tile j adds the DS partials IN SLICE ORDER,
//      ((L_0 + L_1) + L_2) + ...: all waves of the chain tile hold the same bits, whatever the timing;
//   3. every wave runs the Bernoulli epilogue itself (redundant VALU work, but no second exchange and
//      no second barrier); only slice 0 accumulates U (float64 per lane);
//   4. GEMM2, sliced: G[slice i] += X[:, slice i]^T . R with the residual registers as the B operand
//      (the accumulator holds the chain on the lane and 16 rows in the registers: the B layout of the
//      32x32x16 form with the k order permuted, which the packed X^T pieces follow).
// The N x C logit matrix never exists in memory.
//
// X stream.  A wave needs only its slice's pieces, so X never sits in LDS as a whole tile.  The pack
// orders a tile as DS slices x 2 DTS chunks of six 1 KiB fragment-order pieces (6 KiB: the three
// planes of 32 features, for GEMM1 as two k-blocks, for GEMM2 as one d-tile x two k-steps), then
// 256 bytes of labels.  Each slice has a ring of R chunk slots shared by the CT waves of the slice
// and filled by buffer LDS-DMA (wave (j, i) copies the pieces j, j + CT, ... of its slice's chunk);
// one workgroup barrier per chunk says "chunk q has landed in every slice, and chunk q - 1's slot is
// free", after which chunk q + R - 1 is issued into that slot.  The exchange of step 2 rides on the
// barrier of the first GEMM2 chunk.  LDS = DS R 6 KiB of rings + 4 KiB per wave of exchange + labels.
//
// Rows >= n_rows are MASKED: the pack gives them zero X and the label -1, so their residual meets
// zero X^T columns and their U term is dropped by the label's sign.  Features >= D are zero in the
// pack and in the coefficient fragments.
//
// The linear part of U, sum_n y_n l_n = <X^T y, b>, is a float64 table of the pack
// (k_logreg_wide_colsums) added once per chain in the finalize.  The gradient is the in-register
// residual.
//
// Work split: grid = chain-tile groups x S row splits, S a function of n_rows and D only
// (lw_num_splits); split s owns the tiles [s T / S, (s + 1) T / S), each summed in tile order, and
// the per-split slabs are added in a fixed order by k_logreg_wide_finalize.  Workgroups of one split
// sit on one XCD (blockIdx % 8).  No float atomics, no order that depends on arrival: a chain's U
// and dU are bitwise independent of how many chains share the launch, of its position, of a phase
// mask and of the order of an active list.
//
// The likelihood is a compile-time policy LK of the pack, the kernel and the finalize (what the
// tile's 256-byte side slot holds, the pointwise step between the GEMMs, the constants of U);
// everything above is shared.  lk_bernoulli is the model above.  lk_poisson is count regression,
// coefs ~ N(0, 1)^D, obs ~ Poisson(exp(X @ coefs + offset)), 1 <= D <= 1024:
//
//   U(b)  = sum_n [mu_n - y_n eta_n + lgamma(y_n + 1)] + sum_d [b_d^2 / 2 + log(2 pi) / 2]
//   dU/db = X^T (mu - y) + b,      eta = X b + o,  mu = exp(eta)
//
// Its side slot holds y (entries 0..31) and the offset (32..63) in one row permutation; rows >= n_rows
// have y = 0 and the offset -inf, so mu = 0 exactly and the residual and the U term vanish without a
// select.  The kernel accumulates sum mu; sum_n y_n eta_n = <X^T y, b> + sum_n y_n o_n, and with
// sum_n lgamma(y_n + 1) that is the X^T y table plus ONE float64 scalar of the pack.  D <= 64 runs
// the 4 x 1 class with DTS = 1 or 2 (instantiated for this policy and for the horseshoe prior below
// only).  A chain whose eta passes
// float32's exp range gets mu = +inf in its own B-operand column: U = +inf (the float64 parts are
// finite), and no other chain changes by a bit.
//
// The prior is a second compile-time policy PR: where the coefficient fragments at the top of
// k_logreg_wide come from, and which finalize follows.  pr_normal is the prior above (arena row d is
// the coefficient).  pr_horseshoe is sparse regression, for either likelihood and 1 <= D <= 1024:
//
//   lambdas ~ HalfCauchy(1)^D, tau ~ HalfCauchy(1), unscaled_betas ~ N(0, 1)^D,
//   betas = tau lambdas unscaled_betas,  obs ~ LK(X @ betas)
//
// on the 2 D + 1 unconstrained arena rows ul[d] = log lambdas[d] (row d), ut = log tau (row D) and
// z[d] (row D + 1 + d).  With s[d] = exp(ut + ul[d]), beta[d] = s[d] z[d] (hs_coef, float32) and L the
// likelihood part above, G = dL/dbeta = X^T residual:
//
//   U      = L(beta) + sum_d [log(2 cosh ul[d]) + log(pi / 2)] + log(2 cosh ut) + log(pi / 2)
//            + sum_d [z[d]^2 / 2 + log(2 pi) / 2]
//   dU/dz[d] = s[d] G[d] + z[d],  dU/dul[d] = beta[d] G[d] + tanh(ul[d]),
//   dU/dut   = sum_d beta[d] G[d] + tanh(ut)
//
// The tile kernel is the same but for the gather (three arena rows and hs_coef before the split), so
// the slabs hold G.  dU/dut sums over coordinates, which no workgroup of the plain finalize does, so
// the horseshoe has a finalize of its own in two launches:
//   k_horseshoe_finalize  one workgroup per (64 positions, block of HS_BLOCK coordinates), wave w the
//     coordinates w HS_BLOCK / 4 .. of the block, one after the other: G[d] from the S slabs in the
//     plain finalize's order (four quarters, then ((q0 + q1) + q2) + q3), beta[d] by hs_coef again,
//     the z and ul gradient rows, and in float64 the wave's running beta G and its part of U
//     (log 2 cosh ul + z^2 / 2 - xty beta: the linear part of U is in beta); the four waves' sums are
//     added in wave order and go to the block's two workspace rows;
//   k_horseshoe_tau       one workgroup per 64 positions: wave w adds its quarter of the pepart slabs
//     and the blocks [w NB / 4, (w + 1) NB / 4) in block order, the four are added in wave order, then
//     tau's own terms and the constants: the ut gradient row and U.
// NB = ceil(D / HS_BLOCK): every order above is a function of D and S alone.  No atomics.  A chain whose
// ut + ul[d] passes float32's exp range has beta = +-inf in its own B-operand column and in its own
// float64 sums: U is not finite, and no other chain changes by a bit.
//
// lk_negbin is over-dispersed count regression, the first likelihood with a latent of its own:
//
//   coefs ~ N(0, 1)^D,  phi ~ Gamma(a, b),  obs ~ NegativeBinomial2(exp(X @ coefs + offset), phi)
//
// on D + 1 arena rows, row D being u = log phi (pr_normal; 1 <= D <= 1024).  With eta = X b + o,
// l = eta - u, sp(l) = max(l, 0) + log1p(exp(-|l|)) (so log(phi + mu) = u + sp(l): nothing overflows in
// eta), p = sigmoid(l) and R(phi, y) = lgamma(phi + y) - lgamma(phi):
//
//   U      = phi S1 + S2 - sum_n y_n l_n - sum_n R(phi, y_n) + sum_n lgamma(y_n + 1)
//            + sum_d [b_d^2 / 2 + log(2 pi) / 2] - [a u - b phi] + lgamma(a) - a log b
//   res_n  = (phi + y_n) p_n - y_n,   S1 = sum_n sp(l_n),  S2 = sum_n y_n sp(l_n),  S3 = sum_n res_n
//   dU/db  = X^T res + b
//   dU/du  = phi S1 - S3 - phi sum_n [digamma(phi + y_n) - digamma(phi)] - a + b phi
//
// The pack is Poisson's (side slot, X^T y, the constant, the count check).  The tile kernel loads u for
// its lane's chain beside the gather (in the GEMM1 accumulator the chain is the lane), forms
// phi = nb_phi(u) once, and runs the Bernoulli epilogue's arithmetic on l; slice 0 keeps S1, S2 and S3
// as three float64 sums per lane, which leave through three pepart rows per split, added in the U
// slabs' order.  A masked row has l = -inf: sp = 0, p = 0 and res = 0 exactly, no select.
//
// The eta-free part, sum_n R(phi, y_n) and its phi-derivative, is a sum over the DISTINCT counts: the
// pack appends a table (y_k, m_k) of the distinct values in ascending order with their multiplicities
// (float64 pairs, K <= N; built on the host from one copy of y), and k_negbin_rising sums it per chain
// in float64 through the cancellation-free forms of NMX_OP_LRISING (nmx_program.h, restated in
// float64: nb_lrising = R - y log phi and nb_lrising_da = dR/dphi - y / phi, never a difference of two
// lgamma or digamma values).  The y log phi parts meet sum_n y_n l_n = <X^T y, b> + sum y o - u sum y:
// u sum y cancels EXACTLY, so U takes -LR = -sum_k m_k nb_lrising(phi, y_k), and dU/du takes
// -phi LD - sum y with LD = sum_k m_k nb_lrising_da(phi, y_k).  Eight chains x 32 table slices per
// workgroup; slice s adds the entries s, s + 32, ... in table order and the 32 are added by a fixed
// tree: a function of the table alone.  The plain finalize has two more rows for this policy: j = D is
// dU/du and j = D + 1 is U, all float64 until the store.  A chain whose u passes float32's exp range
// has phi = +inf in its own column and its own finalize lane: its U is not finite, and no other chain
// changes by a bit.
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "nmx_api_internal.h"
#include "nmx_common.h"
#include "nmx_split_bf16.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr int LW_ROWS = 32;
constexpr int LW_MAX_D = 1024;
constexpr int LW_CHUNK = 6 * 1024;  // six pieces
constexpr int LW_LABEL_BYTES = 256;

// packed buffer: X^T y as float64[1024] | the policy's head (LK::HEAD_BYTES) | the tiles
constexpr size_t LW_XTY_BYTES = (size_t)LW_MAX_D * sizeof(double);

// Shape class of D: CT chain tiles x DS feature slices of DTS d-tiles (32 features) each, and the
// ring depth R.  D <= 128 runs 4 x 1 (no exchange: the slice is the whole row), not 4 x 2 with
// half-empty slices: the same MFMAs per wave, four waves fewer per workgroup and no LDS round trip.
struct lw_shape {
  int CT, DS, DTS;
};
inline lw_shape lw_class(int D) {
  const int DS = D <= 128 ? 1 : D <= 256 ? 2 : D <= 512 ? 4 : 8;
  const int CT = D <= 256 ? 4 : D <= 512 ? 2 : 1;
  const int DTS = (D + 32 * DS - 1) / (32 * DS);  // 3 or 4 for 65 <= D <= 1024, 1 or 2 below
  return {CT, DS, DTS};
}
inline size_t lw_tile_bytes(int D) {
  const lw_shape c = lw_class(D);
  return (size_t)c.DS * 12 * c.DTS * 1024 + LW_LABEL_BYTES;
}
inline int64_t lw_ntiles(int64_t n) { return (n + LW_ROWS - 1) / LW_ROWS; }

// Row splits: one per 16 tiles, a multiple of 8 for the XCD placement, capped so that the slabs
// (S D ldc floats) stay at 256 MiB for ldc = 4096 at the widest D of each class.
int lw_num_splits(int64_t n_rows, int D) {
  int64_t s = lw_ntiles(n_rows) / 16;
  s = s / 8 * 8;
  const int cap = D <= 256 ? 64 : D <= 512 ? 32 : 16;
  if (s < 8) s = 8;
  if (s > cap) s = cap;
  return (int)s;
}

// xty[d] = sum_n y_n X[n][d] in float64, one workgroup per column, fixed thread count and a
// fixed-order tree: the value depends on the data only
constexpr int CS_THREADS = 256;
__global__ __launch_bounds__(CS_THREADS) void k_logreg_wide_colsums(const float* __restrict__ X,
                                                                    const float* __restrict__ y, int64_t n, int D,
                                                                    double* __restrict__ xty) {
  __shared__ double red[CS_THREADS];
  const int d = blockIdx.x;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += CS_THREADS) acc += (double)y[i] * (double)X[i * D + d];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int k = CS_THREADS / 2; k > 0; k >>= 1) {
    if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    NMX_DCHECK(d < LW_MAX_D);
    xty[d] = red[0];
  }
}

// Poisson pack: head[0] = sum_n lgamma(y_n + 1) - sum_n y_n o_n in float64 (one workgroup, the same
// fixed tree), and the first row whose count is negative, not whole or >= 2^24 (`bad` starts at ~0)
__global__ void k_poisson_bad_reset(unsigned long long* bad) { *bad = ~0ull; }
__global__ __launch_bounds__(CS_THREADS) void k_poisson_const(const float* __restrict__ y,
                                                              const float* __restrict__ off, int64_t n,
                                                              double* __restrict__ head, unsigned long long* bad) {
  __shared__ double red[CS_THREADS];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += CS_THREADS) {
    const float v = y[i];
    if (!(v >= 0.0f) || v != floorf(v) || v >= 16777216.0f) {
      atomicMin(bad, (unsigned long long)i);
      continue;
    }
    acc += lgamma((double)v + 1.0) - (off ? (double)v * (double)off[i] : 0.0);
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int k = CS_THREADS / 2; k > 0; k >>= 1) {
    if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) head[0] = red[0];
}

// Packed tile = DS slices x 2 DTS chunks x 6 pieces of 1 KiB, each piece a 64-lane x 16-byte
// operand fragment in lane order (lane (r, h), elements j = 0..7), then the labels.  Slice i covers
// the features d0 = 32 DTS i ..:
//   chunk c < DTS, piece 3 kk + p     GEMM1 A = X[32 rows][16 cols], plane p, k-block 2 c + kk:
//                                     X[r][d0 + 16 (2 c + kk) + 8 h + j]
//   chunk DTS + dt, piece 2 p + s     GEMM2 A = X^T[32 cols][16 rows], plane p, d-tile dt, k-step s:
//                                     X[16 s + 8 (j >> 2) + 4 h + (j & 3)][d0 + 32 dt + r] -- the k
//                                     order of the GEMM1 accumulator used as the B operand
//   side slot: float[64], LK::side_entry: entry 16 h + i belongs to row (i & 3) + 8 (i >> 2) + 4 h
//           Bernoulli: y, -1 for rows >= n (entries 32.. are zero)
//           Poisson:   y, 0 for rows >= n; entry 32 + 16 h + i the row's offset, -inf for rows >= n
// Rows >= n_rows and features >= D are zero.  One thread per 16 bytes.
template <class LK>
__global__ void k_logreg_wide_pack(const float* __restrict__ X, const float* __restrict__ y,
                                   const float* __restrict__ off, int64_t n, int D, int DS, int DTS, int64_t ntiles,
                                   char* __restrict__ out) {
  const int NP = DS * 12 * DTS;                    // pieces of a tile
  const int64_t per = (int64_t)NP * 64 + LW_LABEL_BYTES / 16;  // 16-byte items of a tile
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ntiles * per) return;
  const int64_t t = i / per;
  const int item = (int)(i % per);
  const int64_t r0 = t * LW_ROWS;
  char* dst = out + (size_t)t * ((size_t)NP * 1024 + LW_LABEL_BYTES) + (size_t)item * 16;
  if (item >= NP * 64) {
    const int q = item - NP * 64;  // entries 4 q .. 4 q + 3
    f32x4 f = {0.0f, 0.0f, 0.0f, 0.0f};
    if (q < LK::SIDE_QUADS) {
      const int hh = (q >> 2) & 1;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int ii = 4 * (q & 3) + k;
        const int64_t row = r0 + (ii & 3) + 8 * (ii >> 2) + 4 * hh;
        f[k] = LK::side_entry(y, off, row, n, q >= 8);
      }
    }
    *reinterpret_cast<f32x4*>(dst) = f;
    return;
  }
  const int lane = item & 63, piece = item >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int sl = piece / (12 * DTS), rem = piece % (12 * DTS);
  const int c = rem / 6, e = rem % 6;
  const int d0 = 32 * DTS * sl;
  float v[8];
  int plane;
  if (c < DTS) {
    plane = e % 3;
    const int kb = 2 * c + e / 3;
    const int64_t row = r0 + r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int d = d0 + 16 * kb + 8 * h + j;
      v[j] = (row < n && d < D) ? X[row * D + d] : 0.0f;
    }
  } else {
    plane = e >> 1;
    const int s = e & 1;
    const int d = d0 + 32 * (c - DTS) + r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int64_t row = r0 + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3);
      v[j] = (row < n && d < D) ? X[row * D + d] : 0.0f;
    }
  }
  nmx_bf16x8 b1, b2, b3;
  nmx_split3(v, b1, b2, b3);
  *reinterpret_cast<nmx_bf16x8*>(dst) = plane == 0 ? b1 : (plane == 1 ? b2 : b3);
}

// The counted waits of the ring (k_logreg_wide step) assume that the DMA copies are the loop's only
// vector-memory operations: true of the release build (no scratch; the resource report says so), not
// of the debug build, whose checks spill -- that build waits for everything.
#ifdef NMX_DEBUG
constexpr bool LW_COUNTED_WAITS = false;
#else
constexpr bool LW_COUNTED_WAITS = true;
#endif

template <int N>
__device__ __forceinline__ void lw_wait_vm() {
  // s_waitcnt vmcnt(N), other counters untouched (gfx9 encoding)
  static_assert(N >= 0 && N < 64, "vmcnt range");
  __builtin_amdgcn_s_waitcnt((N & 15) | (7 << 4) | (15 << 8) | ((N >> 4) << 14));
}

// LDS accesses by inline asm: a compiler-visible LDS access after the rings' DMA issue gets an
// s_waitcnt vmcnt(0), which would drain the prefetch.  lw_lds_wait (all reads and writes done), then
// lw_pin on each value read before its use.
__device__ __forceinline__ unsigned lw_lds_addr(const char* p) {
  return (unsigned)(size_t)((__attribute__((address_space(3))) const char*)p);
}
template <class T>
__device__ __forceinline__ void lw_lds_read(T& v, unsigned addr) {
  static_assert(sizeof(T) == 16, "one ds_read_b128");
  asm volatile("ds_read_b128 %0, %1" : "=&v"(v) : "v"(addr));
}
__device__ __forceinline__ void lw_lds_write(unsigned addr, const f32x4& v) {
  asm volatile("ds_write_b128 %0, %1" : : "v"(addr), "v"(v) : "memory");
}
__device__ __forceinline__ void lw_lds_wait() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
template <class T>
__device__ __forceinline__ void lw_pin(T& v) {
  asm volatile("" : "+v"(v));
}

// Bernoulli-logits epilogue on the summed GEMM1 accumulator (register r = row (r & 3) + 8 (r >> 2)
// + 4 h of the tile, y4 its labels, -1 on a masked row):
//   e = exp(-|l|),  u = 1 + e
//   sigmoid(l) = 1 / u for l >= 0, e / u for l < 0 (full relative precision on both sides)
//   log1p(e) = log(u) e / (u - 1): the quotient repairs the rounding of u (e itself where u == 1)
//   res = sigmoid(l) - y;   U term max(l, 0) + log1p(e), added to `pe` when ACC (slice 0)
template <bool ACC>
__device__ __forceinline__ void lw_epilogue(const nmx_f32x16& acc, const f32x4 (&y4)[4], float (&res)[16], double& pe) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float l = acc[r], yv = y4[r >> 2][r & 3];
    const float e = __builtin_amdgcn_exp2f(-fabsf(l) * LOG2E);
    const float u = 1.0f + e;
    const float s = __builtin_amdgcn_rcpf(u);
    res[r] = (l >= 0.0f ? s : e * s) - yv;
    if constexpr (ACC) {
      const float dm = u - 1.0f;
      const float lg = __builtin_amdgcn_logf(u) * LN2;
      const float l1p = dm == 0.0f ? e : lg * (e * __builtin_amdgcn_rcpf(dm));
      pe += yv >= 0.0f ? (double)(fmaxf(l, 0.0f) + l1p) : 0.0;
    }
  }
}

// Poisson epilogue: mu = exp(l + o) as one exp2, res = mu - y formed here, per row, so the
// cancellation near the mode happens before the bf16 split; U term mu.  A masked row has o = -inf
// and y = 0: mu = 0 exactly.  The relative error of mu is the absolute error of l + o (f32-accurate
// split-bf16 logit, one rounding of the sum, one of the product with log2 e: about |eta| 2^-23), the
// same budget as a float32 evaluation of exp(eta).
// `acc` is eta: the kernel has added the offsets.
template <bool ACC>
__device__ __forceinline__ void lw_epilogue_poisson(const nmx_f32x16& acc, const f32x4 (&y4)[4], float (&res)[16],
                                                    double& pe) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float mu = __builtin_amdgcn_exp2f(acc[r] * LOG2E);
    res[r] = mu - y4[r >> 2][r & 3];
    if constexpr (ACC) pe += (double)mu;
  }
}

// Negative-binomial epilogue: `acc` is eta, `lu` the lane's chain's u = log phi.  The Bernoulli
// epilogue's e, u, sigmoid and log1p on l = eta - lu; res = (phi + y) p - y formed here, per row, before
// the bf16 split; slice 0 adds sp, y sp (an exact float64 product) and res to its three sums.  A masked
// row has eta = -inf and y = 0: e = 0, p = 0, sp = 0 and res = 0 exactly.
__device__ __forceinline__ float nb_phi(float lu) { return expf(lu); }
template <bool ACC>
__device__ __forceinline__ void lw_epilogue_negbin(const nmx_f32x16& acc, int k, const f32x4& yk, float lu, float phi,
                                                   float (&res)[16], double& s1, double& s2, double& s3) {
  // the registers 4 k .. 4 k + 3 and their counts yk
#pragma unroll
  for (int r = 4 * k; r < 4 * k + 4; ++r) {
    const float l = acc[r] - lu, yv = yk[r & 3];
    const float e = __builtin_amdgcn_exp2f(-fabsf(l) * LOG2E);
    const float u = 1.0f + e;
    const float s = __builtin_amdgcn_rcpf(u);
    res[r] = (phi + yv) * (l >= 0.0f ? s : e * s) - yv;
    if constexpr (ACC) {
      const float dm = u - 1.0f;
      const float lg = __builtin_amdgcn_logf(u) * LN2;
      const float l1p = dm == 0.0f ? e : lg * (e * __builtin_amdgcn_rcpf(dm));
      const float sp = fmaxf(l, 0.0f) + l1p;
      s1 += (double)sp;
      s2 = fma((double)yv, (double)sp, s2);
      s3 += (double)res[r];
    }
  }
}

// The likelihood policies: the widths served, the bytes between the X^T y table and the tiles, what
// the pack puts into the side slot, and the epilogue; NPE float64 rows of pepart per split, whether
// arena row D is a latent of the likelihood's own (lk_negbin: two more finalize rows, two workspace
// rows of k_negbin_rising), and the bytes per row that follow the tiles.
struct lk_bernoulli {
  static constexpr int MIN_D = 65, NPE = 1;
  static constexpr bool LATENT = false;
  static constexpr size_t TAIL_PER_ROW = 0;
  static constexpr size_t HEAD_BYTES = 0;
  static constexpr int SIDE_QUADS = 8;      // 16-byte items of the side slot that hold data
  static constexpr bool HAS_OFFSET = false;  // entries 32..63 of the side slot are added to the logits
  static constexpr const char* NAME = "logreg_wide";
  static __device__ __forceinline__ float side_entry(const float* y, const float*, int64_t row, int64_t n, bool) {
    return row < n ? y[row] : -1.0f;
  }
  template <bool ACC>
  static __device__ __forceinline__ void epilogue(const nmx_f32x16& acc, const f32x4 (&y4)[4], float (&res)[16],
                                                  double& pe) {
    lw_epilogue<ACC>(acc, y4, res, pe);
  }
};
struct lk_poisson {
  static constexpr int MIN_D = 1, NPE = 1;
  static constexpr bool LATENT = false;
  static constexpr size_t TAIL_PER_ROW = 0;
  static constexpr size_t HEAD_BYTES = 256;  // float64 constant of U | the bad-count slot
  static constexpr int SIDE_QUADS = 16;
  static constexpr bool HAS_OFFSET = true;
  static constexpr const char* NAME = "poisson";
  static __device__ __forceinline__ float side_entry(const float* y, const float* off, int64_t row, int64_t n,
                                                     bool second) {
    if (!second) return row < n ? y[row] : 0.0f;
    return row < n ? (off ? off[row] : 0.0f) : -INFINITY;
  }
  template <bool ACC>
  static __device__ __forceinline__ void epilogue(const nmx_f32x16& acc, const f32x4 (&y4)[4], float (&res)[16],
                                                  double& pe) {
    lw_epilogue_poisson<ACC>(acc, y4, res, pe);
  }
};
// Poisson's pack and side slot; the kernel calls lw_epilogue_negbin itself (it has the chain's u).
// Head, float64: [0] Poisson's constant, [1] the bad-count slot, then NB_A.. below; after the tiles
// the table of distinct counts, n_rows pairs (y_k, m_k) of which the first head[NB_K] are set.
enum { NB_A = 2, NB_B, NB_PRIOR, NB_K, NB_SUMY, NB_HEAD_END };  // a, b, lgamma(a) - a log b, K, sum_n y_n
struct lk_negbin : lk_poisson {
  static constexpr int NPE = 3;
  static constexpr bool LATENT = true;
  static constexpr size_t TAIL_PER_ROW = 2 * sizeof(double);
  static constexpr const char* NAME = "negbin";
};

// Horseshoe scale and coefficient of one coordinate, s = exp(ut + ul) and beta = s z in float32: the
// gather of k_logreg_wide and k_horseshoe_finalize both go through here, and the pinned sum keeps
// either from contracting it into the exponential's first product, so both see the same bits.
__device__ __forceinline__ void hs_coef(float ul, float ut, float z, float& s, float& beta) {
  float u = ut + ul;
  lw_pin(u);
  s = expf(u);
  beta = s * z;
}

// The prior policies: whether every width from 1 is served (the 4 x 1 class with DTS = 1 and 2 for
// any likelihood), and what the kernel's load of arena row d (rows of ldc) of chain c is.  pr_normal:
// the coefficient itself.  pr_horseshoe: ul[d], which `coef` turns into beta[d].
struct pr_normal {
  static constexpr bool ALL_D = false, HORSESHOE = false;
};
struct pr_horseshoe {
  static constexpr bool ALL_D = true, HORSESHOE = true;
  static __device__ __forceinline__ float coef(float v, const nmx_eval_batch& ev, int d, int D, int ldc, int c) {
    float s, beta;
    hs_coef(v, ev.z[(size_t)D * ldc + c], ev.z[(size_t)(D + 1 + d) * ldc + c], s, beta);
    return beta;
  }
};
template <class LK, class PR>
constexpr int lw_min_d() {
  return PR::ALL_D ? 1 : LK::MIN_D;
}
template <class LK, class PR>
constexpr const char* lw_name() {
  return PR::HORSESHOE ? "horseshoe" : LK::NAME;
}

template <int CT, int DS, int DTS, int R>
struct lw_cfg {
  static constexpr int WAVES = CT * DS, NCH = 2 * DTS, KBS = 2 * DTS, DW = 32 * DTS;
  static constexpr int SLICE_BYTES = 12 * DTS * 1024;
  static constexpr int TILE_BYTES = DS * SLICE_BYTES + LW_LABEL_BYTES;
  // LDS: the waves' label slots | the slices' rings | the waves' exchange slots
  static constexpr int LAB_OFF = 0;
  static constexpr int RING_OFF = WAVES * 2 * LW_LABEL_BYTES;
  static constexpr int EXCH_OFF = RING_OFF + DS * R * LW_CHUNK;
  static constexpr int LDS_BYTES = EXCH_OFF + (DS > 1 ? WAVES * 4096 : 0);
  // pieces of a chunk that wave (j, .) copies: j, j + CT, ... < 6
  static constexpr int MAX_COPIES = (6 + CT - 1) / CT;
  static_assert(R == 2 || R == 3, "ring depth");
  static_assert(LDS_BYTES <= 160 * 1024, "the CU's LDS");
};

template <class LK, class PR, int CT, int DS, int DTS, int R>
__global__ __launch_bounds__(64 * CT * DS) void k_logreg_wide(const char* __restrict__ Xq, int64_t ntiles, int D,
                                                              int S, int Gt, nmx_eval_batch ev,
                                                              float* __restrict__ gpart,
                                                              double* __restrict__ pepart) {
  using C = lw_cfg<CT, DS, DTS, R>;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  // splits sp = x (mod 8) run on XCD x (workgroup b = x mod 8), the chain-tile groups of a split on
  // consecutive workgroups of that XCD, so they share X tiles in its L2
  const int b = blockIdx.x, qb = b >> 3;
  const int ct = qb % Gt, split = (qb / Gt) * 8 + (b & 7);
  const int npos = ev.active_idx ? *ev.active_count : ev.ldc;
  if (ct * CT * 32 >= npos) return;  // past the compacted list: workgroup-uniform

  const int lane = threadIdx.x & 63;
  const int wu = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int sl = wu % DS, jt = wu / DS;  // feature slice, chain tile
  const int h = lane >> 5, col = lane & 31;
  const int ldc = ev.ldc;
  const int pos = (ct * CT + jt) * 32 + col;
  const int c = pos < ldc ? nmx_eval_chain(ev, pos) : -1;
  const bool active = __any(c >= 0);      // wave-uniform, and the same in every slice of a chain tile
  if (!__syncthreads_or(active)) return;  // workgroup-uniform

  const int64_t t0 = (int64_t)split * ntiles / S, t1 = (int64_t)(split + 1) * ntiles / S;
  const int nt = (int)(t1 - t0);
  const int nq = nt * C::NCH;  // chunks of this split, per slice
  NMX_DCHECK(split < S && t0 >= 0 && t1 <= ntiles && nt >= 0);
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(Xq + (size_t)t0 * C::TILE_BYTES), 0, (int)((size_t)nt * C::TILE_BYTES), 0x00020000);

  // coefficient fragments of the slice (B operand: lane (col, h) holds Z[d0 + 16 kb + 8 h + j] of
  // its chain), gathered from the arena once, through the prior policy, and split; features >= D
  // and lanes without a chain hold zero
  // (clamped loads, masked after: a load under `ok` compiles to a branch and a wait per element)
  const int d0 = sl * C::DW;
  const int cz = c >= 0 ? c : 0;
  nmx_bf16x8 z1[C::KBS], z2[C::KBS], z3[C::KBS];
#pragma unroll
  for (int kb = 0; kb < C::KBS; ++kb) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int d = d0 + 16 * kb + 8 * h + j;
      NMX_DCHECK(d >= 0 && cz < ldc);
      v[j] = ev.z[(size_t)(d < D ? d : D - 1) * ldc + cz];
    }
    if constexpr (PR::HORSESHOE) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int d = d0 + 16 * kb + 8 * h + j;
        v[j] = PR::coef(v[j], ev, d < D ? d : D - 1, D, ldc, cz);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (c >= 0 && d0 + 16 * kb + 8 * h + j < D) ? v[j] : 0.0f;
    nmx_split3(v, z1[kb], z2[kb], z3[kb]);
  }
  nmx_f32x16 g[DTS];
#pragma unroll
  for (int dt = 0; dt < DTS; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) g[dt][r] = 0.0f;
  double pe = 0.0;
  // lk_negbin: the chain's u = log phi (arena row D) and phi; pe, pe2 and pe3 are S1, S2 and S3
  [[maybe_unused]] float lu = 0.0f, phi = 0.0f;
  [[maybe_unused]] double pe2 = 0.0, pe3 = 0.0;
  if constexpr (LK::LATENT) {
    lu = ev.z[(size_t)D * ldc + cz];
    phi = nb_phi(lu);
  }

  char* const ring = lds + C::RING_OFF + sl * R * LW_CHUNK;      // the slice's R chunk slots
  char* const lab = lds + C::LAB_OFF + wu * 2 * LW_LABEL_BYTES;  // the wave's two label slots
  // chunk cc of tile kt (q = kt NCH + cc) into slot q % R; with a tile's first chunk every wave
  // also fetches the tile's labels into its own slot kt & 1
  auto issue = [&](int kt, int cc) {
    const int q = kt * C::NCH + cc;
    NMX_DCHECK(kt >= 0 && kt < nt && cc >= 0 && cc < C::NCH);
    const unsigned tile = (unsigned)kt * (unsigned)C::TILE_BYTES;
    if (cc == 0)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (__attribute__((address_space(3))) void*)(lab + (kt & 1) * LW_LABEL_BYTES),
                                               4, lane * 4, tile + (unsigned)(DS * C::SLICE_BYTES), 0, 0);
    char* dst = ring + (q % R) * LW_CHUNK;
    const unsigned src = tile + (unsigned)(sl * C::SLICE_BYTES + cc * LW_CHUNK);
#pragma unroll
    for (int k = 0; k < C::MAX_COPIES; ++k) {
      const int e = jt + CT * k;
      NMX_DCHECK(e >= 6 || (dst + e * 1024 + 1024 <= lds + C::EXCH_OFF && src + e * 1024 + 1024 <= (unsigned)nt * C::TILE_BYTES));
      if (e < 6)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (__attribute__((address_space(3))) void*)(dst + e * 1024), 16,
                                                 lane * 16, src + (unsigned)(e * 1024), 0, 0);
    }
  };
  // chunk q has landed in every wave and every wave is done with chunk q - 1's slot; then chunk
  // q + R - 1 goes into that slot.  The copies return in order: with R = 3 the wave's copies of
  // chunk q + 1 (as many as its copies of any chunk; a label fetch ahead of them is waited for too)
  // may stay in flight, with R = 2 or at the stream's end nothing is in flight behind chunk q.
  auto step = [&](int kt, int cc) {
    const int q = kt * C::NCH + cc;
    if (R == 2 || q + 1 >= nq || !LW_COUNTED_WAITS) lw_wait_vm<0>();
    else if (CT == 4 && jt >= 2) lw_wait_vm<1>();
    else lw_wait_vm<C::MAX_COPIES>();
    lw_lds_wait();  // the wave's exchange writes
    asm volatile("s_barrier" ::: "memory");
    const int cn = (cc + R - 1) % C::NCH, kn = kt + (cc + R - 1) / C::NCH;
    if (kn < nt) issue(kn, cn);
  };
#pragma unroll
  for (int q = 0; q < R - 1; ++q)
    if (q < nq) issue(0, q);  // R - 1 <= NCH: chunks of tile 0

  for (int kt = 0; kt < nt; ++kt) {
    nmx_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    // GEMM1: the slice's partial logits, two k-blocks per chunk
#pragma unroll
    for (int cc = 0; cc < DTS; ++cc) {
      step(kt, cc);
      if (!active) continue;
      const unsigned slot = lw_lds_addr(ring + ((kt * C::NCH + cc) % R) * LW_CHUNK) + lane * 16;
      nmx_bf16x8 a[2][3];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int p = 0; p < 3; ++p) lw_lds_read(a[kk][p], slot + (3 * kk + p) * 1024);
      lw_lds_wait();
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int p = 0; p < 3; ++p) lw_pin(a[kk][p]);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int kb = 2 * cc + kk;
        acc = nmx_mma_bf16(a[kk][2], z1[kb], acc);
        acc = nmx_mma_bf16(a[kk][1], z2[kb], acc);
        acc = nmx_mma_bf16(a[kk][0], z3[kb], acc);
        acc = nmx_mma_bf16(a[kk][1], z1[kb], acc);
        acc = nmx_mma_bf16(a[kk][0], z2[kb], acc);
        acc = nmx_mma_bf16(a[kk][0], z1[kb], acc);
      }
    }
    if constexpr (DS > 1) {
      // the partial goes to the wave's exchange slot: registers 4 k .. 4 k + 3 at k KiB + 16 lane
      if (active) {
        // The stores are inline asm, which the compiler's hazard pass does not look into: the wait
        // states between the last MFMA's write of `acc` and an LDS instruction reading it (18 for a
        // 16-pass MFMA) are spent here by hand.  Without them the store sends the accumulator short
        // of its last products.
        asm volatile("s_nop 15\n\ts_nop 15" : "+v"(acc));
        const unsigned ex = lw_lds_addr(lds + C::EXCH_OFF + wu * 4096) + lane * 16;
        NMX_DCHECK(C::EXCH_OFF + wu * 4096 + 4096 <= C::LDS_BYTES);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const f32x4 v = {acc[4 * k], acc[4 * k + 1], acc[4 * k + 2], acc[4 * k + 3]};
          lw_lds_write(ex + k * 1024, v);
        }
      }
    }
    nmx_bf16x8 rs[2][3];
    // GEMM2: the slice's gradient rows, one d-tile per chunk
#pragma unroll
    for (int dt = 0; dt < DTS; ++dt) {
      step(kt, DTS + dt);
      if (!active) continue;
      if (dt == 0) {
        if constexpr (DS > 1) {
          // the chain tile's DS partials, added in slice order (the next exchange write is several
          // barriers away: one slot per wave is enough)
          const unsigned ex = lw_lds_addr(lds + C::EXCH_OFF + jt * DS * 4096) + lane * 16;
#pragma unroll
          for (int i = 0; i < DS; ++i) {
            f32x4 p[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) lw_lds_read(p[k], ex + i * 4096 + k * 1024);
            lw_lds_wait();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              lw_pin(p[k]);
#pragma unroll
              for (int m = 0; m < 4; ++m) acc[4 * k + m] = i == 0 ? p[k][m] : acc[4 * k + m] + p[k][m];
            }
          }
        }
        f32x4 y4[4];
        const unsigned la = lw_lds_addr(lab + (kt & 1) * LW_LABEL_BYTES) + 64 * h;
        if constexpr (LK::HAS_OFFSET) {
          // the slot's second half joins the accumulator first, so that its four registers are free
          // again before the first half is read (a round trip to LDS per tile, against 12 DW MFMAs)
#pragma unroll
          for (int k = 0; k < 4; ++k) lw_lds_read(y4[k], la + LW_LABEL_BYTES / 2 + 16 * k);
          lw_lds_wait();
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            lw_pin(y4[k]);
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[4 * k + m] += y4[k][m];
          }
        }
        float res[16];
        if constexpr (LK::LATENT) {
          // the counts come four rows at a time (three more LDS round trips per tile): with two float
          // and two float64 values more than Poisson's live across the loop, sixteen counts beside the
          // epilogue's temporaries would not fit the widest slices' registers
          if (sl == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              lw_lds_read(y4[0], la + 16 * k);
              lw_lds_wait();
              lw_pin(y4[0]);
              lw_epilogue_negbin<true>(acc, k, y4[0], lu, phi, res, pe, pe2, pe3);
            }
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              lw_lds_read(y4[0], la + 16 * k);
              lw_lds_wait();
              lw_pin(y4[0]);
              lw_epilogue_negbin<false>(acc, k, y4[0], lu, phi, res, pe, pe2, pe3);
            }
          }
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) lw_lds_read(y4[k], la + 16 * k);
          lw_lds_wait();
#pragma unroll
          for (int k = 0; k < 4; ++k) lw_pin(y4[k]);
          if (sl == 0) LK::template epilogue<true>(acc, y4, res, pe);
          else LK::template epilogue<false>(acc, y4, res, pe);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          float v[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = res[8 * s + j];
          nmx_split3(v, rs[s][0], rs[s][1], rs[s][2]);
        }
      }
      const unsigned slot = lw_lds_addr(ring + ((kt * C::NCH + DTS + dt) % R) * LW_CHUNK) + lane * 16;
      nmx_bf16x8 bt[3][2];
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int s = 0; s < 2; ++s) lw_lds_read(bt[p][s], slot + (2 * p + s) * 1024);
      lw_lds_wait();
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int s = 0; s < 2; ++s) lw_pin(bt[p][s]);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        g[dt] = nmx_mma_bf16(bt[2][s], rs[s][0], g[dt]);
        g[dt] = nmx_mma_bf16(bt[1][s], rs[s][1], g[dt]);
        g[dt] = nmx_mma_bf16(bt[0][s], rs[s][2], g[dt]);
        g[dt] = nmx_mma_bf16(bt[1][s], rs[s][0], g[dt]);
        g[dt] = nmx_mma_bf16(bt[0][s], rs[s][1], g[dt]);
        g[dt] = nmx_mma_bf16(bt[0][s], rs[s][0], g[dt]);
      }
    }
  }
  // a split without a tile stores its zeros: the finalize adds every slab
  if (c < 0) return;
  NMX_DCHECK(pos < ldc);
#pragma unroll
  for (int dt = 0; dt < DTS; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d = d0 + 32 * dt + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (d < D) gpart[((size_t)split * D + d) * ldc + pos] = g[dt][r];
    }
  if (sl == 0) {
    // the two lane halves hold the rows' two halves; lane + 32 is the same chain
    const double p = pe + __shfl_xor(pe, 32);
    if (h == 0) pepart[(size_t)split * LK::NPE * ldc + pos] = p;
    if constexpr (LK::NPE == 3) {
      const double p2 = pe2 + __shfl_xor(pe2, 32), p3 = pe3 + __shfl_xor(pe3, 32);
      if (h == 0) {
        pepart[((size_t)split * 3 + 1) * ldc + pos] = p2;
        pepart[((size_t)split * 3 + 2) * ldc + pos] = p3;
      }
    }
  }
}

// ---- lk_negbin's eta-free term.  The forms of NMX_OP_LRISING (nmx_program.h: the same branches, shift
// and series, whose cuts are below 1e-11) in float64, for whole k >= 0:
//   nb_lrising(a, k)    = lgamma(a + k) - lgamma(a) - k log(a)
//   nb_lrising_da(a, k) = digamma(a + k) - digamma(a) - k / a
// a = +inf or a = 0 (a chain whose u left float32's exp range) gives NaN: that chain's own U.
__device__ __forceinline__ double nb_log1pmx(double t) {  // log1p(t) - t, t >= 0
  if (!(t < 0.5)) return log1p(t) - t;
  const double s = t / (2.0 + t), s2 = s * s;
  double odd = 1.0 / 15 + s2 * (1.0 / 17);
  odd = 1.0 / 9 + s2 * (1.0 / 11 + s2 * (1.0 / 13 + s2 * odd));
  odd = 1.0 / 3 + s2 * (1.0 / 5 + s2 * (1.0 / 7 + s2 * odd));
  return s * (2.0 * s2 * odd - t);
}
__device__ __forceinline__ double nb_stirling_s(double x) {  // lgamma's Stirling tail, x >= 8
  const double r = 1.0 / x, r2 = r * r;
  return (1.0 / 12 - (1.0 / 360 - (1.0 / 1260 - (1.0 / 1680) * r2) * r2) * r2) * r;
}
__device__ __forceinline__ double nb_stirling_ds(double x) {
  const double r = 1.0 / x, r2 = r * r;
  return -r2 * (1.0 / 12 - r2 * (1.0 / 120 - r2 * (1.0 / 252 - r2 * (1.0 / 240))));
}
constexpr int NB_SUM_MAX = 8;  // NMX_LRISING_SUM_MAX
__device__ __forceinline__ void nb_lrising(double a, double k, double& val, double& da) {
  if (!(a > 0.0)) {
    val = da = NAN;
    return;
  }
  if (k <= (double)NB_SUM_MAX) {
    double s = 0.0, t = 0.0;
    for (int j = 1; j < NB_SUM_MAX; ++j)
      if ((double)j < k) {
        s += log1p((double)j / a);
        t += (double)j / (a * (a + (double)j));
      }
    val = s, da = -t;
    return;
  }
  double x = a, shift = 0.0, dshift = 0.0, m = 0.0;
  for (int j = 0; j < 8 && x < 8.0; ++j) {
    shift += log1p(k / x);
    dshift += k / (x * (x + k));
    x += 1.0;
    m += 1.0;
  }
  const double t = k / x, lm = nb_log1pmx(t);
  val = x * lm + (k - 0.5) * log1p(t) + (nb_stirling_s(x + k) - nb_stirling_s(x)) + (k * log1p(m / a) - shift);
  da = lm + 0.5 * k / (x * (x + k)) + (nb_stirling_ds(x + k) - nb_stirling_ds(x)) + (dshift - k * m / (a * x));
}

// rise[pos] = sum_k m_k nb_lrising(phi, y_k) and rise[ldc + pos] = sum_k m_k nb_lrising_da(phi, y_k) of
// the chain at batch position pos, over the table's K = head[NB_K] pairs (y_k, m_k).  A workgroup is
// RS_CHAINS positions x RS_SLICES table slices: slice s adds the entries s, s + RS_SLICES, ... in
// table order, then the slices are added by a fixed tree.  The value depends on the table and the
// chain's u alone.  K is a few hundred for typical counts; K = n_rows is correct and merely slow.
constexpr int RS_THREADS = 256, RS_CHAINS = 8, RS_SLICES = RS_THREADS / RS_CHAINS;
__global__ __launch_bounds__(RS_THREADS) void k_negbin_rising(const double* __restrict__ table,
                                                              const double* __restrict__ head, int64_t n_rows, int D,
                                                              nmx_eval_batch ev, double* __restrict__ rise) {
  __shared__ double red[2][RS_SLICES][RS_CHAINS];
  const int ci = threadIdx.x % RS_CHAINS, sl = threadIdx.x / RS_CHAINS;
  const int pos = blockIdx.x * RS_CHAINS + ci;
  const int ldc = ev.ldc;
  const int c = pos < ldc ? nmx_eval_chain(ev, pos) : -1;
  int64_t K = (int64_t)head[NB_K];
  NMX_DCHECK(K >= 1 && K <= n_rows);
  if (K > n_rows) K = n_rows;  // the table's capacity
  double r = 0.0, d = 0.0;
  if (c >= 0) {
    const double phi = (double)nb_phi(ev.z[(size_t)D * ldc + c]);
    for (int64_t k = sl; k < K; k += RS_SLICES) {
      double v, dv;
      nb_lrising(phi, table[2 * k], v, dv);
      r += table[2 * k + 1] * v;
      d += table[2 * k + 1] * dv;
    }
  }
  red[0][sl][ci] = r;
  red[1][sl][ci] = d;
  __syncthreads();
  for (int k = RS_SLICES / 2; k > 0; k >>= 1) {
    if (sl < k) {
      red[0][sl][ci] += red[0][sl + k][ci];
      red[1][sl][ci] += red[1][sl + k][ci];
    }
    __syncthreads();
  }
  if (sl == 0 && c >= 0) {
    rise[pos] = red[0][0][ci];
    rise[(size_t)ldc + pos] = red[1][0][ci];
  }
}

// One workgroup per (64 batch positions, coordinate j or the U row j = D).  Wave w sums the slabs
// [w S / 4, (w + 1) S / 4) in order -- and, on the U row, its quarter of the coordinates'
// z^2 / 2 - xty z in float64 -- then the four wave sums are added in wave order.  A policy with a
// head adds its float64 constant (xty[LW_MAX_D]) once per chain, last.
// lk_negbin has the rows j = D (dU/du) and j = D + 1 (U): both sum the three pepart rows of every
// split the same way (the coordinates' part joins S2 on the U row), then combine them in float64 with
// phi = nb_phi(u), k_negbin_rising's two rows (behind the pepart slabs), the head and the Gamma prior.
constexpr int FIN_WAVES = 4;
template <class LK>
__global__ __launch_bounds__(64 * FIN_WAVES) void k_logreg_wide_finalize(const float* __restrict__ gpart,
                                                                         const double* __restrict__ pepart, int S,
                                                                         int D, nmx_eval_batch ev,
                                                                         const double* __restrict__ xty) {
  __shared__ double part[LK::NPE][FIN_WAVES][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int pos = blockIdx.x * 64 + lane;
  const int j = blockIdx.y;
  const int ldc = ev.ldc;
  const int c = pos < ldc ? nmx_eval_chain(ev, pos) : -1;
  const int sp0 = w * S / FIN_WAVES, sp1 = (w + 1) * S / FIN_WAVES;
  if (c >= 0) {
    double s = 0.0;
    if (j < D) {
      float f = 0.0f;
      for (int sp = sp0; sp < sp1; ++sp) f += gpart[((size_t)sp * D + j) * ldc + pos];
      s = f;
    } else {
      [[maybe_unused]] double s2 = 0.0, s3 = 0.0;
      for (int sp = sp0; sp < sp1; ++sp) {
        s += pepart[(size_t)sp * LK::NPE * ldc + pos];
        if constexpr (LK::NPE == 3) {
          s2 += pepart[((size_t)sp * 3 + 1) * ldc + pos];
          s3 += pepart[((size_t)sp * 3 + 2) * ldc + pos];
        }
      }
      double q = 0.0;
      if (!LK::LATENT || j == D + 1) {
        const int j0 = w * D / FIN_WAVES, j1 = (w + 1) * D / FIN_WAVES;
        for (int jj = j0; jj < j1; ++jj) {
          const double z = ev.z[(size_t)jj * ldc + c];
          q += 0.5 * z * z - xty[jj] * z;
        }
      }
      if constexpr (LK::NPE == 3) {
        part[1][w][lane] = s2 + q;
        part[2][w][lane] = s3;
      } else {
        s += q;
      }
    }
    part[0][w][lane] = s;
  }
  __syncthreads();
  if (w != 0 || c < 0) return;
  if (j < D) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < FIN_WAVES; ++i) s += (float)part[0][i][lane];
    const size_t idx = (size_t)j * ldc + c;
    ev.grad[idx] = ev.z[idx] + s;
  } else if constexpr (LK::LATENT) {
    double S1 = 0.0, S2 = 0.0, S3 = 0.0;
#pragma unroll
    for (int i = 0; i < FIN_WAVES; ++i) {
      S1 += part[0][i][lane];
      S2 += part[1][i][lane];
      S3 += part[2][i][lane];
    }
    const double* head = xty + LW_MAX_D;
    const double* rise = pepart + (size_t)S * 3 * ldc;
    const size_t iu = (size_t)D * ldc + c;
    const float uf = ev.z[iu];
    const double u = uf, phi = nb_phi(uf), a = head[NB_A], b = head[NB_B];
    if (j == D)
      ev.grad[iu] = (float)(phi * S1 - S3 - phi * rise[(size_t)ldc + pos] - head[NB_SUMY] - a + b * phi);
    else
      ev.pe[c] = (float)(phi * S1 + S2 + 0.9189385332046727 * D + head[0] - rise[pos] - (a * u - b * phi) +
                         head[NB_PRIOR]);
  } else {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < FIN_WAVES; ++i) s += part[0][i][lane];
    s += 0.9189385332046727 * D;
    if constexpr (LK::HEAD_BYTES > 0) s += xty[LW_MAX_D];
    ev.pe[c] = (float)s;
  }
}

// The horseshoe's finalize (see the header): k_horseshoe_finalize per (64 positions, block of
// HS_BLOCK coordinates), then k_horseshoe_tau per 64 positions.  upart / tpart are [NB][ldc] float64
// rows of the workspace, indexed by position like pepart.
constexpr int HS_BLOCK = 8, HS_PER_WAVE = HS_BLOCK / FIN_WAVES;
constexpr double HS_LOG_HALF_PI = 0.4515827052894548, HS_HALF_LOG_2PI = 0.9189385332046727;
inline int hs_num_blocks(int D) { return (D + HS_BLOCK - 1) / HS_BLOCK; }

// log(2 cosh u): -log of HalfCauchy(1)'s density at exp(u) times the Jacobian exp(u), less log(pi / 2)
__device__ __forceinline__ double hs_log2cosh(double u) {
  const double a = fabs(u);
  return a + log1p(exp(-2.0 * a));
}

__global__ __launch_bounds__(64 * FIN_WAVES) void k_horseshoe_finalize(const float* __restrict__ gpart, int S, int D,
                                                                       nmx_eval_batch ev,
                                                                       const double* __restrict__ xty,
                                                                       double* __restrict__ upart,
                                                                       double* __restrict__ tpart) {
  __shared__ double part[2][FIN_WAVES][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int pos = blockIdx.x * 64 + lane;
  const int blk = blockIdx.y;
  const int ldc = ev.ldc;
  const int c = pos < ldc ? nmx_eval_chain(ev, pos) : -1;
  const int Q = S / FIN_WAVES;  // S is a multiple of 8 (lw_num_splits)
  double u = 0.0, t = 0.0;
  if (c >= 0) {
    const float ut = ev.z[(size_t)D * ldc + c];
    for (int k = 0; k < HS_PER_WAVE; ++k) {
      const int j = blk * HS_BLOCK + w * HS_PER_WAVE + k;
      if (j >= D) break;
      // the plain finalize's order: the four quarters of the slabs, each in slab order, then q0..q3
      float f[FIN_WAVES] = {0.0f, 0.0f, 0.0f, 0.0f};
      for (int i = 0; i < Q; ++i)
#pragma unroll
        for (int q = 0; q < FIN_WAVES; ++q) {
          NMX_DCHECK(q * Q + i < S && j < D && pos < ldc);
          f[q] += gpart[((size_t)(q * Q + i) * D + j) * ldc + pos];
        }
      float G = 0.0f;
#pragma unroll
      for (int q = 0; q < FIN_WAVES; ++q) G += f[q];
      const size_t iul = (size_t)j * ldc + c, iz = (size_t)(D + 1 + j) * ldc + c;
      const float ul = ev.z[iul], z = ev.z[iz];
      float s, beta;
      hs_coef(ul, ut, z, s, beta);
      ev.grad[iz] = s * G + z;
      ev.grad[iul] = beta * G + tanhf(ul);
      t += (double)beta * (double)G;
      u += hs_log2cosh((double)ul) + 0.5 * (double)z * (double)z - xty[j] * (double)beta;
    }
  }
  part[0][w][lane] = u;
  part[1][w][lane] = t;
  __syncthreads();
  if (w != 0 || c < 0) return;
  u = 0.0, t = 0.0;
#pragma unroll
  for (int i = 0; i < FIN_WAVES; ++i) {
    u += part[0][i][lane];
    t += part[1][i][lane];
  }
  upart[(size_t)blk * ldc + pos] = u;
  tpart[(size_t)blk * ldc + pos] = t;
}

template <class LK>
__global__ __launch_bounds__(64 * FIN_WAVES) void k_horseshoe_tau(const double* __restrict__ pepart,
                                                                  const double* __restrict__ upart,
                                                                  const double* __restrict__ tpart, int S, int D,
                                                                  int NB, nmx_eval_batch ev,
                                                                  const double* __restrict__ xty) {
  __shared__ double part[2][FIN_WAVES][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int pos = blockIdx.x * 64 + lane;
  const int ldc = ev.ldc;
  const int c = pos < ldc ? nmx_eval_chain(ev, pos) : -1;
  double u = 0.0, t = 0.0;
  if (c >= 0) {
    for (int sp = w * S / FIN_WAVES; sp < (w + 1) * S / FIN_WAVES; ++sp) u += pepart[(size_t)sp * ldc + pos];
    double ub = 0.0;
    for (int b = w * NB / FIN_WAVES; b < (w + 1) * NB / FIN_WAVES; ++b) {
      NMX_DCHECK(b < NB);
      ub += upart[(size_t)b * ldc + pos];
      t += tpart[(size_t)b * ldc + pos];
    }
    u += ub;
  }
  part[0][w][lane] = u;
  part[1][w][lane] = t;
  __syncthreads();
  if (w != 0 || c < 0) return;
  u = 0.0, t = 0.0;
#pragma unroll
  for (int i = 0; i < FIN_WAVES; ++i) {
    u += part[0][i][lane];
    t += part[1][i][lane];
  }
  const size_t iut = (size_t)D * ldc + c;
  const double ut = ev.z[iut];
  ev.grad[iut] = (float)(t + tanh(ut));
  u += hs_log2cosh(ut) + (D + 1) * HS_LOG_HALF_PI + D * HS_HALF_LOG_2PI;
  if constexpr (LK::HEAD_BYTES > 0) u += xty[LW_MAX_D];
  ev.pe[c] = (float)u;
}

bool lw_shape_ok(int64_t n_rows, int dim, int min_d) { return n_rows > 0 && dim >= min_d && dim <= LW_MAX_D; }

int lw_check_shape(const char* name, const char* fn, int64_t n_rows, int dim, int min_d) {
  if (n_rows <= 0)
    return nmx_fail(NMX_ERR_INVALID, "%s_%s: need n_rows >= 1 (got n_rows = %lld)", name, fn, (long long)n_rows);
  if (dim < min_d || dim > LW_MAX_D)
    return nmx_fail(NMX_ERR_INVALID, "%s_%s: need %d <= dim <= %d (got dim = %d)", name, fn, min_d, LW_MAX_D, dim);
  // a split's tiles are addressed by 32-bit byte offsets
  const int64_t per = lw_ntiles(n_rows) / lw_num_splits(n_rows, dim) + 1;
  if (per * (int64_t)lw_tile_bytes(dim) >= (int64_t)1 << 31)
    return nmx_fail(NMX_ERR_INVALID, "%s_%s: n_rows = %lld is past the kernel's 2 GiB of tiles per row split", name, fn,
                    (long long)n_rows);
  return NMX_OK;
}

struct lw_args {
  dim3 grid;
  hipStream_t s;
  const char* Xq;
  int64_t nt;
  int D, S, Gt;
  const nmx_eval_batch& ev;
  float* gpart;
  double* pepart;
};
template <class LK, class PR, int CT, int DS, int DTS, int R>
int lw_launch(const lw_args& a) {
  using C = lw_cfg<CT, DS, DTS, R>;
  if (int st = nmx_lds_limit((const void*)k_logreg_wide<LK, PR, CT, DS, DTS, R>, C::LDS_BYTES, a.s, "k_logreg_wide"))
    return st;
  hipLaunchKernelGGL((k_logreg_wide<LK, PR, CT, DS, DTS, R>), a.grid, dim3(64 * C::WAVES), C::LDS_BYTES, a.s, a.Xq, a.nt,
                     a.D, a.S, a.Gt, a.ev, a.gpart, a.pepart);
  return NMX_OK;
}
// DTS = 3 or 4 from 65 features on; 1 or 2 below, in the 4 x 1 class of policies that serve them
template <class LK, class PR, int CT, int DS, int R>
int lw_launch_dts(int DTS, const lw_args& a) {
  if constexpr (lw_min_d<LK, PR>() <= 64 && DS == 1) {
    if (DTS == 1) return lw_launch<LK, PR, CT, DS, 1, R>(a);
    if (DTS == 2) return lw_launch<LK, PR, CT, DS, 2, R>(a);
  }
  if (DTS == 3) return lw_launch<LK, PR, CT, DS, 3, R>(a);
  return lw_launch<LK, PR, CT, DS, 4, R>(a);
}

// The four entry points of a pair of policies (the pack is the likelihood's alone).
template <class LK, class PR = pr_normal>
size_t lw_packed_bytes(int64_t n_rows, int dim) {
  if (!lw_shape_ok(n_rows, dim, lw_min_d<LK, PR>())) return 0;
  return LW_XTY_BYTES + LK::HEAD_BYTES + (size_t)lw_ntiles(n_rows) * lw_tile_bytes(dim) +
         (size_t)n_rows * LK::TAIL_PER_ROW;
}

template <class LK>
int lw_pack(const float* X, const float* y, const float* off, int64_t n_rows, int dim, void* packed, hipStream_t s) {
  hipLaunchKernelGGL(k_logreg_wide_colsums, dim3(dim), dim3(CS_THREADS), 0, s, X, y, n_rows, dim, (double*)packed);
  if (int st = nmx_check_launch("k_logreg_wide_colsums")) return st;
  const lw_shape c = lw_class(dim);
  const int64_t nt = lw_ntiles(n_rows);
  const int64_t nthreads = nt * (int64_t)(lw_tile_bytes(dim) / 16);
  hipLaunchKernelGGL(k_logreg_wide_pack<LK>, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, s, X, y, off,
                     n_rows, dim, c.DS, c.DTS, nt, (char*)packed + LW_XTY_BYTES + LK::HEAD_BYTES);
  return nmx_check_launch("k_logreg_wide_pack");
}

// workspace: the gradient slabs | the U slabs, LK::NPE rows per split | (horseshoe) the blocks' U rows |
// their beta G rows | (lk_negbin) k_negbin_rising's two rows
template <class LK, class PR = pr_normal>
size_t lw_workspace_bytes(int64_t n_rows, int dim, int num_chains) {
  if (!lw_shape_ok(n_rows, dim, lw_min_d<LK, PR>()) || num_chains <= 0) return 0;
  const size_t ldc = (size_t)(num_chains + 63) / 64 * 64;
  const size_t S = lw_num_splits(n_rows, dim);
  const size_t g = S * dim * ldc * sizeof(float);
  const size_t p =
      (S * LK::NPE + (PR::HORSESHOE ? 2 * hs_num_blocks(dim) : 0) + (LK::LATENT ? 2 : 0)) * ldc * sizeof(double);
  return (g + 255) / 256 * 256 + p;
}

template <class LK, class PR = pr_normal>
int lw_pe_grad(const void* packed, int64_t n_rows, int dim, const nmx_eval_batch* ev, void* workspace, void* stream) {
  constexpr const char* NAME = lw_name<LK, PR>();
  if (int st = lw_check_shape(NAME, "pe_grad", n_rows, dim, lw_min_d<LK, PR>())) return st;
  if (!ev || !ev->z || !ev->grad || !ev->pe)
    return nmx_fail(NMX_ERR_INVALID, "%s_pe_grad: eval batch has NULL pointers", NAME);
  if (ev->num_chains <= 0 || ev->ldc < ev->num_chains || ev->ldc % 64)
    return nmx_fail(NMX_ERR_INVALID, "%s_pe_grad: bad num_chains/ldc (%d/%d)", NAME, ev->num_chains, ev->ldc);
  if (!packed || !workspace) return nmx_fail(NMX_ERR_INVALID, "%s_pe_grad: NULL packed/workspace", NAME);
  hipStream_t s = (hipStream_t)stream;
  const int S = lw_num_splits(n_rows, dim);
  float* gpart = (float*)workspace;
  double* pepart = (double*)((char*)workspace + ((size_t)S * dim * ev->ldc * sizeof(float) + 255) / 256 * 256);
  const lw_shape c = lw_class(dim);
  const int nb = std::min(ev->num_chains, ev->ldc);  // batch positions that can hold a chain
  const int Gt = (nb + 32 * c.CT - 1) / (32 * c.CT);
  const lw_args a = {dim3((unsigned)Gt * S), s,  (const char*)packed + LW_XTY_BYTES + LK::HEAD_BYTES,
                     lw_ntiles(n_rows),      dim, S, Gt, *ev, gpart, pepart};
  int st;
  if (c.DS == 1) st = lw_launch_dts<LK, PR, 4, 1, 3>(c.DTS, a);
  else if (c.DS == 2) st = lw_launch_dts<LK, PR, 4, 2, 3>(c.DTS, a);
  else if (c.DS == 4) st = lw_launch_dts<LK, PR, 2, 4, 3>(c.DTS, a);
  else st = lw_launch_dts<LK, PR, 1, 8, 2>(c.DTS, a);
  if (st) return st;
  if (int e = nmx_check_launch("k_logreg_wide")) return e;
  if constexpr (LK::LATENT) {
    const double* head = (const double*)((const char*)packed + LW_XTY_BYTES);
    const double* table = (const double*)(a.Xq + (size_t)a.nt * lw_tile_bytes(dim));
    hipLaunchKernelGGL(k_negbin_rising, dim3((nb + RS_CHAINS - 1) / RS_CHAINS), dim3(RS_THREADS), 0, s, table, head,
                       n_rows, dim, *ev, pepart + (size_t)S * LK::NPE * ev->ldc);
    if (int e = nmx_check_launch("k_negbin_rising")) return e;
  }
  if constexpr (PR::HORSESHOE) {
    const int NB = hs_num_blocks(dim);
    double* upart = pepart + (size_t)S * ev->ldc;
    double* tpart = upart + (size_t)NB * ev->ldc;
    hipLaunchKernelGGL(k_horseshoe_finalize, dim3((nb + 63) / 64, NB), dim3(64 * FIN_WAVES), 0, s, gpart, S, dim, *ev,
                       (const double*)packed, upart, tpart);
    if (int e = nmx_check_launch("k_horseshoe_finalize")) return e;
    hipLaunchKernelGGL(k_horseshoe_tau<LK>, dim3((nb + 63) / 64), dim3(64 * FIN_WAVES), 0, s, pepart, upart, tpart, S,
                       dim, NB, *ev, (const double*)packed);
    return nmx_check_launch("k_horseshoe_tau");
  } else {
    hipLaunchKernelGGL(k_logreg_wide_finalize<LK>, dim3((nb + 63) / 64, dim + 1 + LK::LATENT), dim3(64 * FIN_WAVES), 0,
                       s, gpart, pepart, S, dim, *ev, (const double*)packed);
    return nmx_check_launch("k_logreg_wide_finalize");
  }
}

// Synchronises the stream once, to refuse a bad count before anything is packed.
int lw_poisson_pack(const char* name, const float* X, const float* y, const float* offset, int64_t n_rows, int dim,
                    void* packed, hipStream_t s) {
  double* head = (double*)((char*)packed + LW_XTY_BYTES);
  unsigned long long* bad = (unsigned long long*)(head + 1);
  hipLaunchKernelGGL(k_poisson_bad_reset, dim3(1), dim3(1), 0, s, bad);
  hipLaunchKernelGGL(k_poisson_const, dim3(1), dim3(CS_THREADS), 0, s, y, offset, n_rows, head, bad);
  if (int st = nmx_check_launch("k_poisson_const")) return st;
  unsigned long long first = 0;
  if (hipMemcpyAsync(&first, bad, sizeof(first), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return nmx_fail(NMX_ERR_HIP, "%s_pack: reading the count check back failed", name);
  if (first != ~0ull)
    return nmx_fail(NMX_ERR_INVALID, "%s_pack: the count of row %llu is not a whole number in [0, 2^24)", name, first);
  return lw_pack<lk_poisson>(X, y, offset, n_rows, dim, packed, s);
}

// Negative-binomial pack: Poisson's count check, constant, X^T y and tiles, then the head's scalars and
// the table of distinct counts, built on the host from the copy of y that comes back with the check
// (sorted, run lengths as float64; sum y is exact, whole numbers below 2^53).  Two synchronisations:
// the check with the copy of y, and the upload from the pinned staging buffer before it is freed.
int lw_negbin_pack(const float* X, const float* y, const float* offset, int64_t n_rows, int dim, double prior_a,
                   double prior_b, void* packed, hipStream_t s) {
  double* head = (double*)((char*)packed + LW_XTY_BYTES);
  unsigned long long* bad = (unsigned long long*)(head + 1);
  hipLaunchKernelGGL(k_poisson_bad_reset, dim3(1), dim3(1), 0, s, bad);
  hipLaunchKernelGGL(k_poisson_const, dim3(1), dim3(CS_THREADS), 0, s, y, offset, n_rows, head, bad);
  if (int st = nmx_check_launch("k_poisson_const")) return st;
  // pinned staging: the table's n_rows pairs | NB_HEAD_END scalars | the copy of y
  const size_t tab_bytes = (size_t)n_rows * lk_negbin::TAIL_PER_ROW;
  char* stage = nullptr;
  if (hipHostMalloc((void**)&stage, tab_bytes + NB_HEAD_END * sizeof(double) + (size_t)n_rows * sizeof(float)) !=
      hipSuccess)
    return nmx_fail(NMX_ERR_HIP, "negbin_pack: no pinned staging memory for %lld counts", (long long)n_rows);
  double* tab = (double*)stage;
  double* hs = tab + 2 * n_rows;
  float* hy = (float*)(hs + NB_HEAD_END);
  unsigned long long* first = (unsigned long long*)hs;  // read before the scalars are written
  int st = NMX_OK;
  if (hipMemcpyAsync(hy, y, (size_t)n_rows * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(first, bad, sizeof(*first), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    st = nmx_fail(NMX_ERR_HIP, "negbin_pack: reading the count check back failed");
  else if (*first != ~0ull)
    st = nmx_fail(NMX_ERR_INVALID, "negbin_pack: the count of row %llu is not a whole number in [0, 2^24)", *first);
  if (st == NMX_OK) {
    std::sort(hy, hy + n_rows);
    int64_t K = 0;
    double sumy = 0.0;
    for (int64_t i = 0; i < n_rows; ++i) {
      if (i == 0 || hy[i] != hy[i - 1]) {
        tab[2 * K] = hy[i];
        tab[2 * K + 1] = 0.0;
        ++K;
      }
      tab[2 * K - 1] += 1.0;
      sumy += hy[i];
    }
    hs[NB_A] = prior_a, hs[NB_B] = prior_b, hs[NB_PRIOR] = lgamma(prior_a) - prior_a * log(prior_b);
    hs[NB_K] = (double)K, hs[NB_SUMY] = sumy;
    char* tiles = (char*)packed + LW_XTY_BYTES + lk_negbin::HEAD_BYTES;
    if (hipMemcpyAsync(head + NB_A, hs + NB_A, (NB_HEAD_END - NB_A) * sizeof(double), hipMemcpyHostToDevice, s) !=
            hipSuccess ||
        hipMemcpyAsync(tiles + (size_t)lw_ntiles(n_rows) * lw_tile_bytes(dim), tab, (size_t)K * 2 * sizeof(double),
                       hipMemcpyHostToDevice, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      st = nmx_fail(NMX_ERR_HIP, "negbin_pack: writing the table of counts failed");
  }
  (void)hipHostFree(stage);
  if (st) return st;
  return lw_pack<lk_poisson>(X, y, offset, n_rows, dim, packed, s);
}

}  // namespace

extern "C" size_t nmx_logreg_wide_packed_bytes(int64_t n_rows, int dim) {
  return lw_packed_bytes<lk_bernoulli>(n_rows, dim);
}

extern "C" int nmx_logreg_wide_pack(const float* X, const float* y, int64_t n_rows, int dim, void* packed,
                                    void* stream) {
  if (int st = lw_check_shape("logreg_wide", "pack", n_rows, dim, lk_bernoulli::MIN_D)) return st;
  if (!X || !y || !packed) return nmx_fail(NMX_ERR_INVALID, "logreg_wide_pack: NULL pointer");
  return lw_pack<lk_bernoulli>(X, y, nullptr, n_rows, dim, packed, (hipStream_t)stream);
}

extern "C" size_t nmx_logreg_wide_workspace_bytes(int64_t n_rows, int dim, int num_chains) {
  return lw_workspace_bytes<lk_bernoulli>(n_rows, dim, num_chains);
}

extern "C" int nmx_logreg_wide_pe_grad(const void* packed, int64_t n_rows, int dim, const nmx_eval_batch* ev,
                                       void* workspace, void* stream) {
  return lw_pe_grad<lk_bernoulli>(packed, n_rows, dim, ev, workspace, stream);
}

extern "C" size_t nmx_poisson_packed_bytes(int64_t n_rows, int dim) { return lw_packed_bytes<lk_poisson>(n_rows, dim); }

// Synchronises the stream once, to refuse a bad count before anything is packed.
extern "C" int nmx_poisson_pack(const float* X, const float* y, const float* offset, int64_t n_rows, int dim,
                                void* packed, void* stream) {
  if (int st = lw_check_shape("poisson", "pack", n_rows, dim, lk_poisson::MIN_D)) return st;
  if (!X || !y || !packed) return nmx_fail(NMX_ERR_INVALID, "poisson_pack: NULL pointer");
  return lw_poisson_pack("poisson", X, y, offset, n_rows, dim, packed, (hipStream_t)stream);
}

extern "C" size_t nmx_poisson_workspace_bytes(int64_t n_rows, int dim, int num_chains) {
  return lw_workspace_bytes<lk_poisson>(n_rows, dim, num_chains);
}

extern "C" int nmx_poisson_pe_grad(const void* packed, int64_t n_rows, int dim, const nmx_eval_batch* ev,
                                   void* workspace, void* stream) {
  return lw_pe_grad<lk_poisson>(packed, n_rows, dim, ev, workspace, stream);
}

// Negative-binomial regression: `dim` is the number of features D, the arena has D + 1 rows.
extern "C" size_t nmx_negbin_packed_bytes(int64_t n_rows, int dim) { return lw_packed_bytes<lk_negbin>(n_rows, dim); }

extern "C" int nmx_negbin_pack(const float* X, const float* y, const float* offset, int64_t n_rows, int dim,
                               double prior_a, double prior_b, void* packed, void* stream) {
  if (int st = lw_check_shape("negbin", "pack", n_rows, dim, lk_negbin::MIN_D)) return st;
  if (!X || !y || !packed) return nmx_fail(NMX_ERR_INVALID, "negbin_pack: NULL pointer");
  if (!(prior_a > 0.0 && prior_a < INFINITY && prior_b > 0.0 && prior_b < INFINITY))
    return nmx_fail(NMX_ERR_INVALID, "negbin_pack: the Gamma prior needs finite a, b > 0 (got %g, %g)", prior_a,
                    prior_b);
  return lw_negbin_pack(X, y, offset, n_rows, dim, prior_a, prior_b, packed, (hipStream_t)stream);
}

extern "C" size_t nmx_negbin_workspace_bytes(int64_t n_rows, int dim, int num_chains) {
  return lw_workspace_bytes<lk_negbin>(n_rows, dim, num_chains);
}

extern "C" int nmx_negbin_pe_grad(const void* packed, int64_t n_rows, int dim, const nmx_eval_batch* ev,
                                  void* workspace, void* stream) {
  return lw_pe_grad<lk_negbin>(packed, n_rows, dim, ev, workspace, stream);
}

// Horseshoe-prior regression: `likelihood` is 0 (Bernoulli logits) or 1 (Poisson, log link); `dim`
// is the number of features D, the arena has 2 D + 1 rows.
namespace {
int hs_check_likelihood(const char* fn, int likelihood) {
  if (likelihood == 0 || likelihood == 1) return NMX_OK;
  return nmx_fail(NMX_ERR_INVALID, "horseshoe_%s: likelihood is 0 (Bernoulli) or 1 (Poisson) (got %d)", fn, likelihood);
}
}  // namespace

extern "C" size_t nmx_horseshoe_packed_bytes(int likelihood, int64_t n_rows, int dim) {
  if (likelihood == 0) return lw_packed_bytes<lk_bernoulli, pr_horseshoe>(n_rows, dim);
  return likelihood == 1 ? lw_packed_bytes<lk_poisson, pr_horseshoe>(n_rows, dim) : 0;
}

extern "C" int nmx_horseshoe_pack(int likelihood, const float* X, const float* y, const float* offset, int64_t n_rows,
                                  int dim, void* packed, void* stream) {
  if (int st = hs_check_likelihood("pack", likelihood)) return st;
  if (int st = lw_check_shape("horseshoe", "pack", n_rows, dim, 1)) return st;
  if (!X || !y || !packed) return nmx_fail(NMX_ERR_INVALID, "horseshoe_pack: NULL pointer");
  if (likelihood == 1) return lw_poisson_pack("horseshoe", X, y, offset, n_rows, dim, packed, (hipStream_t)stream);
  if (offset) return nmx_fail(NMX_ERR_INVALID, "horseshoe_pack: the Bernoulli likelihood takes no offset");
  return lw_pack<lk_bernoulli>(X, y, nullptr, n_rows, dim, packed, (hipStream_t)stream);
}

extern "C" size_t nmx_horseshoe_workspace_bytes(int likelihood, int64_t n_rows, int dim, int num_chains) {
  if (likelihood == 0) return lw_workspace_bytes<lk_bernoulli, pr_horseshoe>(n_rows, dim, num_chains);
  return likelihood == 1 ? lw_workspace_bytes<lk_poisson, pr_horseshoe>(n_rows, dim, num_chains) : 0;
}

extern "C" int nmx_horseshoe_pe_grad(int likelihood, const void* packed, int64_t n_rows, int dim,
                                     const nmx_eval_batch* ev, void* workspace, void* stream) {
  if (int st = hs_check_likelihood("pe_grad", likelihood)) return st;
  if (likelihood == 0) return lw_pe_grad<lk_bernoulli, pr_horseshoe>(packed, n_rows, dim, ev, workspace, stream);
  return lw_pe_grad<lk_poisson, pr_horseshoe>(packed, n_rows, dim, ev, workspace, stream);
}
