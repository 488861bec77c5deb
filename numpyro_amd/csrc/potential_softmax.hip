// Softmax (multinomial logistic) regression potential + gradient for thousands of chains:
// coefs ~ N(0, 1)^(D x K), obs ~ Categorical(logits = X @ coefs).
//
//   U(W)  = sum_n [logsumexp_k l_nk - l_{n, y_n}] + sum_{d,k} [W_dk^2 / 2 + log(2 pi) / 2]
//   dU/dW = X^T (softmax(l) - onehot(y)) + W,      l = X W,   coordinate of W_dk = d K + k
//
// k_softmax: the sibling of k_logreg_x3 (potential_logreg.hip) with the column axis of the
// 32 x 32 tile cut as (chain, class).  KP = the power of two >= K; a wave's 32 columns are
// 32 / KP chains x KP classes, a chain's classes on KP adjacent lanes (column = cl KP + k).
// Classes k >= K are pad columns: their W fragment is zero and the epilogue sets their logit
// to -inf by lane index, so they take no part in max, sum or residual.
//
// Per 32-row tile a wave runs L = X . W (split-bf16, six products per 16-deep k-block, see
// "Split-bf16" below), the softmax epilogue on the accumulator registers, and G += X^T . R with
// the residual registers as the B operand (the accumulator holds the column on the lane and 16
// rows in the registers: the B layout of the 32x32x16 form with the k order permuted, which the
// packed X^T pieces follow).  The N x K x C logit tensor never exists in memory.
//
// Epilogue.  One row of one chain is KP adjacent lanes of one register: max and sum are xor
// butterflies over those lanes (ss_xor: DPP quad permutes for 1 and 2, the half-row and row
// mirrors for 4 and 8 -- after the earlier steps a mirror's partner holds the other subgroup's
// value -- and a swizzle for 16), log2(KP) steps each, all 16 registers.  Every lane of a group
// ends with the same bits (a + b and b + a are the same float), so
//   p = exp(l - m) / s,   lse = m + log s,   R = p - [k == y_row]
// need no broadcast.  Rows >= n_rows are MASKED: the pack gives them zero X and label -1, so their
// residual meets zero X^T columns and their lse is dropped by the label's sign.
//
// The linear part of U, sum_n l_{n, y_n} = <S, W> with S[d][k] = sum_{n: y_n = k} X[n][d], is a
// float64 table of the pack (k_softmax_colsums) added once per chain in the finalize; the row
// loop only accumulates lse (float64 per lane).  The gradient is the in-register residual, not
// X^T p - S, which would cancel at large N.
//
// Work split: workgroup = 4 waves = 4 column tiles sharing each X tile, which streams through a
// two-slot LDS ring by buffer LDS-DMA (one barrier per tile).  Grid = column-tile groups x S row
// splits, S a function of n_rows only (sm_num_splits) and split s owning the tiles
// [s T / S, (s + 1) T / S), each summed in tile order; the per-split slabs are added in a fixed
// order by k_softmax_finalize.  A chain's U and dU are therefore bitwise independent of how many
// chains share the launch, of its position and of the GPU count.
//
// The bf16 split helpers and the piece writers repeat those of potential_logreg.hip (that file
// stays untouched; sharing them through a header is a change of its own).
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "nmx_api_internal.h"
#include "nmx_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr int SM_ROWS = 32;
constexpr int SM_MAX_D = 64, SM_MAX_K = 32;
constexpr int SM_MAX_S = 64;

// Packed buffer: S[D K] float64 (room for 64 x 32) | the bad-label slot | the tiles
constexpr size_t SM_COL_BYTES = (size_t)SM_MAX_D * SM_MAX_K * sizeof(double);
constexpr size_t SM_BAD_OFFSET = SM_COL_BYTES;
constexpr size_t SM_TILE_OFFSET = SM_COL_BYTES + 256;

inline int sm_kb(int D) { return (D + 15) / 16; }
inline int sm_dt(int D) { return (D + 31) / 32; }
inline int sm_np(int D) { return 3 * sm_kb(D) + 6 * sm_dt(D) + 1; }
inline int sm_kp(int K) {
  int kp = 2;
  while (kp < K) kp *= 2;
  return kp;
}
inline int64_t sm_ntiles(int64_t n) { return (n + SM_ROWS - 1) / SM_ROWS; }

// Row splits: a function of n_rows only.  The column axis is K times longer than the binary
// kernel's, so fewer splits fill the device (one per 32 tiles, a multiple of 8 for the XCD
// placement, at most 64: the slabs are S D K ldc floats).
int sm_num_splits(int64_t n_rows) {
  int64_t s = sm_ntiles(n_rows) / 32;
  s = s / 8 * 8;
  if (s < 8) s = 8;
  if (s > SM_MAX_S) s = SM_MAX_S;
  return (int)s;
}

// ---------------------------------------------------------------------------------------
// Split-bf16: every f32 operand v is v1 + v2 + v3 with v1 = bf16(v), v2 = bf16(v - v1),
// v3 = bf16(v - v1 - v2) (the remainders are exact in f32); a product keeps the six terms with
// i + j <= 4, small terms first, each an exact bf16 x bf16 product accumulated in f32 by
// v_mfma_f32_32x32x16_bf16 (header comment of potential_logreg.hip).
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned pk_bf16(float a, float b) {
  const f32x2 v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ float pk_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float pk_hi(unsigned u) { return __uint_as_float(u & 0xFFFF0000u); }
__device__ __forceinline__ void split3(const float (&v)[8], bf16x8& b1, bf16x8& b2, bf16x8& b3) {
  u32x4 w1, w2, w3;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float x0 = v[2 * p], x1 = v[2 * p + 1];
    const unsigned u1 = pk_bf16(x0, x1);
    const float e0 = x0 - pk_lo(u1), e1 = x1 - pk_hi(u1);
    const unsigned u2 = pk_bf16(e0, e1);
    const float f0 = e0 - pk_lo(u2), f1 = e1 - pk_hi(u2);
    w1[p] = u1;
    w2[p] = u2;
    w3[p] = pk_bf16(f0, f1);
  }
  b1 = __builtin_bit_cast(bf16x8, w1);
  b2 = __builtin_bit_cast(bf16x8, w2);
  b3 = __builtin_bit_cast(bf16x8, w3);
}
__device__ __forceinline__ f32x16 sm_mma(const bf16x8& a, const bf16x8& b, f32x16 acc) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
}

// S[d][k] = sum_{n : y_n = k} X[n][d] in float64, one workgroup per (d, k), fixed thread count and
// a fixed-order tree: the value depends on the data only
constexpr int CS_THREADS = 256;
__global__ __launch_bounds__(CS_THREADS) void k_softmax_colsums(const float* __restrict__ X,
                                                                const int32_t* __restrict__ y, int64_t n, int D,
                                                                int K, double* __restrict__ scol) {
  __shared__ double red[CS_THREADS];
  const int d = blockIdx.x, k = blockIdx.y;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += CS_THREADS)
    if (y[i] == k) acc += (double)X[i * D + d];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = CS_THREADS / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    NMX_DCHECK(d * K + k < SM_MAX_D * SM_MAX_K);
    scol[d * K + k] = red[0];
  }
}

// the first row whose label lies outside [0, K) (the slot starts at ~0)
__global__ void k_softmax_bad_reset(unsigned long long* bad) { *bad = ~0ull; }
__global__ void k_softmax_check_labels(const int32_t* __restrict__ y, int64_t n, int K, unsigned long long* bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && (y[i] < 0 || y[i] >= K)) atomicMin(bad, (unsigned long long)i);
}

// Packed tiles, NP = 3 KB + 6 DT + 1 pieces of 1 KB per 32-row tile, each a 64-lane x 16-byte
// operand fragment in lane order (KB = ceil(D / 16), DT = ceil(D / 32)):
//   piece p KB + kb             GEMM1 A = X[32 rows][16 cols], plane p, k-block kb: lane (r, h)
//                               holds X[r][16 kb + 8 h + j]
//   piece 3 KB + p 2 DT + 2 dt + s   GEMM2 A = X^T[32 cols][16 rows], plane p, column tile dt,
//                               k-step s: lane (r, h) element j holds
//                               X[16 s + 8 (j >> 2) + 4 h + (j & 3)][32 dt + r] -- the k order of
//                               the GEMM1 accumulator used as the B operand
//   piece NP - 1                labels as int32 class indices: y[h][i] of row
//                               (i & 3) + 8 (i >> 2) + 4 h at byte 64 h + 4 i; -1 for rows >= n
// Rows >= n_rows and columns >= D are zero.  One thread per (tile, piece, lane).
__global__ void k_softmax_pack(const float* __restrict__ X, const int32_t* __restrict__ y, int64_t n, int D, int KB,
                               int DT, int64_t ntiles, bf16x8* __restrict__ out) {
  const int NP = 3 * KB + 6 * DT + 1;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ntiles * NP * 64) return;
  const int lane = (int)(i & 63);
  const int64_t q = i >> 6;
  const int piece = (int)(q % NP);
  const int64_t t = q / NP;
  const int r = lane & 31, h = lane >> 5;
  const int64_t r0 = t * SM_ROWS;
  float v[8];
  int plane;
  if (piece < 3 * KB) {
    plane = piece / KB;
    const int kb = piece % KB;
    const int64_t row = r0 + r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int d = 16 * kb + 8 * h + j;
      v[j] = (row < n && d < D) ? X[row * D + d] : 0.0f;
    }
  } else if (piece < NP - 1) {
    const int qq = piece - 3 * KB;
    plane = qq / (2 * DT);
    const int rem = qq % (2 * DT);
    const int dt = rem >> 1, s = rem & 1;
    const int d = 32 * dt + r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int64_t row = r0 + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3);
      v[j] = (row < n && d < D) ? X[row * D + d] : 0.0f;
    }
  } else {
    // lane L < 8 holds the labels [h = L / 4][i = 4 (L % 4) .. + 3]; the other lanes -1
    i32x4 f = {-1, -1, -1, -1};
    if (lane < 8) {
      const int hh = lane >> 2;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int ii = 4 * (lane & 3) + k;
        const int64_t row = r0 + (ii & 3) + 8 * (ii >> 2) + 4 * hh;
        f[k] = row < n ? y[row] : -1;
      }
    }
    *reinterpret_cast<i32x4*>(out + i) = f;
    return;
  }
  bf16x8 b1, b2, b3;
  split3(v, b1, b2, b3);
  out[i] = plane == 0 ? b1 : (plane == 1 ? b2 : b3);
}

template <int N>
__device__ __forceinline__ void sm_wait_vm() {
  // s_waitcnt vmcnt(N), other counters untouched (gfx9 encoding)
  static_assert(N >= 0 && N < 64, "vmcnt range");
  __builtin_amdgcn_s_waitcnt((N & 15) | (7 << 4) | (15 << 8) | ((N >> 4) << 14));
}

// LDS reads of the ring by inline asm: a compiler-visible LDS read after the ring's DMA issue gets
// an s_waitcnt vmcnt(0), which would drain the prefetch of the next tile.  sm_lds_wait (all reads
// done), then sm_pin on each value before its use.
__device__ __forceinline__ unsigned sm_lds_addr(const char* p) {
  return (unsigned)(size_t)((__attribute__((address_space(3))) const char*)p);
}
template <class T>
__device__ __forceinline__ void sm_lds_read(T& v, unsigned addr) {
  static_assert(sizeof(T) == 16, "one ds_read_b128");
  asm volatile("ds_read_b128 %0, %1" : "=&v"(v) : "v"(addr));
}
__device__ __forceinline__ void sm_lds_wait() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
template <class T>
__device__ __forceinline__ void sm_pin(T& v) {
  asm volatile("" : "+v"(v));
}

// v of lane (i ^ X) within its group of 2 X lanes, for a value that the earlier butterfly steps
// made uniform over groups of X lanes (X = 1: any value)
template <int X>
__device__ __forceinline__ float ss_xor(float v) {
  static_assert(X == 1 || X == 2 || X == 4 || X == 8 || X == 16, "ss_xor");
  const int i = __float_as_int(v);
  int o;
  if constexpr (X == 1) o = __builtin_amdgcn_update_dpp(i, i, 0xB1, 0xF, 0xF, false);        // quad_perm [1,0,3,2]
  else if constexpr (X == 2) o = __builtin_amdgcn_update_dpp(i, i, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
  else if constexpr (X == 4) o = __builtin_amdgcn_update_dpp(i, i, 0x141, 0xF, 0xF, false);  // row_half_mirror
  else if constexpr (X == 8) o = __builtin_amdgcn_update_dpp(i, i, 0x140, 0xF, 0xF, false);  // row_mirror
  else o = __builtin_amdgcn_ds_swizzle(i, (16 << 10) | 0x1F);  // bit mode: lane ^ 16 in its 32
  return __int_as_float(o);
}
template <int KP, bool MAX>
__device__ __forceinline__ float sm_group_reduce(float v) {
  auto op = [](float a, float b) { return MAX ? fmaxf(a, b) : a + b; };
  v = op(v, ss_xor<1>(v));
  if constexpr (KP >= 4) v = op(v, ss_xor<2>(v));
  if constexpr (KP >= 8) v = op(v, ss_xor<4>(v));
  if constexpr (KP >= 16) v = op(v, ss_xor<8>(v));
  if constexpr (KP >= 32) v = op(v, ss_xor<16>(v));
  return v;
}

// The softmax epilogue on the GEMM1 accumulator (register r = row (r & 3) + 8 (r >> 2) + 4 h of
// the tile, y4 its labels): res = p - [k == y], and the rows' lse added to `pe` (every lane of a
// group adds the same value; lane k = 0 stores it).  pad = a class column k >= K.
template <int KP>
__device__ __forceinline__ void sm_epilogue(const f32x16& acc, const i32x4 (&y4)[4], int k, bool pad, float (&res)[16],
                                            double& pe) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float l = pad ? -INFINITY : acc[r];
    const float m = sm_group_reduce<KP, true>(l);  // finite: K >= 2 real columns
    const float e = __builtin_amdgcn_exp2f((l - m) * LOG2E);
    const float s = sm_group_reduce<KP, false>(e);  // in [1, K]
    const int yr = y4[r >> 2][r & 3];
    res[r] = e * __builtin_amdgcn_rcpf(s) - (k == yr ? 1.0f : 0.0f);
    const float lse = m + __builtin_amdgcn_logf(s) * LN2;
    pe += yr >= 0 ? (double)lse : 0.0;
  }
}

template <int KB, int DT, int KP>
__global__ __launch_bounds__(256, 2) void k_softmax(const char* __restrict__ Xq, int64_t ntiles, int D, int K, int S,
                                                    int Gt, nmx_eval_batch ev, float* __restrict__ gpart,
                                                    double* __restrict__ pepart) {
  constexpr int NP = 3 * KB + 6 * DT + 1, NA = 3 * KB;
  constexpr int CPT = 32 / KP;  // chains of a column tile
  extern __shared__ __attribute__((aligned(16))) char lds[];
  // splits sp = x (mod 8) run on XCD x (workgroup b = x mod 8), the column groups of a split on
  // consecutive workgroups of that XCD, so they share X tiles in its L2
  const int b = blockIdx.x, qb = b >> 3;
  const int ct = qb % Gt, split = (qb / Gt) * 8 + (b & 7);
  const int npos = ev.active_idx ? *ev.active_count : ev.ldc;
  if (ct * 4 * CPT >= npos) return;  // past the compacted list: workgroup-uniform

  const int lane = threadIdx.x & 63;
  const int wu = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = lane >> 5, col = lane & 31;
  const int k = col & (KP - 1), cl = col / KP;
  const int ldc = ev.ldc;
  const int pos = (ct * 4 + wu) * CPT + cl;
  const int c = pos < ldc ? nmx_eval_chain(ev, pos) : -1;
  const bool pad = k >= K;
  const bool active = __any(c >= 0);      // wave-uniform
  if (!__syncthreads_or(active)) return;  // workgroup-uniform

  const int64_t t0 = (int64_t)split * ntiles / S, t1 = (int64_t)(split + 1) * ntiles / S;
  const int nt = (int)(t1 - t0);
  NMX_DCHECK(split < S && t0 >= 0 && t1 <= ntiles && nt >= 0);
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void*)(Xq + (size_t)t0 * NP * 1024), 0,
                                                                       (int)((size_t)nt * NP * 1024), 0x00020000);

  // W fragments of the column tile (B operand: lane (col, h) holds W[16 kb + 8 h + j][k] of its
  // chain), gathered from the arena once and split; pad columns, coordinates >= D and lanes
  // without a chain hold zero
  bf16x8 z1[KB], z2[KB], z3[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int d = 16 * kb + 8 * h + j;
      const bool ok = c >= 0 && !pad && d < D;
      NMX_DCHECK(!ok || ((size_t)(d * K + k) < (size_t)D * K && c < ldc));
      v[j] = ok ? ev.z[(size_t)(d * K + k) * ldc + c] : 0.0f;
    }
    split3(v, z1[kb], z2[kb], z3[kb]);
  }
  f32x16 g[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) g[dt][r] = 0.0f;
  double pe = 0.0;

  // the whole tile (A pieces, X^T pieces, labels) in one ring slot; wave wu copies the pieces
  // wu, wu + 4, ...: iteration k reads slot k & 1 while tile k + 1 fills the other
  auto issue = [&](int kt) {
    char* dst = lds + (kt & 1) * NP * 1024;
#pragma unroll
    for (int j = 0; j < (NP + 3) / 4; ++j) {
      const int i = wu + 4 * j;
      NMX_DCHECK(kt < nt);
      if (i < NP)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (__attribute__((address_space(3))) void*)(dst + i * 1024), 16,
                                                 lane * 16, (unsigned)((kt * NP + i) * 1024), 0, 0);
    }
  };
  if (nt > 0) issue(0);
  for (int kt = 0; kt < nt; ++kt) {
    // tile kt has landed in every wave, and every wave is done with the other slot (tile kt - 1)
    sm_wait_vm<0>();
    asm volatile("s_barrier" ::: "memory");
    if (kt + 1 < nt) issue(kt + 1);
    if (!active) continue;
    const unsigned slot = sm_lds_addr(lds + (kt & 1) * NP * 1024) + lane * 16;
    bf16x8 a[3][KB];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) sm_lds_read(a[p][kb], slot + (p * KB + kb) * 1024);
    i32x4 y4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) sm_lds_read(y4[q], slot - lane * 16 + (NP - 1) * 1024 + 64 * h + 16 * q);
    sm_lds_wait();
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) sm_pin(a[p][kb]);
#pragma unroll
    for (int q = 0; q < 4; ++q) sm_pin(y4[q]);

    // GEMM1: L = X . W
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      acc = sm_mma(a[2][kb], z1[kb], acc);
      acc = sm_mma(a[1][kb], z2[kb], acc);
      acc = sm_mma(a[0][kb], z3[kb], acc);
      acc = sm_mma(a[1][kb], z1[kb], acc);
      acc = sm_mma(a[0][kb], z2[kb], acc);
      acc = sm_mma(a[0][kb], z1[kb], acc);
    }
    // the X^T pieces are read beside the epilogue
    bf16x8 bt[3][DT][2];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int s = 0; s < 2; ++s) sm_lds_read(bt[p][dt][s], slot + (NA + p * 2 * DT + 2 * dt + s) * 1024);

    float res[16];
    sm_epilogue<KP>(acc, y4, k, pad, res, pe);

    sm_lds_wait();
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int s = 0; s < 2; ++s) sm_pin(bt[p][dt][s]);
    // GEMM2: G += X^T . R (k-step s = residual registers 8 s .. 8 s + 7)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = res[8 * s + j];
      bf16x8 r1, r2, r3;
      split3(v, r1, r2, r3);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        g[dt] = sm_mma(bt[2][dt][s], r1, g[dt]);
        g[dt] = sm_mma(bt[1][dt][s], r2, g[dt]);
        g[dt] = sm_mma(bt[0][dt][s], r3, g[dt]);
        g[dt] = sm_mma(bt[1][dt][s], r1, g[dt]);
        g[dt] = sm_mma(bt[0][dt][s], r2, g[dt]);
        g[dt] = sm_mma(bt[0][dt][s], r1, g[dt]);
      }
    }
  }
  // a split without a tile stores its zeros: the finalize adds every slab
  if (c < 0 || pad) return;
  NMX_DCHECK(pos < ldc);
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d = 32 * dt + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (d < D) gpart[((size_t)split * D * K + (size_t)(d * K + k)) * ldc + pos] = g[dt][r];
    }
  // the two lane halves hold the rows' two halves; lane + 32 is the same column
  const double p = pe + __shfl_xor(pe, 32);
  if (h == 0 && k == 0) pepart[(size_t)split * ldc + pos] = p;
}

// One workgroup per (64 batch positions, coordinate j or the U row j = D K).  Wave w sums the
// slabs [w S / 4, (w + 1) S / 4) in order -- and, on the U row, its quarter of the coordinates'
// W^2 / 2 - S W in float64 -- then the four wave sums are added in wave order.
constexpr int FIN_WAVES = 4;
__global__ __launch_bounds__(64 * FIN_WAVES) void k_softmax_finalize(const float* __restrict__ gpart,
                                                                     const double* __restrict__ pepart, int S, int DK,
                                                                     nmx_eval_batch ev,
                                                                     const double* __restrict__ scol) {
  __shared__ double part[FIN_WAVES][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int pos = blockIdx.x * 64 + lane;
  const int j = blockIdx.y;
  const int ldc = ev.ldc;
  const int c = pos < ldc ? nmx_eval_chain(ev, pos) : -1;
  const int sp0 = w * S / FIN_WAVES, sp1 = (w + 1) * S / FIN_WAVES;
  if (c >= 0) {
    double s = 0.0;
    if (j < DK) {
      float f = 0.0f;
      for (int sp = sp0; sp < sp1; ++sp) f += gpart[((size_t)sp * DK + j) * ldc + pos];
      s = f;
    } else {
      for (int sp = sp0; sp < sp1; ++sp) s += pepart[(size_t)sp * ldc + pos];
      const int j0 = w * DK / FIN_WAVES, j1 = (w + 1) * DK / FIN_WAVES;
      double q = 0.0;
      for (int jj = j0; jj < j1; ++jj) {
        const double z = ev.z[(size_t)jj * ldc + c];
        q += 0.5 * z * z - scol[jj] * z;
      }
      s += q;
    }
    part[w][lane] = s;
  }
  __syncthreads();
  if (w != 0 || c < 0) return;
  if (j < DK) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < FIN_WAVES; ++i) s += (float)part[i][lane];
    const size_t idx = (size_t)j * ldc + c;
    ev.grad[idx] = ev.z[idx] + s;
  } else {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < FIN_WAVES; ++i) s += part[i][lane];
    ev.pe[c] = (float)(s + 0.9189385332046727 * DK);
  }
}

int sm_check_shape(const char* what, int64_t n_rows, int dim, int num_classes) {
  if (n_rows <= 0) return nmx_fail(NMX_ERR_INVALID, "%s: need n_rows >= 1 (got %lld)", what, (long long)n_rows);
  if (dim < 1 || dim > SM_MAX_D)
    return nmx_fail(NMX_ERR_INVALID, "%s: need 1 <= dim <= %d (got dim = %d)", what, SM_MAX_D, dim);
  if (num_classes < 2 || num_classes > SM_MAX_K)
    return nmx_fail(NMX_ERR_INVALID, "%s: need 2 <= num_classes <= %d (got num_classes = %d)", what, SM_MAX_K,
                    num_classes);
  // a split's tiles are addressed by 32-bit byte offsets
  const int64_t per = sm_ntiles(n_rows) / sm_num_splits(n_rows) + 1;
  if (per * sm_np(dim) * 1024 >= (int64_t)1 << 31)
    return nmx_fail(NMX_ERR_INVALID, "%s: n_rows = %lld is past the kernel's 2 GiB of tiles per row split", what,
                    (long long)n_rows);
  return NMX_OK;
}

template <int KB, int DT, int KP>
void sm_launch(dim3 grid, hipStream_t s, const char* Xq, int64_t nt, int D, int K, int S, int Gt,
               const nmx_eval_batch& ev, float* gpart, double* pepart) {
  constexpr size_t lds = (size_t)2 * (3 * KB + 6 * DT + 1) * 1024;
  static_assert(lds <= 64 * 1024, "two ring slots fit the default LDS limit");
  hipLaunchKernelGGL((k_softmax<KB, DT, KP>), grid, dim3(256), lds, s, Xq, nt, D, K, S, Gt, ev, gpart, pepart);
}
template <int KB, int DT>
void sm_launch_kp(int KP, dim3 grid, hipStream_t s, const char* Xq, int64_t nt, int D, int K, int S, int Gt,
                  const nmx_eval_batch& ev, float* gpart, double* pepart) {
  switch (KP) {
    case 2: return sm_launch<KB, DT, 2>(grid, s, Xq, nt, D, K, S, Gt, ev, gpart, pepart);
    case 4: return sm_launch<KB, DT, 4>(grid, s, Xq, nt, D, K, S, Gt, ev, gpart, pepart);
    case 8: return sm_launch<KB, DT, 8>(grid, s, Xq, nt, D, K, S, Gt, ev, gpart, pepart);
    case 16: return sm_launch<KB, DT, 16>(grid, s, Xq, nt, D, K, S, Gt, ev, gpart, pepart);
    default: return sm_launch<KB, DT, 32>(grid, s, Xq, nt, D, K, S, Gt, ev, gpart, pepart);
  }
}

}  // namespace

extern "C" size_t nmx_softmax_packed_bytes(int64_t n_rows, int dim, int num_classes) {
  if (n_rows <= 0 || dim < 1 || dim > SM_MAX_D || num_classes < 2 || num_classes > SM_MAX_K) return 0;
  return SM_TILE_OFFSET + (size_t)sm_ntiles(n_rows) * sm_np(dim) * 1024;
}

extern "C" int nmx_softmax_pack(const float* X, const int32_t* y, int64_t n_rows, int dim, int num_classes,
                                void* packed, void* stream) {
  if (int st = sm_check_shape("softmax_pack", n_rows, dim, num_classes)) return st;
  if (!X || !y || !packed) return nmx_fail(NMX_ERR_INVALID, "softmax_pack: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* bad = (unsigned long long*)((char*)packed + SM_BAD_OFFSET);
  hipLaunchKernelGGL(k_softmax_bad_reset, dim3(1), dim3(1), 0, s, bad);
  hipLaunchKernelGGL(k_softmax_check_labels, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, s, y, n_rows,
                     num_classes, bad);
  if (int st = nmx_check_launch("k_softmax_check_labels")) return st;
  unsigned long long first = 0;
  if (hipMemcpyAsync(&first, bad, sizeof(first), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return nmx_fail(NMX_ERR_HIP, "softmax_pack: reading the label check back failed");
  if (first != ~0ull)
    return nmx_fail(NMX_ERR_INVALID, "softmax_pack: the label of row %llu is outside [0, %d)", first, num_classes);
  hipLaunchKernelGGL(k_softmax_colsums, dim3(dim, num_classes), dim3(CS_THREADS), 0, s, X, y, n_rows, dim, num_classes,
                     (double*)packed);
  if (int st = nmx_check_launch("k_softmax_colsums")) return st;
  const int64_t nt = sm_ntiles(n_rows);
  const int64_t nthreads = nt * sm_np(dim) * 64;
  hipLaunchKernelGGL(k_softmax_pack, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, s, X, y, n_rows, dim,
                     sm_kb(dim), sm_dt(dim), nt, (bf16x8*)((char*)packed + SM_TILE_OFFSET));
  return nmx_check_launch("k_softmax_pack");
}

extern "C" size_t nmx_softmax_workspace_bytes(int64_t n_rows, int dim, int num_classes, int num_chains) {
  if (n_rows <= 0 || dim < 1 || dim > SM_MAX_D || num_classes < 2 || num_classes > SM_MAX_K || num_chains <= 0)
    return 0;
  const size_t ldc = (size_t)(num_chains + 63) / 64 * 64;
  const size_t S = sm_num_splits(n_rows);
  const size_t g = S * dim * num_classes * ldc * sizeof(float);
  const size_t p = S * ldc * sizeof(double);
  return (g + 255) / 256 * 256 + p;
}

extern "C" int nmx_softmax_pe_grad(const void* packed, int64_t n_rows, int dim, int num_classes,
                                   const nmx_eval_batch* ev, void* workspace, void* stream) {
  if (int st = sm_check_shape("softmax_pe_grad", n_rows, dim, num_classes)) return st;
  if (!ev || !ev->z || !ev->grad || !ev->pe) return nmx_fail(NMX_ERR_INVALID, "softmax_pe_grad: eval batch has NULL pointers");
  if (ev->num_chains <= 0 || ev->ldc < ev->num_chains || ev->ldc % 64)
    return nmx_fail(NMX_ERR_INVALID, "softmax_pe_grad: bad num_chains/ldc (%d/%d)", ev->num_chains, ev->ldc);
  if (!packed || !workspace) return nmx_fail(NMX_ERR_INVALID, "softmax_pe_grad: NULL packed/workspace");
  hipStream_t s = (hipStream_t)stream;
  const int S = sm_num_splits(n_rows), DK = dim * num_classes;
  float* gpart = (float*)workspace;
  double* pepart = (double*)((char*)workspace + ((size_t)S * DK * ev->ldc * sizeof(float) + 255) / 256 * 256);
  const int64_t nt = sm_ntiles(n_rows);
  const int KB = sm_kb(dim), KP = sm_kp(num_classes);
  const char* Xq = (const char*)packed + SM_TILE_OFFSET;
  const int nb = std::min(ev->num_chains, ev->ldc);  // batch positions that can hold a chain
  const int per_group = 4 * (32 / KP);                // chains of a workgroup
  const int Gt = (nb + per_group - 1) / per_group;
  const dim3 grid((unsigned)Gt * S);
  if (KB == 4) sm_launch_kp<4, 2>(KP, grid, s, Xq, nt, dim, num_classes, S, Gt, *ev, gpart, pepart);
  else if (KB == 3) sm_launch_kp<3, 2>(KP, grid, s, Xq, nt, dim, num_classes, S, Gt, *ev, gpart, pepart);
  else if (KB == 2) sm_launch_kp<2, 1>(KP, grid, s, Xq, nt, dim, num_classes, S, Gt, *ev, gpart, pepart);
  else sm_launch_kp<1, 1>(KP, grid, s, Xq, nt, dim, num_classes, S, Gt, *ev, gpart, pepart);
  if (int st = nmx_check_launch("k_softmax")) return st;
  hipLaunchKernelGGL(k_softmax_finalize, dim3((nb + 63) / 64, DK + 1), dim3(64 * FIN_WAVES), 0, s, gpart, pepart, S,
                     DK, *ev, (const double*)packed);
  return nmx_check_launch("k_softmax_finalize");
}
