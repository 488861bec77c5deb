// Softmax regression after sampling: the pointwise log-likelihood table and posterior predictive
// labels of obs ~ Categorical(logits = X @ W_s) for posterior samples W [S, D, K] (the layout of
// get_samples()["coefs"]), D <= 64, K <= 32.
//
//   log-likelihood   out[s ld + n] = l[n, y_n] - logsumexp_k l[n, k],   l = X W_s        (float32)
//   draws            out[s ld + n] = the first k with sum_{j <= k} e_j > u sum_j e_j,    (int32)
//                    e_j = exp(l[n, j] - max_k l[n, k]), clamped to K - 1: no division and no
//                    probability tensor; u = Philox(seed; sample s, site 0, row n) as
//                    predictive.hip keys it, so a draw depends on (seed, sample, row) only
//
// k_softmax_predictive: one kernel, two epilogues.  The S x N x K logits never exist in memory.
//
// Transposed product.  The potential (potential_softmax.hip) puts rows of X on the A operand and
// (chain, class) on the B operand, because its residual feeds a second GEMM; a row's softmax is
// then spread over KP lanes.  Nothing follows the softmax here, so the product is turned round:
//   A = W columns [32 x 16], (sample, class) on the M axis;   B = X^T [16 x 32], rows on the N axis.
// The accumulator of lane (n, h) holds row row0 + n of X against the M indices
// m = (r & 3) + 8 (r >> 2) + 4 h, r = 0..15 (nmx_split_bf16.h), and which W column sits in A row m
// is the gather's choice.  KP = the power of two >= K:
//   KP <= 16: register r of lane half h = class r % KP of tile sample 2 (r / KP) + h, so a tile is
//             32 / KP samples and each sample's classes are KP registers of ONE lane: max, exp,
//             sum, log and the label select are register arithmetic without a cross-lane step
//   KP == 32: one sample per tile, class r + 16 h: the halves exchange max and sum once (lane ^ 32)
// Classes k >= K are a register-uniform predicate set to -inf (their A rows are zero).  The label
// select is an unrolled ly = (k == y) ? l_k : ly from NaN: no memory is indexed by a label, and a
// label outside [0, K) gives NaN.
//
// Stores.  For a fixed sample the 32 lanes of a half hold 32 consecutive rows, so each store
// instruction writes whole 128-byte runs of out[s, row0 .. row0 + 31] from registers; rows >= N and
// samples >= S are masked per lane and register.  Nothing outside out[s, 0 .. N), s < S, is written.
//
// Work split.  X is split once per call into bf16 planes in the B fragment's lane order
// (k_softmax_xsplit; 3 KB pieces of 1 KB per 32-row tile, piece p KB + kb = plane p of k-block kb,
// KB = ceil(D / 16)): every column group rereads it, S / (4 * 32 / KP) times.  A workgroup is 4
// waves = 4 column tiles sharing each X tile through a two-slot LDS ring (<= 24 KB): tile t + 1 is
// loaded to registers (and the tile's 32 labels, one per lane) before the products of tile t and
// written to the other slot after them, one barrier per tile.  Each wave gathers its W fragments
// once, splits them once and keeps them in registers for all its row tiles.  Grid = G column
// groups x R row ranges, R = a multiple of 8 with G R >= SP_TARGET_GROUPS (a few workgroups per
// CU whether S is 1 or 10^4); rows are never reduced over, so the ranges are independent and the
// table does not depend on R.  Workgroup b runs on XCD b mod 8: the column groups of one row range
// are consecutive workgroups of one XCD and share the range's X tiles in its L2.
//
// A sample's row of the table depends on W_s and X only: not on S, on its position or on ld.
#include <math.h>

#include <algorithm>

#include "nmx_api_internal.h"
#include "nmx_common.h"
#include "nmx_split_bf16.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr int SP_ROWS = 32;
constexpr int SP_MAX_D = 64, SP_MAX_K = 32;
constexpr int SP_WAVES = 4;
constexpr int SP_TARGET_GROUPS = 2048;
constexpr int64_t SP_MAX_DRAW_ROWS = (int64_t)1 << 24;  // the Philox counter's element field

inline int sp_kb(int D) { return (D + 15) / 16; }
inline int sp_kp(int K) {
  int kp = 2;
  while (kp < K) kp *= 2;
  return kp;
}
inline int64_t sp_ntiles(int64_t n) { return (n + SP_ROWS - 1) / SP_ROWS; }

// One thread per (tile, k-block, lane): the lane's eight floats X[row0 + n][16 kb + 8 h + j], split
// once, stored to the three planes' pieces.  Rows >= n_rows and columns >= D are zero.
__global__ __launch_bounds__(256) void k_softmax_xsplit(const float* __restrict__ X, int64_t n_rows, int D, int KB,
                                                        int64_t ntiles, nmx_bf16x8* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ntiles * KB * 64) return;
  const int lane = (int)(i & 63);
  const int64_t q = i >> 6;
  const int kb = (int)(q % KB);
  const int64_t t = q / KB;
  const int64_t row = t * SP_ROWS + (lane & 31);
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int d = 16 * kb + 8 * (lane >> 5) + j;
    v[j] = (row < n_rows && d < D) ? X[row * D + d] : 0.0f;
  }
  nmx_bf16x8 b[3];
  nmx_split3(v, b[0], b[1], b[2]);
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    const int64_t idx = ((t * 3 + p) * KB + kb) * 64 + lane;
    NMX_DCHECK(idx >= 0 && idx < ntiles * 3 * KB * 64);
    out[idx] = b[p];
  }
}

struct sp_args {
  const uint4* Xq;   // the split X: ntiles x 3 KB pieces
  const int32_t* y;  // labels (log-likelihood)
  const float* W;    // [S][D][K]
  void* out;         // float (log-likelihood) or int32 (draws), row stride ld
  int64_t n_rows, ntiles, ld;
  uint64_t seed;
  int D, K, S, G, R;
};

// The epilogue of one tile on the accumulator of lane (n, h): `row` = row0 + n, `y` its label,
// s_base the first sample of the wave's column tile.
template <int KP, bool DRAW>
__device__ __forceinline__ void sp_epilogue(const nmx_f32x16& acc, const sp_args& a, int s_base, int h, int64_t row,
                                            int y) {
  constexpr int NS = KP == 32 ? 1 : 16 / KP;  // samples of this lane
  constexpr int NK = KP == 32 ? 16 : KP;      // classes of a sample in this lane
  const bool row_ok = row < a.n_rows;
#pragma unroll
  for (int q = 0; q < NS; ++q) {
    const int s = KP == 32 ? s_base : s_base + 2 * q + h;
    const int k0 = KP == 32 ? 16 * h : 0;
    float l[NK], cum[NK];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      l[k] = k0 + k < a.K ? acc[q * NK + k] : -INFINITY;
      m = fmaxf(m, l[k]);
    }
    if constexpr (KP == 32) m = fmaxf(m, __shfl_xor(m, 32));  // finite: K >= 2 real classes
    float c = 0.0f, ly = NAN;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      c += __builtin_amdgcn_exp2f((l[k] - m) * LOG2E);  // a pad class adds exp2(-inf) = 0
      cum[k] = c;
      ly = k0 + k == y ? l[k] : ly;
    }
    float total = c, below = 0.0f;  // below: the sum of the classes before this lane's
    if constexpr (KP == 32) {
      const float other = __shfl_xor(c, 32);
      total = c + other;  // the same bits in both halves
      below = h ? other : 0.0f;
      const float ly_other = __shfl_xor(ly, 32);
      ly = ly == ly ? ly : ly_other;
    }
    const bool ok = row_ok && s < a.S && (KP != 32 || h == 0);
    const int64_t idx = (int64_t)s * a.ld + row;
    NMX_DCHECK(!ok || (s >= 0 && row >= 0 && row < a.ld));
    if constexpr (DRAW) {
      const nmx_u4 rnd = nmx_rng(a.seed, (uint32_t)s, 0u, NMX_EV_PREDICT, (uint32_t)row, 0u);
      const float thr = nmx_u01(rnd.x) * total;
      // the running sums do not decrease, so the first k above thr is the count of those not above
      int cnt = 0;
#pragma unroll
      for (int k = 0; k < NK; ++k) cnt += (k0 + k < a.K && below + cum[k] <= thr) ? 1 : 0;
      if constexpr (KP == 32) cnt += __shfl_xor(cnt, 32);
      if (ok) static_cast<int32_t*>(a.out)[idx] = min(cnt, a.K - 1);
    } else {
      if (ok) static_cast<float*>(a.out)[idx] = (ly - m) - __builtin_amdgcn_logf(total) * LN2;
    }
  }
}

template <int KB, int KP, bool DRAW>
__global__ __launch_bounds__(64 * SP_WAVES, 2) void k_softmax_predictive(sp_args a) {
  constexpr int NP = 3 * KB;               // pieces of a tile
  constexpr int NE = NP * 64;              // 16-byte elements of a tile
  static_assert(NE <= 768, "a thread stages at most three elements");
  constexpr int SPT = 32 / KP;             // samples of a column tile
  __shared__ uint4 ring[2][NE];
  static_assert(sizeof(ring) <= 64 * 1024, "two ring slots fit the default LDS limit");

  const int b = blockIdx.x, qb = b >> 3;
  const int cg = qb % a.G, rr = (qb / a.G) * 8 + (b & 7);
  NMX_DCHECK(cg < a.G && rr < a.R);
  const int64_t t0 = (int64_t)rr * a.ntiles / a.R, t1 = (int64_t)(rr + 1) * a.ntiles / a.R;
  if (t0 >= t1) return;  // a range without a tile: workgroup-uniform

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, n = lane & 31;
  const int s_base = (cg * SP_WAVES + wave) * SPT;
  const bool active = s_base < a.S;  // wave-uniform; an idle wave still stages its share of X

  // W fragments (A operand): lane (m, h) holds W_s[16 kb + 8 h + j][k] for the (sample, class) of
  // A row m = n, that is of accumulator register r = (m & 3) + 4 (m >> 3) in lane half (m >> 2) & 1
  nmx_bf16x8 w[KB][3];
  {
    const int r = (n & 3) + 4 * (n >> 3), hr = (n >> 2) & 1;
    const int s = KP == 32 ? s_base : s_base + 2 * (r / KP) + hr;
    const int k = KP == 32 ? r + 16 * hr : r % KP;
    const bool ok = s < a.S && k < a.K;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int d = 16 * kb + 8 * h + j;
        const size_t idx = ((size_t)s * a.D + d) * a.K + k;
        NMX_DCHECK(!(ok && d < a.D) || idx < (size_t)a.S * a.D * a.K);
        v[j] = (ok && d < a.D) ? a.W[idx] : 0.0f;
      }
      nmx_split3(v, w[kb][0], w[kb][1], w[kb][2]);
    }
  }

  // a thread stages the tile's elements tid, tid + 256 and tid + 512 (named registers: an array
  // indexed in a loop stays in scratch here)
  const uint4 zero = {0u, 0u, 0u, 0u};
  uint4 st0 = zero, st1 = zero, st2 = zero;
  auto fetch = [&](int64_t t) {  // tile t -> registers
    const uint4* src = a.Xq + t * NE + tid;
    NMX_DCHECK(t >= 0 && t < a.ntiles);
    if (tid < NE) st0 = src[0];
    if constexpr (NE > 256)
      if (tid + 256 < NE) st1 = src[256];
    if constexpr (NE > 512)
      if (tid + 512 < NE) st2 = src[512];
  };
  auto stash = [&](int slot) {  // registers -> ring slot
    uint4* dst = ring[slot] + tid;
    if (tid < NE) dst[0] = st0;
    if constexpr (NE > 256)
      if (tid + 256 < NE) dst[256] = st1;
    if constexpr (NE > 512)
      if (tid + 512 < NE) dst[512] = st2;
  };
  auto label = [&](int64_t t) {
    const int64_t row = t * SP_ROWS + n;
    return (!DRAW && row < a.n_rows) ? a.y[row] : -1;
  };

  fetch(t0);
  int y = label(t0);
  stash(0);
  __syncthreads();
  for (int64_t t = t0; t < t1; ++t) {
    const int slot = (int)(t - t0) & 1;
    const bool more = t + 1 < t1;
    int y_next = -1;
    if (more) {
      fetch(t + 1);
      y_next = label(t + 1);
    }
    if (active) {
      nmx_f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        nmx_bf16x8 x[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) x[p] = __builtin_bit_cast(nmx_bf16x8, ring[slot][(p * KB + kb) * 64 + lane]);
        acc = nmx_mma_split(w[kb], x, acc);
      }
      sp_epilogue<KP, DRAW>(acc, a, s_base, h, t * SP_ROWS + n, y);
    }
    // every wave has read slot ^ 1 (tile t - 1) before the barrier that ended the last iteration
    if (more) stash(slot ^ 1);
    __syncthreads();
    y = y_next;
  }
}

template <int KB, int KP, bool DRAW>
void sp_launch(const sp_args& a, hipStream_t s) {
  hipLaunchKernelGGL((k_softmax_predictive<KB, KP, DRAW>), dim3((unsigned)a.G * a.R), dim3(64 * SP_WAVES), 0, s, a);
}
template <int KB, bool DRAW>
void sp_launch_kp(int KP, const sp_args& a, hipStream_t s) {
  switch (KP) {
    case 2: return sp_launch<KB, 2, DRAW>(a, s);
    case 4: return sp_launch<KB, 4, DRAW>(a, s);
    case 8: return sp_launch<KB, 8, DRAW>(a, s);
    case 16: return sp_launch<KB, 16, DRAW>(a, s);
    default: return sp_launch<KB, 32, DRAW>(a, s);
  }
}

int sp_check_shape(const char* what, int64_t n_rows, int dim) {
  if (n_rows <= 0) return nmx_fail(NMX_ERR_INVALID, "%s: need n_rows >= 1 (got %lld)", what, (long long)n_rows);
  if (dim < 1 || dim > SP_MAX_D)
    return nmx_fail(NMX_ERR_INVALID, "%s: need 1 <= dim <= %d (got dim = %d)", what, SP_MAX_D, dim);
  if (n_rows >= (int64_t)1 << 31)
    return nmx_fail(NMX_ERR_INVALID, "%s: n_rows = %lld is past the kernel's 2^31 rows", what, (long long)n_rows);
  return NMX_OK;
}

// The checks and the launch both entry points share; `y` is NULL for draws.
template <bool DRAW>
int sp_run(const char* what, const void* packed, const int32_t* y, int64_t n_rows, int dim, int num_classes,
           const float* W, int num_samples, uint64_t seed, void* out, int64_t ld, void* stream) {
  if (int st = sp_check_shape(what, n_rows, dim)) return st;
  if (num_classes < 2 || num_classes > SP_MAX_K)
    return nmx_fail(NMX_ERR_INVALID, "%s: need 2 <= num_classes <= %d (got num_classes = %d)", what, SP_MAX_K,
                    num_classes);
  if (num_samples < 1)
    return nmx_fail(NMX_ERR_INVALID, "%s: need num_samples >= 1 (got num_samples = %d)", what, num_samples);
  if (ld < n_rows)
    return nmx_fail(NMX_ERR_INVALID, "%s: need ld >= n_rows (got ld = %lld, n_rows = %lld)", what, (long long)ld,
                    (long long)n_rows);
  if (DRAW && n_rows > SP_MAX_DRAW_ROWS)
    return nmx_fail(NMX_ERR_INVALID, "%s: n_rows = %lld is past the 2^24 rows the draw counter's element field holds",
                    what, (long long)n_rows);
  if (!packed || !W || !out || (!DRAW && !y)) return nmx_fail(NMX_ERR_INVALID, "%s: NULL pointer", what);
  const int KB = sp_kb(dim), KP = sp_kp(num_classes);
  const int64_t nt = sp_ntiles(n_rows);
  const int per_group = SP_WAVES * (32 / KP);  // samples of a workgroup
  const int64_t G = ((int64_t)num_samples + per_group - 1) / per_group;
  // row ranges: enough workgroups for the device, no more ranges than tiles (rounded up to the 8 XCDs)
  int64_t R = std::min<int64_t>((SP_TARGET_GROUPS + G - 1) / G, nt);
  R = (R + 7) / 8 * 8;
  if (G * R >= (int64_t)1 << 31)
    return nmx_fail(NMX_ERR_INVALID, "%s: num_samples = %d needs %lld workgroups, past the grid's 2^31", what,
                    num_samples, (long long)(G * R));
  sp_args a;
  a.Xq = (const uint4*)packed;
  a.y = y;
  a.W = W;
  a.out = out;
  a.n_rows = n_rows;
  a.ntiles = nt;
  a.ld = ld;
  a.seed = seed;
  a.D = dim;
  a.K = num_classes;
  a.S = num_samples;
  a.G = (int)G;
  a.R = (int)R;
  hipStream_t s = (hipStream_t)stream;
  if (KB == 4) sp_launch_kp<4, DRAW>(KP, a, s);
  else if (KB == 3) sp_launch_kp<3, DRAW>(KP, a, s);
  else if (KB == 2) sp_launch_kp<2, DRAW>(KP, a, s);
  else sp_launch_kp<1, DRAW>(KP, a, s);
  return nmx_check_launch("k_softmax_predictive");
}

}  // namespace

extern "C" size_t nmx_softmax_predictive_workspace_bytes(int64_t n_rows, int dim) {
  if (n_rows <= 0 || n_rows >= (int64_t)1 << 31 || dim < 1 || dim > SP_MAX_D) return 0;
  return (size_t)sp_ntiles(n_rows) * 3 * sp_kb(dim) * 1024;
}

extern "C" int nmx_softmax_predictive_pack(const float* X, int64_t n_rows, int dim, void* workspace, void* stream) {
  if (int st = sp_check_shape("softmax_predictive_pack", n_rows, dim)) return st;
  if (!X || !workspace) return nmx_fail(NMX_ERR_INVALID, "softmax_predictive_pack: NULL pointer");
  const int64_t nt = sp_ntiles(n_rows);
  const int KB = sp_kb(dim);
  const int64_t nthreads = nt * KB * 64;
  hipLaunchKernelGGL(k_softmax_xsplit, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, X,
                     n_rows, dim, KB, nt, (nmx_bf16x8*)workspace);
  return nmx_check_launch("k_softmax_xsplit");
}

extern "C" int nmx_softmax_loglik(const void* workspace, const int32_t* y, int64_t n_rows, int dim, int num_classes,
                                  const float* W, int num_samples, float* out, int64_t ld, void* stream) {
  return sp_run<false>("softmax_loglik", workspace, y, n_rows, dim, num_classes, W, num_samples, 0, out, ld, stream);
}

extern "C" int nmx_softmax_predict(const void* workspace, int64_t n_rows, int dim, int num_classes, const float* W,
                                   int num_samples, uint64_t seed, int32_t* out, int64_t ld, void* stream) {
  return sp_run<true>("softmax_predict", workspace, nullptr, n_rows, dim, num_classes, W, num_samples, seed, out, ld,
                      stream);
}
