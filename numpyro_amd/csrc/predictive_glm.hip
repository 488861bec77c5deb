// Bernoulli (logistic) and Poisson regression after sampling: the pointwise log-likelihood table
// and posterior predictive counts for posterior samples W [S, D] (the layout of
// get_samples()["coefs"]), data X [N, D], an optional offset [N] and 1 <= D <= 1024.
//
//   eta[s, n] = X[n, :] . W[s, :] + offset[n]
//   Bernoulli log-likelihood   out[s ld + n] = y eta - max(eta, 0) - log1p(exp(-|eta|))      (float32)
//   Poisson   log-likelihood   out[s ld + n] = y eta - exp(eta) - lgamma(y + 1)              (float32)
//   Poisson   draws            out[s ld + n] = nmx_draw_poisson(exp(eta); seed, sample0 + s, site 0,
//                              row n), -1 where it gives NaN (a rate >= NMX_POISSON_MAX_RATE) (int32)
//
// k_glm_predictive: a sample-by-row GEMM with a pointwise epilogue on the accumulator registers.
// The S x N matrix of eta never exists in memory.
//
// Orientation (predictive_softmax.hip's): A = W [32 samples x 16], B = X^T [16 x 32 rows], both
// contiguous along D, so one split kernel (k_glm_split) serves both operands: lane (i, h) of a
// fragment holds src[base + i][16 kb + 8 h + j], j = 0..7, as three bf16 planes (nmx_split_bf16.h;
// the six plane pairs, small terms first).  Register r of lane (i, h) of an accumulator is sample
// (r & 3) + 8 (r >> 2) + 4 h against row i: for a fixed register the 32 lanes of a half hold 32
// consecutive rows, so every store instruction writes whole 128-byte runs of out[s, row0 .. row0 + 31],
// once.
//
// Blocking.  1024 features of 128 samples are 768 KiB of planes: they do not stay in registers, so
// this is a blocked GEMM with a K-loop.  A workgroup of 4 waves owns a 128 sample x 128 row block of
// the table; wave w holds the 64 x 64 sub-block of sample tiles 2 (w >> 1) + {0, 1} and row tiles
// 2 (w & 1) + {0, 1} in four nmx_f32x16 accumulators that persist over the whole loop: no cross-wave
// reduction, no exchange.  The loop walks D one 16-deep k-block per chunk.  A chunk is 4 tiles x 3
// planes x 1 KiB of each operand = 24 KiB, staged through a two-slot LDS ring (48 KiB, three
// workgroups per CU by LDS): chunk c + 1 is loaded to registers (6 x 16 bytes per thread) before the
// 24 MFMAs of chunk c and written to the other slot after them, one barrier per chunk.  A wave reads
// 12 fragments (ds_read_b128, lanes 16 bytes apart) per chunk.  A (sample tile, row tile) pair wholly
// past S or N is skipped wave-uniformly, so S = 1 costs 4 of the 16 pairs.
//
// Operands.  Both are stored block-major so that a workgroup's chunk is one contiguous 12 KiB run:
//   piece(blk, kb, tile, p) = ((blk KB + kb) 4 + tile) 3 + p,   KB = ceil(D / 16), 64 lanes x 16 bytes
// X is split once per data set (nmx_glm_predictive_pack) with the per-row side data y, offset and
// (Poisson) lgamma(y + 1), computed in float64 and stored as float32; rows >= N and features >= D
// are zero.  W is split once per launch by the same kernel into the scratch region of the workspace;
// samples >= S are zero.  The main kernel never splits anything.
//
// Work split.  Grid = G sample blocks x R row blocks (R rounded up to the 8 XCDs; a workgroup past
// the last row block leaves at once).  Workgroup b runs on XCD b mod 8: the G sample blocks of one
// row block are consecutive workgroups of one XCD and share that block's X planes in its L2
// (predictive_softmax.hip's placement).  Rows are never reduced over and a sample is one A row of one
// MFMA, so a sample's row of the table depends on W_s, X, y and offset only: not on S, on the
// sample's position, on ld or on the grid.
//
// A draw is keyed as predictive.hip keys it, (seed, sample0 + s, site 0, NMX_EV_PREDICT, row,
// attempt), so it depends on (seed, sample, row) only.  Non-finite coefficients make the sample's
// planes NaN and with them that sample's row of the table, no other.  exp(eta) = +inf gives a
// log-likelihood of -inf (y eta is finite), never NaN.
#include <math.h>

#include <algorithm>

#include "nmx_api_internal.h"
#include "nmx_common.h"
#include "nmx_program.h"
#include "nmx_split_bf16.h"

namespace {

constexpr int GP_MAX_D = 1024;
constexpr int GP_BLOCK = 128;                 // samples and rows of a workgroup's block
constexpr int GP_TILES = GP_BLOCK / 32;       // 32-wide tiles of a block, per operand
constexpr int GP_CHUNK = GP_TILES * 3 * 64;   // 16-byte elements of one operand's chunk (12 KiB)
constexpr size_t GP_HEAD_BYTES = 256;         // the pack's bad-row word
constexpr int64_t GP_MAX_DRAW_ROWS = (int64_t)1 << 24;  // the Philox counter's element field

inline int gp_kb(int D) { return (D + 15) / 16; }
inline int64_t gp_blocks(int64_t n) { return (n + GP_BLOCK - 1) / GP_BLOCK; }
inline size_t gp_planes_bytes(int64_t n, int D) { return (size_t)gp_blocks(n) * gp_kb(D) * GP_CHUNK * 16; }
inline size_t gp_side_bytes(int64_t n) { return (size_t)gp_blocks(n) * GP_BLOCK * 3 * sizeof(float); }

// One thread per (block, k-block, tile, lane): the lane's eight floats src[row][16 kb + 8 h + j] of
// row = 128 blk + 32 tile + i, split once, stored to the three planes' pieces.  Rows >= n and columns
// >= D are zero.
__global__ __launch_bounds__(256) void k_glm_split(const float* __restrict__ src, int64_t n, int D, int KB,
                                                   int64_t nblocks, nmx_bf16x8* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nblocks * KB * GP_TILES * 64) return;
  const int lane = (int)(i & 63);
  const int64_t q = i >> 6;  // (blk KB + kb) 4 + tile
  const int tile = (int)(q & (GP_TILES - 1));
  const int kb = (int)((q / GP_TILES) % KB);
  const int64_t blk = q / GP_TILES / KB;
  const int64_t row = blk * GP_BLOCK + tile * 32 + (lane & 31);
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int d = 16 * kb + 8 * (lane >> 5) + j;
    NMX_DCHECK(!(row < n && d < D) || row * D + d < n * D);
    v[j] = (row < n && d < D) ? src[row * D + d] : 0.0f;
  }
  nmx_bf16x8 b[3];
  nmx_split3(v, b[0], b[1], b[2]);
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    const int64_t idx = (q * 3 + p) * 64 + lane;
    NMX_DCHECK(idx >= 0 && idx < nblocks * KB * GP_CHUNK);
    out[idx] = b[p];
  }
}

__global__ void k_glm_bad_reset(unsigned long long* bad) { *bad = ~0ull; }

// The side data of row i < npad: side[i] = y, side[npad + i] = offset, side[2 npad + i] =
// lgamma(y + 1) (Poisson); zero for rows >= n and where y or offset is NULL.  The first row whose y
// the family refuses goes to *bad.
__global__ __launch_bounds__(256) void k_glm_side(const float* __restrict__ y, const float* __restrict__ off,
                                                  int64_t n, int64_t npad, int family, float* __restrict__ side,
                                                  unsigned long long* bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npad) return;
  float v = 0.0f, o = 0.0f, lg = 0.0f;
  if (i < n) {
    if (y) v = y[i];
    if (off) o = off[i];
    const bool ok = family == NMX_GLM_BERNOULLI ? (v == 0.0f || v == 1.0f)
                                                : (v >= 0.0f && v == floorf(v) && v < 16777216.0f);
    if (!ok) {
      atomicMin(bad, (unsigned long long)i);
      v = 0.0f;
    }
    if (family == NMX_GLM_POISSON) lg = (float)lgamma((double)v + 1.0);
  }
  NMX_DCHECK(i >= 0 && 2 * npad + i < 3 * npad);
  side[i] = v;
  side[npad + i] = o;
  side[2 * npad + i] = lg;
}

struct gp_args {
  const uint4* Xq;    // the split X: R blocks x KB chunks
  const uint4* Wq;    // the split W: G blocks x KB chunks
  const float* side;  // y, offset, lgamma(y + 1): 3 x npad
  void* out;          // float (log-likelihood) or int32 (draws), row stride ld
  int64_t n_rows, npad, ld;
  uint64_t seed;
  uint32_t sample0;
  int KB, S, G, R;    // R: row blocks that exist (the grid has R rounded up to 8)
};

// The epilogue of one accumulator of lane (i, h): `row` = the lane's row, s_base the first sample
// of the accumulator's sample tile; y, off, lg the row's side data.
template <int FAMILY, bool DRAW>
__device__ __forceinline__ void gp_epilogue(const nmx_f32x16& acc, const gp_args& a, int s_base, int h, int64_t row,
                                            float y, float off, float lg) {
  const bool row_ok = row < a.n_rows;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int s = s_base + (r & 3) + 8 * (r >> 2) + 4 * h;
    const bool ok = row_ok && s < a.S;
    const int64_t idx = (int64_t)s * a.ld + row;
    NMX_DCHECK(!ok || (s >= 0 && row >= 0 && row < a.ld));
    const float eta = acc[r] + off;
    if constexpr (DRAW) {
      const float k = ok ? nmx_draw_poisson(expf(eta), a.seed, a.sample0 + (uint32_t)s, 0u, (uint32_t)row) : 0.0f;
      if (ok) static_cast<int32_t*>(a.out)[idx] = k == k ? (int32_t)k : -1;
    } else if constexpr (FAMILY == NMX_GLM_BERNOULLI) {
      if (ok) static_cast<float*>(a.out)[idx] = y * eta - fmaxf(eta, 0.0f) - log1pf(expf(-fabsf(eta)));
    } else {
      if (ok) static_cast<float*>(a.out)[idx] = y * eta - expf(eta) - lg;
    }
  }
}

template <int FAMILY, bool DRAW>
__global__ __launch_bounds__(256) void k_glm_predictive(gp_args a) {
  __shared__ uint4 ring[2][2 * GP_CHUNK];  // slot: the A chunk, then the B chunk
  static_assert(sizeof(ring) == 48 * 1024, "two ring slots of 24 KiB");

  const int b = blockIdx.x, qb = b >> 3;
  const int cg = qb % a.G, rb = (qb / a.G) * 8 + (b & 7);
  NMX_DCHECK(cg < a.G);
  if (rb >= a.R) return;  // the grid's rows are rounded up to the 8 XCDs: workgroup-uniform

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, n = lane & 31;
  const int st0 = 2 * (wave >> 1), rt0 = 2 * (wave & 1);  // the wave's first sample and row tile
  const int s_base = cg * GP_BLOCK + 32 * st0;
  const int64_t row_base = (int64_t)rb * GP_BLOCK + 32 * rt0;
  // wave-uniform: the pairs with work (tile 0 of a block always holds a sample and a row)
  const bool s_on[2] = {s_base < a.S, s_base + 32 < a.S};
  const bool r_on[2] = {row_base < a.n_rows, row_base + 32 < a.n_rows};

  // the lane's side data of its two rows (npad covers every row of every block)
  float y[2], off[2], lg[2];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    const int64_t row = row_base + 32 * rt + n;
    NMX_DCHECK(row >= 0 && row < a.npad);
    y[rt] = a.side[row];
    off[rt] = a.side[a.npad + row];
    lg[rt] = FAMILY == NMX_GLM_POISSON && !DRAW ? a.side[2 * a.npad + row] : 0.0f;
  }

  // a thread stages elements tid, tid + 256 and tid + 512 of each operand's chunk (named registers)
  const uint4* asrc = a.Wq + (int64_t)cg * a.KB * GP_CHUNK + tid;
  const uint4* bsrc = a.Xq + (int64_t)rb * a.KB * GP_CHUNK + tid;
  uint4 a0, a1, a2, b0, b1, b2;
  auto fetch = [&](int kb) {
    NMX_DCHECK(kb >= 0 && kb < a.KB);
    const uint4* pa = asrc + (int64_t)kb * GP_CHUNK;
    const uint4* pb = bsrc + (int64_t)kb * GP_CHUNK;
    a0 = pa[0], a1 = pa[256], a2 = pa[512];
    b0 = pb[0], b1 = pb[256], b2 = pb[512];
  };
  auto stash = [&](int slot) {
    uint4* d = ring[slot] + tid;
    d[0] = a0, d[256] = a1, d[512] = a2;
    d[GP_CHUNK] = b0, d[GP_CHUNK + 256] = b1, d[GP_CHUNK + 512] = b2;
  };

  nmx_f32x16 acc[2][2];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q >> 1][q & 1][r] = 0.0f;

  fetch(0);
  stash(0);
  __syncthreads();
  for (int kb = 0; kb < a.KB; ++kb) {
    const int slot = kb & 1;
    const bool more = kb + 1 < a.KB;
    if (more) fetch(kb + 1);
    nmx_bf16x8 wf[2][3], xf[2][3];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        wf[t][p] = __builtin_bit_cast(nmx_bf16x8, ring[slot][((st0 + t) * 3 + p) * 64 + lane]);
        xf[t][p] = __builtin_bit_cast(nmx_bf16x8, ring[slot][GP_CHUNK + ((rt0 + t) * 3 + p) * 64 + lane]);
      }
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
        if (s_on[st] && r_on[rt]) acc[st][rt] = nmx_mma_split(wf[st], xf[rt], acc[st][rt]);
    // every wave has read slot ^ 1 (chunk kb - 1) before the barrier that ended the last iteration
    if (more) stash(slot ^ 1);
    __syncthreads();
  }

#pragma unroll
  for (int st = 0; st < 2; ++st)
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
      if (s_on[st] && r_on[rt])
        gp_epilogue<FAMILY, DRAW>(acc[st][rt], a, s_base + 32 * st, h, row_base + 32 * rt + n, y[rt], off[rt], lg[rt]);
}

int gp_check_shape(const char* what, int64_t n_rows, int dim, int family) {
  if (n_rows <= 0) return nmx_fail(NMX_ERR_INVALID, "%s: need n_rows >= 1 (got %lld)", what, (long long)n_rows);
  if (dim < 1 || dim > GP_MAX_D)
    return nmx_fail(NMX_ERR_INVALID, "%s: need 1 <= dim <= %d (got dim = %d)", what, GP_MAX_D, dim);
  if (n_rows >= (int64_t)1 << 31)
    return nmx_fail(NMX_ERR_INVALID, "%s: n_rows = %lld is past the kernel's 2^31 rows", what, (long long)n_rows);
  if (family != NMX_GLM_BERNOULLI && family != NMX_GLM_POISSON)
    return nmx_fail(NMX_ERR_INVALID, "%s: unknown family %d (NMX_GLM_BERNOULLI = %d, NMX_GLM_POISSON = %d)", what,
                    family, NMX_GLM_BERNOULLI, NMX_GLM_POISSON);
  return NMX_OK;
}

// The checks and the two launches (W split, then the product) both entry points share.
template <bool DRAW>
int gp_run(const char* what, void* workspace, int64_t n_rows, int dim, int family, const float* W, int num_samples,
           int64_t sample0, uint64_t seed, void* out, int64_t ld, void* stream) {
  if (int st = gp_check_shape(what, n_rows, dim, family)) return st;
  if (DRAW && family != NMX_GLM_POISSON)
    return nmx_fail(NMX_ERR_INVALID, "%s: family %d has no draw kernel (Bernoulli draws are nmx_predict_logreg's)",
                    what, family);
  if (num_samples < 1)
    return nmx_fail(NMX_ERR_INVALID, "%s: need num_samples >= 1 (got num_samples = %d)", what, num_samples);
  if (ld < n_rows)
    return nmx_fail(NMX_ERR_INVALID, "%s: need ld >= n_rows (got ld = %lld, n_rows = %lld)", what, (long long)ld,
                    (long long)n_rows);
  if (DRAW && n_rows > GP_MAX_DRAW_ROWS)
    return nmx_fail(NMX_ERR_INVALID, "%s: n_rows = %lld is past the 2^24 rows the draw counter's element field holds",
                    what, (long long)n_rows);
  if (DRAW && (sample0 < 0 || sample0 + num_samples > 0xFFFFFFFFll))  // the sample index is one counter word
    return nmx_fail(NMX_ERR_INVALID, "%s: bad sample0 (%lld) for num_samples = %d", what, (long long)sample0,
                    num_samples);
  if (!workspace || !W || !out) return nmx_fail(NMX_ERR_INVALID, "%s: NULL pointer", what);
  const int KB = gp_kb(dim);
  const int64_t R = gp_blocks(n_rows), G = gp_blocks(num_samples), R8 = (R + 7) / 8 * 8;
  if (G * R8 >= (int64_t)1 << 31)
    return nmx_fail(NMX_ERR_INVALID, "%s: num_samples = %d needs %lld workgroups, past the grid's 2^31", what,
                    num_samples, (long long)(G * R8));
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  gp_args a;
  a.Xq = (const uint4*)(ws + GP_HEAD_BYTES);
  a.side = (const float*)(ws + GP_HEAD_BYTES + gp_planes_bytes(n_rows, dim));
  nmx_bf16x8* wq = (nmx_bf16x8*)(ws + GP_HEAD_BYTES + gp_planes_bytes(n_rows, dim) + gp_side_bytes(n_rows));
  a.Wq = (const uint4*)wq;
  a.out = out;
  a.n_rows = n_rows;
  a.npad = R * GP_BLOCK;
  a.ld = ld;
  a.seed = seed;
  a.sample0 = (uint32_t)sample0;
  a.KB = KB;
  a.S = num_samples;
  a.G = (int)G;
  a.R = (int)R;
  const int64_t nthreads = G * KB * GP_TILES * 64;
  hipLaunchKernelGGL(k_glm_split, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, s, W, (int64_t)num_samples,
                     dim, KB, G, wq);
  if (int st = nmx_check_launch("k_glm_split")) return st;
  const dim3 grid((unsigned)(G * R8)), block(256);
  if (DRAW) hipLaunchKernelGGL((k_glm_predictive<NMX_GLM_POISSON, true>), grid, block, 0, s, a);
  else if (family == NMX_GLM_POISSON) hipLaunchKernelGGL((k_glm_predictive<NMX_GLM_POISSON, false>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((k_glm_predictive<NMX_GLM_BERNOULLI, false>), grid, block, 0, s, a);
  return nmx_check_launch("k_glm_predictive");
}

}  // namespace

extern "C" size_t nmx_glm_predictive_workspace_bytes(int64_t n_rows, int dim, int max_samples) {
  if (n_rows <= 0 || n_rows >= (int64_t)1 << 31 || dim < 1 || dim > GP_MAX_D || max_samples < 1) return 0;
  return GP_HEAD_BYTES + gp_planes_bytes(n_rows, dim) + gp_side_bytes(n_rows) + gp_planes_bytes(max_samples, dim);
}

// Synchronises the stream once, to refuse a bad label or count by row.
extern "C" int nmx_glm_predictive_pack(const float* X, const float* y, const float* offset, int64_t n_rows, int dim,
                                       int family, void* workspace, void* stream) {
  if (int st = gp_check_shape("glm_predictive_pack", n_rows, dim, family)) return st;
  if (!X || !workspace) return nmx_fail(NMX_ERR_INVALID, "glm_predictive_pack: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  unsigned long long* bad = (unsigned long long*)ws;
  const int KB = gp_kb(dim);
  const int64_t R = gp_blocks(n_rows), npad = R * GP_BLOCK;
  hipLaunchKernelGGL(k_glm_bad_reset, dim3(1), dim3(1), 0, s, bad);
  hipLaunchKernelGGL(k_glm_side, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, s, y, offset, n_rows, npad,
                     family, (float*)(ws + GP_HEAD_BYTES + gp_planes_bytes(n_rows, dim)), bad);
  if (int st = nmx_check_launch("k_glm_side")) return st;
  const int64_t nthreads = R * KB * GP_TILES * 64;
  hipLaunchKernelGGL(k_glm_split, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, s, X, n_rows, dim, KB, R,
                     (nmx_bf16x8*)(ws + GP_HEAD_BYTES));
  if (int st = nmx_check_launch("k_glm_split")) return st;
  unsigned long long first = 0;
  if (hipMemcpyAsync(&first, bad, sizeof(first), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return nmx_fail(NMX_ERR_HIP, "glm_predictive_pack: reading the label check back failed");
  if (first != ~0ull)
    return nmx_fail(NMX_ERR_INVALID, family == NMX_GLM_BERNOULLI
                                         ? "glm_predictive_pack: the label y of row %llu is not 0 or 1"
                                         : "glm_predictive_pack: the count y of row %llu is not a whole number in [0, 2^24)",
                    first);
  return NMX_OK;
}

extern "C" int nmx_glm_loglik(void* workspace, int64_t n_rows, int dim, int family, const float* W, int num_samples,
                              float* out, int64_t ld, void* stream) {
  return gp_run<false>("glm_loglik", workspace, n_rows, dim, family, W, num_samples, 0, 0, out, ld, stream);
}

extern "C" int nmx_glm_predict(void* workspace, int64_t n_rows, int dim, int family, const float* W, int num_samples,
                               int64_t sample0, uint64_t seed, int32_t* out, int64_t ld, void* stream) {
  return gp_run<true>("glm_predict", workspace, n_rows, dim, family, W, num_samples, sample0, seed, out, ld, stream);
}
