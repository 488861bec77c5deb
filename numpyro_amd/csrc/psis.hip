// PSIS-LOO: Pareto-smoothed importance-sampling leave-one-out cross-validation of a
// log-likelihood table [S][ld], one value of elpd_loo and of the Pareto-k diagnostic per column
// (Vehtari, Gelman and Gabry 2017; the generalised Pareto fit of Zhang and Stephens 2009 with the
// weak prior of the loo package).  include/numpyro_amd.h "PSIS-LOO" states the arithmetic.
//
// Two launches.  k_psis_transpose copies the table into the workspace column by column
// ([num_columns][S], 64 x 64 tiles through LDS: both the reads and the writes are coalesced).
// k_psis_column gives one workgroup of 256 threads to a column and streams it six times (it stays
// in L2 / the Infinity Cache between the passes): the minimum and finiteness; four rounds of a
// radix select (8, 8, 8 and 7 bits of the 31-bit key |r|, a histogram in LDS filled with integer
// atomics) for the (M+1)-th largest ratio; the compaction of the tail into LDS with the body's
// sum of exp(r).  The tail (<= M <= NMX_PSIS_MAX_TAIL entries) is then sorted in LDS (bitonic,
// padded with +inf) and fitted and smoothed in float64.  The integer atomics only count, and the
// order in which the tail reaches LDS is erased by the sort, so every floating-point sum has an
// order fixed by (S, M): two launches are bitwise equal, and a column's result depends on no
// other column.
#include <cmath>

#include "nmx_api_internal.h"
#include "nmx_common.h"

namespace {

constexpr int PSIS_THREADS = 256;
constexpr int PSIS_WAVES = PSIS_THREADS / 64;
constexpr int PSIS_REPS = 8;        // copies of every histogram bin (lane & 7), so that a crowded bin
                                    // is an 8-way and not a 64-way collision of LDS atomics
constexpr int PSIS_MAX_CAND = 128;  // J = 30 + floor(sqrt(T)) <= 30 + 90 at T = 8192
constexpr float PSIS_FLOOR = -(NMX_PSIS_LOG_FLT_MIN);  // the largest |r| a tail entry may have

static_assert(30 + 91 <= PSIS_MAX_CAND && NMX_PSIS_MAX_TAIL <= 91 * 91, "candidate arrays of the fit");

// the kernel's LDS: e [P] f64, t [P] f32, the histogram, the candidates' b and L, the reduction scratch
__host__ __device__ inline size_t psis_lds_bytes(int P) {
  return (size_t)P * 12 + 256 * PSIS_REPS * 4 + 2 * PSIS_MAX_CAND * 8 + PSIS_WAVES * 8 + 16;
}

__global__ __launch_bounds__(256) void k_psis_transpose(const float* __restrict__ table, int S, int64_t ld, int N,
                                                        float* __restrict__ cols) {
  __shared__ float tile[64][65];
  const int s0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int i = ty; i < 64; i += 4) {
    const int s = s0 + i, c = c0 + tx;
    if (s < S && c < N) tile[i][tx] = table[(size_t)s * ld + c];
  }
  __syncthreads();
  for (int i = ty; i < 64; i += 4) {
    const int c = c0 + i, s = s0 + tx;
    if (s < S && c < N) cols[(size_t)c * S + s] = tile[tx][i];
  }
}

__device__ inline double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// the sum over the workgroup: lanes by the xor butterfly, then the four waves in order
__device__ inline double block_sum(double v, double* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double tot = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return tot;
}

// f(x_s) for the rows s = tid, tid + 256, ... of a column, in that order; the loads of eight rows
// are issued before the first is used (one workgroup per CU has little else to hide their latency)
template <class F>
__device__ inline void for_rows(const float* __restrict__ x, int S, F f) {
  constexpr int U = 8;
  int s = threadIdx.x;
  for (; s + (U - 1) * PSIS_THREADS < S; s += U * PSIS_THREADS) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = x[s + u * PSIS_THREADS];
#pragma unroll
    for (int u = 0; u < U; ++u) f(v[u]);
  }
  for (; s < S; s += PSIS_THREADS) f(x[s]);
}

__global__ __launch_bounds__(256) void k_psis_column(const float* __restrict__ cols, int S, int M, int P,
                                                     float* __restrict__ elpd_loo, float* __restrict__ pareto_k) {
  extern __shared__ __align__(16) unsigned char smem[];
  double* e_sh = (double*)smem;                     // [P] exp(t_i) - exp(cut)
  double* b_sh = e_sh + P;                          // [PSIS_MAX_CAND] the candidates b_j
  double* L_sh = b_sh + PSIS_MAX_CAND;              // [PSIS_MAX_CAND] their profile log likelihoods
  double* red = L_sh + PSIS_MAX_CAND;               // [PSIS_WAVES]
  float* t_sh = (float*)(red + PSIS_WAVES);         // [P] the tail
  int* hist = (int*)(t_sh + P);                     // [256][PSIS_REPS]
  int* misc = hist + 256 * PSIS_REPS;               // [4]: digit, rank, tail count, -
  float* fmisc = (float*)misc;

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int col = blockIdx.x;
  const float* __restrict__ x = cols + (size_t)col * S;

  // ---- pass 1: the minimum (m = -min x) and finiteness
  float mn = INFINITY;
  int bad = 0;
  for_rows(x, S, [&](float v) {
    bad |= !(fabsf(v) < INFINITY);
    mn = fminf(mn, v);
  });
  for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o));
  if (lane == 0) fmisc[wv] = mn;
  bad = __syncthreads_or(bad);
  if (bad) {
    if (tid == 0) {
      if (elpd_loo) elpd_loo[col] = NAN;
      if (pareto_k) pareto_k[col] = NAN;
    }
    return;
  }
  const float m = -fminf(fminf(fmisc[0], fmisc[1]), fminf(fmisc[2], fmisc[3]));
  __syncthreads();

  // ---- pass 2: radix select of the key of rank M (0-based, ascending) among |r_s|: the
  //      (M+1)-th largest r.  r <= 0, so the bits of |r| order as |r| does.
  unsigned prefix = 0;
  int rank = M;
  for (int round = 0; round < 4; ++round) {
    const int hi = 31 - 8 * round;               // the bits above the digit: key >> hi == prefix
    const int lo = round < 3 ? hi - 8 : 0;       // the digit: (key >> lo) & mask
    const unsigned mask = round < 3 ? 0xffu : 0x7fu;
    for (int i = tid; i < 256 * PSIS_REPS; i += PSIS_THREADS) hist[i] = 0;
    __syncthreads();
    for_rows(x, S, [&](float v) {
      const float r = (-v) - m;
      const unsigned key = __float_as_uint(r) & 0x7fffffffu;
      if ((key >> hi) == prefix) atomicAdd(&hist[((key >> lo) & mask) * PSIS_REPS + (lane & (PSIS_REPS - 1))], 1);
    });
    __syncthreads();
    if (wv == 0) {  // lane l owns the bins 4 l .. 4 l + 3; an inclusive scan over the lanes finds the digit
      int c[4], tot = 0;
      for (int q = 0; q < 4; ++q) {
        int n = 0;
        for (int rep = 0; rep < PSIS_REPS; ++rep) n += hist[(4 * lane + q) * PSIS_REPS + rep];
        c[q] = n;
        tot += n;
      }
      int incl = tot;
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
      }
      int below = incl - tot;
      if (below <= rank && rank < incl) {  // exactly one lane: the counts of the matching keys sum past rank
        int q = 0;
        while (below + c[q] <= rank) below += c[q++];
        misc[0] = 4 * lane + q;
        misc[1] = rank - below;
      }
    }
    __syncthreads();
    prefix = (prefix << (round < 3 ? 8 : 7)) | (unsigned)misc[0];
    rank = misc[1];
    __syncthreads();
  }
  // cut = max(the (M+1)-th largest r, log FLT_MIN); the tail is r > cut, i.e. |r| < |cut|
  const float cut_abs = fminf(__uint_as_float(prefix), PSIS_FLOOR);

  // ---- pass 3: the tail into LDS, the body's sum of exp(r)
  if (tid == 0) misc[2] = 0;
  __syncthreads();
  double body = 0.0;
  for_rows(x, S, [&](float v) {
    const float r = (-v) - m;
    if (fabsf(r) < cut_abs) {
      const int pos = atomicAdd(&misc[2], 1);
      if (pos < P) t_sh[pos] = r;  // pos < T <= M <= P by the choice of the cutoff
    } else {
      body += (double)expf(r);
    }
  });
  __syncthreads();
  const int T = min(misc[2], P);
  body = block_sum(body, red);

  // ---- the tail ascending: bitonic sort of the power of two >= T entries, padded with +inf
  int P2 = 1;
  while (P2 < T) P2 <<= 1;
  for (int i = T + tid; i < P2; i += PSIS_THREADS) t_sh[i] = INFINITY;
  __syncthreads();
  for (int k = 2; k <= P2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P2; i += PSIS_THREADS) {
        const int p = i ^ j;
        if (p > i) {
          const float a = t_sh[i], b = t_sh[p];
          if ((a > b) == ((i & k) == 0)) {
            t_sh[i] = b;
            t_sh[p] = a;
          }
        }
      }
      __syncthreads();
    }
  }

  // ---- the generalised Pareto fit (float64)
  const double cut = -(double)cut_abs, expcut = exp(cut);
  double k = INFINITY, sigma = 0.0;
  bool smooth = false;
  if (T > 4) {
    for (int i = tid; i < T; i += PSIS_THREADS) e_sh[i] = exp((double)t_sh[i]) - expcut;
    __syncthreads();
    const double dT = (double)T;
    const double q = e_sh[((T + 2) >> 2) - 1], emax = e_sh[T - 1];
    const int J = 30 + (int)sqrt(dT);
    for (int j = wv + 1; j <= J; j += PSIS_WAVES) {
      const double bj = (1.0 - sqrt((double)J / ((double)j - 0.5))) / (3.0 * q) + 1.0 / emax;
      double acc = 0.0;
      for (int i = lane; i < T; i += 64) acc += log1p(-bj * e_sh[i]);
      const double kj = wave_sum(acc) / dT;
      if (lane == 0) {
        b_sh[j - 1] = bj;
        L_sh[j - 1] = dT * (log(-bj / kj) - kj - 1.0);
      }
    }
    __syncthreads();
    if (tid == 0) {  // the softmax over J <= 120 candidates, in order
      double mx = L_sh[0];
      for (int j = 1; j < J; ++j) mx = fmax(mx, L_sh[j]);
      bool undefined = false;  // fmax skips a NaN: a candidate without a likelihood leaves no fit
      for (int j = 0; j < J; ++j) undefined |= L_sh[j] != L_sh[j];
      double sw = 0.0;
      for (int j = 0; j < J; ++j) sw += exp(L_sh[j] - mx);
      double b = 0.0;
      for (int j = 0; j < J; ++j) b += b_sh[j] * (exp(L_sh[j] - mx) / sw);
      red[0] = undefined ? NAN : b;
    }
    __syncthreads();
    const double b = red[0];
    __syncthreads();
    double acc = 0.0;
    for (int i = tid; i < T; i += PSIS_THREADS) acc += log1p(-b * e_sh[i]);
    const double kappa = block_sum(acc, red) / dT;
    sigma = -kappa / b;
    k = (dT * kappa + 5.0) / (dT + 10.0);
    smooth = isfinite(k) && isfinite(sigma);
  }

  // ---- the smoothed tail and the two sums
  double s1 = 0.0, s2 = 0.0;
  for (int i = tid; i < T; i += PSIS_THREADS) {
    const double t = (double)t_sh[i];
    double lw = t;
    if (smooth) {
      const double l1 = log1p(-((double)i + 0.5) / (double)T);
      const double g = fabs(k) < NMX_PSIS_K_ZERO ? -sigma * l1 : sigma * expm1(-k * l1) / k;
      lw = fmin(log(g + expcut), 0.0);
    }
    s1 += exp(lw);
    s2 += exp(lw - t);
  }
  s1 = block_sum(s1, red);
  s2 = block_sum(s2, red);
  if (tid == 0) {
    const double den = body + s1, num = (double)(S - T) + s2;
    if (elpd_loo) elpd_loo[col] = (float)((log(num) - (double)m) - log(den));
    if (pareto_k) pareto_k[col] = (float)k;
  }
}

}  // namespace

extern "C" size_t nmx_psis_workspace_bytes(int num_rows, int num_columns) {
  if (num_rows <= 0 || num_columns <= 0) return 0;
  return (size_t)num_rows * (size_t)num_columns * sizeof(float);
}

extern "C" int nmx_psis_loo(const float* table, int num_rows, int64_t ld, int num_columns, int tail, void* workspace,
                            float* elpd_loo, float* pareto_k, void* stream) {
  if (!table) return nmx_fail(NMX_ERR_INVALID, "psis_loo: NULL table");
  if (num_rows < 2) return nmx_fail(NMX_ERR_INVALID, "psis_loo: num_rows = %d, need at least 2", num_rows);
  if (num_rows > NMX_PSIS_MAX_ROWS)
    return nmx_fail(NMX_ERR_INVALID, "psis_loo: num_rows = %d above NMX_PSIS_MAX_ROWS = %d", num_rows, NMX_PSIS_MAX_ROWS);
  if (tail < 1 || tail >= num_rows)
    return nmx_fail(NMX_ERR_INVALID, "psis_loo: tail = %d outside [1, num_rows = %d)", tail, num_rows);
  if (tail > NMX_PSIS_MAX_TAIL)
    return nmx_fail(NMX_ERR_INVALID, "psis_loo: tail = %d above NMX_PSIS_MAX_TAIL = %d", tail, NMX_PSIS_MAX_TAIL);
  if (num_columns <= 0) return nmx_fail(NMX_ERR_INVALID, "psis_loo: num_columns = %d", num_columns);
  if (ld < num_columns) return nmx_fail(NMX_ERR_INVALID, "psis_loo: ld = %lld below num_columns = %d", (long long)ld, num_columns);
  if (!elpd_loo && !pareto_k) return nmx_fail(NMX_ERR_INVALID, "psis_loo: both outputs (elpd_loo, pareto_k) are NULL");
  if (!workspace) return nmx_fail(NMX_ERR_INVALID, "psis_loo: NULL workspace");
  int P = 1;
  while (P < tail) P <<= 1;
  const size_t lds = psis_lds_bytes(P);
  hipStream_t s = (hipStream_t)stream;
  if (const int st = nmx_lds_limit((const void*)k_psis_column, lds, s, "psis_loo")) return st;
  float* cols = (float*)workspace;
  const dim3 tgrid((num_rows + 63) / 64, (num_columns + 63) / 64);
  hipLaunchKernelGGL(k_psis_transpose, tgrid, dim3(256), 0, s, table, num_rows, ld, num_columns, cols);
  if (const int st = nmx_check_launch("k_psis_transpose")) return st;
  hipLaunchKernelGGL(k_psis_column, dim3(num_columns), dim3(PSIS_THREADS), lds, s, cols, num_rows, tail, P, elpd_loo,
                     pareto_k);
  return nmx_check_launch("k_psis_column");
}
