// Log-likelihood programs and the pointwise reductions of their tables (numpyro/infer/util.py:
// 1094-1170 log_likelihood: the model re-run per posterior sample, log_prob of every observed
// site; include/numpyro_amd.h "log-likelihood programs").
//
// k_program_loglik: one wave (a 64-thread workgroup) per posterior sample runs the draw-free
// program forward on the sample's tape row (NmxProgram::forward and its barrier rule,
// nmx_program.h) and copies the output values into the dense table out[num_samples][ldo].
//
// The reduce kernels turn a table [rows][ld] into, per column, lppd = logsumexp over rows - log S
// and p_waic = the (S - 1) variance over rows, through a running per-column state so that the
// rows may arrive chunk after chunk.  A state is { m, s, n, mean, M2 }: the largest entry so far,
// sum exp(x - shift(m)) with NmxProgram::lse_shift's rule (the maximum, or 0 where that is not
// finite), the count, and Welford's mean and sum of squared deviations; two states merge by
// rescaling the sums to the common shift and by Chan's formula.  k_pointwise_partial gives one
// partial state per (row split, column); k_pointwise_merge merges a column's partials by a
// butterfly over the splits and folds the result into the running state.  Every order is fixed
// by the shapes alone: no atomics, two launches are bitwise equal.
#include <algorithm>
#include <vector>

#include "nmx_api_internal.h"
#include "nmx_common.h"
#include "nmx_program.h"

namespace {

__global__ __launch_bounds__(64) void k_program_loglik(NmxProgram prog, const float* __restrict__ samples,
                                                       int num_samples, const int32_t* __restrict__ outputs,
                                                       int num_outputs, float* __restrict__ tape,
                                                       float* __restrict__ out, int64_t ldo) {
  const int row = blockIdx.x, lane = threadIdx.x;
  if (row >= num_samples) return;
  const nmx_program& p = prog.p;
  float* v = tape + (size_t)row * p.num_slots;
  for (int d = lane; d < p.dim; d += 64) v[d] = samples[(size_t)row * p.dim + d];
  __syncthreads();
  for (int k = 0; k < p.num_ops; ++k) {
    const NmxOp o = prog.load(k);
    if (NmxProgram::crosses(o) || NmxProgram::reads_scalar_slot(o)) __syncthreads();
    prog.forward(o, v, lane);
  }
  __syncthreads();  // an output may start inside a value: its elements come from other lanes
  float* dst = out + (size_t)row * ldo;
  for (int j = 0; j < num_outputs; ++j) {
    const int slot = outputs[3 * j], n = outputs[3 * j + 1], column = outputs[3 * j + 2];
    NMX_DCHECK(slot >= 0 && slot + n <= p.num_slots && column >= 0 && column + n <= ldo);
    for (int i = lane; i < n; i += 64) dst[column + i] = v[slot + i];
  }
}

// ---- pointwise reductions
struct PwState {
  float m, s, mean, m2;
  int n;
};

__device__ __forceinline__ PwState pw_empty() { return PwState{-INFINITY, 0.0f, 0.0f, 0.0f, 0}; }

// the factor that takes a sum at the shift of maximum `m` to the shift `sh`; a state that has seen
// no finite entry holds s = 0 (or NaN) at shift 0 and must not meet exp(0 - sh) = inf
__device__ __forceinline__ float pw_rescale(float m, float sh) {
  return m == -INFINITY ? 0.0f : expf(NmxProgram::lse_shift(m) - sh);
}

__device__ __forceinline__ void pw_push(PwState& a, float x) {
  const float m = fmaxf(a.m, x);  // a NaN entry leaves the maximum and reaches s through exp
  const float sh = NmxProgram::lse_shift(m);
  a.s = a.s * pw_rescale(a.m, sh) + expf(x - sh);
  a.m = m;
  a.n += 1;
  const float delta = x - a.mean;
  a.mean += delta / (float)a.n;
  a.m2 += delta * (x - a.mean);
  if (!(fabsf(x) < INFINITY)) a.m2 = NAN;  // the variance of a column with a non-finite entry
}

// a then b: `a` holds the earlier rows
__device__ __forceinline__ PwState pw_merge(const PwState& a, const PwState& b) {
  if (b.n == 0) return a;
  if (a.n == 0) return b;
  PwState r;
  r.m = fmaxf(a.m, b.m);
  const float sh = NmxProgram::lse_shift(r.m);
  r.s = a.s * pw_rescale(a.m, sh) + b.s * pw_rescale(b.m, sh);
  r.n = a.n + b.n;
  const float na = (float)a.n, nb = (float)b.n, n = (float)r.n;
  const float delta = b.mean - a.mean;
  r.mean = a.mean + delta * (nb / n);
  r.m2 = (a.m2 + b.m2) + (delta * delta) * (na * nb / n);
  return r;
}

// state block q of `state`: five arrays of num_columns words (m, s, mean, M2, n)
__device__ __forceinline__ PwState pw_load(const float* state, int q, int C, int c) {
  const float* b = state + (size_t)q * 5 * C;
  return PwState{b[c], b[C + c], b[2 * C + c], b[3 * C + c], __float_as_int(b[4 * C + c])};
}
__device__ __forceinline__ void pw_store(float* state, int q, int C, int c, const PwState& a) {
  float* b = state + (size_t)q * 5 * C;
  b[c] = a.m;
  b[C + c] = a.s;
  b[2 * C + c] = a.mean;
  b[3 * C + c] = a.m2;
  b[4 * C + c] = __int_as_float(a.n);
}

__device__ __forceinline__ PwState pw_shfl_xor(const PwState& a, int off) {
  return PwState{__shfl_xor(a.m, off, 64), __shfl_xor(a.s, off, 64), __shfl_xor(a.mean, off, 64),
                 __shfl_xor(a.m2, off, 64), __shfl_xor(a.n, off, 64)};
}

// Partial states of the row split blockIdx.y (rows [y * rows_per_split, ...)) into block 1 + y.
// wide (num_columns >= 64): lane = column blockIdx.x * 64 + lane, its rows in order: a wave reads
//   64 consecutive words per row.
// narrow (num_columns < 64, cpad = the power of two >= num_columns, G = 64 / cpad row groups):
//   lane = g * cpad + c pushes the rows g, g + G, ... of the split, then the G states of a column
//   merge by a butterfly over the lane bits 32 ... cpad, the lower lane's state first.
__global__ __launch_bounds__(64) void k_pointwise_partial(const float* __restrict__ table, int num_rows, int64_t ld,
                                                          int num_columns, int rows_per_split, int cpad,
                                                          float* __restrict__ state) {
  const int lane = threadIdx.x, split = blockIdx.y;
  const int r0 = split * rows_per_split;
  const int r1 = min(num_rows, r0 + rows_per_split);
  PwState a = pw_empty();
  if (cpad == 64) {
    const int c = blockIdx.x * 64 + lane;
    if (c >= num_columns) return;
#pragma unroll 4
    for (int r = r0; r < r1; ++r) pw_push(a, table[(size_t)r * ld + c]);
    pw_store(state, 1 + split, num_columns, c, a);
  } else {
    const int c = lane & (cpad - 1), g = lane / cpad, G = 64 / cpad;
    if (c < num_columns)
      for (int r = r0 + g; r < r1; r += G) pw_push(a, table[(size_t)r * ld + c]);
    for (int off = 32; off >= cpad; off >>= 1) {
      const PwState o = pw_shfl_xor(a, off);
      a = (lane & off) ? pw_merge(o, a) : pw_merge(a, o);
    }
    if (g == 0 && c < num_columns) pw_store(state, 1 + split, num_columns, c, a);
  }
}

// One wave per column: lane q holds the partial state of split q (an empty state from num_splits
// on), the 64 merge by the same butterfly (split q with split q + 32, the lower first, then 16,
// ...), and the running state (block 0) becomes running state, then that.  A serial walk over the
// splits by one lane per column measured 45 us at 64 splits: a chain of 64 dependent merges.
__global__ __launch_bounds__(64) void k_pointwise_merge(float* __restrict__ state, int num_columns, int num_splits,
                                                        int first) {
  const int c = blockIdx.x, lane = threadIdx.x;
  NMX_DCHECK(c < num_columns && num_splits <= NMX_POINTWISE_MAX_SPLITS);
  PwState a = lane < num_splits ? pw_load(state, 1 + lane, num_columns, c) : pw_empty();
  for (int off = 32; off >= 1; off >>= 1) {
    const PwState o = pw_shfl_xor(a, off);
    a = (lane & off) ? pw_merge(o, a) : pw_merge(a, o);
  }
  if (lane == 0) pw_store(state, 0, num_columns, c, first ? a : pw_merge(pw_load(state, 0, num_columns, c), a));
}

__global__ __launch_bounds__(64) void k_pointwise_finish(const float* __restrict__ state, int num_columns,
                                                         float* __restrict__ lppd, float* __restrict__ p_waic) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= num_columns) return;
  const PwState a = pw_load(state, 0, num_columns, c);
  if (lppd) lppd[c] = a.n > 0 ? (logf(a.s) + NmxProgram::lse_shift(a.m)) - logf((float)a.n) : NAN;
  if (p_waic) p_waic[c] = a.n > 1 ? a.m2 / (float)(a.n - 1) : NAN;
}

// rows of one split and the number of splits of a chunk of num_rows rows
inline int pw_rows_per_split(int num_rows) {
  const int by_min = NMX_POINTWISE_MIN_SPLIT_ROWS;
  const int by_max = (num_rows + NMX_POINTWISE_MAX_SPLITS - 1) / NMX_POINTWISE_MAX_SPLITS;
  return std::max(by_min, by_max);
}

}  // namespace

extern "C" int nmx_loglik_program_check(const nmx_program* hp, const int32_t* outputs, int num_outputs, int64_t ldo) {
  if (!hp || !hp->ops) return nmx_fail(NMX_ERR_INVALID, "program has NULL arrays");
  for (int k = 0; k < hp->num_ops; ++k) {
    const int op = hp->ops[(size_t)k * NMX_OP_WORDS];
    if (op >= NMX_DRAW_NORMAL && op < NMX_DRAW_END)
      return nmx_fail(NMX_ERR_INVALID, "op %d: a draw op (opcode %d) in a log-likelihood program", k, op);
  }
  if (num_outputs <= 0 || !outputs) return nmx_fail(NMX_ERR_INVALID, "a log-likelihood program needs outputs");
  std::vector<int32_t> pairs((size_t)num_outputs * 2);
  for (int j = 0; j < num_outputs; ++j) {
    pairs[2 * j] = outputs[3 * j];
    pairs[2 * j + 1] = outputs[3 * j + 1];
  }
  const int st = nmx_program_check_impl(hp, true, pairs.data(), num_outputs);
  if (st) return st;
  // the columns of the dense table: inside ldo, and no two outputs share one
  std::vector<std::pair<int64_t, int>> by_column;
  for (int j = 0; j < num_outputs; ++j) {
    const int64_t n = outputs[3 * j + 1], column = outputs[3 * j + 2];
    if (column < 0 || column + n > ldo)
      return nmx_fail(NMX_ERR_INVALID, "output %d: columns [%lld, %lld) outside the table's row of %lld", j,
                      (long long)column, (long long)(column + n), (long long)ldo);
    by_column.emplace_back(column, j);
  }
  std::sort(by_column.begin(), by_column.end());
  for (size_t t = 1; t < by_column.size(); ++t) {
    const int i = by_column[t - 1].second, j = by_column[t].second;
    if (by_column[t - 1].first + outputs[3 * i + 1] > by_column[t].first)
      return nmx_fail(NMX_ERR_INVALID, "outputs %d and %d overlap: columns [%lld, %lld) and [%lld, %lld)", i, j,
                      (long long)by_column[t - 1].first, (long long)(by_column[t - 1].first + outputs[3 * i + 1]),
                      (long long)by_column[t].first, (long long)(by_column[t].first + outputs[3 * j + 1]));
  }
  return NMX_OK;
}

extern "C" int nmx_loglik_program(const nmx_program* program, const float* samples, int num_samples,
                                  const int32_t* outputs, int num_outputs, float* tape, float* out, int64_t ldo,
                                  void* stream) {
  if (!program || !program->ops || !program->consts || !tape || program->num_ops <= 0 || program->dim < 0 ||
      program->num_slots <= program->dim || (program->num_index > 0 && !program->index))
    return nmx_fail(NMX_ERR_INVALID, "loglik_program: bad program or tape");
  if (program->dim > 0 && !samples) return nmx_fail(NMX_ERR_INVALID, "loglik_program: NULL samples with dim %d", program->dim);
  if (num_samples <= 0 || num_outputs <= 0 || !outputs || !out || ldo <= 0)
    return nmx_fail(NMX_ERR_INVALID, "loglik_program: bad num_samples / outputs / table (%d / %d / ldo %lld)", num_samples,
                    num_outputs, (long long)ldo);
  hipLaunchKernelGGL(k_program_loglik, dim3(num_samples), dim3(64), 0, (hipStream_t)stream,
                     NmxProgram{*program, nullptr}, samples, num_samples, outputs, num_outputs, tape, out, ldo);
  return nmx_check_launch("k_program_loglik");
}

extern "C" size_t nmx_pointwise_state_bytes(int num_columns) {
  if (num_columns <= 0) return 0;
  return (size_t)(1 + NMX_POINTWISE_MAX_SPLITS) * 5 * (size_t)num_columns * sizeof(float);
}

extern "C" int nmx_pointwise_accumulate(const float* table, int num_rows, int64_t ld, int num_columns, void* state,
                                        int first, void* stream) {
  if (!table || !state || num_rows <= 0 || num_columns <= 0 || ld < num_columns)
    return nmx_fail(NMX_ERR_INVALID, "pointwise_accumulate: bad table (%d rows, %d columns, ld %lld) or state", num_rows,
                    num_columns, (long long)ld);
  const int rows_per_split = pw_rows_per_split(num_rows);
  const int splits = (num_rows + rows_per_split - 1) / rows_per_split;  // <= NMX_POINTWISE_MAX_SPLITS
  int cpad = 64;
  if (num_columns < 64) {
    cpad = 1;
    while (cpad < num_columns) cpad <<= 1;
  }
  const int col_blocks = cpad == 64 ? (num_columns + 63) / 64 : 1;
  hipLaunchKernelGGL(k_pointwise_partial, dim3(col_blocks, splits), dim3(64), 0, (hipStream_t)stream, table, num_rows,
                     ld, num_columns, rows_per_split, cpad, (float*)state);
  int st = nmx_check_launch("k_pointwise_partial");
  if (st) return st;
  hipLaunchKernelGGL(k_pointwise_merge, dim3(num_columns), dim3(64), 0, (hipStream_t)stream, (float*)state,
                     num_columns, splits, first);
  return nmx_check_launch("k_pointwise_merge");
}

extern "C" int nmx_pointwise_finish(const void* state, int num_columns, float* lppd, float* p_waic, void* stream) {
  if (!state || num_columns <= 0 || (!lppd && !p_waic))
    return nmx_fail(NMX_ERR_INVALID, "pointwise_finish: bad state or outputs (%d columns)", num_columns);
  hipLaunchKernelGGL(k_pointwise_finish, dim3((num_columns + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                     (const float*)state, num_columns, lppd, p_waic);
  return nmx_check_launch("k_pointwise_finish");
}
