// Per-position body of the program potential (include/numpyro_amd.h "program potential"): one
// wave evaluates a straight-line program and its reverse-mode adjoint for one chain.  Kept as a
// struct, like the small models (nmx_small_models.h), so another kernel can inline the same body.
//
// Lane mapping: element i of every value is computed, and its adjoint accumulated, by lane
// i % 64 (scalars by lane 0).  An op whose operands are read at the element it writes needs no
// synchronisation; the ops that read across lanes (reduce, gather, matvec, cumsum, logsumexp,
// concat, a broadcast scalar slot) are preceded by a workgroup barrier, and every one of them
// writes only elements its lane owns.  Every sum has an order fixed by the program:
// a lane adds its elements i = lane, lane + 64, ... in order, the 64 partial sums are combined by
// a butterfly (every lane ends with the same bits); a cumsum is a wave scan per chunk of 64 with
// the carry of the chunk before.  No atomics.
//
// The dense ops (cholesky, trisolve; n <= NMX_CHOL_MAX_N = 128, so a lane holds at most two rows)
// work by matrix row: row i belongs to lane i % 64, which is not the owner of the flat element
// i * n + j.  The cholesky forward therefore ends with a barrier (its factor is written by row
// owners); every other final write of the four bodies is made by the element's owner lane: the
// solution of a trisolve by lane i % 64, the operands' adjoints in a last pass over the flat
// elements, after a barrier.  n comes from the op word, so all 64 lanes reach every barrier.
#pragma once
#include <math.h>

#include "nmx_common.h"

__device__ __forceinline__ float nmx_wave_sum(float x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
  return x;
}

// digamma(x), x > 0: the recurrence psi(x) = psi(x + 1) - 1/x up to x >= 8 (at most 8 steps; a
// non-finite or non-positive x leaves the loop by its bound), then the asymptotic series
// ln x - 1/(2x) - 1/(12x^2) + 1/(120x^4) - 1/(252x^6) (next term 1/(240 x^8) < 3e-9 at x = 8).
__device__ __forceinline__ float nmx_digammaf(float x) {
  float shift = 0.0f;
  for (int k = 0; k < 8 && x < 8.0f; ++k) {
    shift += 1.0f / x;
    x += 1.0f;
  }
  const float r = 1.0f / x, r2 = r * r;
  const float tail = r2 * (1.0f / 12 - r2 * (1.0f / 120 - r2 * (1.0f / 252)));
  return logf(x) - 0.5f * r - tail - shift;
}

// ---- NMX_OP_LRISING (include/numpyro_amd.h): R(a, k) = lgamma(a + k) - lgamma(a) - k log(a) and
// dR/da = digamma(a + k) - digamma(a) - k / a, neither as a difference of two lgamma / digamma
// values.  program.py _host_lrising restates both in float64 and float32.
//
// log1p(t) - t, t >= 0: below 1/2 the series of 2 atanh(s) - t at s = t / (2 + t), whose first
// term 2 s - t is -s t exactly (s^2 <= 0.04: the term after s^16 / 17 is below 1e-12 of the sum, so
// the float64 restatement of the host interpreter runs the same series)
__device__ __forceinline__ float nmx_log1pmx(float t) {
  if (!(t < 0.5f)) return log1pf(t) - t;
  const float s = t / (2.0f + t), s2 = s * s;
  float odd = 1.0f / 15 + s2 * (1.0f / 17);
  odd = 1.0f / 9 + s2 * (1.0f / 11 + s2 * (1.0f / 13 + s2 * odd));
  odd = 1.0f / 3 + s2 * (1.0f / 5 + s2 * (1.0f / 7 + s2 * odd));
  return s * (2.0f * s2 * odd - t);
}

// the Stirling tail lgamma(x) - ((x - 1/2) log x - x + log(2 pi) / 2) and its derivative, x >= 8
// (the next terms, 1 / (1188 x^9) and 1 / (132 x^10), are below 1e-11 there: the float64 restatement
// of the host interpreter runs the same series)
__device__ __forceinline__ float nmx_stirling_s(float x) {
  const float r = 1.0f / x, r2 = r * r;
  return (1.0f / 12 - (1.0f / 360 - (1.0f / 1260 - (1.0f / 1680) * r2) * r2) * r2) * r;
}
__device__ __forceinline__ float nmx_stirling_ds(float x) {
  const float r = 1.0f / x, r2 = r * r;
  return -r2 * (1.0f / 12 - r2 * (1.0f / 120 - r2 * (1.0f / 252 - r2 * (1.0f / 240))));
}

__device__ __forceinline__ bool nmx_lrising_by_sum(float k) { return k <= (float)NMX_LRISING_SUM_MAX && k == floorf(k); }

__device__ __forceinline__ float nmx_lrising(float a, float k) {
  if (!(a > 0.0f) || !(k >= 0.0f)) return NAN;
  if (nmx_lrising_by_sum(k)) {
    float s = 0.0f;
    for (int j = 1; j < NMX_LRISING_SUM_MAX; ++j)
      if ((float)j < k) s += log1pf((float)j / a);
    return s;
  }
  float x = a, shift = 0.0f, m = 0.0f;
  for (int j = 0; j < 8 && x < 8.0f; ++j) {
    shift += log1pf(k / x);
    x += 1.0f;
    m += 1.0f;
  }
  const float t = k / x;
  const float body = x * nmx_log1pmx(t) + (k - 0.5f) * log1pf(t) + (nmx_stirling_s(x + k) - nmx_stirling_s(x));
  return body + (k * log1pf(m / a) - shift);
}

__device__ __forceinline__ float nmx_lrising_da(float a, float k) {
  if (!(a > 0.0f) || !(k >= 0.0f)) return NAN;
  if (nmx_lrising_by_sum(k)) {
    float s = 0.0f;
    for (int j = 1; j < NMX_LRISING_SUM_MAX; ++j)
      if ((float)j < k) s += (float)j / (a * (a + (float)j));
    return -s;
  }
  float x = a, shift = 0.0f, m = 0.0f;
  for (int j = 0; j < 8 && x < 8.0f; ++j) {
    shift += k / (x * (x + k));
    x += 1.0f;
    m += 1.0f;
  }
  const float body =
      nmx_log1pmx(k / x) + 0.5f * k / (x * (x + k)) + (nmx_stirling_ds(x + k) - nmx_stirling_ds(x));
  return body + (shift - k * m / (a * x));
}

struct NmxOp {
  int op, dst, a, b, n, sa, sb, aux;
};

struct NmxProgram {
  nmx_program p;
  float* ws;  // [position][2][num_slots]: values, adjoints

  __device__ __forceinline__ NmxOp load(int k) const {
    const int32_t* w = p.ops + (size_t)k * NMX_OP_WORDS;
    return NmxOp{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]};
  }
  __device__ __forceinline__ float operand(const float* v, int ref, int i) const {
    NMX_DCHECK(ref >= 0 ? ref + i < p.num_slots : ~ref + i < p.num_consts);
    return ref >= 0 ? v[ref + i] : p.consts[~ref + i];
  }
  // the special ops (nmx_special_opcode) are elementwise and binary, numbered after the ops that are neither
  __device__ __forceinline__ static bool special(int op) { return op >= NMX_OP_LRISING && op < NMX_SPECIAL_END; }
  __device__ __forceinline__ static bool elementwise(int op) { return op < NMX_OP_REDUCE_SUM || special(op); }
  // the ops that read values other lanes wrote
  __device__ __forceinline__ static bool crosses(const NmxOp& o) { return !elementwise(o.op); }
  __device__ __forceinline__ static bool wave_per_row(int rows, int cols) { return rows < 64 && cols >= 64; }

  __device__ __forceinline__ static float fwd(int op, float x, float y) {
    switch (op) {
      case NMX_OP_NEG: return -x;
      case NMX_OP_EXP: return expf(x);
      case NMX_OP_LOG: return logf(x);
      case NMX_OP_SQRT: return sqrtf(x);
      case NMX_OP_TANH: return tanhf(x);
      case NMX_OP_LOG1P: return log1pf(x);
      case NMX_OP_SQUARE: return x * x;
      case NMX_OP_SOFTPLUS: return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x)));
      case NMX_OP_LGAMMA: return lgammaf(x);
      case NMX_OP_ADD: return x + y;
      case NMX_OP_SUB: return x - y;
      case NMX_OP_MUL: return x * y;
      case NMX_OP_DIV: return x / y;
      case NMX_OP_LRISING: return nmx_lrising(x, y);
      case NMX_OP_LOGADDEXP: return fmaxf(x, y) + log1pf(expf(x == y ? 0.0f : -fabsf(x - y)));
      default: return powf(x, y);  // NMX_OP_POW
    }
  }
  // adjoints of the operands from the result's (gd), the operands and the result
  __device__ __forceinline__ static void rev(int op, float gd, float x, float y, float out, float& da, float& db) {
    db = 0.0f;
    switch (op) {
      case NMX_OP_NEG: da = -gd; break;
      case NMX_OP_EXP: da = gd * out; break;
      case NMX_OP_LOG: da = gd / x; break;
      case NMX_OP_SQRT: da = gd * 0.5f / out; break;
      case NMX_OP_TANH: da = gd * (1.0f - out * out); break;
      case NMX_OP_LOG1P: da = gd / (1.0f + x); break;
      case NMX_OP_SQUARE: da = gd * (2.0f * x); break;
      case NMX_OP_SOFTPLUS: da = gd / (1.0f + expf(-x)); break;
      case NMX_OP_LGAMMA: da = gd * nmx_digammaf(x); break;
      case NMX_OP_ADD: da = gd; db = gd; break;
      case NMX_OP_SUB: da = gd; db = -gd; break;
      case NMX_OP_MUL: da = gd * y; db = gd * x; break;
      case NMX_OP_DIV: da = gd / y; db = -(gd * out) / y; break;
      case NMX_OP_LRISING: da = gd * nmx_lrising_da(x, y); break;  // k is data: no adjoint
      case NMX_OP_LOGADDEXP:
        da = out == -INFINITY ? 0.0f : gd * expf(x - out);
        db = out == -INFINITY ? 0.0f : gd * expf(y - out);
        break;
      default: da = gd * (y * powf(x, y - 1.0f)); db = gd * (out * logf(x)); break;  // NMX_OP_POW
    }
  }

  __device__ __forceinline__ void forward(const NmxOp& o, float* v, int lane) const {
    if (elementwise(o.op)) {
      const bool binary = o.op >= NMX_OP_ADD;
      for (int i = lane; i < o.n; i += 64) {
        const float x = operand(v, o.a, i * o.sa);
        const float y = binary ? operand(v, o.b, i * o.sb) : 0.0f;
        v[o.dst + i] = fwd(o.op, x, y);
      }
    } else if (o.op == NMX_OP_REDUCE_SUM) {
      float s = 0.0f;
      for (int i = lane; i < o.n; i += 64) s += v[o.a + i];
      s = nmx_wave_sum(s);
      if (lane == 0) v[o.dst] = s;
    } else if (o.op == NMX_OP_GATHER) {
      const int32_t* idx = p.index + o.aux;
      for (int i = lane; i < o.n; i += 64) v[o.dst + i] = v[o.a + idx[i]];
    } else if (o.op == NMX_OP_MATVEC) {
      const int K = o.aux;
      const float* M = p.consts + ~o.b;
      const float* Mt = M + (size_t)o.n * K;
      if (wave_per_row(o.n, K)) {
        for (int i = 0; i < o.n; ++i) {
          float s = 0.0f;
          for (int k = lane; k < K; k += 64) s += M[(size_t)i * K + k] * v[o.a + k];
          s = nmx_wave_sum(s);
          if (lane == (i & 63)) v[o.dst + i] = s;
        }
      } else {
        for (int i = lane; i < o.n; i += 64) {
          float s = 0.0f;
          for (int k = 0; k < K; ++k) s += Mt[(size_t)k * o.n + i] * v[o.a + k];
          v[o.dst + i] = s;
        }
      }
    } else if (__builtin_expect(o.op == NMX_OP_CUMSUM, 0)) {
      // inclusive scan of each chunk of 64 over the wave; the carry is the chunk's last element
      float carry = 0.0f;
      for (int base = 0; base < o.n; base += 64) {
        const int i = base + lane;
        float x = i < o.n ? v[o.a + i] : 0.0f;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
          const float y = __shfl_up(x, m, 64);
          if (lane >= m) x += y;
        }
        x += carry;
        if (i < o.n) v[o.dst + i] = x;
        carry = __shfl(x, 63, 64);
      }
    } else if (__builtin_expect(o.op == NMX_OP_LOGSUMEXP, 0)) {
      const int K = o.aux;
      if (wave_per_row(o.n, K)) {
        for (int i = 0; i < o.n; ++i) {
          const float* row = v + o.a + (size_t)i * K;
          float m = -INFINITY;
          for (int k = lane; k < K; k += 64) m = fmaxf(m, row[k]);
#pragma unroll
          for (int w = 32; w >= 1; w >>= 1) m = fmaxf(m, __shfl_xor(m, w, 64));
          m = lse_shift(m);
          float s = 0.0f;
          for (int k = lane; k < K; k += 64) s += expf(row[k] - m);
          s = nmx_wave_sum(s);
          if (lane == (i & 63)) v[o.dst + i] = logf(s) + m;
        }
      } else {
        for (int i = lane; i < o.n; i += 64) {
          const float* row = v + o.a + (size_t)i * K;
          float m = -INFINITY;
          for (int k = 0; k < K; ++k) m = fmaxf(m, row[k]);
          m = lse_shift(m);
          float s = 0.0f;
          for (int k = 0; k < K; ++k) s += expf(row[k] - m);
          v[o.dst + i] = logf(s) + m;
        }
      }
    } else if (__builtin_expect(o.op == NMX_OP_CHOLESKY, 0)) {
      cholesky_forward(o, v, lane);
    } else if (__builtin_expect(o.op == NMX_OP_TRISOLVE, 0)) {
      trisolve_forward(o, v, lane);
    } else {  // NMX_OP_CONCAT
      for (int i = lane; i < o.n; i += 64) v[o.dst + i] = i < o.aux ? operand(v, o.a, i) : operand(v, o.b, i - o.aux);
    }
  }
  // the shift of a log-sum-exp row: its maximum, or 0 where that is not finite (a row of -inf is
  // then log 0 = -inf, one with +inf is +inf, neither is inf - inf)
  __device__ __forceinline__ static float lse_shift(float m) { return fabsf(m) < INFINITY ? m : 0.0f; }

  __device__ __forceinline__ void reverse(const NmxOp& o, const float* v, float* g, int lane) const {
    if (elementwise(o.op)) {
      const bool binary = o.op >= NMX_OP_ADD;
      const bool ga = o.a >= 0, gb = binary && o.b >= 0;
      float pa = 0.0f, pb = 0.0f;  // adjoint of a broadcast scalar: this lane's part
      for (int i = lane; i < o.n; i += 64) {
        const float x = operand(v, o.a, i * o.sa);
        const float y = binary ? operand(v, o.b, i * o.sb) : 0.0f;
        float da, db;
        rev(o.op, g[o.dst + i], x, y, v[o.dst + i], da, db);
        if (ga) {
          if (o.sa) g[o.a + i] += da;
          else pa += da;
        }
        if (gb) {
          if (o.sb) g[o.b + i] += db;
          else pb += db;
        }
      }
      if (ga && !o.sa) {
        pa = nmx_wave_sum(pa);
        if (lane == 0) g[o.a] += pa;
      }
      if (gb && !o.sb) {
        pb = nmx_wave_sum(pb);
        if (lane == 0) g[o.b] += pb;
      }
    } else if (o.op == NMX_OP_REDUCE_SUM) {
      const float gd = g[o.dst];
      for (int i = lane; i < o.n; i += 64) g[o.a + i] += gd;
    } else if (o.op == NMX_OP_GATHER) {
      // segmented sum over the transposed index: source element j collects the results that read it
      const int32_t* start = p.index + o.aux + o.n;
      const int32_t* who = start + o.b + 1;
      for (int j = lane; j < o.b; j += 64) {
        float s = 0.0f;
        for (int t = start[j]; t < start[j + 1]; ++t) s += g[o.dst + who[t]];
        g[o.a + j] += s;
      }
    } else if (o.op == NMX_OP_MATVEC) {  // g_a += M^T g_dst
      const int K = o.aux;
      const float* M = p.consts + ~o.b;
      const float* Mt = M + (size_t)o.n * K;
      if (wave_per_row(K, o.n)) {
        for (int k = 0; k < K; ++k) {
          float s = 0.0f;
          for (int i = lane; i < o.n; i += 64) s += Mt[(size_t)k * o.n + i] * g[o.dst + i];
          s = nmx_wave_sum(s);
          if (lane == (k & 63)) g[o.a + k] += s;
        }
      } else {
        for (int k = lane; k < K; k += 64) {
          float s = 0.0f;
          for (int i = 0; i < o.n; ++i) s += M[(size_t)i * K + k] * g[o.dst + i];
          g[o.a + k] += s;
        }
      }
    } else if (__builtin_expect(o.op == NMX_OP_CUMSUM, 0)) {
      // g_a[j] += sum_{i >= j} g_dst[i]: the suffix scan, from the last chunk downwards
      float carry = 0.0f;
      for (int base = (o.n - 1) & ~63; base >= 0; base -= 64) {
        const int i = base + lane;
        float x = i < o.n ? g[o.dst + i] : 0.0f;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
          const float y = __shfl_down(x, m, 64);
          if (lane + m < 64) x += y;
        }
        x += carry;
        if (i < o.n) g[o.a + i] += x;
        carry = __shfl(x, 0, 64);
      }
    } else if (__builtin_expect(o.op == NMX_OP_LOGSUMEXP, 0)) {
      // by the owner of each flat element: reads its row's result and adjoint, writes its own
      const int K = o.aux, total = o.n * K;
      for (int e = lane; e < total; e += 64) {
        const int i = e / K;
        const float d = v[o.dst + i];
        const float w = d == -INFINITY ? 0.0f : expf(v[o.a + e] - d);
        g[o.a + e] += g[o.dst + i] * w;
      }
    } else if (__builtin_expect(o.op == NMX_OP_CHOLESKY, 0)) {
      cholesky_reverse(o, v, g, lane);
    } else if (__builtin_expect(o.op == NMX_OP_TRISOLVE, 0)) {
      trisolve_reverse(o, v, g, lane);
    } else {  // NMX_OP_CONCAT: each part by the owner of the operand's element
      if (o.a >= 0)
        for (int i = lane; i < o.aux; i += 64) g[o.a + i] += g[o.dst + i];
      if (o.b >= 0)
        for (int j = lane; j < o.n - o.aux; j += 64) g[o.b + j] += g[o.dst + o.aux + j];
    }
  }

  // ---- the dense ops: row i of a matrix is worked on by lane i % 64, rows `lane` and `lane + 64`
  // (n <= NMX_CHOL_MAX_N = 128).  No loop depends on a value: bad input gives NaN and returns.
  //
  // L = chol(A) column by column, left-looking: column j needs row j's earlier columns (written by
  // lane j % 64, hence the barrier) and the lane's own rows; the pivot travels by a shuffle.
  __device__ __forceinline__ void cholesky_forward(const NmxOp& o, float* v, int lane) const {
    const int n = o.aux;
    NMX_DCHECK(n >= 1 && n <= NMX_CHOL_MAX_N && o.n == n * n && o.a >= 0 && o.a + o.n <= o.dst);
    const float* A = v + o.a;
    float* L = v + o.dst;
    for (int e = lane; e < o.n; e += 64) {  // the strict upper triangle, by the owner of each element
      const int i = e / n;
      if (e - i * n > i) L[e] = 0.0f;
    }
    const int i0 = lane, i1 = lane + 64;
    for (int j = 0; j < n; ++j) {
      __syncthreads();
      const float* Lj = L + j * n;
      float s0 = 0.0f, s1 = 0.0f;
      if (i0 >= j && i0 < n) {
        float s = 0.0f;
        for (int k = 0; k < j; ++k) s += L[i0 * n + k] * Lj[k];
        s0 = A[i0 * n + j] - s;
      }
      if (i1 >= j && i1 < n) {
        float s = 0.0f;
        for (int k = 0; k < j; ++k) s += L[i1 * n + k] * Lj[k];
        s1 = A[i1 * n + j] - s;
      }
      const float pivot = __shfl(j < 64 ? s0 : s1, j & 63, 64);
      const float d = (pivot > 0.0f && pivot < INFINITY) ? sqrtf(pivot) : NAN;
      if (i0 >= j && i0 < n) L[i0 * n + j] = i0 == j ? d : s0 / d;
      if (i1 >= j && i1 < n) L[i1 * n + j] = i1 == j ? d : s1 / d;
    }
    __syncthreads();  // the factor was written by row owners: later ops read it by flat element
  }

  // Murray (2016), "Differentiation of the Cholesky decomposition", the unblocked level-2 reverse
  // sweep, in place on the lower triangle of Lbar (the adjoint slots of dst, dead after this op).
  // Column j of Lbar is final once step j has run and is never written afterwards, so its scaling
  // by 1 / L[j][j] waits for the last pass, where the owner of each flat element (r, c) of A adds
  // half of the (max, min) entry: g_a += (P + P^T) / 2 without a write to another lane's element.
  __device__ __forceinline__ void cholesky_reverse(const NmxOp& o, const float* v, float* g, int lane) const {
    const int n = o.aux;
    const float* L = v + o.dst;
    float* Lb = g + o.dst;
    for (int j = n - 1; j >= 0; --j) {
      __syncthreads();
      const float* Lj = L + j * n;
      float* Lbj = Lb + j * n;
      const float d = Lj[j];
      float t = 0.0f;
      for (int i = lane; i < n; i += 64)
        if (i > j) t += L[i * n + j] * Lb[i * n + j];
      t = nmx_wave_sum(t);
      const float db = (Lbj[j] - t / d) / d;
      for (int k = lane; k < j; k += 64) {  // row j, by column
        float s = 0.0f;
        for (int i = j + 1; i < n; ++i) s += Lb[i * n + j] * L[i * n + k];
        Lbj[k] -= db * Lj[k] + s / d;
      }
      for (int i = lane; i < n; i += 64) {  // the rows below, by row
        if (i <= j) continue;
        const float cb = Lb[i * n + j] / d;
        for (int k = 0; k < j; ++k) Lb[i * n + k] -= cb * Lj[k];
      }
      __syncthreads();  // every lane has read the diagonal's adjoint
      if (lane == (j & 63)) Lbj[j] = db;
    }
    __syncthreads();
    for (int e = lane; e < o.n; e += 64) {
      const int r = e / n, c = e - r * n;
      const int i = r > c ? r : c, j = r > c ? c : r;
      const float m = i > j ? Lb[i * n + j] / L[j * n + j] : Lb[e];
      g[o.a + e] += 0.5f * m;
    }
  }

  // x = L^-1 b by columns: once x[k] is known (a shuffle from its row's lane) every later row
  // subtracts L[i][k] x[k]; an element's updates run in column order and stay in its lane's registers
  __device__ __forceinline__ void trisolve_forward(const NmxOp& o, float* v, int lane) const {
    const int n = o.n;
    NMX_DCHECK(n >= 1 && n <= NMX_CHOL_MAX_N);
    const float* L = o.a >= 0 ? v + o.a : p.consts + ~o.a;
    const int i0 = lane, i1 = lane + 64;
    float y0 = i0 < n ? operand(v, o.b, i0) : 0.0f;
    float y1 = i1 < n ? operand(v, o.b, i1) : 0.0f;
    for (int k = 0; k < n; ++k) {
      const float xk = __shfl(k < 64 ? y0 : y1, k & 63, 64) / L[k * n + k];
      if (i0 == k) y0 = xk;
      else if (i0 > k && i0 < n) y0 -= L[i0 * n + k] * xk;
      if (i1 == k) y1 = xk;
      else if (i1 > k && i1 < n) y1 -= L[i1 * n + k] * xk;
    }
    if (i0 < n) v[o.dst + i0] = y0;
    if (i1 < n) v[o.dst + i1] = y1;
  }

  // w = L^-T g_dst by back substitution, columns from the last; g_b += w; then, w stored in dst's
  // adjoint slots (dead after this op), g_L[i][j] -= w[i] x[j] by the owner of each flat element
  __device__ __forceinline__ void trisolve_reverse(const NmxOp& o, const float* v, float* g, int lane) const {
    const int n = o.n;
    const float* L = o.a >= 0 ? v + o.a : p.consts + ~o.a;
    const int i0 = lane, i1 = lane + 64;
    float y0 = i0 < n ? g[o.dst + i0] : 0.0f;
    float y1 = i1 < n ? g[o.dst + i1] : 0.0f;
    for (int k = n - 1; k >= 0; --k) {
      const float wk = __shfl(k < 64 ? y0 : y1, k & 63, 64) / L[k * n + k];
      if (i0 == k) y0 = wk;
      else if (i0 < k) y0 -= L[k * n + i0] * wk;
      if (i1 == k) y1 = wk;
      else if (i1 < k) y1 -= L[k * n + i1] * wk;
    }
    if (o.b >= 0) {
      if (i0 < n) g[o.b + i0] += y0;
      if (i1 < n) g[o.b + i1] += y1;
    }
    if (o.a >= 0) {
      if (i0 < n) g[o.dst + i0] = y0;
      if (i1 < n) g[o.dst + i1] = y1;
      __syncthreads();
      for (int e = lane; e < n * n; e += 64) {
        const int i = e / n, j = e - i * n;
        if (j <= i) g[o.a + e] -= g[o.dst + i] * v[o.dst + j];
      }
    }
  }

  // a broadcast scalar slot is read by every lane and was written by lane 0
  __device__ __forceinline__ static bool reads_scalar_slot(const NmxOp& o) {
    if (!elementwise(o.op) || o.n == 1) return false;
    return (o.a >= 0 && !o.sa) || (o.op >= NMX_OP_ADD && o.b >= 0 && !o.sb);
  }
  // z slots are referenced at any offset: their adjoints have no fixed lane
  __device__ __forceinline__ bool touches_z(const NmxOp& o) const {
    const bool b_is_operand =
        (o.op >= NMX_OP_ADD && elementwise(o.op)) || o.op == NMX_OP_CONCAT || o.op == NMX_OP_TRISOLVE;
    return (o.a >= 0 && o.a < p.dim) || (b_is_operand && o.b >= 0 && o.b < p.dim);
  }

  // chain c at position pos of the batch; called by all 64 lanes of a one-wave workgroup
  __device__ __forceinline__ void operator()(const nmx_eval_batch& ev, int c, int pos, int lane) const {
    const int S = p.num_slots, D = p.dim;
    NMX_DCHECK(pos >= 0 && pos < ev.ldc && c >= 0 && c < ev.ldc);
    float* v = ws + (size_t)pos * 2 * S;
    float* g = v + S;
    for (int i = lane; i < S; i += 64) g[i] = 0.0f;
    for (int d = lane; d < D; d += 64) v[d] = ev.z[(size_t)d * ev.ldc + c];
    __syncthreads();
    for (int k = 0; k < p.num_ops; ++k) {
      const NmxOp o = load(k);
      if (crosses(o) || reads_scalar_slot(o)) __syncthreads();
      forward(o, v, lane);
    }
    __syncthreads();
    if (lane == 0) g[S - 1] = 1.0f;
    for (int k = p.num_ops - 1; k >= 0; --k) {
      const NmxOp o = load(k);
      if (crosses(o) || touches_z(o)) __syncthreads();
      reverse(o, v, g, lane);
    }
    __syncthreads();
    for (int d = lane; d < D; d += 64) ev.grad[(size_t)d * ev.ldc + c] = g[d];
    if (lane == 0) ev.pe[c] = v[S - 1];
  }
};

// ---- predictive programs (include/numpyro_amd.h "predictive programs"): the forward half of
// the interpreter plus draw ops, one wave per posterior sample.  Element i of a draw is produced
// by lane i % 64 from its own Philox blocks nmx_rng(seed, sample, stream, NMX_EV_PREDICT, i,
// attempt): no cross-lane traffic, no atomics.  Word assignment (the header states it in full,
// program.py PredictiveProgram.run_host is its float64 restatement):
//   normal       Box-Muller cos branch of (w0.x, w0.y)        exponential  -log u01_open0(w0.x)
//   cauchy       tan(pi (mid24(w0.x) - 0.5))                  bernoulli    u01(w0.x) < p
//   gamma        attempt t: normal of (wt.x, wt.y), accept uniform wt.z, boost uniform wt.w
//   poisson      rate < 10: inversion of u01(w0.x); else PTRS, attempt t: (wt.x, wt.y)
//   uniform      u01(w0.x)
//   binomial     q = min(p, 1 - p); n q < 10: inversion of u01(w0.x); else BTRS, attempt t: (wt.x, wt.y)
// Every loop has a compile-time bound (NMX_DRAW_MAX_ATTEMPTS, NMX_POISSON_MAX_STEPS,
// NMX_BINOMIAL_MAX_STEPS) and a parameter outside the support returns NaN before any loop: bad
// input cannot make a lane spin.
__device__ __forceinline__ float nmx_draw_normal(const nmx_u4& w) {
  float z, unused;
  nmx_box_muller(w.x, w.y, z, unused);
  return z;
}

__device__ __forceinline__ float nmx_draw_gamma(float a, uint64_t seed, uint32_t s, uint32_t stream, uint32_t i) {
  if (!(a > 0.0f) || a == INFINITY) return NAN;
  const bool boost = a < 1.0f;
  const float a1 = boost ? a + 1.0f : a;
  const float d = a1 - 1.0f / 3.0f, c = 1.0f / sqrtf(9.0f * d);
  for (uint32_t t = 0; t < NMX_DRAW_MAX_ATTEMPTS; ++t) {
    const nmx_u4 w = nmx_rng(seed, s, stream, NMX_EV_PREDICT, i, t);
    const float x = nmx_draw_normal(w);
    const float y = 1.0f + c * x;
    if (!(y > 0.0f)) continue;
    const float v = y * y * y;
    if (logf(nmx_u01_open0(w.z)) < 0.5f * x * x + d - d * v + d * logf(v))
      return boost ? d * v * expf(logf(nmx_u01_open0(w.w)) / a) : d * v;
  }
  return NAN;
}

// log(j!) minus the Stirling formula at j + 1 (Hoermann 1993, the f(k) of BTRS), j >= 0 whole
static __device__ const float NMX_STIRLING_TAIL[10] = {
    0.08106146679532726f, 0.04134069595540929f, 0.02767792568499834f, 0.02079067210376509f, 0.01664469118982119f,
    0.01387612882307075f, 0.01189670994589177f, 0.01041126526197209f, 0.009255462182712733f, 0.008330563433362871f};

__device__ __forceinline__ float nmx_stirling_tail(float j) {
  if (j < 10.0f) return NMX_STIRLING_TAIL[(int)j];
  const float r = 1.0f / (j + 1.0f), r2 = r * r;
  return (1.0f / 12 - (1.0f / 360 - (1.0f / 1260) * r2) * r2) * r;
}

// The slow acceptance compares with log pmf(k) = -rate + k log rate - log k!, whose terms are of
// size k log k (1.4e7 at rate 1e6, where one f32 ulp is 1) and whose value is of order 1.  With
// log k! as the Stirling formula at k1 = k + 1 plus its tail they cancel inside one log1p:
//   k log1p((rate - k1) / k1) - (rate - k1) - log(k1) / 2 - log(2 pi) / 2 - tail(k)
__device__ __forceinline__ float nmx_draw_poisson(float rate, uint64_t seed, uint32_t s, uint32_t stream,
                                                  uint32_t i) {
  if (!(rate >= 0.0f && rate < NMX_POISSON_MAX_RATE)) return NAN;
  if (rate == 0.0f) return 0.0f;
  if (rate < NMX_POISSON_PTRS_RATE) {
    const float u = nmx_u01(nmx_rng(seed, s, stream, NMX_EV_PREDICT, i, 0).x);
    float p = expf(-rate), sum = p, k = 0.0f;
    for (int step = 0; step < NMX_POISSON_MAX_STEPS; ++step) {
      if (u <= sum) return k;
      k += 1.0f;
      p = p * rate / k;
      sum += p;
      if (p < 0x1p-40f && k > rate) return k;
    }
    return NAN;
  }
  const float b = 0.931f + 2.53f * sqrtf(rate), a = -0.059f + 0.02483f * b;
  const float inv_alpha = 1.1239f + 1.1328f / (b - 3.4f), v_r = 0.9277f - 3.6224f / (b - 2.0f);
  for (uint32_t t = 0; t < NMX_DRAW_MAX_ATTEMPTS; ++t) {
    const nmx_u4 w = nmx_rng(seed, s, stream, NMX_EV_PREDICT, i, t);
    const float U = nmx_u01(w.x) - 0.5f, V = nmx_u01_open0(w.y);
    const float us = 0.5f - fabsf(U);
    const float k = floorf((2.0f * a / us + b) * U + rate + 0.43f);
    if (us >= 0.07f && V <= v_r) return k;
    if (!(k >= 0.0f) || (us < 0.013f && V > us)) continue;
    const float k1 = k + 1.0f, excess = rate - k1;
    const float log_pmf =
        k * log1pf(excess / k1) - excess - 0.5f * logf(k1) - 0.9189385332046727f - nmx_stirling_tail(k);
    if (logf(V * inv_alpha / (a / (us * us) + b)) <= log_pmf) return k;
  }
  return NAN;
}

// Inlined like the other draws: k_program_predict keeps its occupancy (80 VGPRs, 6 waves / SIMD),
// while the out-of-line form measured 106 VGPRs and 4 waves (DESIGN.md "Predictive programs").
// log((n - j + 1) q / ((j + 1) (1 - q))) is one log1p of ((n + 2) q - (j + 1)) / ((j + 1) (1 - q)) with
// n q - j from one fmaf: as log((n - j + 1) / (j + 1)) + log(q / (1 - q)) the two logs cancel near the
// mode and the quotient's rounding error, times j, reaches 1 at counts near 2^24.
__device__ __forceinline__ float nmx_binomial_log_odds(float n, float q, float j) {
  return log1pf((fmaf(n, q, -j) + (2.0f * q - 1.0f)) / ((j + 1.0f) * (1.0f - q)));
}

__device__ __forceinline__ float nmx_draw_binomial(float n, float p, uint64_t seed, uint32_t s, uint32_t stream,
                                                uint32_t i) {
  if (!(p >= 0.0f && p <= 1.0f) || !(n >= 0.0f && n < NMX_BINOMIAL_MAX_COUNT) || n != floorf(n)) return NAN;
  if (p == 0.0f || n == 0.0f) return 0.0f;
  if (p == 1.0f) return n;
  const bool mirror = p > 0.5f;
  const float q = mirror ? 1.0f - p : p;
  const float mu = n * q, log1_q = log1pf(-q);
  if (mu < NMX_BINOMIAL_BTRS_MEAN) {
    const float u = nmx_u01(nmx_rng(seed, s, stream, NMX_EV_PREDICT, i, 0).x);
    const float odds = q / (1.0f - q);
    float f = expf(n * log1_q), sum = f, k = 0.0f;
    for (int step = 0; step < NMX_BINOMIAL_MAX_STEPS; ++step) {
      if (u <= sum || k >= n) return mirror ? n - k : k;
      k += 1.0f;
      f = f * (n - k + 1.0f) / k * odds;
      sum += f;
      if (f < 0x1p-40f && k > mu) return mirror ? n - k : k;
    }
    return NAN;
  }
  const float spq = sqrtf(mu * (1.0f - q)), c = mu + 0.5f;
  const float b = 1.15f + 2.53f * spq, a = -0.0873f + 0.0248f * b + 0.01f * q;
  const float alpha = (2.83f + 5.1f / b) * spq, v_r = 0.92f - 4.2f / b;
  const float m = floorf((n + 1.0f) * q);
  const float log_h =
      (nmx_stirling_tail(m) + nmx_stirling_tail(n - m)) - (m + 0.5f) * nmx_binomial_log_odds(n, q, m);
  for (uint32_t t = 0; t < NMX_DRAW_MAX_ATTEMPTS; ++t) {
    const nmx_u4 w = nmx_rng(seed, s, stream, NMX_EV_PREDICT, i, t);
    const float U = nmx_u01(w.x) - 0.5f, V = nmx_u01_open0(w.y);
    const float us = 0.5f - fabsf(U);
    const float k = floorf((2.0f * a / us + b) * U + c);
    if (us >= 0.07f && V <= v_r) return mirror ? n - k : k;
    if (!(k >= 0.0f && k <= n)) continue;
    const float log_f = (n + 1.0f) * log1pf((k - m) / (n - k + 1.0f)) +
                        (k + 0.5f) * nmx_binomial_log_odds(n, q, k) +
                        (nmx_stirling_tail(k) - nmx_stirling_tail(n - k)) + log_h;
    if (logf(V * alpha / (a / (us * us) + b)) <= log_f) return mirror ? n - k : k;
  }
  return NAN;
}

struct NmxPredict {
  NmxProgram prog;  // p.dim = given coordinates; ws unused (the tape holds values only)
  uint64_t seed;

  __device__ __forceinline__ static bool is_draw(const NmxOp& o) { return o.op >= NMX_DRAW_NORMAL; }
  __device__ __forceinline__ static bool has_param(const NmxOp& o) {
    return o.op >= NMX_DRAW_GAMMA && o.op != NMX_DRAW_UNIFORM;
  }
  __device__ __forceinline__ static bool has_param_b(const NmxOp& o) { return o.op == NMX_DRAW_BINOMIAL; }
  // the barrier rule of NmxProgram::reads_scalar_slot for a draw's parameters
  __device__ __forceinline__ static bool reads_scalar_slot(const NmxOp& o) {
    if (o.n == 1) return false;
    return (has_param(o) && o.a >= 0 && !o.sa) || (has_param_b(o) && o.b >= 0 && !o.sb);
  }

  __device__ __forceinline__ void draw(const NmxOp& o, float* v, int lane, uint32_t s) const {
    const uint32_t stream = (uint32_t)o.aux;
    for (int i = lane; i < o.n; i += 64) {
      const float a = has_param(o) ? prog.operand(v, o.a, i * o.sa) : 0.0f;
      float r;
      switch (o.op) {
        case NMX_DRAW_NORMAL: r = nmx_draw_normal(nmx_rng(seed, s, stream, NMX_EV_PREDICT, i, 0)); break;
        case NMX_DRAW_EXPONENTIAL:
          r = -logf(nmx_u01_open0(nmx_rng(seed, s, stream, NMX_EV_PREDICT, i, 0).x));
          break;
        case NMX_DRAW_CAUCHY: {
          const uint32_t x = nmx_rng(seed, s, stream, NMX_EV_PREDICT, i, 0).x;
          r = tanf(3.14159265358979323846f * (((float)(x >> 8) + 0.5f) * 5.9604644775390625e-08f - 0.5f));
          break;
        }
        case NMX_DRAW_GAMMA: r = nmx_draw_gamma(a, seed, s, stream, i); break;
        case NMX_DRAW_BERNOULLI:
          r = (a >= 0.0f && a <= 1.0f) ? (nmx_u01(nmx_rng(seed, s, stream, NMX_EV_PREDICT, i, 0).x) < a ? 1.0f : 0.0f)
                                       : NAN;
          break;
        case NMX_DRAW_POISSON: r = nmx_draw_poisson(a, seed, s, stream, i); break;
        case NMX_DRAW_UNIFORM: r = nmx_u01(nmx_rng(seed, s, stream, NMX_EV_PREDICT, i, 0).x); break;
        default:  // NMX_DRAW_BINOMIAL
          r = nmx_draw_binomial(a, prog.operand(v, o.b, i * o.sb), seed, s, stream, i);
          break;
      }
      NMX_DCHECK(o.dst >= prog.p.dim && o.dst + i < prog.p.num_slots);
      v[o.dst + i] = r;
    }
  }

  // row `row` of samples / tape, global sample index s; called by all 64 lanes of a one-wave workgroup
  __device__ __forceinline__ void operator()(const float* samples, float* tape, int row, uint32_t s, int lane) const {
    const nmx_program& p = prog.p;
    float* v = tape + (size_t)row * p.num_slots;
    NMX_DCHECK(row >= 0 && p.dim >= 0 && p.dim <= p.num_slots && (p.dim == 0 || samples));
    for (int d = lane; d < p.dim; d += 64) v[d] = samples[(size_t)row * p.dim + d];
    __syncthreads();
    for (int k = 0; k < p.num_ops; ++k) {
      const NmxOp o = prog.load(k);
      if (is_draw(o)) {
        if (reads_scalar_slot(o)) __syncthreads();
        draw(o, v, lane, s);
      } else {
        if (NmxProgram::crosses(o) || NmxProgram::reads_scalar_slot(o)) __syncthreads();
        prog.forward(o, v, lane);
      }
    }
  }
};
