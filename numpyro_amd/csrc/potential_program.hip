// Program potential: the generic path of the model front end.  One wave (a 64-thread
// workgroup) per evaluated position interprets the traced model's program and its adjoint
// (per-position body in nmx_program.h); nmx_program_check validates a program on the host
// before it may be uploaded, so every address the kernel forms comes from checked fields.
#include <math.h>

#include <vector>

#include "nmx_api_internal.h"
#include "nmx_common.h"
#include "nmx_program.h"

namespace {

// 7 waves / SIMD was the kernel's occupancy before the special ops (67 VGPRs); their cases made the
// allocator take 75 (6 waves) although no path needs them all at once.  With the occupancy stated
// it allocates 72, without a spill or scratch (as k_program_predict, predictive_program.hip).
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(7))) void k_program(NmxProgram prog,
                                                                                        nmx_eval_batch ev) {
  const int pos = blockIdx.x;
  const int c = nmx_eval_chain(ev, pos);
  if (c < 0) return;
  prog(ev, c, pos, threadIdx.x);
}

const char* const OP_NAMES[NMX_NUM_OPCODES] = {"neg", "exp", "log", "sqrt", "tanh", "log1p", "square", "softplus",
                                               "lgamma", "add", "sub", "mul", "div", "pow", "reduce_sum",
                                               "gather", "matvec", "cumsum", "logsumexp", "concat"};
const char* const LINALG_NAMES[NMX_LINALG_END - NMX_OP_CHOLESKY] = {"cholesky", "trisolve"};
const char* const SPECIAL_NAMES[NMX_SPECIAL_END - NMX_OP_LRISING] = {"lrising", "logaddexp"};
const char* const DRAW_NAMES[NMX_DRAW_END - NMX_DRAW_NORMAL] = {"draw_normal", "draw_exponential", "draw_cauchy",
                                                                "draw_gamma", "draw_bernoulli", "draw_poisson",
                                                                "draw_uniform", "draw_binomial"};

}  // namespace

// The check of both program kinds.  A potential program (predictive = false) has dim > 0, the
// arithmetic ops alone and U as its last slot; a predictive program may have dim = 0 and draw
// ops, has no U, and its outputs { slot, n } must lie in z or inside one defined value.
int nmx_program_check_impl(const nmx_program* hp, bool predictive, const int32_t* outputs, int num_outputs) {
  if (!hp || !hp->ops || !hp->consts) return nmx_fail(NMX_ERR_INVALID, "program has NULL arrays");
  const nmx_program& p = *hp;
  if (p.num_ops <= 0 || p.dim < (predictive ? 0 : 1) || p.num_slots <= p.dim || p.num_consts < 0 || p.num_index < 0)
    return nmx_fail(NMX_ERR_INVALID, "program sizes: %d ops, %d slots, dim %d, %d constants, %d indices", p.num_ops,
                    p.num_slots, p.dim, p.num_consts, p.num_index);
  if (p.num_index > 0 && !p.index) return nmx_fail(NMX_ERR_INVALID, "program has a NULL index pool");
  // length of the value defined at each slot (0: not the start of a value)
  std::vector<int32_t> def_len((size_t)p.num_slots, 0);
  int64_t cursor = p.dim;
  int num_draws = 0;
  for (int k = 0; k < p.num_ops; ++k) {
    const int32_t* w = p.ops + (size_t)k * NMX_OP_WORDS;
    const int op = w[0], dst = w[1], a = w[2], b = w[3], n = w[4], sa = w[5], sb = w[6], aux = w[7];
    const bool draw = predictive && op >= NMX_DRAW_NORMAL && op < NMX_DRAW_END;
    const bool linalg = op >= NMX_OP_CHOLESKY && op < NMX_LINALG_END;
    const bool special = op >= NMX_OP_LRISING && op < NMX_SPECIAL_END;
    if (!draw && !linalg && !special && (op < 0 || op >= NMX_NUM_OPCODES))
      return nmx_fail(NMX_ERR_INVALID, "op %d: bad opcode %d", k, op);
    const char* nm = draw      ? DRAW_NAMES[op - NMX_DRAW_NORMAL]
                     : linalg  ? LINALG_NAMES[op - NMX_OP_CHOLESKY]
                     : special ? SPECIAL_NAMES[op - NMX_OP_LRISING]
                               : OP_NAMES[op];
    if (n <= 0) return nmx_fail(NMX_ERR_INVALID, "op %d (%s): count %d <= 0", k, nm, n);
    const int64_t dst_len = op == NMX_OP_REDUCE_SUM ? 1 : n;
    if (dst != cursor || cursor + dst_len > p.num_slots)
      return nmx_fail(NMX_ERR_INVALID, "op %d (%s): destination slot %d (+%lld) out of range or out of order "
                      "(next free slot %lld of %d)", k, nm, dst, (long long)dst_len, (long long)cursor, p.num_slots);
    // a slot operand of `len` elements: inside z, or the start of an earlier op's value
    auto slot_ok = [&](int ref, int64_t len) {
      if (ref < 0 || ref >= dst) return false;
      if (ref < p.dim) return ref + len <= p.dim;
      return def_len[ref] >= len;
    };
    auto const_ok = [&](int ref, int64_t len) { return ref < 0 && (int64_t)~ref + len <= p.num_consts; };
    if (draw) {
      if (n > 0x01000000)
        return nmx_fail(NMX_ERR_INVALID, "op %d (%s): count %d above 2^24 (the counter's element field)", k, nm, n);
      if (aux != num_draws)
        return nmx_fail(NMX_ERR_INVALID, "op %d (%s): stream id %d is not the draw's ordinal %d", k, nm, aux, num_draws);
      ++num_draws;
      if (op >= NMX_DRAW_GAMMA && op != NMX_DRAW_UNIFORM) {
        if (sa != 0 && sa != 1) return nmx_fail(NMX_ERR_INVALID, "op %d (%s): stride %d not 0 or 1", k, nm, sa);
        const int64_t la = sa ? n : 1;
        if (a >= 0 ? !slot_ok(a, la) : !const_ok(a, la))
          return nmx_fail(NMX_ERR_INVALID, "op %d (%s): parameter %s %d (x%lld) out of range", k, nm,
                          a >= 0 ? "slot" : "constant", a >= 0 ? a : ~a, (long long)la);
      }
      if (op == NMX_DRAW_BINOMIAL) {
        if (sb != 0 && sb != 1)
          return nmx_fail(NMX_ERR_INVALID, "op %d (%s): second stride %d not 0 or 1", k, nm, sb);
        const int64_t lb = sb ? n : 1;
        if (b >= 0 ? !slot_ok(b, lb) : !const_ok(b, lb))
          return nmx_fail(NMX_ERR_INVALID, "op %d (%s): second parameter %s %d (x%lld) out of range", k, nm,
                          b >= 0 ? "slot" : "constant", b >= 0 ? b : ~b, (long long)lb);
      }
    } else if (op == NMX_OP_CHOLESKY) {
      if (aux < 1 || aux > NMX_CHOL_MAX_N)
        return nmx_fail(NMX_ERR_INVALID, "op %d (%s): matrix dimension %d (aux) outside [1, %d]", k, nm, aux,
                        NMX_CHOL_MAX_N);
      if (n != aux * aux)
        return nmx_fail(NMX_ERR_INVALID, "op %d (%s): count %d is not %d x %d", k, nm, n, aux, aux);
      if (!slot_ok(a, n))
        return nmx_fail(NMX_ERR_INVALID, "op %d (%s): matrix operand slot %d of %d x %d elements out of range", k, nm, a,
                        aux, aux);
    } else if (op == NMX_OP_TRISOLVE) {
      if (n > NMX_CHOL_MAX_N)
        return nmx_fail(NMX_ERR_INVALID, "op %d (%s): dimension %d above %d", k, nm, n, NMX_CHOL_MAX_N);
      const int64_t la = (int64_t)n * n, lb = n;
      if (a >= 0 ? !slot_ok(a, la) : !const_ok(a, la))
        return nmx_fail(NMX_ERR_INVALID, "op %d (%s): matrix operand %s %d of %d x %d elements out of range", k, nm,
                        a >= 0 ? "slot" : "constant", a >= 0 ? a : ~a, n, n);
      if (b >= 0 ? !slot_ok(b, lb) : !const_ok(b, lb))
        return nmx_fail(NMX_ERR_INVALID, "op %d (%s): right-hand side %s %d (x%d) out of range", k, nm,
                        b >= 0 ? "slot" : "constant", b >= 0 ? b : ~b, n);
      if (a < 0 && b < 0) return nmx_fail(NMX_ERR_INVALID, "op %d (%s): both operands constant", k, nm);
      // as for the elementwise ops: no barrier between the two updates of the reverse op
      if (!predictive && a >= 0 && b >= 0 && a < p.dim && b < p.dim && a < b + lb && b < a + la)
        return nmx_fail(NMX_ERR_INVALID, "op %d (%s): operands z[%d:%lld] and z[%d:%lld] overlap", k, nm, a,
                        (long long)(a + la), b, (long long)(b + lb));
    } else if (op < NMX_OP_REDUCE_SUM || special) {
      const bool binary = op >= NMX_OP_ADD;
      if ((sa != 0 && sa != 1) || (sb != 0 && sb != 1))
        return nmx_fail(NMX_ERR_INVALID, "op %d (%s): strides %d, %d not 0 or 1", k, nm, sa, sb);
      const int64_t la = sa ? n : 1, lb = sb ? n : 1;
      if (a >= 0 ? !slot_ok(a, la) : (!binary || !const_ok(a, la)))
        return nmx_fail(NMX_ERR_INVALID, "op %d (%s): first operand %s %d (x%lld) out of range", k, nm,
                        a >= 0 ? "slot" : "constant", a >= 0 ? a : ~a, (long long)la);
      if (binary) {
        if (b >= 0 ? !slot_ok(b, lb) : !const_ok(b, lb))
          return nmx_fail(NMX_ERR_INVALID, "op %d (%s): second operand %s %d (x%lld) out of range", k, nm,
                          b >= 0 ? "slot" : "constant", b >= 0 ? b : ~b, (long long)lb);
        if (a < 0 && b < 0) return nmx_fail(NMX_ERR_INVALID, "op %d (%s): both operands constant", k, nm);
        if (op == NMX_OP_LRISING && b >= 0)
          return nmx_fail(NMX_ERR_INVALID, "op %d (%s): the step count k is slot %d, it must be a constant (the op has "
                          "no adjoint for it)", k, nm, b);
        // the adjoint of a z element has no fixed lane and the reverse op has no barrier between
        // its two updates: two z operands may share elements only as the same reference
        if (!predictive && a >= 0 && b >= 0 && a != b && a < p.dim && b < p.dim && a < b + lb && b < a + la)
          return nmx_fail(NMX_ERR_INVALID, "op %d (%s): operands z[%d:%lld] and z[%d:%lld] overlap at different "
                          "offsets", k, nm, a, (long long)(a + la), b, (long long)(b + lb));
      }
    } else if (op == NMX_OP_REDUCE_SUM) {
      if (!slot_ok(a, n)) return nmx_fail(NMX_ERR_INVALID, "op %d (%s): operand slot %d (x%d) out of range", k, nm, a, n);
    } else if (op == NMX_OP_GATHER) {
      if (b <= 0 || !slot_ok(a, b))
        return nmx_fail(NMX_ERR_INVALID, "op %d (%s): source slot %d of length %d out of range", k, nm, a, b);
      if (aux < 0 || (int64_t)aux + 2 * (int64_t)n + b + 1 > p.num_index)
        return nmx_fail(NMX_ERR_INVALID, "op %d (%s): index reference %d (+%lld) outside the pool of %d", k, nm, aux,
                        (long long)(2 * (int64_t)n + b + 1), p.num_index);
      const int32_t* idx = p.index + aux;
      const int32_t* start = idx + n;
      const int32_t* who = start + b + 1;
      for (int i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= b)
          return nmx_fail(NMX_ERR_INVALID, "op %d (%s): index %d at element %d outside its source of length %d", k, nm,
                          idx[i], i, b);
      if (start[0] != 0 || start[b] != n)
        return nmx_fail(NMX_ERR_INVALID, "op %d (%s): transposed index does not cover %d elements", k, nm, n);
      for (int j = 0; j < b; ++j) {
        if (start[j + 1] < start[j] || start[j + 1] > n)
          return nmx_fail(NMX_ERR_INVALID, "op %d (%s): transposed index row %d is not ordered", k, nm, j);
        for (int t = start[j]; t < start[j + 1]; ++t)
          if (who[t] < 0 || who[t] >= n || idx[who[t]] != j)
            return nmx_fail(NMX_ERR_INVALID, "op %d (%s): transposed index entry %d does not match the index", k, nm, t);
      }
    } else if (op == NMX_OP_MATVEC) {
      if (aux <= 0 || !slot_ok(a, aux))
        return nmx_fail(NMX_ERR_INVALID, "op %d (%s): vector slot %d of length %d out of range", k, nm, a, aux);
      if (!const_ok(b, 2 * (int64_t)n * aux))
        return nmx_fail(NMX_ERR_INVALID, "op %d (%s): matrix constant %d (%d x %d and its transpose) outside the pool "
                        "of %d", k, nm, b < 0 ? ~b : b, n, aux, p.num_consts);
    } else if (op == NMX_OP_CUMSUM) {
      if (!slot_ok(a, n)) return nmx_fail(NMX_ERR_INVALID, "op %d (%s): operand slot %d (x%d) out of range", k, nm, a, n);
    } else if (op == NMX_OP_LOGSUMEXP) {
      if (aux < 1) return nmx_fail(NMX_ERR_INVALID, "op %d (%s): %d columns (aux) < 1", k, nm, aux);
      const int64_t len = (int64_t)n * aux;  // a value of `len` slots fits the int32 slot count
      if (!slot_ok(a, len))
        return nmx_fail(NMX_ERR_INVALID, "op %d (%s): operand slot %d of %d x %d = %lld elements out of range", k, nm, a,
                        n, aux, (long long)len);
    } else {  // NMX_OP_CONCAT
      if (aux <= 0 || aux >= n)
        return nmx_fail(NMX_ERR_INVALID, "op %d (%s): first part of %d elements (aux) not inside (0, %d)", k, nm, aux, n);
      const int64_t la = aux, lb = n - aux;
      if (a >= 0 ? !slot_ok(a, la) : !const_ok(a, la))
        return nmx_fail(NMX_ERR_INVALID, "op %d (%s): first operand %s %d (x%lld) out of range", k, nm,
                        a >= 0 ? "slot" : "constant", a >= 0 ? a : ~a, (long long)la);
      if (b >= 0 ? !slot_ok(b, lb) : !const_ok(b, lb))
        return nmx_fail(NMX_ERR_INVALID, "op %d (%s): second operand %s %d (x%lld) out of range", k, nm,
                        b >= 0 ? "slot" : "constant", b >= 0 ? b : ~b, (long long)lb);
      if (a < 0 && b < 0) return nmx_fail(NMX_ERR_INVALID, "op %d (%s): both operands constant", k, nm);
      // as for the elementwise ops: the reverse op has no barrier between its two updates
      if (!predictive && a >= 0 && b >= 0 && a != b && a < p.dim && b < p.dim && a < b + lb && b < a + la)
        return nmx_fail(NMX_ERR_INVALID, "op %d (%s): operands z[%d:%lld] and z[%d:%lld] overlap at different "
                        "offsets", k, nm, a, (long long)(a + la), b, (long long)(b + lb));
    }
    def_len[dst] = (int32_t)dst_len;
    cursor += dst_len;
    if (!predictive && k == p.num_ops - 1 && dst_len != 1)
      return nmx_fail(NMX_ERR_INVALID, "op %d (%s): the last op must define one slot (U), not %d", k, nm, n);
  }
  if (cursor != p.num_slots)
    return nmx_fail(NMX_ERR_INVALID, "program defines %lld slots, num_slots is %d", (long long)cursor, p.num_slots);
  if (num_outputs < 0 || (num_outputs > 0 && !outputs)) return nmx_fail(NMX_ERR_INVALID, "bad output list");
  for (int j = 0; j < num_outputs; ++j) {
    const int64_t slot = outputs[2 * j], n = outputs[2 * j + 1];
    bool ok = n > 0 && slot >= 0 && slot + n <= p.num_slots;
    if (ok && slot < p.dim) ok = slot + n <= p.dim;
    // inside one defined value: walk back to the value's first slot
    if (ok && slot >= p.dim) {
      int64_t first = slot;
      while (def_len[first] == 0) --first;  // slot p.dim starts a value (checked above)
      ok = slot + n <= first + def_len[first];
    }
    if (!ok)
      return nmx_fail(NMX_ERR_INVALID, "output %d: slots [%lld, %lld) are not a given site or inside one defined "
                      "value (%d slots, dim %d)", j, (long long)slot, (long long)(slot + n), p.num_slots, p.dim);
  }
  return NMX_OK;
}

extern "C" int nmx_program_check(const nmx_program* hp) { return nmx_program_check_impl(hp, false, nullptr, 0); }

extern "C" size_t nmx_pe_program_workspace_bytes(int num_slots, int ldc) {
  if (num_slots <= 0 || ldc <= 0) return 0;
  return (size_t)ldc * 2 * (size_t)num_slots * sizeof(float);
}

extern "C" int nmx_pe_program(const nmx_program* program, const nmx_eval_batch* ev, void* workspace, void* stream) {
  if (!ev || !ev->z || !ev->grad || !ev->pe) return nmx_fail(NMX_ERR_INVALID, "eval batch has NULL pointers");
  if (ev->num_chains <= 0 || ev->ldc < ev->num_chains)
    return nmx_fail(NMX_ERR_INVALID, "bad num_chains/ldc (%d/%d)", ev->num_chains, ev->ldc);
  if (!program || !program->ops || !program->consts || !workspace || program->num_ops <= 0 || program->dim <= 0 ||
      program->num_slots <= program->dim || (program->num_index > 0 && !program->index))
    return nmx_fail(NMX_ERR_INVALID, "bad program or workspace");
  hipLaunchKernelGGL(k_program, dim3(ev->num_chains), dim3(64), 0, (hipStream_t)stream,
                     NmxProgram{*program, (float*)workspace}, *ev);
  return nmx_check_launch("k_program");
}
