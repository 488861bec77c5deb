"""Program compiler: the generic device path of the model front end.

The reference turns any model into ``potential_fn`` by running its effect handlers
(numpyro/infer/util.py:546-611 potential_fn_gen / get_potential_fn) and differentiates it with
JAX.  Here ``compile_model`` traces the model once (frontend.trace_model), expands every site's
``log_prob`` into primitive operations and lowers U(z) = -log p(z) - log|J|(z) to a
straight-line *program* over f32 vectors (include/numpyro_amd.h "program potential"): a flat
int32 op array, a constant pool and an index pool.  One HIP kernel (csrc/potential_program.hip)
evaluates the program and its reverse-mode adjoint for every evaluated chain in one launch,
behind the ``Potential.evaluate`` contract, so dense mass, HMC / NUTS, sharding, diagnostics
and deterministic sites work as for the fused kernels.

The kernel knows nothing about distributions: a new distribution is a ``_LOGPROB`` entry here.
Host passes: subexpressions without a latent are folded in float64 into the constant pool
(every normalising constant ends there), common subexpressions are shared (a ``Sym`` used twice
is one value), ``log(exp(x))`` is ``x``, ``log1p(-x)`` of a unit-interval site's own value is
``-softplus(u)``.  ``Program.run_host`` is a float64 NumPy interpreter
of the same program, forward and reverse: it defines the kernel's semantics op by op.  Its forward
pass, ``Program._forward_host``, is the one forward interpreter of every program kind: the
predictive and log-likelihood programs (``_ForwardProgram``) run it in float64 and float32.

Model class: latent sites of rank 0 or 1 with support ``real``, ``positive`` (the kernel
sees u = log x and the program adds -sum(u), as NmxEightSchools does), ``unit_interval`` /
``interval`` (x = lo + width sigmoid(u), built from -softplus(-u) and -softplus(u)) or
``greater_than`` (x = lo + exp(u)), with constant bounds, from Normal, StudentT, Cauchy,
HalfCauchy, HalfNormal, LogNormal, Exponential, Gamma, Uniform, Beta, Pareto, and one Dirichlet
vector per site (``simplex``: K - 1 unconstrained coordinates, stick breaking built in log space
from the cumsum and concat ops); observed sites from those plus BernoulliLogits / BernoulliProbs /
Poisson / BinomialLogits / BinomialProbs (with a total_count that is data), the count likelihoods of
``_COUNT_LOGPROB`` (GammaPoisson, NegativeBinomialProbs / Logits, NegativeBinomial2, BetaBinomial,
GeometricProbs / Logits, ZeroInflatedProbs / Logits over any of these: every parameter constant or
symbolic, their lgamma(c + y) - lgamma(c) through the lrising op, zero inflation through logaddexp:
include/numpyro_amd.h nmx_special_opcode), CategoricalProbs /
CategoricalLogits (a parameter of rank 1) and MixtureSameFamily of a Categorical with univariate
continuous components (the N x K table through a row-wise logsumexp); MultivariateNormal as an
observed site (loc constant or symbolic) or as one latent vector (loc constant), its
covariance_matrix or scale_tril constant or symbolic, n <= 128: -0.5 |L^-1 (x - loc)|^2 -
sum(log diag L) - n/2 log 2 pi from the cholesky and trisolve ops (include/numpyro_amd.h), a
constant covariance factorised here and applied through matvec; parameters that are constants or
expressions of latents over numpyro_amd.jnp's operations.  Values of rank 2 (a kernel matrix built
from latents) are flat row-major values: elementwise operations between equal shapes and with
scalars are the ops unchanged, any other NumPy-broadcastable pair gathers the smaller operand;
reductions, indexing and products of rank-2 values, latents of rank 2, rank > 2, a symbolic
precision_matrix, and batched or plated MultivariateNormal sites are refused.  Anything else raises
NotImplementedError naming the site.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import distributions as dist
from . import native
from .frontend import _base, _host, _with_traced_deterministics, trace_model
from .jnp import Sym
from .native import OPCODE
from .potentials import LOWER, POSITIVE, REAL, SIMPLEX, UNIT, Potential

_UNARY = ("neg", "exp", "log", "sqrt", "tanh", "log1p", "square", "softplus", "lgamma")
_BINARY = ("add", "sub", "mul", "div", "pow")
# the special ops (native.SPECIAL_OPCODES): elementwise and binary like _BINARY, with functions of their own
_SPECIAL = ("lrising", "logaddexp")
_TWO_OPERAND = _BINARY + _SPECIAL  # every elementwise op of two operands


_DRAW_NAME = {v: k for k, v in native.DRAW_OPCODE.items()}


def _lgamma(x, dtype=np.float64):
    import torch

    return torch.lgamma(torch.as_tensor(np.require(x, dtype, "C"))).numpy()


def _digamma(x):
    """digamma in the dtype of x (float64, or float32 for the float32 restatement)."""
    import torch

    x = np.asarray(x)
    return torch.special.digamma(torch.as_tensor(np.require(x, x.dtype if x.dtype == np.float32 else np.float64,
                                                            "C"))).numpy()


# ---- the special ops, written once for float64 and float32 with the kernel's algorithm
# (csrc/nmx_program.h nmx_lrising / nmx_lrising_da, include/numpyro_amd.h NMX_OP_LRISING)
def _log1pmx(t, T):
    """log1p(t) - t, t >= 0: the atanh series below 1/2 (nmx_log1pmx)."""
    s = t / (T(2.0) + t)
    s2 = s * s
    odd = T(1 / 15) + s2 * T(1 / 17)
    for d in (13, 11, 9, 7, 5, 3):
        odd = T(1 / d) + s2 * odd
    return np.where(t < T(0.5), s * (T(2.0) * s2 * odd - t), np.log1p(t) - t)


def _stirling_s(x, T):
    r = T(1.0) / x
    r2 = r * r
    return (T(1 / 12) - (T(1 / 360) - (T(1 / 1260) - T(1 / 1680) * r2) * r2) * r2) * r


def _stirling_ds(x, T):
    r = T(1.0) / x
    r2 = r * r
    return -r2 * (T(1 / 12) - r2 * (T(1 / 120) - r2 * (T(1 / 252) - r2 * T(1 / 240))))


def _host_lrising(a, k, derivative=False):
    """R(a, k) = lgamma(a + k) - lgamma(a) - k log(a), or dR/da = digamma(a + k) - digamma(a) - k / a,
    in the dtype of the operands: whole k <= LRISING_SUM_MAX by sums over j < k, otherwise a shifted
    up to x >= 8 and the Stirling difference through log1p(k / x) - k / x; NaN unless a > 0, k >= 0."""
    a, k = np.broadcast_arrays(np.asarray(a), np.asarray(k))
    T = np.result_type(a, k).type
    a, k = a.astype(T), k.astype(T)
    by_sum = (k <= T(native.LRISING_SUM_MAX)) & (k == np.floor(k))
    total = np.zeros(a.shape, T)
    for j in range(1, native.LRISING_SUM_MAX):
        term = T(j) / (a * (a + T(j))) if derivative else np.log1p(T(j) / a)
        total = total + np.where(T(j) < k, term, T(0.0))
    x, shift, m = a.copy(), np.zeros(a.shape, T), np.zeros(a.shape, T)
    for _ in range(8):
        low = x < T(8.0)
        term = k / (x * (x + k)) if derivative else np.log1p(k / x)
        shift = shift + np.where(low, term, T(0.0))
        x = np.where(low, x + T(1.0), x)
        m = m + np.where(low, T(1.0), T(0.0))
    t = k / x
    if derivative:
        body = _log1pmx(t, T) + T(0.5) * k / (x * (x + k)) + (_stirling_ds(x + k, T) - _stirling_ds(x, T))
        out = np.where(by_sum, -total, body + (shift - k * m / (a * x)))
    else:
        body = x * _log1pmx(t, T) + (k - T(0.5)) * np.log1p(t) + (_stirling_s(x + k, T) - _stirling_s(x, T))
        out = np.where(by_sum, total, body + (k * np.log1p(m / a) - shift))
    return np.where((a > 0) & (k >= 0), out, T(np.nan))


def _host_logaddexp(x, y):
    """max + log1p(exp(-|x - y|)), the gap 0 where x == y (two -inf give -inf)."""
    x, y = np.broadcast_arrays(np.asarray(x), np.asarray(y))
    T = np.result_type(x, y).type
    with np.errstate(invalid="ignore"):  # inf - inf where x == y, not taken
        gap = np.where(x == y, T(0.0), -np.abs(x - y))
    return (np.maximum(x, y) + np.log1p(np.exp(gap))).astype(T)


_HOST_FWD = {
    "neg": lambda x: -x, "exp": np.exp, "log": np.log, "sqrt": np.sqrt, "tanh": np.tanh, "log1p": np.log1p,
    "square": np.square, "softplus": lambda x: np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x))),
    "lgamma": _lgamma,
    "add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide, "pow": np.power,
    "lrising": _host_lrising, "logaddexp": _host_logaddexp,
}


def _host_rev(op, gd, x, y, out):
    """(adjoint of a, adjoint of b) of one elementwise op, as the kernel's NmxProgram::rev."""
    if op == "neg":
        return -gd, None
    if op == "exp":
        return gd * out, None
    if op == "log":
        return gd / x, None
    if op == "sqrt":
        return gd * 0.5 / out, None
    if op == "tanh":
        return gd * (1.0 - out * out), None
    if op == "log1p":
        return gd / (1.0 + x), None
    if op == "square":
        return gd * (2.0 * x), None
    if op == "softplus":
        return gd / (1.0 + np.exp(-x)), None
    if op == "lgamma":
        return gd * _digamma(x), None
    if op == "lrising":
        return gd * _host_lrising(x, y, derivative=True), None
    if op == "logaddexp":
        dead = out == -np.inf
        with np.errstate(invalid="ignore"):  # -inf - -inf where the result is dead, not taken
            return np.where(dead, 0 * gd, gd * np.exp(x - out)), np.where(dead, 0 * gd, gd * np.exp(y - out))
    if op == "add":
        return gd, gd
    if op == "sub":
        return gd, -gd
    if op == "mul":
        return gd * y, gd * x
    if op == "div":
        return gd / y, -(gd * out) / y
    return gd * (y * np.power(x, y - 1.0)), gd * (out * np.log(x))  # pow


def _operand(v, cp, ref, n, stride):
    """An elementwise op's operand: n tape slots (one where the stride is 0) or constants (ref < 0)."""
    ln = n if stride else 1
    return v[:, ref:ref + ln] if ref >= 0 else cp[None, ~ref:~ref + ln]


def _host_logsumexp(x):
    """Row-wise over the last axis, as the kernel: max + log sum exp(x - max), the max replaced by
    0 where it is not finite (jax.scipy.special.logsumexp's rule: a row of -inf gives -inf)."""
    m = x.max(-1)
    m = np.where(np.isfinite(m), m, x.dtype.type(0.0))
    return np.log(np.exp(x - m[..., None]).sum(-1)) + m


def _host_scan_fwd(nm, v, cp, dst, a, b, n, aux):
    """Forward of cumsum / logsumexp / concat on the value table v [C, S] (any float dtype)."""
    C = v.shape[0]
    if nm == "cumsum":
        v[:, dst:dst + n] = np.cumsum(v[:, a:a + n], 1)
    elif nm == "logsumexp":
        v[:, dst:dst + n] = _host_logsumexp(v[:, a:a + n * aux].reshape(C, n, aux))
    else:  # concat
        v[:, dst:dst + aux] = v[:, a:a + aux] if a >= 0 else cp[None, ~a:~a + aux]
        v[:, dst + aux:dst + n] = v[:, b:b + n - aux] if b >= 0 else cp[None, ~b:~b + n - aux]


def _host_scan_rev(nm, v, g, dst, a, b, n, aux):
    """Reverse of cumsum / logsumexp / concat: the operands' adjoints in g [C, S]."""
    C = v.shape[0]
    gd = g[:, dst:dst + n]
    if nm == "cumsum":  # the suffix sums
        g[:, a:a + n] += np.cumsum(gd[:, ::-1], 1)[:, ::-1]
    elif nm == "logsumexp":
        x, out = v[:, a:a + n * aux].reshape(C, n, aux), v[:, dst:dst + n]
        w = np.where(out[..., None] == -np.inf, x.dtype.type(0.0), np.exp(x - out[..., None]))
        g[:, a:a + n * aux] += (gd[..., None] * w).reshape(C, n * aux)
    else:
        if a >= 0:
            g[:, a:a + aux] += gd[:, :aux]
        if b >= 0:
            g[:, b:b + n - aux] += gd[:, aux:]


_SCAN = ("cumsum", "logsumexp", "concat")
_LINALG = ("cholesky", "trisolve")


def _host_cholesky(A):
    """Lower Cholesky factors of A [C, n, n] (its lower triangle), column by column as the kernel:
    L[i][j] = (A[i][j] - sum_{k < j} L[i][k] L[j][k]) / L[j][j]; a pivot that is not positive and
    finite is NaN, and so is everything computed from it."""
    n = A.shape[-1]
    L = np.zeros_like(A)
    for j in range(n):
        s = A[:, j:, j] - np.einsum("cik,ck->ci", L[:, j:, :j], L[:, j, :j])
        piv = s[:, 0]
        ok = (piv > 0) & np.isfinite(piv)
        d = np.where(ok, np.sqrt(np.where(ok, piv, 1)), np.nan).astype(A.dtype)
        L[:, j:, j] = s / d[:, None]
        L[:, j, j] = d
    return L


def _host_cholesky_rev(L, Lbar):
    """Adjoint of A from the adjoint of L = chol(A) [C, n, n]: (P + P^T) / 2 with
    P = L^-T Phi(L^T Lbar) L^-1, by the unblocked reverse sweep of Murray (2016), "Differentiation of
    the Cholesky decomposition", without its last halving of the diagonal: M = tril(P + P^T)."""
    n = L.shape[-1]
    M = np.tril(Lbar).copy()
    for j in range(n - 1, -1, -1):
        d = L[:, j, j]
        cb = M[:, j + 1:, j]
        db = (M[:, j, j] - (L[:, j + 1:, j] * cb).sum(1) / d) / d
        cb = cb / d[:, None]
        M[:, j + 1:, j] = cb
        M[:, j, :j] -= db[:, None] * L[:, j, :j] + np.einsum("ci,cik->ck", cb, L[:, j + 1:, :j])
        M[:, j + 1:, :j] -= cb[:, :, None] * L[:, j, None, :j]
        M[:, j, j] = db
    return 0.5 * (M + np.swapaxes(np.tril(M, -1), 1, 2))


def _host_trisolve(L, b, transpose=False):
    """L^-1 b (or L^-T b) for L [C or 1, n, n] lower triangular and b [C or 1, n], by columns."""
    n = L.shape[-1]
    y = np.broadcast_to(b, (max(L.shape[0], b.shape[0]), n)).copy()
    for k in (range(n - 1, -1, -1) if transpose else range(n)):
        y[:, k] = y[:, k] / L[:, k, k]
        if transpose:
            y[:, :k] -= L[:, k, :k] * y[:, k:k + 1]
        else:
            y[:, k + 1:] -= L[:, k + 1:, k] * y[:, k:k + 1]
    return y


def _host_linalg_operands(v, cp, a, b, n):
    """(L [C or 1, n, n], rhs [C or 1, n]) of a trisolve."""
    L = v[:, a:a + n * n] if a >= 0 else cp[None, ~a:~a + n * n]
    rhs = v[:, b:b + n] if b >= 0 else cp[None, ~b:~b + n]
    return L.reshape(-1, n, n), rhs


def _host_linalg_fwd(nm, v, cp, dst, a, b, n, aux):
    """Forward of cholesky / trisolve on the value table v [C, S] (any float dtype)."""
    C = v.shape[0]
    if nm == "cholesky":
        v[:, dst:dst + n] = _host_cholesky(v[:, a:a + n].reshape(C, aux, aux)).reshape(C, n)
    else:
        v[:, dst:dst + n] = _host_trisolve(*_host_linalg_operands(v, cp, a, b, n))


def _host_linalg_rev(nm, v, g, cp, dst, a, b, n, aux):
    """Reverse of cholesky / trisolve: the operands' adjoints in g [C, S]."""
    C = v.shape[0]
    if nm == "cholesky":
        g[:, a:a + n] += _host_cholesky_rev(v[:, dst:dst + n].reshape(C, aux, aux),
                                            g[:, dst:dst + n].reshape(C, aux, aux)).reshape(C, n)
        return
    L, _ = _host_linalg_operands(v, cp, a, b, n)
    w = _host_trisolve(L, g[:, dst:dst + n], transpose=True)
    if b >= 0:
        g[:, b:b + n] += w
    if a >= 0:
        g[:, a:a + n * n] -= np.tril(w[:, :, None] * v[:, None, dst:dst + n]).reshape(C, n * n)


class Program:
    """A lowered model: ``ops`` int32 [num_ops, 8] = (opcode, dst, a, b, n, sa, sb, aux),
    ``consts`` (float64 here, float32 on the device), ``index`` int32; slots [0, dim) are z."""

    def __init__(self, ops, consts, index, num_slots, dim):
        self.ops = np.ascontiguousarray(np.asarray(ops, np.int32).reshape(-1, native.OP_WORDS))
        self.consts64 = np.ascontiguousarray(np.asarray(consts, np.float64).reshape(-1))
        if self.consts64.size == 0:
            self.consts64 = np.zeros(1)
        with np.errstate(over="ignore"):
            self.consts = np.ascontiguousarray(self.consts64.astype(np.float32))
        self.index = np.ascontiguousarray(np.asarray(index, np.int32).reshape(-1))
        self.num_slots, self.dim = int(num_slots), int(dim)
        # the host interpreters read M alone; the kernel's per-lane forward and wave-per-row reverse
        # read the transposed copy behind it.  A pool whose halves disagree is refused once, here
        # (a pool reference out of range is nmx_program_check's to name)
        for k, (op, dst, a, b, n, sa, sb, aux) in enumerate(self.ops.tolist()):
            if op == OPCODE["matvec"] and b < 0 and n > 0 and aux > 0 and ~b + 2 * n * aux <= self.consts64.size:
                M = self.consts64[~b:~b + n * aux].reshape(n, aux)
                Mt = self.consts64[~b + n * aux:~b + 2 * n * aux].reshape(aux, n)
                if not np.array_equal(M.T, Mt, equal_nan=True):
                    raise ValueError(f"op {k} (matvec): the second half of its constant pool is not the transpose "
                                     f"of the {n} x {aux} matrix in the first half")

    @property
    def num_ops(self):
        return self.ops.shape[0]

    def native_struct(self, ops=None, consts=None, index=None):
        """nmx_program over the given arrays' pointers (default: this program's host arrays)."""
        def p(a):
            return None if a is None or a.size == 0 else int(a.ctypes.data)

        ops = self.ops if ops is None else ops
        consts = self.consts if consts is None else consts
        index = self.index if index is None else index
        return native.Program(ops=p(ops), consts=p(consts), index=p(index), num_ops=ops.shape[0],
                              num_slots=self.num_slots, num_consts=consts.size, num_index=index.size, dim=self.dim)

    _CHECK = "nmx_program_check"  # the library's check of this kind of program

    def native_check(self, *extra):
        """(status, message) of the kind's check (``_CHECK``) on the host arrays: needs no GPU."""
        lib = native.lib()
        st = getattr(lib, self._CHECK)(ctypes.byref(self.native_struct()), *extra)
        return st, (lib.nmx_last_error().decode(errors="replace") if st else "")

    def upload(self, device):
        """This program checked and on ``device``: a _DeviceProgram."""
        return _DeviceProgram(self, device)

    def op_names(self):
        return [_DRAW_NAME[o] if o >= native.DRAW_BASE else native.op_name(o) for o in self.ops[:, 0].tolist()]

    def describe(self):
        return [f"{k}: {nm} dst={o[1]} a={o[2]} b={o[3]} n={o[4]} sa={o[5]} sb={o[6]} aux={o[7]}"
                for k, (nm, o) in enumerate(zip(self.op_names(), self.ops.tolist()))]

    # ------------------------------------------------------------------ NumPy interpreter
    def _forward_host(self, Z, dtype, cp, draw=None):
        """The tape v [rows, num_slots] of the rows of Z [rows, dim]: every op forward in ``dtype``
        arithmetic over the constant pool ``cp``, op by op as the kernels run it (only the order inside
        sums differs).  ``draw(name, op words, v)`` fills a draw op's slots (predictive programs).  The
        one forward interpreter of the three program kinds: an op it does not know is an error."""
        assert Z.shape[1] == self.dim
        v = np.zeros((Z.shape[0], self.num_slots), dtype)
        v[:, :self.dim] = Z
        ix = self.index
        fwd = dict(_HOST_FWD, lgamma=lambda x: _lgamma(x, dtype))
        with np.errstate(all="ignore"):
            for o, nm in zip(self.ops.tolist(), self.op_names()):
                op, dst, a, b, n, sa, sb, aux = o
                if nm in _UNARY:
                    v[:, dst:dst + n] = fwd[nm](_operand(v, cp, a, n, sa))
                elif nm in _TWO_OPERAND:
                    v[:, dst:dst + n] = fwd[nm](_operand(v, cp, a, n, sa), _operand(v, cp, b, n, sb))
                elif nm == "reduce_sum":
                    v[:, dst] = v[:, a:a + n].sum(1)
                elif nm == "gather":
                    v[:, dst:dst + n] = v[:, a + ix[aux:aux + n]]
                elif nm == "matvec":
                    M = cp[~b:~b + n * aux].reshape(n, aux)
                    v[:, dst:dst + n] = v[:, a:a + aux] @ M.T
                elif nm in _LINALG:
                    _host_linalg_fwd(nm, v, cp, dst, a, b, n, aux)
                elif nm in _SCAN:
                    _host_scan_fwd(nm, v, cp, dst, a, b, n, aux)
                else:
                    assert op >= native.DRAW_BASE and draw is not None, nm
                    draw(nm, o, v)
        return v

    def run_host(self, Z, f32_consts=False, dtype=np.float64):
        """(U [C], dU/dz [C, D]) of the rows of Z [C, D], in float64: the program forward
        (_forward_host) and reverse, op by op as the kernel runs it.
        ``f32_consts``: with the constant pool rounded to float32, as the device holds it.
        ``dtype=np.float32``: the float32 restatement, every value, adjoint, constant and operation
        in float32 (returned as float64): what float32 arithmetic alone costs."""
        dtype = np.dtype(dtype).type
        Z = np.atleast_2d(np.asarray(Z, dtype))
        C, S, D = Z.shape[0], self.num_slots, self.dim
        if dtype is np.float32:
            cp = self.consts
        else:
            cp = self.consts.astype(np.float64) if f32_consts else self.consts64
        ix = self.index
        v = self._forward_host(Z, dtype, cp)
        g = np.zeros((C, S), dtype)
        g[:, S - 1] = 1.0
        with np.errstate(all="ignore"):
            for op, dst, a, b, n, sa, sb, aux in reversed(self.ops.tolist()):
                nm = native.op_name(op)
                gd = g[:, dst:dst + (1 if nm == "reduce_sum" else n)]
                if nm in _UNARY or nm in _TWO_OPERAND:
                    x = _operand(v, cp, a, n, sa)
                    y = _operand(v, cp, b, n, sb) if nm in _TWO_OPERAND else None
                    da, db = _host_rev(nm, gd, x, y, v[:, dst:dst + n])
                    for ref, stride, d in ((a, sa, da), (b, sb, db)):
                        if d is None or ref < 0:
                            continue
                        d = np.broadcast_to(d, (C, n))
                        if stride:
                            g[:, ref:ref + n] += d
                        else:
                            g[:, ref] += d.sum(1)
                elif nm == "reduce_sum":
                    g[:, a:a + n] += gd
                elif nm == "gather":
                    np.add.at(g, (slice(None), a + ix[aux:aux + n]), gd)
                elif nm == "matvec":
                    M = cp[~b:~b + n * aux].reshape(n, aux)
                    g[:, a:a + aux] += gd @ M
                elif nm in _LINALG:
                    _host_linalg_rev(nm, v, g, cp, dst, a, b, n, aux)
                else:
                    _host_scan_rev(nm, v, g, dst, a, b, n, aux)
        return v[:, S - 1].astype(np.float64), g[:, :D].astype(np.float64)

    # ------------------------------------------------------------------ cost model
    def flops_per_eval(self, num_chains=1):
        """Arithmetic operations of one evaluation, forward + reverse (a transcendental counts 1)."""
        f = 0.0
        for op, dst, a, b, n, sa, sb, aux in self.ops.tolist():
            nm = native.op_name(op)
            if nm == "logsumexp":  # per element: max, subtract, exp, add; and subtract, exp, multiply, add
                f += 8.0 * n * aux
            elif nm == "cholesky":  # aux^3 / 3 forward, twice that in the reverse sweep
                f += float(aux) ** 3
            elif nm == "trisolve":  # n^2 forward, n^2 back substitution, n^2 for the factor's adjoint
                f += 3.0 * n * n
            elif nm == "concat":  # moves only
                continue
            else:
                f += 4.0 * n * aux if nm == "matvec" else 2.0 * n if nm in ("reduce_sum", "gather", "cumsum") else 4.0 * n
        return f * num_chains

    def bytes_per_eval(self):
        """Bytes one chain evaluation moves through its tape (values and adjoints, f32): the
        adjoints' zero fill, each op's operand reads and result write forward, and backward the
        result's adjoint, the operands and the read-modify-write of the operands' adjoints.
        Constants and indices are shared by all chains and stay cached."""
        el = self.num_slots + 2 * self.dim  # zero fill, z in, grad out
        for op, dst, a, b, n, sa, sb, aux in self.ops.tolist():
            nm = native.op_name(op)
            if nm == "matvec":
                src = [aux]
            elif nm == "trisolve":
                src = [ln for r, ln in ((a, n * n), (b, n)) if r >= 0]
            elif nm == "gather":
                src = [n]
            elif nm in ("reduce_sum", "cumsum", "cholesky"):
                src = [n]
            elif nm == "logsumexp":
                src = [n * aux]
            elif nm == "concat":
                src = [ln for r, ln in ((a, aux), (b, n - aux)) if r >= 0]
            else:
                src = [(n if s else 1) for r, s in ((a, sa), (b, sb) if nm in _TWO_OPERAND else (-1, 0)) if r >= 0]
            nd = 1 if nm == "reduce_sum" else n
            el += sum(src) + nd  # forward
            el += nd + sum(src) + nd + 2 * sum(src)  # reverse: adjoint in, operands, result, adjoints +=
        return 4 * el


class _DeviceProgram:
    """A program's arrays on a device and the nmx_program over them (``struct``).  A malformed program
    never reaches the device; the tensors live as long as this object, so keep it while the struct's
    pointers are in use."""

    def __init__(self, prog, device):
        import torch

        st, msg = prog.native_check()
        if st:
            raise native.NativeError(f"{prog._CHECK} failed (status {st}): {msg}")
        self.d_ops = torch.from_numpy(prog.ops).to(device)
        self.d_consts = torch.from_numpy(prog.consts).to(device)
        self.d_index = torch.from_numpy(prog.index).to(device) if prog.index.size else None
        self.struct = native.Program(ops=native.ptr(self.d_ops), consts=native.ptr(self.d_consts),
                                     index=native.ptr(self.d_index), num_ops=prog.num_ops, num_slots=prog.num_slots,
                                     num_consts=prog.consts.size, num_index=prog.index.size, dim=prog.dim)


class _ForwardProgram(Program):
    """A forward-only program run once per sample (predictive_program.py, loglik_program.py): slots
    [0, dim) hold the given sites, ``inputs``: (name, offset, n, shape) in sorted name order,
    constrained values; ``outputs`` name tape slots (each kind has its own output_table)."""

    def __init__(self, ops, consts, index, num_slots, dim, inputs, outputs):
        super().__init__(ops, consts, index, num_slots, dim)
        self.inputs, self.outputs = list(inputs), list(outputs)

    @classmethod
    def empty(cls, dim, inputs, *rest):
        """The program with nothing to run on the device (no op, no output)."""
        return cls(np.zeros((0, native.OP_WORDS)), [], [], dim, dim, inputs, [], *rest)

    def native_check(self, outputs=None, *extra):
        """(status, message) of the kind's check on the host arrays and an output table (default:
        this program's): needs no GPU."""
        table = self.output_table() if outputs is None else np.ascontiguousarray(np.asarray(outputs, np.int32))
        return super().native_check(int(table.ctypes.data) if table.size else None, table.shape[0], *extra)

    def flatten_inputs(self, samples, dtype=np.float64):
        """[S, dim] from a dict name -> [S, *site shape] (or an array [S, dim], or S when dim = 0)."""
        if isinstance(samples, (int, np.integer)):
            assert self.dim == 0, "a sample count alone needs a program without given sites"
            return np.zeros((int(samples), 0), dtype)
        if isinstance(samples, dict):
            S = len(next(iter(samples.values())))
            cols = [np.asarray(samples[name], dtype).reshape(S, n) for name, _, n, _ in self.inputs]
            return np.concatenate(cols, 1) if cols else np.zeros((S, 0), dtype)
        return np.atleast_2d(np.asarray(samples, dtype))

    def _pool(self, dtype):
        """The constant pool of run_host in ``dtype``: the float64 one, else the device's float32 one."""
        return self.consts64 if np.dtype(dtype) == np.float64 else self.consts.astype(dtype)

    # ------------------------------------------------------------------ device
    def sample_device(self, flat, what):
        """The device this program runs on for the samples ``flat`` {site: [S, *shape]}, whose
        shapes per draw must be the model's: the current GPU; the CPU for a program without ops."""
        import torch

        for name, _, n, shape in self.inputs:
            if tuple(flat[name].shape[1:]) != tuple(shape):
                raise ValueError(f"posterior samples of site {name!r} have shape {tuple(flat[name].shape[1:])} per "
                                 f"draw, the model's site has {tuple(shape)}")
        if torch.cuda.is_available():
            return torch.device("cuda", torch.cuda.current_device())
        if self.num_ops:
            raise RuntimeError(f"{what} needs a GPU (the program runs on a HIP kernel)")
        return torch.device("cpu")

    def bind_samples(self, flat, S, device, max_bytes, what, limit):
        """(the uploaded program, x [S, dim] float32 of the samples ``flat`` or None without inputs,
        the samples per launch, their tape [chunk, num_slots]) on ``device``, the tape under
        ``max_bytes``; the refusal names the caller ``what`` and its ``limit``."""
        import torch

        bound = self.upload(device)
        x = (torch.cat([flat[name].to(device, torch.float32).reshape(S, n) for name, _, n, _ in self.inputs], 1)
             .contiguous() if self.inputs else None)
        row_bytes = native.lib().nmx_predict_program_workspace_bytes(self.num_slots, 1)
        chunk = min(S, max_bytes // row_bytes)
        if chunk <= 0:
            raise NotImplementedError(f"{what}: one sample's tape of {self.num_slots} slots needs {row_bytes} bytes, "
                                      f"above {limit} = {max_bytes}")
        return bound, x, chunk, torch.empty(chunk, self.num_slots, dtype=torch.float32, device=device)


# ------------------------------------------------------------------------------------------
# Builder: values, folding, sharing
# ------------------------------------------------------------------------------------------
class _V:
    """Compile-time value of n elements: a float64 constant (``c``) or program slots (``slot``)."""

    __slots__ = ("b", "n", "c", "slot")

    def __init__(self, b, n, c=None, slot=None):
        self.b, self.n, self.c, self.slot = b, int(n), c, slot

    @property
    def is_const(self):
        return self.c is not None

    def __add__(self, o): return self.b.ew("add", self, o)
    def __radd__(self, o): return self.b.ew("add", o, self)
    def __sub__(self, o): return self.b.ew("sub", self, o)
    def __rsub__(self, o): return self.b.ew("sub", o, self)
    def __mul__(self, o): return self.b.ew("mul", self, o)
    def __rmul__(self, o): return self.b.ew("mul", o, self)
    def __truediv__(self, o): return self.b.ew("div", self, o)
    def __rtruediv__(self, o): return self.b.ew("div", o, self)
    def __pow__(self, o): return self.b.ew("pow", self, o)
    def __neg__(self): return self.b.ew("neg", self)


class _Builder:
    def __init__(self, dim):
        self.dim = dim
        self.ops, self.consts, self.index = [], [], []
        self.n_consts = 0
        self.next_slot = dim
        self.memo = {}  # (op, operand keys) -> value: common subexpressions
        self.pool = {}  # constant bytes -> pool offset
        self.made_by = {}  # slot -> (op name, operand value) for the log(exp(x)) rewrite
        self.log1m = {}  # slot of a unit site's value x -> log(1 - x), for the log1p(-x) rewrite
        self.n_draws = 0  # draw ops of a predictive program (predictive_program.py)

    def const(self, x):
        if isinstance(x, _V):
            return x
        a = np.asarray(x, np.float64)
        if a.ndim > 1:
            raise NotImplementedError("a constant of rank > 1 is only supported as the matrix of a matmul")
        return _V(self, max(a.size, 1), c=a.reshape(-1).copy())

    def _pool(self, arr):
        arr = np.asarray(arr, np.float64).reshape(-1)
        key = arr.tobytes()
        if key not in self.pool:
            self.pool[key] = self.n_consts
            self.consts.append(arr)
            self.n_consts += arr.size
        return self.pool[key]

    def _ref(self, v):
        return v.slot if not v.is_const else ~self._pool(v.c)

    def _emit(self, name, n_dst, a, b, n, sa, sb, aux, key):
        if key in self.memo:
            return self.memo[key]
        dst = self.next_slot
        self.next_slot += n_dst
        self.ops.append([OPCODE[name] if name in OPCODE else native.DRAW_OPCODE[name], dst, a, b, n, sa, sb, aux])
        out = _V(self, n_dst, slot=dst)
        self.memo[key] = out
        return out

    def ew(self, name, a, b=None):
        a = self.const(a)
        b = None if b is None else self.const(b)
        if a.is_const and (b is None or b.is_const):
            with np.errstate(all="ignore"):
                return self.const(_HOST_FWD[name](a.c) if b is None else _HOST_FWD[name](a.c, b.c))
        n = a.n if b is None else max(a.n, b.n)
        for v in (a, b):
            if v is not None and v.n not in (1, n):
                raise NotImplementedError(f"operands of {v.n} and {n} elements do not broadcast")
        # identities with constants (Normal(0, 1) has loc 0 and scale 1)
        if b is not None and b.is_const and a.n == n:
            if (name in ("add", "sub") and np.all(b.c == 0.0)) or (name in ("mul", "div", "pow") and np.all(b.c == 1.0)):
                return a
        if b is not None and a.is_const and b.n == n:
            if (name == "add" and np.all(a.c == 0.0)) or (name == "mul" and np.all(a.c == 1.0)):
                return b
        if name == "log" and self.made_by.get(a.slot, ("",))[0] == "exp":
            return self.made_by[a.slot][1]
        # log1p(-x) of a unit site's own value x = sigmoid(u) is -softplus(u): the direct form is
        # -inf in float32 from u of about 17
        if name == "log1p" and self.made_by.get(a.slot, ("",))[0] == "neg" \
                and self.made_by[a.slot][1].slot in self.log1m:
            return self.log1m[self.made_by[a.slot][1].slot]
        # ... and 1 - x of it is sigmoid(-u) = exp(-softplus(u)): in float32 the subtraction is a
        # multiple of 2^-24, wrong by half from u of about 16 (Beta(m kappa, (1 - m) kappa))
        if name == "sub" and a.is_const and np.all(a.c == 1.0) and b.slot in self.log1m and b.n == n:
            return self.ew("exp", self.log1m[b.slot])
        # x + (-y) is x - y (log densities are written as sums of negated terms); the negation
        # left without a reader is dropped by program()
        if name == "add" and not b.is_const and self.made_by.get(b.slot, ("",))[0] == "neg":
            return self.ew("sub", a, self.made_by[b.slot][1])
        if name == "add" and not a.is_const and self.made_by.get(a.slot, ("",))[0] == "neg":
            return self.ew("sub", b, self.made_by[a.slot][1])
        ra, rb = self._ref(a), (0 if b is None else self._ref(b))
        sa, sb = int(a.n == n), int(b is not None and b.n == n)
        out = self._emit(name, n, ra, rb, n, sa, sb, 0, (name, ra, rb, n, sa, sb))
        self.made_by.setdefault(out.slot, (name, a))
        return out

    def rsum(self, a):
        a = self.const(a)
        if a.is_const:
            return self.const(a.c.sum())
        if a.n == 1:
            return a
        return self._emit("reduce_sum", 1, a.slot, 0, a.n, 1, 0, 0, ("reduce_sum", a.slot, a.n))

    def gather(self, a, idx):
        idx = np.asarray(idx, np.int64).reshape(-1)
        if a.is_const:
            return self.const(a.c[idx])
        if idx.size == a.n and np.array_equal(idx, np.arange(a.n)):
            return a
        key = ("gather", a.slot, idx.tobytes())
        if key in self.memo:
            return self.memo[key]
        # forward indices, then the transposed (CSR) index of the adjoint's segmented sum
        who = np.argsort(idx, kind="stable")
        start = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=a.n))])
        aux = len(self.index)
        self.index += idx.tolist() + start.tolist() + who.tolist()
        return self._emit("gather", idx.size, a.slot, a.n, idx.size, 1, 0, aux, key)

    def matvec(self, M, a):
        M = np.asarray(M, np.float64)
        if a.is_const:
            return self.const(M @ a.c)
        off = self._pool(np.concatenate([M.reshape(-1), M.T.reshape(-1)]))
        return self._emit("matvec", M.shape[0], a.slot, ~off, M.shape[0], 1, 0, M.shape[1], ("matvec", a.slot, off))

    def cumsum(self, a):
        a = self.const(a)
        if a.is_const:
            return self.const(np.cumsum(a.c))
        if a.n == 1:
            return a
        return self._emit("cumsum", a.n, a.slot, 0, a.n, 1, 0, 0, ("cumsum", a.slot, a.n))

    def logsumexp(self, a, rows, cols):
        """Row-wise over the flat row-major rows x cols value a: `rows` elements."""
        a = self.const(a)
        assert a.n == rows * cols and cols >= 1, (a.n, rows, cols)
        if a.is_const:
            with np.errstate(all="ignore"):
                return self.const(_host_logsumexp(a.c.reshape(rows, cols)))
        if cols == 1:
            return a
        return self._emit("logsumexp", rows, a.slot, 0, rows, 1, 0, cols, ("logsumexp", a.slot, rows, cols))

    def concat(self, a, b):
        a, b = self.const(a), self.const(b)
        if a.is_const and b.is_const:
            return self.const(np.concatenate([a.c, b.c]))
        ra, rb, n = self._ref(a), self._ref(b), a.n + b.n
        return self._emit("concat", n, ra, rb, n, 1, 1, a.n, ("concat", ra, rb, a.n, b.n))

    def cholesky(self, a, m):
        """The lower Cholesky factor of the flat row-major m x m value a: m * m elements."""
        a = self.const(a)
        assert a.n == m * m, (a.n, m)
        if a.is_const:
            return self.const(_const_cholesky(a.c.reshape(m, m)).reshape(-1))
        return self._emit("cholesky", m * m, a.slot, 0, m * m, 1, 0, m, ("cholesky", a.slot, m))

    def trisolve(self, L, b):
        """L^-1 b for the flat row-major n x n lower-triangular L and b of n elements."""
        L, b = self.const(L), self.const(b)
        n = b.n
        assert L.n == n * n, (L.n, n)
        if L.is_const and b.is_const:
            with np.errstate(all="ignore"):
                return self.const(_host_trisolve(L.c.reshape(1, n, n), b.c[None])[0])
        ra, rb = self._ref(L), self._ref(b)
        return self._emit("trisolve", n, ra, rb, n, 1, 1, 0, ("trisolve", ra, rb, n))

    def unary(self, name):
        return lambda x: self.ew(name, x)

    def lrising(self, a, k):
        """lgamma(a + k) - lgamma(a) - k log(a) of the data k (the lrising op; 0 where every k is 0)."""
        a, k = self.const(a), self.const(k)
        if not k.is_const:
            raise NotImplementedError("the step count of a log rising factorial depends on a latent site: it must be data")
        if not a.is_const and np.all(k.c == 0.0):
            return self.const(np.zeros(max(a.n, k.n)))
        return self.ew("lrising", a, k)

    def draw(self, name, n, a=None, b=None):
        """A draw op of n elements (predictive programs only): never shared, never folded.  The
        stream id is the draw's ordinal."""
        refs = []
        for par in (a, b):
            if par is None:
                refs += [0, 0]
                continue
            par = self.const(par)
            if par.n not in (1, n):
                raise NotImplementedError(f"a parameter of {par.n} elements at a site of {n}")
            refs += [self._ref(par), int(par.n == n)]
        stream = self.n_draws
        self.n_draws += 1
        return self._emit(name, n, refs[0], refs[2], n, refs[1], refs[3], stream, ("draw", stream))

    def program(self):
        """The ops the last one (U) depends on, renumbered so that each defines the next free slots."""
        return Program(*self.arrays([len(self.ops) - 1])[0])

    def arrays(self, roots):
        """((ops, consts, index, num_slots, dim), old slot -> new slot) of compact(roots): the
        leading arguments of a Program."""
        ops, moved, num_slots = self.compact(roots)
        consts = np.concatenate(self.consts) if self.consts else np.zeros(0)
        return (ops, consts, self.index, num_slots, self.dim), moved

    def forward_arrays(self, outputs):
        """The Program arguments of the ops that the output sites depend on; the outputs' slots are
        renumbered with the ops (an output that is a given site's own slots keeps them)."""
        made = {op[1]: k for k, op in enumerate(self.ops)}
        arrays, moved = self.arrays([made[o.slot] for o in outputs if o.slot >= self.dim])
        for o in outputs:
            o.slot = moved.get(o.slot, o.slot)
        return arrays

    def compact(self, roots):
        """(ops, old slot -> new slot, num_slots) of the ops that the ops `roots` depend on,
        renumbered so that each defines the next free slots (draw ops: the next stream ids)."""
        ops, dim = self.ops, self.dim
        made = {o[1]: k for k, o in enumerate(ops)}
        binary = set(range(OPCODE["add"], OPCODE["reduce_sum"])) | {OPCODE[nm] for nm in _SPECIAL}
        draws = native.DRAW_OPCODE

        def fields(o):  # the words of an op that are operand references
            if o[0] >= native.DRAW_BASE:
                if o[0] == draws["draw_binomial"]:
                    return (2, 3)
                return (2,) if o[0] >= draws["draw_gamma"] and o[0] != draws["draw_uniform"] else ()
            return (2, 3) if o[0] in binary or o[0] in (OPCODE["concat"], OPCODE["trisolve"]) else (2,)

        def slot_refs(o):
            return [o[f] for f in fields(o) if o[f] >= dim]

        live, todo = set(), list(roots)
        while todo:
            k = todo.pop()
            if k not in live:
                live.add(k)
                todo += [made[r] for r in slot_refs(ops[k])]
        moved, cursor, out, n_draws = {}, dim, [], 0
        for k, o in enumerate(ops):
            if k not in live:
                continue
            o = list(o)
            for f in fields(o):
                if o[f] >= dim:
                    o[f] = moved[o[f]]
            if o[0] >= native.DRAW_BASE:
                o[7] = n_draws
                n_draws += 1
            moved[o[1]] = cursor
            o[1] = cursor
            cursor += 1 if o[0] == OPCODE["reduce_sum"] else o[4]
            out.append(o)
        return out, moved, cursor


# ------------------------------------------------------------------------------------------
# log_prob expansions (numpyro/distributions/continuous.py, discrete.py): each returns the
# terms of the elementwise log density, kept apart so that scalar and constant terms are not
# broadcast to the site's size.
# ------------------------------------------------------------------------------------------
_LOG_PI = math.log(math.pi)
_HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)


def _lp_normal(B, d, x, logx):
    z = (x - d["loc"]) / d["scale"]
    return [-0.5 * B.ew("square", z), -B.ew("log", d["scale"]), B.const(-_HALF_LOG_2PI)]


def _lp_student_t(B, d, x, logx):
    df, y = d["df"], (x - d["loc"]) / d["scale"]
    return [B.ew("lgamma", (df + 1.0) * 0.5) - B.ew("lgamma", df * 0.5), -0.5 * B.ew("log", df),
            B.const(-0.5 * _LOG_PI), -B.ew("log", d["scale"]),
            -0.5 * (df + 1.0) * B.ew("log1p", B.ew("square", y) / df)]


def _lp_cauchy(B, d, x, logx):
    return [B.const(-_LOG_PI), -B.ew("log", d["scale"]), -B.ew("log1p", B.ew("square", (x - d["loc"]) / d["scale"]))]


def _lp_half_cauchy(B, d, x, logx):
    return [B.const(math.log(2.0) - _LOG_PI), -B.ew("log", d["scale"]),
            -B.ew("log1p", B.ew("square", x / d["scale"]))]


def _lp_half_normal(B, d, x, logx):
    return [-0.5 * B.ew("square", x / d["scale"]), -B.ew("log", d["scale"]), B.const(0.5 * math.log(2.0 / math.pi))]


def _lp_log_normal(B, d, x, logx):
    return [-0.5 * B.ew("square", (logx - d["loc"]) / d["scale"]), -B.ew("log", d["scale"]),
            B.const(-_HALF_LOG_2PI), -logx]


def _lp_exponential(B, d, x, logx):
    return [B.ew("log", d["rate"]), -(d["rate"] * x)]


def _lp_gamma(B, d, x, logx):
    c = d["concentration"]
    return [c * B.ew("log", d["rate"]), -B.ew("lgamma", c), (c - 1.0) * logx, -(d["rate"] * x)]


def _lp_bernoulli_logits(B, d, x, logx):
    return [x * d["logits"], -B.ew("softplus", d["logits"])]


def _lp_bernoulli_probs(B, d, x, logx):
    return [x * B.ew("log", d["probs"]), (1.0 - x) * B.ew("log1p", -d["probs"])]


def _lp_poisson(B, d, x, logx):
    return [x * B.ew("log", d["rate"]), -d["rate"], -B.ew("lgamma", x + 1.0)]


def _lp_uniform(B, d, x, logx):
    return [-B.ew("log", d["high"] - d["low"])]


def _lp_beta(B, d, x, logx):
    # at a latent site x is the site's own sigmoid: log(x) is logx and log1p(-x) resolves to
    # -softplus(u) (_Builder.ew), neither is formed from x
    a, b = d["concentration1"], d["concentration0"]
    logx = B.ew("log", x) if logx is None else logx
    return [(a - 1.0) * logx, (b - 1.0) * B.ew("log1p", -x),
            B.ew("lgamma", a + b) - B.ew("lgamma", a) - B.ew("lgamma", b)]


def _lp_pareto(B, d, x, logx):
    alpha = d["alpha"]
    return [B.ew("log", alpha), alpha * B.ew("log", d["scale"]), -((alpha + 1.0) * B.ew("log", x))]


def _binomial_coefficient(B, n, k):
    # data alone: folded on the host
    return B.ew("lgamma", n + 1.0) - B.ew("lgamma", k + 1.0) - B.ew("lgamma", n - k + 1.0)


def _lp_binomial_probs(B, d, x, logx):
    n, p = d["total_count"], d["probs"]
    return [x * B.ew("log", p), (n - x) * B.ew("log1p", -p), _binomial_coefficient(B, n, x)]


def _lp_binomial_logits(B, d, x, logx):
    n = d["total_count"]
    return [x * d["logits"], -(n * B.ew("softplus", d["logits"])), _binomial_coefficient(B, n, x)]


# ---- distributions over a whole vector: their expansions return the terms of the site's total
# log density (scalars), not elementwise terms
def _lp_dirichlet(B, d, x, logx):
    a = d["concentration"]
    if a.n < 2:
        raise NotImplementedError("a Dirichlet of fewer than 2 components")
    if x.n != a.n:
        raise NotImplementedError(f"a value of {x.n} elements under a concentration of {a.n}")
    logx = B.ew("log", x) if logx is None else logx
    return [B.rsum((a - 1.0) * logx), B.ew("lgamma", B.rsum(a)), -B.rsum(B.ew("lgamma", a))]


def _category_index(x, K):
    idx = np.asarray(x.c)
    if K < 2:
        raise NotImplementedError("a Categorical of fewer than 2 categories")
    if not np.all(np.isfinite(idx)) or np.any(idx != np.floor(idx)) or np.any(idx < 0) or np.any(idx >= K):
        raise NotImplementedError(f"observations that are not integers in [0, {K})")
    return idx.astype(np.int64)


def _ew_categorical_probs(B, d, x, logx):
    p = d["probs"]
    return [B.gather(B.ew("log", p), _category_index(x, p.n))]


def _lp_categorical_probs(B, d, x, logx):
    return [B.rsum(t) for t in _ew_categorical_probs(B, d, x, logx)]


def _ew_categorical_logits(B, d, x, logx):
    lg = d["logits"]
    return [B.gather(lg, _category_index(x, lg.n)), -B.logsumexp(lg, 1, lg.n)]


def _lp_categorical_logits(B, d, x, logx):
    lg = d["logits"]
    idx = _category_index(x, lg.n)
    return [B.rsum(B.gather(lg, idx)), -(float(idx.size) * B.logsumexp(lg, 1, lg.n))]


_CATEGORICAL = (dist.CategoricalProbs, dist.CategoricalLogits)


def _const_cholesky(A):
    """float64 factor of a constant covariance; one that is not positive definite is refused."""
    try:
        return np.linalg.cholesky(0.5 * (A + A.T))
    except np.linalg.LinAlgError:
        raise NotImplementedError("a constant matrix that is not positive definite") from None


def _lp_mvn(B, lower, base, x, site):
    """MultivariateNormal at the vector x [n]: -0.5 |L^-1 (x - loc)|^2 - sum log diag L - n/2 log 2 pi.
    A symbolic covariance goes through the cholesky op and a symbolic factor through trisolve; a
    constant one is factorised here in float64, its L^-1 applied by matvec and its log-determinant
    folded, so that a model with constant covariances alone emits neither op."""
    n, ms = int(base.event_shape[0]), tuple(base.matrix_shape)
    if len(ms) != 2 or ms[0] != ms[1]:
        _refuse(site.name, f"a MultivariateNormal with a matrix of shape {ms}: batch dimensions are not supported "
                           "(one n x n matrix is)")
    if site.plates:
        _refuse(site.name, f"a MultivariateNormal inside plates {list(site.plates)} is not supported")
    if n > native.CHOL_MAX_N:
        _refuse(site.name, f"a MultivariateNormal of {n} dimensions: at most {native.CHOL_MAX_N} are supported (one "
                           "wave factorises the matrix of a chain)")
    if isinstance(base.precision_matrix, Sym):
        _refuse(site.name, "a precision_matrix that depends on a latent site (supported: a symbolic "
                           "covariance_matrix or scale_tril, a constant precision_matrix)")
    loc_shape = tuple(np.shape(_host(base.loc)) if not isinstance(base.loc, Sym) else base.loc.shape)
    if loc_shape not in ((), (1,), (n,)) or x.n != n or tuple(site.shape) != (n,):
        _refuse(site.name, f"a MultivariateNormal with loc of shape {loc_shape} and a value of {x.n} elements at a "
                           f"site of shape {tuple(site.shape)}: batch dimensions are not supported (one vector of "
                           f"{n} is)")
    if site.obs is None and isinstance(base.loc, Sym):
        _refuse(site.name, "a latent MultivariateNormal whose loc depends on a latent site (supported: a constant "
                           "loc with a constant or symbolic covariance_matrix or scale_tril)")
    diff = x - lower.vector(base.loc, site.name)
    if base.scale_tril is not None:
        L = lower(base.scale_tril, site.name)
    elif isinstance(base.covariance_matrix, Sym):
        L = B.cholesky(lower(base.covariance_matrix, site.name), n)
    elif base.covariance_matrix is not None:
        L = B.const(_const_cholesky(np.asarray(_host(base.covariance_matrix), np.float64)).reshape(-1))
    else:
        prec = np.asarray(_host(base.precision_matrix), np.float64)
        _const_cholesky(prec)  # refuses a precision that is not positive definite
        L = B.const(_const_cholesky(np.linalg.inv(prec)).reshape(-1))
    diag = np.arange(n) * (n + 1)
    if L.is_const:
        Lc = L.c.reshape(n, n)
        with np.errstate(all="ignore"):
            Linv = _host_trisolve(Lc[None], np.eye(n)).T  # row k of the solve is L^-1 e_k
        w = B.matvec(Linv, diff) if not diff.is_const else B.const(Linv @ diff.c)
        log_det = B.const(np.log(Lc.reshape(-1)[diag]).sum())
    else:
        w = B.trisolve(L, diff)
        log_det = B.rsum(B.ew("log", B.gather(L, diag)))
    return [-0.5 * B.rsum(B.ew("square", w)), -log_det, B.const(-n * _HALF_LOG_2PI)]


def _lp_mixture(B, lower, base, xv, site):
    """MixtureSameFamily at observations xv [N]: the site's total, the sum of _ew_mixture."""
    return [B.rsum(t) for t in _ew_mixture(B, lower, base, xv, site)]


def _ew_mixture(B, lower, base, xv, site):
    """MixtureSameFamily at observations xv [N]: the N x K table of component log densities plus
    log weights, flat and row-major, through logsumexp(rows = N, cols = K): N elements."""
    mixing, comp = _base(base.mixing_distribution), _base(base.component_distribution)
    if not isinstance(mixing, _CATEGORICAL):
        _refuse(site, f"a mixing distribution {type(mixing).__name__} (a Categorical is supported)")
    entry = _LOGPROB.get(type(comp))
    if entry is None or not entry[2] or isinstance(comp, _VECTOR) or comp.event_shape:
        _refuse(site, f"a mixture of {type(comp).__name__} components (supported: the univariate continuous "
                      "distributions)")
    w = lower.vector(mixing.probs if isinstance(mixing, dist.CategoricalProbs) else mixing.logits, site)
    K, N = w.n, xv.size
    if K < 2:
        _refuse(site, "a mixture of fewer than 2 components")
    if tuple(comp.batch_shape) not in ((), (K,)):
        _refuse(site, f"component batch shape {tuple(comp.batch_shape)} under {K} mixing weights")
    logw = B.ew("log", w) if isinstance(mixing, dist.CategoricalProbs) else w - B.logsumexp(w, 1, K)
    col = np.tile(np.arange(K), N)  # the component of each element of the flat table
    d = {}
    for p in entry[1]:
        val = lower.vector(getattr(comp, p), site)
        if val.n not in (1, K):
            _refuse(site, f"component parameter {p!r} of {val.n} elements under {K} mixing weights")
        d[p] = B.gather(val, col) if val.n == K else val  # a scalar keeps stride 0
    x = B.const(np.repeat(xv, K))
    with np.errstate(all="ignore"):
        logx = B.const(np.log(x.c)) if comp.support == "positive" else None
    table = B.gather(logw, col)
    for t in entry[0](B, d, x, logx):
        table = table + t
    return [B.logsumexp(table, N, K)]


# distribution -> (expansion, parameter names, may be latent)
_LOGPROB = {
    dist.Normal: (_lp_normal, ("loc", "scale"), True),
    dist.StudentT: (_lp_student_t, ("df", "loc", "scale"), True),
    dist.Cauchy: (_lp_cauchy, ("loc", "scale"), True),
    dist.HalfCauchy: (_lp_half_cauchy, ("scale",), True),
    dist.HalfNormal: (_lp_half_normal, ("scale",), True),
    dist.LogNormal: (_lp_log_normal, ("loc", "scale"), True),
    dist.Exponential: (_lp_exponential, ("rate",), True),
    dist.Gamma: (_lp_gamma, ("concentration", "rate"), True),
    dist.BernoulliLogits: (_lp_bernoulli_logits, ("logits",), False),
    dist.BernoulliProbs: (_lp_bernoulli_probs, ("probs",), False),
    dist.Poisson: (_lp_poisson, ("rate",), False),
    dist.Uniform: (_lp_uniform, ("low", "high"), True),
    dist.Beta: (_lp_beta, ("concentration1", "concentration0"), True),
    dist.Pareto: (_lp_pareto, ("scale", "alpha"), True),
    dist.BinomialProbs: (_lp_binomial_probs, ("total_count", "probs"), False),
    dist.BinomialLogits: (_lp_binomial_logits, ("total_count", "logits"), False),
    dist.Dirichlet: (_lp_dirichlet, ("concentration",), True),
    dist.CategoricalProbs: (_lp_categorical_probs, ("probs",), False),
    dist.CategoricalLogits: (_lp_categorical_logits, ("logits",), False),
    dist.MixtureSameFamily: (None, (), False),  # _lp_mixture lowers the two distributions it holds
    dist.MultivariateNormal: (None, (), True),  # _lp_mvn lowers loc and the matrix, which is of rank 2
}
_BINOMIAL = (dist.BinomialProbs, dist.BinomialLogits)
# whole-vector distributions: one log density per site, returned as scalar terms
_VECTOR = (dist.Dirichlet, dist.CategoricalProbs, dist.CategoricalLogits, dist.MixtureSameFamily,
           dist.MultivariateNormal)


# ---- the logit likelihoods elementwise.  x eta - n softplus(eta) is right as a term of a site's
# total, but one element alone cancels where the outcome is all but certain (x = n, eta large:
# eta - softplus(eta) = -softplus(-eta), 1e-9 from operands of 20).  The same density without a
# difference: -x softplus(-eta) - (n - x) softplus(eta).
def _ew_bernoulli_logits(B, d, x, logx, n=1.0):
    eta = d["logits"]
    return [-(x * B.ew("softplus", -eta)), -((n - x) * B.ew("softplus", eta))]


def _ew_binomial_logits(B, d, x, logx):
    n = d["total_count"]
    return _ew_bernoulli_logits(B, d, x, logx, n) + [_binomial_coefficient(B, n, x)]


# elementwise expansions where they differ from _LOGPROB's (loglik_program.py): the whole-vector
# distributions before their final rsum, one term list of N elements per site (a Dirichlet vector
# is one observation: its _lp terms are its elementwise ones), and the logit likelihoods
_ELEMENTWISE = {dist.CategoricalProbs: _ew_categorical_probs, dist.CategoricalLogits: _ew_categorical_logits,
                dist.Dirichlet: _lp_dirichlet, dist.BernoulliLogits: _ew_bernoulli_logits,
                dist.BinomialLogits: _ew_binomial_logits}
# ---- count likelihoods (numpyro/distributions/conjugate.py, discrete.py).  Every log mass with a
# concentration c holds lgamma(c + y) - lgamma(c), which cancels in float32 as a difference of two
# lgamma ops; the lrising op gives R(c, y) = lgamma(c + y) - lgamma(c) - y log(c), which tends to 0
# as c grows, and the y log(c) it leaves out joins the other logarithms so that the near-Poisson
# (near-binomial) limit has no large terms of opposite sign:
#   GammaPoisson(c, mean m = c / rate):  R(c, y) + y log(m) - (c + y) log1p(m / c) - log y!
def _log_factorial(B, x):
    return B.ew("lgamma", x + 1.0)  # data alone: folded on the host


def _lp_gamma_poisson(B, d, x, logx):
    c, rate = d["concentration"], d["rate"]
    return [B.lrising(c, x), x * B.ew("log", c / rate), -((c + x) * B.ew("log1p", 1.0 / rate)), -_log_factorial(B, x)]


def _lp_negative_binomial2(B, d, x, logx):
    c, m = d["concentration"], d["mean"]
    return [B.lrising(c, x), x * B.ew("log", m), -((c + x) * B.ew("log1p", m / c)), -_log_factorial(B, x)]


def _lp_negative_binomial_probs(B, d, x, logx):
    # rate = 1 / p - 1: log1p(1 / rate) = -log1p(-p) and the mean is n p / (1 - p)
    n, p = d["total_count"], d["probs"]
    return [B.lrising(n, x), x * B.ew("log", n * p), n * B.ew("log1p", -p), -_log_factorial(B, x)]


def _lp_negative_binomial_logits(B, d, x, logx):
    # the reference's -(n softplus(logits) + y softplus(-logits) + log_beta_1(n, y))
    n, lg = d["total_count"], d["logits"]
    return [B.lrising(n, x), x * B.ew("log", n), -(x * B.ew("softplus", -lg)), -(n * B.ew("softplus", lg)),
            -_log_factorial(B, x)]


def _lp_beta_binomial(B, d, x, logx):
    # C(n, y) B(c1 + y, c0 + n - y) / B(c1, c0) as three rising factorials; what they leave out is
    # y log(c1 / (c1 + c0)) + (n - y) log(c0 / (c1 + c0)), the binomial limit, each through a log1p
    c1, c0, n = d["concentration1"], d["concentration0"], d["total_count"]
    return [B.lrising(c1, x), B.lrising(c0, n - x), -B.lrising(c1 + c0, n),
            -(x * B.ew("log1p", c0 / c1)), -((n - x) * B.ew("log1p", c1 / c0)), _binomial_coefficient(B, n, x)]


def _lp_geometric_probs(B, d, x, logx):
    p = d["probs"]
    return [x * B.ew("log1p", -p), B.ew("log", p)]


def _lp_geometric_logits(B, d, x, logx):
    lg = d["logits"]
    return [-((x + 1.0) * B.ew("softplus", lg)), lg]


def _lp_zero_inflated(B, lower, base, x, site):
    """ZeroInflatedProbs / ZeroInflatedLogits at the observations x: with lg = log gate, l1 =
    log(1 - gate) and lp the base's elementwise log mass, l1 + lp where y > 0 and
    logaddexp(lg, l1 + lp) where y = 0 (the reference's ZeroInflatedLogits algebra), the two joined
    by the data's 0 / 1 mask.  Both branches are finite at every y for the bases accepted here.  The
    base's data-only terms (log y!, the binomial coefficient) stay host constants."""
    inner = _base(base.base_dist)
    entry = _logprob_entry(inner)
    if entry is None or not isinstance(inner, _ZERO_INFLATABLE):
        _refuse(site, f"a zero-inflated {type(inner).__name__} (supported bases: "
                      f"{', '.join(t.__name__ for t in _ZERO_INFLATABLE)})")
    d = {p: lower.vector(getattr(inner, p), site) for p in entry[1]}
    _check_count_data(inner, d, site)
    if isinstance(base, dist.ZeroInflatedLogits):
        gl = lower.vector(base.gate_logits, site)
        log_gate, log_1m = -B.ew("softplus", -gl), -B.ew("softplus", gl)
    else:
        gate = lower.vector(base.gate, site)
        log_gate, log_1m = B.ew("log", gate), B.ew("log1p", -gate)
    dyn, cst = log_1m, B.const(np.zeros(1))
    for t in _ELEMENTWISE.get(type(inner), entry[0])(B, d, x, None):
        t = B.const(t)
        if t.is_const:
            cst = cst + t
        else:
            dyn = dyn + t
    zero = B.const((x.c == 0.0).astype(np.float64))
    return [zero * B.ew("logaddexp", log_gate, dyn + zero * cst), (1.0 - zero) * dyn, (1.0 - zero) * cst]


# distribution -> (expansion, parameter names, may be latent), as _LOGPROB, whose keys existing
# tests pin: the lowering consults this table after it (_logprob_entry)
_COUNT_LOGPROB = {
    dist.GammaPoisson: (_lp_gamma_poisson, ("concentration", "rate"), False),
    dist.NegativeBinomial2: (_lp_negative_binomial2, ("mean", "concentration"), False),
    dist.NegativeBinomialProbs: (_lp_negative_binomial_probs, ("total_count", "probs"), False),
    dist.NegativeBinomialLogits: (_lp_negative_binomial_logits, ("total_count", "logits"), False),
    dist.BetaBinomial: (_lp_beta_binomial, ("concentration1", "concentration0", "total_count"), False),
    dist.GeometricProbs: (_lp_geometric_probs, ("probs",), False),
    dist.GeometricLogits: (_lp_geometric_logits, ("logits",), False),
    dist.ZeroInflatedProbs: (None, (), False),  # _lp_zero_inflated lowers the gate and the base it holds
    dist.ZeroInflatedLogits: (None, (), False),
    dist.ZeroInflatedPoisson: (None, (), False),
}
_ZERO_INFLATED = (dist.ZeroInflatedProbs, dist.ZeroInflatedLogits)
_ZERO_INFLATABLE = (dist.Poisson, dist.GammaPoisson, dist.NegativeBinomial2, dist.NegativeBinomialProbs,
                    dist.NegativeBinomialLogits, dist.GeometricProbs, dist.GeometricLogits, dist.BinomialProbs,
                    dist.BinomialLogits, dist.BetaBinomial)


def _logprob_entry(base):
    """The (expansion, parameter names, may be latent) of a distribution, or None."""
    return _LOGPROB.get(type(base)) or _COUNT_LOGPROB.get(type(base))


def _check_count_data(base, d, site):
    """Binomial and BetaBinomial take their total_count as data."""
    if isinstance(base, _BINOMIAL + (dist.BetaBinomial,)) and not d["total_count"].is_const:
        _refuse(site, "a total_count that depends on a latent site: it must be data")


# support -> transform code of a latent site
_SUPPORT_CODE = {"real": REAL, "positive": POSITIVE, "unit_interval": UNIT, "interval": UNIT, "greater_than": LOWER,
                 "simplex": SIMPLEX}


def _site_bounds(base, name):
    """(lo, width) float64 of a latent site's affine part, or None: the bounds are host constants."""
    if isinstance(base, dist.Uniform):
        bounds = (base.low, base.high)
    elif isinstance(base, dist.Pareto):
        bounds = (base.scale,)
    else:
        return None
    for b in bounds:
        if isinstance(b, Sym):
            _refuse(name, f"a bound of {type(base).__name__} that depends on a latent site ({b!r}): bounds must be "
                          "constants")
    vals = [np.asarray(_host(b), np.float64) for b in bounds]
    if any(v.ndim > 1 for v in vals):
        _refuse(name, "a bound of rank > 1")
    if len(vals) == 2:
        if not np.all(vals[1] > vals[0]):
            _refuse(name, "Uniform needs low < high")
        return vals[0], vals[1] - vals[0]
    return vals[0], np.float64(1.0)


class _Refuse(NotImplementedError):
    pass


def _refuse(site, why):
    raise _Refuse(f"program compiler: site {site!r}: {why}")


class _Lowering:
    """Sym expressions -> builder values, one value per Sym object."""

    def __init__(self, B, latents):
        self.B, self.latents = B, latents  # latents: name -> constrained value
        self.seen = {}  # id(Sym) -> (Sym, value)

    def __call__(self, x, site):
        if not isinstance(x, Sym):
            a = np.asarray(_host(x), np.float64)
            if a.ndim > 2:
                _refuse(site, f"a constant of shape {a.shape} (rank > 2)")
            return self.B.const(a.reshape(-1))  # rank 2: flat, row-major
        hit = self.seen.get(id(x))
        if hit is not None:
            return hit[1]
        if len(x.shape) > 2:
            _refuse(site, f"expression {x!r} of shape {x.shape}: values of rank > 2 are not supported")
        out = self._lower(x, site)
        self.seen[id(x)] = (x, out)
        return out

    def vector(self, x, site):
        """A value of rank <= 1: a distribution's parameter (the matrix of a MultivariateNormal is
        lowered by _lp_mvn) or the operand of an operation that takes vectors."""
        if isinstance(x, Sym):
            if len(x.shape) > 1:
                _refuse(site, f"expression {x!r} of shape {x.shape}: values of rank > 1 are not supported")
        elif np.ndim(_host(x)) > 1:
            _refuse(site, f"a constant of shape {np.shape(_host(x))} (rank > 1) outside a matmul")
        return self(x, site)

    def _lower(self, x, site):
        B, op = self.B, x.op
        if op == "latent":
            if x.args[0] not in self.latents:
                _refuse(site, f"unknown latent {x.args[0]!r}")
            return self.latents[x.args[0]]
        if op in ("neg", "exp", "log", "sqrt", "tanh", "log1p", "square"):
            return B.ew(op, self(x.args[0], site))
        if op == "expit":  # exp(-softplus(-x)): log(expit(x)) then folds to -softplus(-x)
            return B.ew("exp", B.ew("neg", B.ew("softplus", B.ew("neg", self(x.args[0], site)))))
        if op in _BINARY or op == "logaddexp":
            return B.ew(op, *(self._broadcast(a, x.shape, site) for a in x.args))
        if op == "cholesky":
            return B.cholesky(self(x.args[0], site), x.shape[0])
        # reductions, joins, indexing and products take vectors: self.vector refuses a value of rank 2
        if op == "sum":
            return B.rsum(self.vector(x.args[0], site))
        if op == "cumsum":
            return B.cumsum(self.vector(x.args[0], site))
        if op == "logsumexp":
            v = self.vector(x.args[0], site)
            return B.logsumexp(v, 1, v.n)
        if op == "concatenate":
            parts = [self.vector(a, site) for a in x.args]
            for a, v in zip(x.args, parts):
                if v.n != int(np.prod(np.shape(_host(a)) if not isinstance(a, Sym) else a.shape, dtype=np.int64)):
                    _refuse(site, "concatenate of a part whose size is not its shape's")
            out = parts[0]
            for v in parts[1:]:
                out = B.concat(out, v)
            return out
        if op == "getitem":
            src, idx = self.vector(x.args[0], site), x.args[1]
            sel = np.arange(src.n)[idx] if isinstance(idx, (int, slice)) else np.asarray(_host(idx))
            if np.ndim(sel) > 1:
                _refuse(site, "indexing with an index array of rank > 1")
            sel = np.asarray(sel, np.int64).reshape(-1)
            return B.gather(src, np.where(sel < 0, sel + src.n, sel))
        if op == "matmul":
            a, b = x.args
            if isinstance(a, Sym) == isinstance(b, Sym):
                _refuse(site, "matmul of two symbolic values (supported: a constant matrix with a symbolic vector)")
            if isinstance(b, Sym):  # M @ v
                M, vec = np.asarray(_host(a), np.float64), self.vector(b, site)
                M = M.reshape(1, -1) if M.ndim == 1 else M
            else:  # v @ M
                M, vec = np.asarray(_host(b), np.float64), self.vector(a, site)
                M = M.reshape(1, -1) if M.ndim == 1 else M.T
            if M.ndim != 2 or M.shape[1] != vec.n or len(x.shape) > 1:
                _refuse(site, f"matmul of shapes {np.shape(_host(a)) if not isinstance(a, Sym) else a.shape} and "
                              f"{np.shape(_host(b)) if not isinstance(b, Sym) else b.shape}")
            return B.matvec(M, vec)
        _refuse(site, f"operation {op!r} is not supported (supported: {sorted(_UNARY[:7] + _BINARY)}, expit, logaddexp, sum, "
                      "cumsum, logsumexp, concatenate, getitem, matmul, linalg.cholesky)")

    def _broadcast(self, a, out_shape, site):
        """The operand a of an elementwise op of shape out_shape: itself where it has as many elements
        or one (the ops' stride 0), else broadcast by NumPy's rules: a constant on the host, a symbolic
        value by a gather with the index np.broadcast_to gives."""
        size = int(np.prod(out_shape, dtype=np.int64))
        if not isinstance(a, Sym):
            c = np.asarray(_host(a), np.float64)
            if c.size in (1, size) or c.ndim > 2:
                return self(c.reshape(-1) if c.ndim <= 2 else c, site)
            return self.B.const(np.broadcast_to(c, out_shape).reshape(-1))
        v = self(a, site)
        if v.n in (1, size):
            return v
        idx = np.broadcast_to(np.arange(v.n).reshape(a.shape), out_shape).reshape(-1)
        return self.B.gather(v, idx)


def _trace(model, args, kwargs):
    """The trace of ``model(*args, **kwargs)``, a reparam wrapper unwrapped; reparam configs are refused."""
    trace = trace_model(getattr(model, "_nmx_model", model), args, kwargs, getattr(model, "_nmx_reparam", None))
    for name in trace.reparam:
        _refuse(name, "reparam configs are not supported")
    return trace


def _forward_prologue(model, args, kwargs, given, missing, observed=lambda s: None):
    """The start of compile_predictive and compile_log_likelihood: the trace, the per-site checks,
    the given sites without data laid out as inputs in sorted name order, and a builder over them:
    (trace, sizes, inputs, B, values, lower).  ``missing(s, base)`` sees a site that has neither
    data nor a given value, ``observed(s)`` a site with data once its shape has passed."""
    trace = _trace(model, args, kwargs)
    given = set(given)
    sizes = {}
    for s in trace.sites.values():
        base = _base(s.fn)
        if _logprob_entry(base) is None:
            _refuse(s.name, f"{type(base).__name__} is not supported")
        if s.obs is None and s.name not in given:
            missing(s, base)
        if len(s.shape) > 1:
            _refuse(s.name, f"site of shape {s.shape}: sites of rank > 1 are not supported")
        if s.obs is not None:
            if np.ndim(_host(s.obs)) > 1:
                _refuse(s.name, f"observations of shape {np.shape(_host(s.obs))}: rank > 1 is not supported")
            observed(s)
        n = int(np.prod(s.shape, dtype=np.int64))
        if n <= 0:
            _refuse(s.name, "empty site")
        sizes[s.name] = n
    inputs, dim = [], 0
    for s in sorted((s for s in trace.sites.values() if s.obs is None and s.name in given), key=lambda s: s.name):
        inputs.append((s.name, dim, sizes[s.name], tuple(s.shape)))
        dim += sizes[s.name]
    B = _Builder(dim)
    values = {name: _V(B, n, slot=off) for name, off, n, _ in inputs}
    return trace, sizes, inputs, B, values, _Lowering(B, values)


def compile_model(model, args=(), kwargs=None, max_workspace_bytes=1 << 30):
    """Trace ``model(*args, **kwargs)`` and lower its potential to a ProgramPotential."""
    trace = _trace(model, args, kwargs)
    lat = sorted((s for s in trace.sites.values() if s.obs is None), key=lambda s: s.name)
    if not lat:
        raise _Refuse("program compiler: the model has no latent sample sites")
    sites, offsets, affine, o = [], {}, {}, 0
    for s in lat:
        base = _base(s.fn)
        if len(s.shape) > 1:
            _refuse(s.name, f"latent of shape {s.shape}: latents of rank > 1 are not supported")
        entry = _logprob_entry(base)
        if entry is None or not entry[2]:
            _refuse(s.name, f"{type(base).__name__} is not supported as a latent site")
        if base.support not in _SUPPORT_CODE:
            _refuse(s.name, f"support {base.support!r} is not supported ({', '.join(_SUPPORT_CODE)} are)")
        n = int(np.prod(s.shape, dtype=np.int64))
        if n <= 0:
            _refuse(s.name, "empty site")
        shape = tuple(s.shape)
        if base.support == "simplex":  # K - 1 unconstrained coordinates: the site's shape in `sites`
            if len(shape) != 1 or shape != tuple(base.event_shape) or n < 2:
                _refuse(s.name, f"a simplex site of shape {shape} (supported: one vector of K >= 2 components, "
                                "without batch or plate dimensions)")
            n, shape = n - 1, (n - 1,)
        bounds = _site_bounds(base, s.name)
        if bounds is not None:
            if any(b.size not in (1, n) for b in bounds):
                _refuse(s.name, f"bounds of {[b.size for b in bounds]} elements at a site of {n}")
            affine[s.name] = bounds
        sites.append((s.name, shape, _SUPPORT_CODE[base.support]))
        offsets[s.name] = (o, n)
        o += n
    B = _Builder(o)
    unconstrained = {name: _V(B, n, slot=off) for name, (off, n) in offsets.items()}
    # per site: the constrained value, log x where the transform gives it (None otherwise) and
    # the terms of log|J|
    constrained, log_value, log_jac = {}, {}, {}
    for name, _, tr in sites:
        u = unconstrained[name]
        lo, width = affine.get(name, (0.0, 1.0))
        if tr == REAL:
            constrained[name], log_value[name], log_jac[name] = u, None, []
        elif tr == POSITIVE:  # ExpTransform: log|J| = u
            constrained[name], log_value[name], log_jac[name] = B.ew("exp", u), u, [u]
        elif tr == UNIT:  # sigmoid, in its stable forms: log x = -softplus(-u), log(1 - x) = -softplus(u)
            logx, log1mx = -B.ew("softplus", -u), -B.ew("softplus", u)
            x = B.ew("exp", logx)
            B.log1m[x.slot] = log1mx
            constrained[name] = B.ew("add", lo, B.ew("mul", width, x))
            log_value[name] = logx if constrained[name] is x else None
            log_jac[name] = [logx, log1mx, B.const(np.log(width))]
        elif tr == SIMPLEX:
            # stick breaking with the reference's offset (StickBreakingTransform: u = 0 is the uniform
            # point), in log space: t = u - log(K - 1 - k), log z = -softplus(-t), log(1 - z) =
            # -softplus(t), log x = (log z, 0) + (0, cumsum log(1 - z)).  log|J| = sum_{k < K-1}
            # (log x_k + log(1 - z_k)), and the second terms sum to the scan's last element log x_{K-1}:
            # log|J| = sum(log x) over all K.  x = exp(log x), so every log x of a density folds back
            # to log x itself (ew: log(exp(v)) = v) and never sees an underflowed x.
            t = u - np.log(np.arange(u.n, 0, -1, dtype=np.float64))
            log_z, log_1mz = -B.ew("softplus", -t), -B.ew("softplus", t)
            logx = B.concat(log_z, B.const([0.0])) + B.concat(B.const([0.0]), B.cumsum(log_1mz))
            constrained[name], log_value[name], log_jac[name] = B.ew("exp", logx), logx, [B.rsum(logx)]
        else:  # LOWER: x = lo + exp(u), log|J| = u
            constrained[name], log_value[name], log_jac[name] = B.ew("add", lo, B.ew("exp", u)), None, [u]
    lower = _Lowering(B, constrained)

    const_total = 0.0
    scalars = []  # scalar terms of log p + log|J|
    for s in trace.sites.values():
        base = _base(s.fn)
        entry = _logprob_entry(base)
        if entry is None:
            _refuse(s.name, f"{type(base).__name__} is not supported")
        expand, pnames, _ = entry
        try:
            d = {p: lower.vector(getattr(base, p), s.name) for p in pnames}
            _check_count_data(base, d, s.name)
            if s.obs is None:
                x = constrained[s.name]
                logx = log_value[s.name]
                n_site = offsets[s.name][1]
            else:
                xv = np.asarray(_host(s.obs), np.float64)
                if xv.ndim > 1:
                    _refuse(s.name, f"observations of shape {xv.shape}: rank > 1 is not supported")
                x = B.const(xv)
                with np.errstate(all="ignore"):
                    logx = B.const(np.log(x.c)) if base.support in ("positive", "simplex") else None
                n_site = max(int(np.prod(s.shape, dtype=np.int64)), x.n)
            if isinstance(base, _VECTOR):
                n_site = 1
            if isinstance(base, dist.MixtureSameFamily):
                terms = _lp_mixture(B, lower, base, np.asarray(x.c, np.float64).reshape(-1), s.name)
            elif isinstance(base, dist.MultivariateNormal):
                terms = _lp_mvn(B, lower, base, x, s)
            elif isinstance(base, _ZERO_INFLATED):
                terms = _lp_zero_inflated(B, lower, base, x, s.name)
            else:
                terms = expand(B, d, x, logx)
            if s.obs is None:
                terms += log_jac[s.name]
        except _Refuse:
            raise
        except NotImplementedError as e:
            _refuse(s.name, str(e))
        vec = None
        for t in terms:
            t = B.const(t)
            if t.n not in (1, n_site):
                _refuse(s.name, f"a log-density term of {t.n} elements at a site of {n_site}")
            if t.is_const:
                const_total += float(t.c.sum()) if t.n == n_site else float(t.c[0]) * n_site
            elif t.n == n_site and n_site > 1:
                vec = t if vec is None else vec + t
            else:
                scalars.append(t * float(n_site) if n_site > 1 else t)
        if vec is not None:
            scalars.append(B.rsum(vec))
    if not scalars:
        raise _Refuse("program compiler: the log density does not depend on the latent sites")
    total = scalars[0]
    for t in scalars[1:]:
        total = total + t
    u = B.ew("sub", B.const(-const_total), total)  # U = -log p; always the program's last op
    assert u.slot == B.next_slot - 1
    pot = ProgramPotential(B.program(), sites, max_workspace_bytes, affine)
    return _with_traced_deterministics(pot, trace)


class ProgramPotential(Potential):
    """A traced model's potential as a program (nmx_pe_program): one launch per evaluation."""

    def __init__(self, program, sites, max_workspace_bytes=1 << 30, affine=None):
        self.program = program
        self.sites = list(sites)
        self.affine = dict(affine or {})  # name -> (lo, width) of the UNIT / LOWER sites with bounds
        self.dim = program.dim
        self.max_workspace_bytes = int(max_workspace_bytes)
        assert self.dim == sum(int(np.prod(s, dtype=np.int64)) for _, s, _ in self.sites)

    # a single workspace: `slots` stays unset, so the engine keeps the potential on one stream

    def _bind(self, C, ldc, device):
        import torch

        prog = self.program
        device_program = prog.upload(device)
        wb = native.lib().nmx_pe_program_workspace_bytes(prog.num_slots, ldc)
        if wb > self.max_workspace_bytes:
            raise NotImplementedError(
                f"program potential: the tape of {prog.num_slots} slots for {C} chains (ldc {ldc}) needs a workspace "
                f"of {wb} bytes, above max_workspace_bytes = {self.max_workspace_bytes}; run fewer chains per engine")
        self.workspace = torch.empty(wb, dtype=torch.uint8, device=device)
        self._device_program, self._cprog = device_program, device_program.struct  # the holder keeps the arrays

    def evaluate(self, ev, stream):
        native.check(native.lib().nmx_pe_program(ctypes.byref(self._cprog), ctypes.byref(ev),
                                                 native.ptr(self.workspace), stream), "nmx_pe_program")

    def flops_per_eval(self, num_chains):
        return self.program.flops_per_eval(num_chains)

    def bytes_per_eval(self):
        return self.program.bytes_per_eval()
