"""Cases for the cumsum / logsumexp / concat ops of the program kernel and for the models built on
them (simplex latents by stick breaking, Categorical and mixture likelihoods): tests/test_simplex.py
on the host, tests/test_gpu_simplex.py on the device.

Op cases are hand-assembled programs in the manner of tests/program_op_cases.py (``Asm`` below
extends its assembler): each ends in reduce_sum(w * f(...)) with w = linspace(0.5, 1.5, n) and has
an independent float64 torch reference (torch.cumsum, torch.logsumexp, torch.cat; the adjoint by
autograd).  ``Program.run_host`` is never the reference.

Families (``cases(family)``):

cumsum      n in CUMSUM_SIZES (one chunk, the carry across one and several chunks); the operand
            a computed value, or a z slice at offset 3.
logsumexp   (rows, cols) in LSE_SHAPES: both regimes of the kernel (a wave per row when rows < 64
            and cols >= 64, a lane per row otherwise), the regime's edge, rows that straddle lanes;
            the operand a computed value, or a z slice at offset 3.
lse_limits  entries 200 apart; all entries 1e4; one -inf entry in a row (a constant log 0 added to a
            slot).  ``all_inf_row()`` is apart: its U is +inf, so it has no finite reference.
concat      (na, nb) in CONCAT_SHAPES with a constant on either side, two computed values, and two
            disjoint z ranges in swapped order.

Models (``MODELS``): Dirichlet-Categorical, a Dirichlet with a symbolic concentration, categorical
logits, and a Normal mixture with latent weights, locations and scales.  Each has two float64
references: ``torch_reference`` (torch.distributions: Dirichlet, StickBreakingTransform,
Categorical, MixtureSameFamily, autograd) and ``logspace_reference`` (the log-space formulas of
the stick breaking written out: U in NumPy, the gradient by autograd of the same statement in
torch, the two U asserted equal).

``run_host_f32`` restates ``Program.run_host`` in float32 NumPy for every op."""
import functools
import math

import numpy as np
import torch
import torch.distributions as td

import numpyro_amd as numpyro
import program_op_cases as OC
from numpyro_amd import distributions as dist
from numpyro_amd import native
from numpyro_amd.native import OPCODE
from numpyro_amd.program import _BINARY, _HOST_FWD, _UNARY, Program, _host_rev

ROWS = OC.ROWS
CUMSUM_SIZES = (1, 63, 64, 65, 129, 200)
LSE_SHAPES = ((1, 1), (1, 65), (1, 200), (7, 9), (3, 64), (63, 64), (64, 64), (70, 3), (129, 2))
CONCAT_SHAPES = ((1, 1), (63, 2), (64, 64), (65, 70), (1, 129))
FAMILIES = ("cumsum", "logsumexp", "lse_limits", "concat")
_ANY = (-2.0, 2.0, "u")
_WIDE = (-3.0, 3.0, "u")


class Asm(OC.Asm):
    """program_op_cases.Asm with the three ops."""

    def cumsum(self, a):
        assert a.stride == 1
        return self._emit("cumsum", a.ref, 0, a.length, 1, 0, 0, a.length, lambda Z: torch.cumsum(a.fn(Z), 1))

    def logsumexp(self, a, rows, cols):
        assert a.stride == 1 and a.length == rows * cols
        return self._emit("logsumexp", a.ref, 0, rows, 1, 0, cols, rows,
                          lambda Z: torch.logsumexp(a.fn(Z).expand(Z.shape[0], rows * cols).reshape(-1, rows, cols), 2))

    def concat(self, a, b):
        n = a.length + b.length
        return self._emit("concat", a.ref, b.ref, n, 1, 1, a.length, n,
                          lambda Z: torch.cat([a.fn(Z).expand(Z.shape[0], a.length),
                                               b.fn(Z).expand(Z.shape[0], b.length)], 1))


def _cumsum():
    out = []
    for n in CUMSUM_SIZES:
        A = Asm(f"slot.n{n}", "cumsum")
        out.append(A.case(A.cumsum(A.slot(n, _ANY))))
        A = Asm(f"z3.n{n}", "cumsum")
        A.pad()
        out.append(A.case(A.cumsum(A.z(n, _ANY))))
    return out


def _logsumexp():
    out = []
    for rows, cols in LSE_SHAPES:
        A = Asm(f"slot.{rows}x{cols}", "logsumexp")
        out.append(A.case(A.logsumexp(A.slot(rows * cols, _WIDE), rows, cols)))
        A = Asm(f"z3.{rows}x{cols}", "logsumexp")
        A.pad()
        out.append(A.case(A.logsumexp(A.z(rows * cols, _WIDE), rows, cols)))
    return out


def _lse_limits():
    out = []
    rows, cols = 5, 7
    n = rows * cols
    A = Asm("apart200", "lse_limits")
    shift = 200.0 * (np.arange(n) % 3 - 1)  # -200, 0, 200 in turn: every row has entries 200 and 400 apart
    out.append(A.case(A.logsumexp(A.ew("add", A.slot(n, _ANY), A.const(shift)), rows, cols)))
    A = Asm("all1e4", "lse_limits")
    out.append(A.case(A.logsumexp(A.z(n, None, values=np.full((ROWS, n), 1e4)), rows, cols)))
    A = Asm("one_minus_inf", "lse_limits")
    log0 = np.zeros(n)
    log0[[3, 9, 34]] = -np.inf  # rows 0, 1 and 4 have one entry log 0
    out.append(A.case(A.logsumexp(A.ew("add", A.slot(n, _ANY), A.const(log0)), rows, cols)))
    return out


def all_inf_row():
    """(potential, Z, rows x cols, the all -inf row, float64 gradient): U = sum_i w_i (-lse_i) of
    x = 0.5 z + c, c = -inf on row 1 of 3 x 4.  U is +inf on every row of Z; the gradient is
    -0.5 w_i softmax(x_i) on the finite rows and exactly 0 on row 1."""
    rows, cols, dead = 3, 4, 1
    n = rows * cols
    A = Asm("all_inf_row", "lse_limits")
    c = np.zeros(n)
    c[dead * cols:(dead + 1) * cols] = -np.inf
    case = A.case(A.ew("neg", A.logsumexp(A.ew("add", A.slot(n, _ANY), A.const(c)), rows, cols)))
    x = 0.5 * case.Z.reshape(ROWS, rows, cols)
    soft = np.exp(x - x.max(2, keepdims=True))
    soft /= soft.sum(2, keepdims=True)
    G = -0.5 * OC.weights(rows)[None, :, None] * soft
    G[:, dead] = 0.0
    return case.pot, case.Z, (rows, cols), dead, G.reshape(ROWS, n)


def _concat():
    out = []
    for na, nb in CONCAT_SHAPES:
        A = Asm(f"slot-const.{na}+{nb}", "concat")
        out.append(A.case(A.ew("square", A.concat(A.slot(na, _ANY), A.const(OC._draw(A.rs, _ANY, nb))))))
        A = Asm(f"const-slot.{na}+{nb}", "concat")
        out.append(A.case(A.ew("square", A.concat(A.const(OC._draw(A.rs, _ANY, na)), A.slot(nb, _ANY)))))
        A = Asm(f"slot-slot.{na}+{nb}", "concat")
        out.append(A.case(A.ew("square", A.concat(A.slot(na, _ANY), A.ew("tanh", A.z(nb, _ANY))))))
        # the second part first in z, three unread coordinates before and between the two ranges
        A = Asm(f"z-z.{na}+{nb}", "concat")
        A.pad()
        b = A.z(nb, _ANY)
        A.pad()
        a = A.z(na, _ANY)
        out.append(A.case(A.ew("square", A.concat(a, b))))
    return out


_BUILD = {"cumsum": _cumsum, "logsumexp": _logsumexp, "lse_limits": _lse_limits, "concat": _concat}
ONE_PER_OP = (("cumsum", "z3.n200"), ("logsumexp", "slot.3x64"), ("logsumexp", "slot.70x3"), ("concat", "z-z.65+70"))


@functools.lru_cache(maxsize=None)
def cases(family):
    return tuple(_BUILD[family]())


def case(family, name):
    return next(c for c in cases(family) if c.name == name)


# ------------------------------------------------------------------------------------------ refused programs
def _raw(rows, dim, consts=(0.0,)):
    """A Program from rows whose last op is appended here: reduce_sum of the last value."""
    rows = [list(r) for r in rows]
    dst, n = rows[-1][1], rows[-1][4]
    rows.append([OPCODE["reduce_sum"], dst + n, dst, 0, n, 1, 0, 0])
    return Program(rows, list(consts), [], dst + n + 1, dim)


def refused_programs():
    """(name, program, op name): programs nmx_program_check must refuse naming the op.  Slots
    [0, 8) are z; constants: eight zeros."""
    C, L, K, T = OPCODE["cumsum"], OPCODE["logsumexp"], OPCODE["concat"], OPCODE["tanh"]
    z8 = [0.0] * 8
    tanh4 = [T, 8, 0, 0, 4, 1, 0, 0]  # a value of 4 elements at slot 8
    return [
        ("cumsum past z", _raw([[C, 8, 5, 0, 4, 1, 0, 0]], 8, z8), "cumsum"),
        ("cumsum past its value", _raw([tanh4, [C, 12, 8, 0, 5, 1, 0, 0]], 8, z8), "cumsum"),
        ("logsumexp past z", _raw([[L, 8, 2, 0, 2, 1, 0, 4]], 8, z8), "logsumexp"),
        ("logsumexp past its value", _raw([tanh4, [L, 12, 8, 0, 2, 1, 0, 3]], 8, z8), "logsumexp"),
        ("logsumexp n * aux wraps int32", _raw([[L, 8, 0, 0, 65536, 1, 0, 65536]], 8, z8), "logsumexp"),
        ("logsumexp aux 0", _raw([[L, 8, 0, 0, 2, 1, 0, 0]], 8, z8), "logsumexp"),
        ("concat aux 0", _raw([[K, 8, 0, ~0, 4, 1, 1, 0]], 8, z8), "concat"),
        ("concat aux n", _raw([[K, 8, 0, ~0, 4, 1, 1, 4]], 8, z8), "concat"),
        ("concat both constant", _raw([[K, 8, ~0, ~4, 4, 1, 1, 2]], 8, z8), "concat"),
        ("concat first part past z", _raw([[K, 8, 6, ~0, 5, 1, 1, 3]], 8, z8), "concat"),
        ("concat constant past the pool", _raw([[K, 8, 0, ~6, 5, 1, 1, 2]], 8, z8), "concat"),
        ("concat z overlap", _raw([[K, 8, 0, 2, 8, 1, 1, 4]], 8, z8), "concat"),
    ]


# ------------------------------------------------------------------------------------------ float32 emulation
def run_host_f32(program, Z):
    """Program.run_host restated in float32 NumPy for every op: values, adjoints, constants and
    every operation in float32 (sums and scans in NumPy's order)."""
    f4 = np.float32
    Z = np.atleast_2d(np.asarray(Z, f4))
    C, S, D = Z.shape[0], program.num_slots, program.dim
    assert Z.shape[1] == D
    cp, ix, names = program.consts, program.index, native.OPCODES
    v = np.zeros((C, S), f4)
    g = np.zeros((C, S), f4)
    v[:, :D] = Z

    def operand(ref, n, stride):
        ln = n if stride else 1
        return v[:, ref:ref + ln] if ref >= 0 else cp[None, ~ref:~ref + ln]

    def fwd(nm, x, y=None):
        if nm == "lgamma":
            return OC._lgamma32(x)
        r = _HOST_FWD[nm](x) if y is None else _HOST_FWD[nm](x, y)
        assert r.dtype == f4, (nm, r.dtype)
        return r

    def rev(nm, gd, x, y, out):
        if nm == "lgamma":
            return gd * OC._digamma32(x), None
        da, db = _host_rev(nm, gd, x, y, out)
        assert da.dtype == f4 and (db is None or db.dtype == f4), (nm, da.dtype)
        return da, db

    ops = program.ops.tolist()
    with np.errstate(all="ignore"):
        for op, dst, a, b, n, sa, sb, aux in ops:
            nm = names[op]
            if nm in _UNARY:
                v[:, dst:dst + n] = fwd(nm, operand(a, n, sa))
            elif nm in _BINARY:
                v[:, dst:dst + n] = fwd(nm, operand(a, n, sa), operand(b, n, sb))
            elif nm == "reduce_sum":
                v[:, dst] = v[:, a:a + n].sum(1)
            elif nm == "gather":
                v[:, dst:dst + n] = v[:, a + ix[aux:aux + n]]
            elif nm == "matvec":
                M = cp[~b:~b + n * aux].reshape(n, aux)
                v[:, dst:dst + n] = v[:, a:a + aux] @ M.T
            elif nm == "cumsum":
                v[:, dst:dst + n] = np.cumsum(v[:, a:a + n], 1, dtype=f4)
            elif nm == "logsumexp":
                x = v[:, a:a + n * aux].reshape(C, n, aux)
                m = x.max(2)
                m = np.where(np.isfinite(m), m, f4(0.0))
                r = np.log(np.exp(x - m[..., None]).sum(2, dtype=f4)) + m
                assert r.dtype == f4
                v[:, dst:dst + n] = r
            else:
                assert nm == "concat", nm
                v[:, dst:dst + aux] = operand(a, aux, 1)
                v[:, dst + aux:dst + n] = operand(b, n - aux, 1)
        g[:, S - 1] = 1.0
        for op, dst, a, b, n, sa, sb, aux in reversed(ops):
            nm = names[op]
            gd = g[:, dst:dst + (1 if nm == "reduce_sum" else n)]
            if nm in _UNARY or nm in _BINARY:
                x = operand(a, n, sa)
                y = operand(b, n, sb) if nm in _BINARY else None
                da, db = rev(nm, gd, x, y, v[:, dst:dst + n])
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
            elif nm == "cumsum":
                g[:, a:a + n] += np.cumsum(gd[:, ::-1], 1, dtype=f4)[:, ::-1]
            elif nm == "logsumexp":
                x, out = v[:, a:a + n * aux].reshape(C, n, aux), v[:, dst:dst + n]
                w = np.where(out[..., None] == -np.inf, f4(0.0), np.exp(x - out[..., None]))
                d = gd[..., None] * w
                assert d.dtype == f4
                g[:, a:a + n * aux] += d.reshape(C, n * aux)
            else:
                if a >= 0:
                    g[:, a:a + aux] += gd[:, :aux]
                if b >= 0:
                    g[:, b:b + n - aux] += gd[:, aux:]
    return v[:, S - 1].astype(np.float64), g[:, :D].astype(np.float64)


# ------------------------------------------------------------------------------------------ models
_HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)


class _Np:
    """The array functions of the log-space statement, in NumPy."""

    log, exp, logaddexp, cumsum = np.log, np.exp, np.logaddexp, staticmethod(lambda x: np.cumsum(x, -1))
    lgamma = staticmethod(np.vectorize(math.lgamma, otypes=[np.float64]))

    @staticmethod
    def cat(parts):
        return np.concatenate(parts, -1)

    @staticmethod
    def logsumexp(x):
        m = x.max(-1, keepdims=True)
        return np.log(np.exp(x - m).sum(-1)) + m[..., 0]

    @staticmethod
    def const(x):
        return np.asarray(x, np.float64)


class _Torch:
    """The same functions in torch (float64), for the gradient by autograd."""

    log, exp, logaddexp, lgamma = torch.log, torch.exp, torch.logaddexp, torch.lgamma
    cumsum = staticmethod(lambda x: torch.cumsum(x, -1))

    @staticmethod
    def cat(parts):
        return torch.cat(parts, -1)

    @staticmethod
    def logsumexp(x):
        return torch.logsumexp(x, -1)

    @staticmethod
    def const(x):
        return torch.as_tensor(np.asarray(x, np.float64))


def _stick_log(xp, u):
    """(log x [C, K], log|J| [C]) of u [C, K - 1]: t = u - log(K - 1 - k), log z = -softplus(-t),
    log(1 - z) = -softplus(t), log x = (log z, 0) + (0, cumsum log(1 - z)),
    log|J| = sum(log x[:-1] + log(1 - z))."""
    m = u.shape[-1]
    t = u - xp.const(np.log(np.arange(m, 0, -1.0)))
    zero = t[..., :1] * 0.0
    log_z, log_1mz = -xp.logaddexp(-t, zero), -xp.logaddexp(t, zero)
    logx = xp.cat([log_z, zero]) + xp.cat([zero, xp.cumsum(log_1mz)])
    return logx, (logx[..., :-1] + log_1mz).sum(-1)


def _dirichlet_log(xp, a, logx):
    return ((a - 1.0) * logx).sum(-1) + xp.lgamma(a.sum(-1)) - xp.lgamma(a).sum(-1)


class Model:
    """A compiled-model case: ``model(*args)`` with numpyro_amd's primitives, its unconstrained
    dimension, and the two float64 references over rows of Z (sites in sorted order)."""

    def __init__(self, name, model, args, dim, logspace, torch_dist, simplex=None):
        self.name, self.model, self.args, self.dim = name, model, args, dim
        self._logspace, self._torch_dist = logspace, torch_dist
        self.simplex = simplex  # the columns of Z that are the simplex site's coordinates

    def min_weight(self, Z):
        """The smallest stick-breaking weight over the rows of Z (1 for a model without a simplex)."""
        if self.simplex is None:
            return 1.0
        return float(td.StickBreakingTransform()(torch.as_tensor(np.asarray(Z, np.float64)[:, self.simplex])).min())

    def torch_reference(self, Z):
        """(U, dU/dz) by torch.distributions in float64."""
        zt = torch.tensor(np.asarray(Z, np.float64), requires_grad=True)
        U = self._torch_dist(zt)
        (G,) = torch.autograd.grad(U.sum(), zt)
        return U.detach().numpy().copy(), G.numpy().copy()

    def logspace_reference(self, Z):
        """(U, dU/dz): U of the log-space statement in NumPy; the gradient by autograd of the same
        statement in torch, whose U is asserted equal to NumPy's."""
        Z = np.asarray(Z, np.float64)
        U = self._logspace(_Np, Z)
        zt = torch.tensor(Z, requires_grad=True)
        Ut = self._logspace(_Torch, zt)
        (G,) = torch.autograd.grad(Ut.sum(), zt)
        np.testing.assert_allclose(Ut.detach().numpy(), U, rtol=1e-12, atol=1e-12)
        return U, G.numpy().copy()


def _counts_data(K, N, seed):
    return np.random.RandomState(seed).randint(0, K, N)


def dirichlet_categorical(K, N=40):
    a = np.linspace(0.6, 2.5, K).astype(np.float32).astype(np.float64)  # constants are float32 numbers
    y = _counts_data(K, N, K)

    def model(y):
        w = numpyro.sample("w", dist.Dirichlet(a))
        numpyro.sample("y", dist.Categorical(probs=w), obs=y)

    def logspace(xp, Z):
        logx, lj = _stick_log(xp, Z)
        return -(_dirichlet_log(xp, xp.const(a), logx) + lj + logx[..., y].sum(-1))

    def torch_dist(Z):
        tr = td.StickBreakingTransform()
        x = tr(Z)
        lp = td.Dirichlet(torch.as_tensor(a)).log_prob(x) + tr.log_abs_det_jacobian(Z, x)
        return -(lp + td.Categorical(probs=x).log_prob(torch.as_tensor(y)[:, None]).sum(0))

    return Model(f"dirichlet_categorical.K{K}", model, (y,), K - 1, logspace, torch_dist, slice(0, K - 1))


def dirichlet_symbolic(K=4, N=30):
    """s ~ HalfNormal(2) (a positive site: u = log s), w ~ Dirichlet(0.5 + s a0).  Sorted: s, w."""
    a0 = np.linspace(0.5, 1.5, K).astype(np.float32).astype(np.float64)
    y = _counts_data(K, N, 100 + K)

    def model(y):
        s = numpyro.sample("s", dist.HalfNormal(2.0))
        w = numpyro.sample("w", dist.Dirichlet(0.5 + s * a0))
        numpyro.sample("y", dist.Categorical(probs=w), obs=y)

    def logspace(xp, Z):
        u = Z[..., 0]
        s = xp.exp(u)
        lp = -0.5 * (s / 2.0) ** 2 - math.log(2.0) + 0.5 * math.log(2.0 / math.pi) + u
        logx, lj = _stick_log(xp, Z[..., 1:])
        a = 0.5 + s[..., None] * xp.const(a0)
        return -(lp + _dirichlet_log(xp, a, logx) + lj + logx[..., y].sum(-1))

    def torch_dist(Z):
        u = Z[:, 0]
        s = torch.exp(u)
        tr = td.StickBreakingTransform()
        x = tr(Z[:, 1:])
        lp = td.HalfNormal(torch.tensor(2.0, dtype=torch.float64)).log_prob(s) + u
        lp = lp + td.Dirichlet(0.5 + s[:, None] * torch.as_tensor(a0)).log_prob(x) + tr.log_abs_det_jacobian(Z[:, 1:], x)
        return -(lp + td.Categorical(probs=x).log_prob(torch.as_tensor(y)[:, None]).sum(0))

    return Model(f"dirichlet_symbolic.K{K}", model, (y,), K, logspace, torch_dist, slice(1, K))


def categorical_logits(K=7, N=50):
    y = _counts_data(K, N, 200 + K)

    def model(y):
        b = numpyro.sample("b", dist.Normal(np.zeros(K), 2.0 * np.ones(K)))
        numpyro.sample("y", dist.Categorical(logits=b), obs=y)

    def logspace(xp, Z):
        lp = (-0.5 * (Z / 2.0) ** 2 - math.log(2.0) - _HALF_LOG_2PI).sum(-1)
        return -(lp + Z[..., y].sum(-1) - y.size * xp.logsumexp(Z))

    def torch_dist(Z):
        lp = td.Normal(torch.zeros(K, dtype=torch.float64), 2.0).log_prob(Z).sum(1)
        return -(lp + td.Categorical(logits=Z).log_prob(torch.as_tensor(y)[:, None]).sum(0))

    return Model(f"categorical_logits.K{K}", model, (y,), K, logspace, torch_dist)


def normal_mixture(N, K):
    """w ~ Dirichlet(2), mu ~ Normal(0, 5)^K, sigma ~ HalfNormal(2)^K, y ~ sum_k w_k Normal(mu_k,
    sigma_k).  Sorted: mu [K], sigma [K] (u = log sigma), w [K - 1]."""
    y = np.random.RandomState(300 + N).normal(0.0, 3.0, N).astype(np.float32).astype(np.float64)  # as the device holds it
    a = 2.0 * np.ones(K)

    def model(y):
        w = numpyro.sample("w", dist.Dirichlet(a))
        mu = numpyro.sample("mu", dist.Normal(np.zeros(K), 5.0 * np.ones(K)))
        sigma = numpyro.sample("sigma", dist.HalfNormal(2.0 * np.ones(K)))
        numpyro.sample("y", dist.MixtureSameFamily(dist.Categorical(probs=w), dist.Normal(mu, sigma)), obs=y)

    def logspace(xp, Z):
        mu, u = Z[..., :K], Z[..., K:2 * K]
        sig = xp.exp(u)
        lp = (-0.5 * (mu / 5.0) ** 2 - math.log(5.0) - _HALF_LOG_2PI).sum(-1)
        lp = lp + (-0.5 * (sig / 2.0) ** 2 - math.log(2.0) + 0.5 * math.log(2.0 / math.pi) + u).sum(-1)
        logx, lj = _stick_log(xp, Z[..., 2 * K:])
        lp = lp + _dirichlet_log(xp, xp.const(a), logx) + lj
        yy = xp.const(y)[:, None]  # [N, 1] against [C, 1, K]
        comp = -0.5 * ((yy - mu[..., None, :]) / sig[..., None, :]) ** 2 - u[..., None, :] - _HALF_LOG_2PI
        return -(lp + xp.logsumexp(comp + logx[..., None, :]).sum(-1))

    def torch_dist(Z):
        mu, u = Z[:, :K], Z[:, K:2 * K]
        sig = torch.exp(u)
        tr = td.StickBreakingTransform()
        x = tr(Z[:, 2 * K:])
        lp = td.Normal(torch.zeros(K, dtype=torch.float64), 5.0).log_prob(mu).sum(1)
        lp = lp + (td.HalfNormal(torch.tensor(2.0, dtype=torch.float64)).log_prob(sig) + u).sum(1)
        lp = lp + td.Dirichlet(torch.as_tensor(a)).log_prob(x) + tr.log_abs_det_jacobian(Z[:, 2 * K:], x)
        mix = td.MixtureSameFamily(td.Categorical(probs=x), td.Normal(mu, sig))
        return -(lp + mix.log_prob(torch.as_tensor(y)[:, None]).sum(0))

    return Model(f"normal_mixture.N{N}K{K}", model, (y,), 3 * K - 1, logspace, torch_dist, slice(2 * K, 3 * K - 1))


MODELS = {
    **{f"dirichlet_categorical.K{K}": functools.partial(dirichlet_categorical, K) for K in (2, 3, 65, 130)},
    "dirichlet_symbolic.K4": dirichlet_symbolic,
    "categorical_logits.K7": categorical_logits,
    **{f"normal_mixture.N{N}K{K}": functools.partial(normal_mixture, N, K) for N, K in ((5, 3), (70, 5), (7, 65))},
}


# torch.distributions clamps probabilities at the float64 epsilon (Categorical's probs -> logits;
# StickBreakingTransform clips its sigmoid likewise), so it is a reference only where every
# stick-breaking weight is far above 2.2e-16.  At Z ~ U(-8, 8) a weight of K components is at least
# prod_k sigmoid(-8 - log(K - 1 - k)) over K - 1 sticks: above e^-27.3 = 1.4e-12 for K <= 4 and below
# the epsilon from K = 6.  These models are compared with torch.distributions at R = 8 (every model
# is at R = 2); the others with the log-space statement, which the same test holds to
# torch.distributions wherever that is valid.
TORCH_VALID_WEIGHT = 1e-12
TORCH_AT_8 = ("dirichlet_categorical.K2", "dirichlet_categorical.K3", "dirichlet_symbolic.K4", "categorical_logits.K7",
              "normal_mixture.N5K3")


def wide_rows(dim, R, rows=200, seed=31):
    return np.random.RandomState(seed).uniform(-R, R, (rows, dim)).astype(np.float32).astype(np.float64)
