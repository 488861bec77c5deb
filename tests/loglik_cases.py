"""Shared pieces of the log-likelihood tests (tests/test_loglik_program.py on the host interpreter,
tests/test_gpu_loglik.py on the device): the models of tests/program_zoo.py, tests/bounded_zoo.py
and tests/simplex_cases.py, each with

* unconstrained points Z [S, dim] drawn from U(-3, 3) and their constrained site values (textbook
  bijections, float64), so that every value is strictly inside its support;
* ``reference(samples)``: the elementwise log likelihood of every observed site by
  ``torch.distributions`` in float64, written here from the model's definition (never from the
  compiler's expansions);
* ``potential64(Z)``: the float64 potential of the zoo's own hand-written statement.
"""
import math

import numpy as np
import torch
import torch.distributions as td

import bounded_zoo as BZ
import program_zoo as PZ
import simplex_cases as SC
from numpyro_amd.potentials import LOWER, POSITIVE, REAL, UNIT

_T = torch.as_tensor


class LLCase:
    def __init__(self, name, model, args, sites, constrain, reference, potential64):
        self.name, self.model, self.args = name, model, args
        self.sites = sites  # [(name, unconstrained size, constrained shape)] in sorted order
        self._constrain, self.reference, self.potential64 = constrain, reference, potential64
        self.dim = sum(n for _, n, _ in sites)

    def points(self, S, seed=0):
        """Z [S, dim] ~ U(-3, 3), as float32 numbers (the device holds them exactly)."""
        rs = np.random.RandomState(seed + sum(map(ord, self.name)))
        return rs.uniform(-3.0, 3.0, (S, self.dim)).astype(np.float32).astype(np.float64)

    def constrain(self, Z):
        """{site: [S, *shape]} float64 constrained values of the rows of Z."""
        out, o = {}, 0
        for name, n, shape in self.sites:
            out[name] = self._constrain(name, Z[:, o:o + n]).reshape((Z.shape[0],) + tuple(shape))
            o += n
        return out

    def samples(self, S, seed=0):
        """Constrained values rounded to float32 (what the device is given), as float64 arrays."""
        return {k: v.astype(np.float32).astype(np.float64) for k, v in self.constrain(self.points(S, seed)).items()}


def _sigmoid(u):
    return 1.0 / (1.0 + np.exp(-u))


# ------------------------------------------------------------------------------ program_zoo
def _pz_reference(name, data):
    d = {k: _T(v) for k, v in data.items()}

    def robust8(s):
        return {"obs": td.StudentT(4.0, s["theta"], d["sigma"]).log_prob(d["y"])}

    def poisson(s):
        eta = s["a"][:, d["group"]] + s["b"] @ d["X"].T
        return {"y": td.Poisson(torch.exp(eta)).log_prob(d["y"])}

    def treg(s):
        return {"y": td.StudentT(s["nu"][:, None], s["b"] @ d["X"].T, s["sigma"][:, None]).log_prob(d["y"])}

    def logit(s):
        return {"y": td.Bernoulli(logits=s["b0"][:, None] + s["b"] @ d["X"].T).log_prob(d["y"])}

    def edge(s):
        tau, w, v = s["tau"], s["w"], s["v"]
        sd = torch.sqrt((tau ** 2).sum(1, keepdim=True))
        loc1 = v @ d["M1"].T + tau[:, d["idx1"]]
        return {"y1": td.Normal(loc1, sd).log_prob(d["y1"]),
                "y2": td.Normal(w[:, None] * tau, 1.0).log_prob(d["y2"])}

    return {"robust8": robust8, "poisson": poisson, "treg": treg, "logit": logit, "edge": edge}[name]


def _program_zoo(name):
    c = PZ.CASES[name]()
    positive = {n: p for n, _, p in c.sites}
    sites = [(n, int(np.prod(shape, dtype=np.int64)), tuple(shape)) for n, shape, _ in c.sites]
    return LLCase(name, c.model, c.args, sites, lambda n, u: np.exp(u) if positive[n] else u,
                  _pz_reference(name, c.data), lambda Z: c.pe_grad64(Z)[0])


# ------------------------------------------------------------------------------ bounded_zoo
def _bz_reference(name):
    n, k = _T(BZ.AT_BATS), _T(BZ.HITS)
    if name == "fully_pooled":
        return lambda s: {"obs": td.Binomial(n, probs=s["phi"][:, None].expand(-1, 18)).log_prob(k)}
    if name in ("not_pooled", "partially_pooled"):
        return lambda s: {"obs": td.Binomial(n, probs=s["phi"]).log_prob(k)}
    if name == "partially_pooled_with_logit":
        return lambda s: {"obs": td.Binomial(n, logits=s["alpha"]).log_prob(k)}
    return lambda s: {"y": td.Normal(1.0, s["sigma"][:, None]).log_prob(_T(BZ.Y_SIGMA))}


def _bounded_zoo(name):
    c = BZ.CASES[name]()
    code = {n: t for n, _, t in c.sites}
    affine = BZ.AFFINE[name]

    def constrain(n, u):
        lo, width = affine.get(n, (0.0, 1.0))
        if code[n] == REAL:
            return u
        if code[n] == POSITIVE:
            return np.exp(u)
        if code[n] == UNIT:
            return lo + width * _sigmoid(u)
        assert code[n] == LOWER
        return lo + np.exp(u)

    sites = [(n, int(np.prod(shape, dtype=np.int64)), tuple(shape)) for n, shape, _ in c.sites]
    return LLCase(name, c.model, c.args, sites, constrain, _bz_reference(name), lambda Z: c.pe_grad64(Z)[0])


# ------------------------------------------------------------------------------ simplex_cases
def _stick(u):
    return td.StickBreakingTransform()(_T(u)).numpy()


def _simplex(name):
    if name == "dirichlet_categorical":
        K = 3
        m = SC.dirichlet_categorical(K)
        y = _T(m.args[0])
        sites = [("w", K - 1, (K,))]
        constrain = lambda n, u: _stick(u)  # noqa: E731
        ref = lambda s: {"y": td.Categorical(probs=s["w"]).log_prob(y[:, None]).T}  # noqa: E731
    elif name == "categorical_logits":
        K = 7
        m = SC.categorical_logits(K)
        y = _T(m.args[0])
        sites = [("b", K, (K,))]
        constrain = lambda n, u: u  # noqa: E731
        ref = lambda s: {"y": td.Categorical(logits=s["b"]).log_prob(y[:, None]).T}  # noqa: E731
    else:
        N, K = 70, 5  # 350 table elements: several per lane; rows straddle lanes
        m = SC.normal_mixture(N, K)
        y = _T(m.args[0])
        sites = [("mu", K, (K,)), ("sigma", K, (K,)), ("w", K - 1, (K,))]
        constrain = lambda n, u: u if n == "mu" else np.exp(u) if n == "sigma" else _stick(u)  # noqa: E731

        def ref(s):
            mix = td.MixtureSameFamily(td.Categorical(probs=s["w"]), td.Normal(s["mu"], s["sigma"]))
            return {"y": mix.log_prob(y[:, None]).T}

    return LLCase(name, m.model, m.args, sites, constrain, ref, lambda Z: m.torch_reference(Z)[0])


CASES = {**{n: (lambda n=n: _program_zoo(n)) for n in PZ.CASES},
         **{n: (lambda n=n: _bounded_zoo(n)) for n in BZ.CASES},
         **{n: (lambda n=n: _simplex(n)) for n in ("dirichlet_categorical", "categorical_logits", "normal_mixture")}}


def reference64(case, samples):
    """{site: [S, *shape]} float64 NumPy arrays of case.reference at a dict of NumPy samples."""
    out = case.reference({k: _T(np.asarray(v, np.float64)) for k, v in samples.items()})
    return {k: v.numpy().copy() for k, v in out.items()}


# ------------------------------------------------------------------------------ calibration
U24 = 2.0 ** -24


def scaled_error(x, ref):
    """The largest |x - ref| / (1 + |ref|)."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(x - ref) / (1.0 + np.abs(ref))).max())


def calibrated_bound(r32, r64):
    """The project's calibration rule: 4 x the float32 host run's deviation from the float64 run on
    the same inputs (the factor covers another float32 libm and another order of the sums), plus
    16 x 2^-24."""
    return 4.0 * scaled_error(r32, r64) + 16.0 * U24


# ------------------------------------------------------------------------------ pointwise reductions in NumPy
_F = np.float32
_INF = _F(np.inf)


def _shift(m):
    return np.where(np.abs(m) < _INF, m, _F(0.0))


def _rescale(m, sh):
    return np.where(m == -_INF, _F(0.0), np.exp(_shift(m) - sh))


def _empty(C):
    return [np.full(C, -_INF, _F), np.zeros(C, _F), np.zeros(C, _F), np.zeros(C, _F), 0]


def _push(st, x):
    m, s, mean, m2, n = st
    mn = np.fmax(m, x)  # ignores a NaN entry, as fmaxf
    sh = _shift(mn)
    s = s * _rescale(m, sh) + np.exp(x - sh)
    n += 1
    delta = x - mean
    mean = mean + delta / _F(n)
    m2 = np.where(np.abs(x) < _INF, m2 + delta * (x - mean), _F(np.nan))
    return [mn, s, mean, m2, n]


def _merge(a, b):
    if b[4] == 0:
        return a
    if a[4] == 0:
        return b
    m = np.fmax(a[0], b[0])
    sh = _shift(m)
    s = a[1] * _rescale(a[0], sh) + b[1] * _rescale(b[0], sh)
    n = a[4] + b[4]
    na, nb, nn = _F(a[4]), _F(b[4]), _F(n)
    delta = b[2] - a[2]
    return [m, s, a[2] + delta * (nb / nn), (a[3] + b[3]) + (delta * delta) * (na * nb / nn), n]


def _halve(states):
    """State g with state g + half, the lower first, until one is left."""
    while len(states) > 1:
        half = len(states) // 2
        states = [_merge(states[g], states[g + half]) for g in range(half)]
    return states[0]


def pointwise32(table, chunks=None, max_splits=64, min_split_rows=16):
    """(lppd, p_waic) per column of table [S, C]: the device's reduction restated in float32 NumPy
    with the same states, merges and orders (include/numpyro_amd.h "log-likelihood programs"); only
    exp and log are NumPy's.  ``chunks``: row counts of successive accumulate calls."""
    t = np.asarray(table, _F)
    S, C = t.shape
    cpad = 64
    if C < 64:
        cpad = 1
        while cpad < C:
            cpad *= 2
    G = 64 // cpad
    running, r = _empty(C), 0
    with np.errstate(all="ignore"):
        for rows in (chunks or [S]):
            chunk = t[r:r + rows]
            r += rows
            per = max(min_split_rows, -(-rows // max_splits))
            splits = []
            for r0 in range(0, rows, per):
                part = chunk[r0:r0 + per]
                groups = []
                for g in range(G):  # G = 1 with 64 columns or more: the split's rows in order
                    st = _empty(C)
                    for x in part[g::G]:
                        st = _push(st, x)
                    groups.append(st)
                splits.append(_halve(groups))
            running = _merge(running, _halve(splits + [_empty(C)] * (max_splits - len(splits))))
        assert r == S and running[4] == S
        m, s, mean, m2, n = running
        lppd = (np.log(s) + _shift(m)) - np.log(_F(n))
        p_waic = m2 / _F(n - 1) if n > 1 else np.full(C, np.nan, _F)
    assert lppd.dtype == _F and p_waic.dtype == _F
    return lppd, p_waic


def pointwise64(table):
    """(lppd, p_waic) per column of table [S, N] in float64 NumPy."""
    t = np.asarray(table, np.float64)
    with np.errstate(all="ignore"):
        lppd = np.logaddexp.reduce(t, 0) - math.log(t.shape[0])
        p_waic = t.var(0, ddof=1) if t.shape[0] > 1 else np.full(t.shape[1:], np.nan)
    return lppd, p_waic
