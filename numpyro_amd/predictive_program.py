"""Predictive programs: posterior and prior predictive draws for the generic path of the model
front end.

The reference's ``Predictive`` re-runs the model once per posterior sample with the given sites
substituted and every other site sampled (numpyro/infer/util.py:803-885 _predictive, :888-1090).
``compile_predictive`` traces the model once (frontend.trace_model) and lowers that forward run
to a straight-line program of the program compiler's format (numpyro_amd/program.py, the same
builder: folding, sharing and refusals are the same) in which a site that is neither observed
nor given is *drawn*: a draw op fills its slots with base variates (standard normal, exponential,
Cauchy, uniform; gamma(concentration), Bernoulli(probs), Poisson(rate); Binomial(total_count,
probs), the one draw with two parameters) and the existing arithmetic ops
build the distribution from them (``_DRAW``; ``_COUNT_DRAW`` for the count likelihoods: a gamma,
exponential or beta draw feeds a Poisson or binomial draw, a Bernoulli draw of the gate zeroes a
zero-inflated one; the outputs are integer sites, and an element whose mixed rate is at or above
``POISSON_MAX_RATE`` is what ``draw_poisson`` gives there, NaN).  A drawn site's value then parameterises the later
sites, so prior predictive of a hierarchical model runs ``mu -> theta -> obs`` in one program.
One HIP kernel (csrc/predictive_program.hip) runs the program once per posterior sample.

Randomness is the device's Philox stream for predictive draws: element i of sample s of the draw
op with stream id k (its ordinal in the program) uses the blocks ``words(s, k, i, attempt)``; a
draw depends only on (seed, sample, stream, element).  ``PredictiveProgram.run_host`` runs the same
program on the one NumPy forward interpreter (program.py ``Program._forward_host``) and hands it
the draw ops, which are defined here word by word (float64; float32 runs the same arithmetic in
float32, the calibration of the device tests).
"""
from __future__ import annotations

import math

import numpy as np

from . import distributions as dist
from . import native
from .frontend import _base
from .jnp import Sym, shape_of
from .program import (_COUNT_LOGPROB, _LOGPROB, _ZERO_INFLATABLE, _ZERO_INFLATED, _ForwardProgram, _Refuse,
                      _forward_prologue, _logprob_entry, _operand, _refuse)

_U24 = 5.9604644775390625e-08  # 2^-24


# ------------------------------------------------------------------------------------------
# samplers (numpyro/distributions/continuous.py, discrete.py `sample`): base draws + arithmetic
# ------------------------------------------------------------------------------------------
def _dr_normal(B, d, n):
    return d["loc"] + d["scale"] * B.draw("draw_normal", n)


def _dr_student_t(B, d, n):
    # z sqrt(df / chi2(df)), chi2(df) = 2 gamma(df / 2)
    z = B.draw("draw_normal", n)
    g = B.draw("draw_gamma", n, d["df"] * 0.5)
    return d["loc"] + d["scale"] * (z * B.ew("sqrt", d["df"] / (2.0 * g)))


def _dr_cauchy(B, d, n):
    return d["loc"] + d["scale"] * B.draw("draw_cauchy", n)


def _dr_half_cauchy(B, d, n):
    return B.ew("sqrt", B.ew("square", d["scale"] * B.draw("draw_cauchy", n)))


def _dr_half_normal(B, d, n):
    return B.ew("sqrt", B.ew("square", d["scale"] * B.draw("draw_normal", n)))


def _dr_log_normal(B, d, n):
    return B.ew("exp", d["loc"] + d["scale"] * B.draw("draw_normal", n))


def _dr_exponential(B, d, n):
    return B.draw("draw_exponential", n) / d["rate"]


def _dr_gamma(B, d, n):
    return B.draw("draw_gamma", n, d["concentration"]) / d["rate"]


def _dr_bernoulli_logits(B, d, n):
    return B.draw("draw_bernoulli", n, 1.0 / (1.0 + B.ew("exp", -d["logits"])))


def _dr_bernoulli_probs(B, d, n):
    return B.draw("draw_bernoulli", n, d["probs"])


def _dr_poisson(B, d, n):
    rate = d["rate"]
    if rate.is_const and np.any(rate.c >= native.POISSON_MAX_RATE):
        raise NotImplementedError(f"a rate of {rate.c.max():g} (2^24 or more: counts are float32 whole numbers)")
    return B.draw("draw_poisson", n, rate)


def _dr_uniform(B, d, n):
    return d["low"] + (d["high"] - d["low"]) * B.draw("draw_uniform", n)


def _dr_pareto(B, d, n):
    # scale exp(E / alpha), E standard exponential (continuous.py:2230 Pareto as a transformed Exponential)
    return d["scale"] * B.ew("exp", B.draw("draw_exponential", n) / d["alpha"])


def _dr_beta(B, d, n):
    # g1 / (g1 + g0) of two gamma draws; where both underflow to 0 (concentrations far below 1)
    # this is 0 / 0 = NaN (DESIGN.md "Predictive programs")
    g1 = B.draw("draw_gamma", n, d["concentration1"])
    g0 = B.draw("draw_gamma", n, d["concentration0"])
    return g1 / (g1 + g0)


def _binomial_count(d):
    n = d["total_count"]
    if n.is_const and np.any(n.c >= native.BINOMIAL_MAX_COUNT):
        raise NotImplementedError(f"a total_count of {n.c.max():g} (2^24 or more: counts are float32 whole numbers)")
    return n


def _dr_binomial_probs(B, d, n):
    return B.draw("draw_binomial", n, _binomial_count(d), d["probs"])


def _dr_binomial_logits(B, d, n):
    return B.draw("draw_binomial", n, _binomial_count(d), 1.0 / (1.0 + B.ew("exp", -d["logits"])))


def _dr_dirichlet(B, d, n):
    # normalised gamma draws; where every draw underflows to 0 (concentrations far below 1) this is
    # 0 / 0 = NaN, as _dr_beta
    a = d["concentration"]
    if a.n != n or n < 2:
        raise NotImplementedError(f"a Dirichlet of {n} components with a concentration of {a.n} elements (supported: "
                                  "one vector of K >= 2 components)")
    g = B.draw("draw_gamma", n, a)
    return g / B.rsum(g)


_DRAW = {
    dist.Normal: _dr_normal, dist.StudentT: _dr_student_t, dist.Cauchy: _dr_cauchy,
    dist.HalfCauchy: _dr_half_cauchy, dist.HalfNormal: _dr_half_normal, dist.LogNormal: _dr_log_normal,
    dist.Exponential: _dr_exponential, dist.Gamma: _dr_gamma, dist.BernoulliLogits: _dr_bernoulli_logits,
    dist.BernoulliProbs: _dr_bernoulli_probs, dist.Poisson: _dr_poisson,
    dist.Uniform: _dr_uniform, dist.Beta: _dr_beta, dist.Pareto: _dr_pareto,
    dist.BinomialProbs: _dr_binomial_probs, dist.BinomialLogits: _dr_binomial_logits,
    dist.Dirichlet: _dr_dirichlet,
}
# drawing one of these needs an index that depends on a draw (the category, the component): the
# program has no such op, so they are supported with data only
_UNDRAWABLE = (dist.CategoricalProbs, dist.CategoricalLogits, dist.MixtureSameFamily, dist.MultivariateNormal)
assert set(_DRAW) | set(_UNDRAWABLE) == set(_LOGPROB) and not set(_DRAW) & set(_UNDRAWABLE)


# ---- the count likelihoods (program.py _COUNT_LOGPROB), composed from the draw ops above: a gamma
# (or exponential, or beta) draw of the latent rate (probability) feeds a Poisson (binomial) draw.
# The mixed rate is itself random: where it reaches POISSON_MAX_RATE = 2^24 the element is what
# draw_poisson documents there, NaN.  Kept apart from _DRAW, whose keys the draw tests pin.
def _dr_gamma_poisson(B, d, n):
    return B.draw("draw_poisson", n, B.draw("draw_gamma", n, d["concentration"]) / d["rate"])


def _dr_negative_binomial2(B, d, n):
    c = d["concentration"]
    return B.draw("draw_poisson", n, B.draw("draw_gamma", n, c) * (d["mean"] / c))


def _dr_negative_binomial_probs(B, d, n):
    p = d["probs"]  # 1 / rate = p / (1 - p)
    return B.draw("draw_poisson", n, B.draw("draw_gamma", n, d["total_count"]) * (p / (1.0 - p)))


def _dr_negative_binomial_logits(B, d, n):
    return B.draw("draw_poisson", n, B.draw("draw_gamma", n, d["total_count"]) * B.ew("exp", d["logits"]))


def _dr_geometric_probs(B, d, n):
    # the negative binomial of total_count 1: its gamma draw is an exponential one
    p = d["probs"]
    return B.draw("draw_poisson", n, B.draw("draw_exponential", n) * ((1.0 - p) / p))


def _dr_geometric_logits(B, d, n):
    return B.draw("draw_poisson", n, B.draw("draw_exponential", n) * B.ew("exp", -d["logits"]))


def _dr_beta_binomial(B, d, n):
    return B.draw("draw_binomial", n, _binomial_count(d), _dr_beta(B, d, n))


_COUNT_DRAW = {
    dist.GammaPoisson: _dr_gamma_poisson, dist.NegativeBinomial2: _dr_negative_binomial2,
    dist.NegativeBinomialProbs: _dr_negative_binomial_probs, dist.NegativeBinomialLogits: _dr_negative_binomial_logits,
    dist.GeometricProbs: _dr_geometric_probs, dist.GeometricLogits: _dr_geometric_logits,
    dist.BetaBinomial: _dr_beta_binomial,
}
assert set(_COUNT_DRAW) | set(_ZERO_INFLATED) | {dist.ZeroInflatedPoisson} == set(_COUNT_LOGPROB)
assert set(_ZERO_INFLATABLE) <= set(_DRAW) | set(_COUNT_DRAW)


def _dr_zero_inflated(B, lower, base, n, site):
    """(1 - b) * the base's draw, b a Bernoulli draw of the gate."""
    inner = _base(base.base_dist)
    if not isinstance(inner, _ZERO_INFLATABLE):
        _refuse(site, f"a zero-inflated {type(inner).__name__} (supported bases: "
                      f"{', '.join(t.__name__ for t in _ZERO_INFLATABLE)})")
    d = {p: lower.vector(getattr(inner, p), site) for p in _logprob_entry(inner)[1]}
    if isinstance(base, dist.ZeroInflatedLogits):
        gate = 1.0 / (1.0 + B.ew("exp", -lower.vector(base.gate_logits, site)))
    else:
        gate = lower.vector(base.gate, site)
    for p, val in list(d.items()) + [("gate", B.const(gate))]:
        if val.n not in (1, n):
            _refuse(site, f"parameter {p!r} of {val.n} elements at a site of {n}")
    b = B.draw("draw_bernoulli", n, gate)
    return (1.0 - b) * (_DRAW.get(type(inner)) or _COUNT_DRAW[type(inner)])(B, d, n)


_INTEGER = (dist.BernoulliLogits, dist.BernoulliProbs, dist.Poisson, dist.BinomialProbs, dist.BinomialLogits,
            dist.CategoricalProbs, dist.CategoricalLogits) + tuple(_COUNT_LOGPROB)


class Output:
    """A site the program computes: ``n`` tape slots from ``slot``, of the site's ``shape``;
    ``streams`` are the stream ids of the site's own draw ops."""

    def __init__(self, name, slot, n, shape, integer, streams=()):
        self.name, self.slot, self.n, self.shape = name, int(slot), int(n), tuple(shape)
        self.integer, self.streams = bool(integer), tuple(streams)

    def __iter__(self):  # (name, slot, n, shape, integer?)
        return iter((self.name, self.slot, self.n, self.shape, self.integer))

    def __repr__(self):
        return f"{self.name}: slots [{self.slot}, {self.slot + self.n}) shape {self.shape}" + \
            (" int" if self.integer else "")


def _sym_latents(x, out):
    if isinstance(x, Sym):
        if x.op == "latent":
            out.add(x.args[0])
        else:
            for a in (x.args[:1] if x.op == "getitem" else x.args):
                _sym_latents(a, out)
    return out


class PredictiveProgram(_ForwardProgram):
    """A forward-only program with draw ops (program.py _ForwardProgram): ``outputs`` are the drawn
    sites and the deterministic sites that depend on one; ``observed`` the sites that keep their data
    (name -> (data, integer?)) and ``host_deterministics`` the deterministic expressions of given
    sites alone."""

    _CHECK = "nmx_predict_program_check"

    def __init__(self, ops, consts, index, num_slots, dim, inputs, outputs, observed, host_deterministics):
        super().__init__(ops, consts, index, num_slots, dim, inputs, outputs)
        self.observed, self.host_deterministics = dict(observed), dict(host_deterministics)

    @property
    def num_draws(self):
        return int((self.ops[:, 0] >= native.DRAW_BASE).sum())

    def output_table(self):
        return np.ascontiguousarray(np.asarray([[o.slot, o.n] for o in self.outputs], np.int32).reshape(-1, 2))

    # ------------------------------------------------------------------ NumPy interpreter
    def run_host(self, samples, seed, words, dtype=np.float64, sample_offset=0, info=None):
        """The program on every row of ``samples`` (see flatten_inputs) in ``dtype`` arithmetic:
        {output site: [S, *shape]} as ``dtype`` arrays (an integer site holds whole numbers, or NaN
        where the draw is undefined).  ``words(seed, sample, stream, element, attempt)`` ->
        [..., 4] uint32 are the Philox blocks of nmx_rng(seed, sample, stream, NMX_EV_PREDICT,
        element, attempt) over broadcasting index arrays (this module does not generate them: the
        tests pass the oracle's Philox).  ``info``, a dict, receives {stream id: accepted attempt
        [S, n]} of every draw op (-1: none).  The draw ops are defined here word by word; the
        kernel's header (csrc/nmx_program.h, include/numpyro_amd.h) states the same assignment."""
        T = np.dtype(dtype).type
        Z, cp = self.flatten_inputs(samples, dtype), self._pool(dtype)
        S = Z.shape[0]
        rows = (np.arange(S, dtype=np.int64) + int(sample_offset))[:, None]

        def blocks(stream, n, attempt):
            return np.asarray(words(seed, rows, stream, np.arange(n, dtype=np.int64)[None, :], attempt), np.uint32)

        def draw(nm, op, v):
            _, dst, a, b, n, sa, sb, aux = op
            par = None if nm in _NO_PARAM else np.broadcast_to(_operand(v, cp, a, n, sa), (S, n))
            if nm == "draw_binomial":
                par = (par, np.broadcast_to(_operand(v, cp, b, n, sb), (S, n)))
            steps = {}
            out, att = _host_draw(nm, par, lambda t: blocks(aux, n, t), (S, n), T, steps)
            v[:, dst:dst + n] = out
            if info is not None:
                info[aux] = att
                if steps:  # the inversion walk's step count per element (binomial)
                    info[("steps", aux)] = steps["steps"]

        v = self._forward_host(Z, dtype, cp, draw)
        return {o.name: v[:, o.slot:o.slot + o.n].reshape((S,) + o.shape).copy() for o in self.outputs}


def _u01(x, T):
    return (x >> np.uint32(8)).astype(T) * T(_U24)


def _u01_open0(x, T):
    return ((x >> np.uint32(8)).astype(T) + T(1.0)) * T(_U24)


def _box_muller(w, T):
    rad = np.sqrt(T(-2.0) * np.log(_u01_open0(w[..., 0], T)))
    return rad * np.cos(T(6.283185307179586) * _u01(w[..., 1], T))


_NO_PARAM = ("draw_normal", "draw_exponential", "draw_cauchy", "draw_uniform")


def _host_draw(name, par, blocks, shape, T, steps=None):
    """(values, accepted attempt) of one draw op over [S, n]; `blocks(t)` are attempt t's words."""
    nan = T(np.nan)
    att = np.zeros(shape, np.int32)
    if name == "draw_uniform":
        return _u01(blocks(0)[..., 0], T), att
    if name == "draw_binomial":
        return _host_binomial(par[0], par[1], blocks, T, steps)
    if name == "draw_normal":
        return _box_muller(blocks(0), T), att
    if name == "draw_exponential":
        return -np.log(_u01_open0(blocks(0)[..., 0], T)), att
    if name == "draw_cauchy":
        u = ((blocks(0)[..., 0] >> np.uint32(8)).astype(T) + T(0.5)) * T(_U24)
        return np.tan(T(math.pi) * (u - T(0.5))), att
    if name == "draw_bernoulli":
        ok = (par >= 0) & (par <= 1)
        return np.where(ok, (_u01(blocks(0)[..., 0], T) < par).astype(T), nan), np.where(ok, 0, -1).astype(np.int32)
    if name == "draw_gamma":
        return _host_gamma(par, blocks, T)
    return _host_poisson(par, blocks, T)


def _host_gamma(a, blocks, T):
    """Marsaglia & Tsang (2000), one block per attempt: normal (x, y), accept uniform z, boost w."""
    ok = (a > 0) & np.isfinite(a)
    boost = a < 1
    a1 = np.where(boost, a + T(1.0), a)
    d = a1 - T(1.0) / T(3.0)
    c = T(1.0) / np.sqrt(T(9.0) * d)
    out = np.full(a.shape, np.nan, T)
    att = np.full(a.shape, -1, np.int32)
    pending = ok.copy()
    for t in range(native.DRAW_MAX_ATTEMPTS):
        if not pending.any():
            break
        w = blocks(t)
        x = _box_muller(w, T)
        y = T(1.0) + c * x
        vv = y * y * y
        acc = pending & (y > 0) & (np.log(_u01_open0(w[..., 2], T)) < T(0.5) * x * x + d - d * vv + d * np.log(vv))
        g = np.where(boost, d * vv * np.exp(np.log(_u01_open0(w[..., 3], T)) / a), d * vv)
        out[acc] = g[acc]
        att[acc] = t
        pending &= ~acc
    return out, att


def _host_poisson(rate, blocks, T):
    """rate < 10: inversion of one uniform; else Hoermann's PTRS (1993), one block per attempt;
    NaN before any loop unless 0 <= rate < NMX_POISSON_MAX_RATE."""
    ok = (rate >= 0) & (rate < T(native.POISSON_MAX_RATE))
    out = np.full(rate.shape, np.nan, T)
    att = np.full(rate.shape, -1, np.int32)
    zero = ok & (rate == 0)
    out[zero], att[zero] = 0, 0
    small = ok & (rate > 0) & (rate < T(native.POISSON_PTRS_RATE))
    if small.any():
        u = _u01(blocks(0)[..., 0], T)
        p = np.exp(-rate)
        total = p.copy()
        k = np.zeros(rate.shape, T)
        pending = small.copy()
        for _ in range(native.POISSON_MAX_STEPS):
            done = pending & (u <= total)
            out[done], att[done] = k[done], 0
            pending &= ~done
            if not pending.any():
                break
            k = k + T(1.0)
            p = p * rate / k
            total = total + p
            done = pending & (p < T(2.0 ** -40)) & (k > rate)
            out[done], att[done] = k[done], 0
            pending &= ~done
    pending = ok & (rate >= T(native.POISSON_PTRS_RATE))
    if pending.any():
        b = T(0.931) + T(2.53) * np.sqrt(rate)
        a = T(-0.059) + T(0.02483) * b
        inv_alpha = T(1.1239) + T(1.1328) / (b - T(3.4))
        v_r = T(0.9277) - T(3.6224) / (b - T(2.0))
        for t in range(native.DRAW_MAX_ATTEMPTS):
            if not pending.any():
                break
            w = blocks(t)
            U = _u01(w[..., 0], T) - T(0.5)
            V = _u01_open0(w[..., 1], T)
            us = T(0.5) - np.abs(U)
            k = np.floor((T(2.0) * a / us + b) * U + rate + T(0.43))
            fast = (us >= T(0.07)) & (V <= v_r)
            rej = ~(k >= 0) | ((us < T(0.013)) & (V > us))
            # log pmf(k) = -rate + k log rate - log k! with log k! as the Stirling formula at k + 1 plus
            # its tail: the terms of size k log k cancel inside the log1p, not in the sum
            k1 = np.where(k >= 0, k, T(0.0)) + T(1.0)
            log_pmf = k * np.log1p((rate - k1) / k1) - (rate - k1) - T(0.5) * np.log(k1) - \
                T(0.9189385332046727) - _stirling_tail(k1 - T(1.0), T)
            slow = np.log(V * inv_alpha / (a / (us * us) + b)) <= log_pmf
            acc = pending & (fast | (~rej & slow))
            out[acc], att[acc] = k[acc], t
            pending &= ~acc
    return out, att


_STIRLING_TAIL = (0.08106146679532726, 0.04134069595540929, 0.02767792568499834, 0.02079067210376509,
                  0.01664469118982119, 0.01387612882307075, 0.01189670994589177, 0.01041126526197209,
                  0.009255462182712733, 0.008330563433362871)


def _stirling_tail(j, T):
    """log(j!) minus the Stirling formula at j + 1 (j >= 0 whole): table below 10, else the series."""
    table = np.asarray(_STIRLING_TAIL, T)
    small = j < T(10.0)
    r = T(1.0) / (np.where(small, T(10.0), j) + T(1.0))
    r2 = r * r
    series = (T(1.0) / T(12) - (T(1.0) / T(360) - (T(1.0) / T(1260)) * r2) * r2) * r
    return np.where(small, table[np.where(small, j, 0).astype(np.int64)], series)


def _fma(x, y, z, T):
    """x y + z rounded once (fmaf): two float32 factors have an exact float64 product."""
    if T is np.float32:
        return (x.astype(np.float64) * y.astype(np.float64) + np.asarray(z, np.float64)).astype(np.float32)
    return x * y + z


def _host_binomial(n, p, blocks, T, steps=None):
    """q = min(p, 1 - p); n q < 10: inversion of one uniform; else Hoermann's BTRS (1993), one
    block per attempt (include/numpyro_amd.h NMX_DRAW_BINOMIAL states the assignment)."""
    ok = (p >= 0) & (p <= 1) & (n >= 0) & (n < T(native.BINOMIAL_MAX_COUNT)) & (n == np.floor(n))
    out = np.full(n.shape, np.nan, T)
    att = np.full(n.shape, -1, np.int32)
    walked = np.zeros(n.shape, np.int32)
    fixed = ok & ((p == 0) | (n == 0))
    out[fixed], att[fixed] = 0, 0
    fixed = ok & (p == 1) & (n != 0)
    out[fixed], att[fixed] = n[fixed], 0
    live = ok & (p > 0) & (p < 1) & (n > 0)
    mirror = p > T(0.5)
    q = np.where(live, np.where(mirror, T(1.0) - p, p), T(0.25)).astype(T)
    nn = np.where(live, n, T(1.0)).astype(T)
    mu, log1_q = nn * q, np.log1p(-q)

    def put(mask, k):
        out[mask] = np.where(mirror, nn - k, k)[mask]

    small = live & (mu < T(native.BINOMIAL_BTRS_MEAN))
    if small.any():
        u = _u01(blocks(0)[..., 0], T)
        odds = q / (T(1.0) - q)
        f = np.exp(nn * log1_q)
        total = f.copy()
        k = np.zeros(n.shape, T)
        pending = small.copy()
        for _ in range(native.BINOMIAL_MAX_STEPS):
            done = pending & ((u <= total) | (k >= nn))
            put(done, k)
            att[done] = 0
            pending &= ~done
            if not pending.any():
                break
            walked[pending] += 1
            k = k + T(1.0)
            f = f * (nn - k + T(1.0)) / k * odds
            total = total + f
            done = pending & (f < T(2.0 ** -40)) & (k > mu)
            put(done, k)
            att[done] = 0
            pending &= ~done
    pending = live & ~small
    if pending.any():
        spq, c = np.sqrt(mu * (T(1.0) - q)), mu + T(0.5)
        b = T(1.15) + T(2.53) * spq
        a = T(-0.0873) + T(0.0248) * b + T(0.01) * q
        alpha, v_r = (T(2.83) + T(5.1) / b) * spq, T(0.92) - T(4.2) / b
        m = np.floor((nn + T(1.0)) * q)

        def log_odds(j):
            # log((n - j + 1) q / ((j + 1) (1 - q))) as the log1p of ((n + 2) q - (j + 1)) / ((j + 1) (1 - q)):
            # n q - j is one fused multiply-add, rounded once, where the two logs would cancel
            return np.log1p((_fma(nn, q, -j, T) + (T(2.0) * q - T(1.0))) / ((j + T(1.0)) * (T(1.0) - q)))

        log_h = (_stirling_tail(m, T) + _stirling_tail(nn - m, T)) - (m + T(0.5)) * log_odds(m)
        for t in range(native.DRAW_MAX_ATTEMPTS):
            if not pending.any():
                break
            w = blocks(t)
            U = _u01(w[..., 0], T) - T(0.5)
            V = _u01_open0(w[..., 1], T)
            us = T(0.5) - np.abs(U)
            k = np.floor((T(2.0) * a / us + b) * U + c)
            fast = (us >= T(0.07)) & (V <= v_r)
            inside = (k >= 0) & (k <= nn)
            kk = np.where(inside, k, m)
            log_f = (nn + T(1.0)) * np.log1p((kk - m) / (nn - kk + T(1.0))) + \
                (kk + T(0.5)) * log_odds(kk) + \
                (_stirling_tail(kk, T) - _stirling_tail(nn - kk, T)) + log_h
            slow = np.log(V * alpha / (a / (us * us) + b)) <= log_f
            acc = pending & (fast | (inside & slow))
            put(acc, k)
            att[acc] = t
            pending &= ~acc
    if steps is not None:
        steps["steps"] = walked
    return out, att


# ------------------------------------------------------------------------------------------
# compiler
# ------------------------------------------------------------------------------------------
def compile_predictive(model, args=(), kwargs=None, given=()):
    """Trace ``model(*args, **kwargs)`` and lower its forward run to a PredictiveProgram.  The
    sample sites without data whose name is in ``given`` are the inputs (sorted by name,
    constrained values); every other site without data is drawn.  Raises NotImplementedError
    naming the site for a model outside the program compiler's class."""
    def drawn(s, base):  # a site that has neither data nor a given value
        if isinstance(base, dist.MultivariateNormal):
            _refuse(s.name, "drawing a MultivariateNormal site is not supported (predictive programs have no "
                            "product of a factor with a drawn vector): pass its data, or leave the site out of "
                            "the model")
        if type(base) in _UNDRAWABLE:
            _refuse(s.name, f"drawing a {type(base).__name__} site needs a data-dependent index, which predictive "
                            "programs do not have: pass its data, or leave the site out of the model")

    trace, sizes, inputs, B, values, lower = _forward_prologue(model, args, kwargs, given, drawn)
    outputs, observed = [], {}
    for s in trace.sites.values():
        if s.obs is not None:
            observed[s.name] = (s.obs, isinstance(_base(s.fn), _INTEGER))
            continue
        if s.name in values:
            continue
        base, n = _base(s.fn), sizes[s.name]
        if n > native.DRAW_MAX_ELEMENTS:
            _refuse(s.name, f"a drawn site of {n} elements (more than 2^24, the draw counter's element field)")
        first = B.n_draws
        try:
            d = {p: lower.vector(getattr(base, p), s.name) for p in _logprob_entry(base)[1]}
            for p, val in d.items():
                if val.n not in (1, n):
                    _refuse(s.name, f"parameter {p!r} of {val.n} elements at a site of {n}")
            if isinstance(base, _ZERO_INFLATED):
                val = _dr_zero_inflated(B, lower, base, n, s.name)
            else:
                val = (_DRAW.get(type(base)) or _COUNT_DRAW[type(base)])(B, d, n)
        except _Refuse:
            raise
        except NotImplementedError as e:
            _refuse(s.name, str(e))
        assert not val.is_const and val.n == n
        values[s.name] = val
        outputs.append(Output(s.name, val.slot, n, s.shape, isinstance(base, _INTEGER), range(first, B.n_draws)))
    drawn = {o.name for o in outputs}
    host_dets = {}
    for name, expr in trace.deterministics.items():
        if not (_sym_latents(expr, set()) & drawn):
            host_dets[name] = expr  # given sites alone: evaluated from the samples (frontend.eval_sym)
            continue
        shape = tuple(shape_of(expr))
        if len(shape) > 1:
            _refuse(name, f"deterministic site of shape {shape}: rank > 1 is not supported")
        val = lower(expr, name)
        outputs.append(Output(name, val.slot, val.n, shape, False))
    if not outputs:  # nothing to run on the device: every site is given or observed
        return PredictiveProgram.empty(B.dim, inputs, observed, host_dets)
    prog = PredictiveProgram(*B.forward_arrays(outputs), inputs, outputs, observed, host_dets)
    # stream ids are ordinals both before and after compaction: every draw feeds an output site
    assert prog.ops[prog.ops[:, 0] >= native.DRAW_BASE, 7].tolist() == list(range(B.n_draws))
    return prog
