"""Shared pieces of the count-likelihood tests (tests/test_count.py on the host interpreter,
tests/test_gpu_count.py on the device): the distributions of numpyro_amd.distributions' count family
with every parameter a latent site and their exact laws by scipy.stats, the models whose float32
accuracy is at stake, hand-assembled programs of the two special ops (lrising, logaddexp) in the
manner of tests/program_op_cases.py, and the draw cases with their exact pmfs.

Conventions.  scipy's ``nbinom(n, p)`` counts failures before n successes, so for
GammaPoisson(c, rate) its success probability is rate / (1 + rate); ``geom`` starts at 1.  The lrising
op is R(a, k) = lgamma(a + k) - lgamma(a) - k log(a) (include/numpyro_amd.h)."""
import collections
import functools
import math

import numpy as np
import scipy.special as sp
import scipy.stats as st

import numpyro_amd as numpyro
import draw_cases as DC
import program_op_cases as OC
from numpyro_amd import distributions as dist
from numpyro_amd import jnp


def f32(x):
    """float32 numbers as float64: what host and device both hold exactly."""
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def sigmoid(x):
    return np.exp(-np.logaddexp(0.0, -np.asarray(x, np.float64)))


# ------------------------------------------------------------------------------ 1: the exact log masses
Y = np.array([0.0, 0.0, 1.0, 0.0, 3.0, 17.0, 0.0, 250.0])  # y = 0 and y > 0
TOTAL = np.array([1.0, 1.0, 1.0, 5.0, 5.0, 40.0, 300.0, 300.0])  # total_count of the (beta-)binomial cases, >= Y
GATES = (1e-12, 0.3, 1.0 - 1e-6)
GATE_LOGITS = (-40.0, 0.0, 40.0)

_PRIOR = {"pos": lambda: dist.LogNormal(0.0, 3.0), "unit": lambda: dist.Beta(1.0, 1.0),
          "real": lambda: dist.Normal(0.0, 50.0)}
# unconstrained coordinate of a constrained value, and the prior's log density + log|J| there (scipy)
_UNCONSTRAIN = {"pos": np.log, "unit": lambda p: np.log(p) - np.log1p(-p), "real": lambda x: x}


def _log_nb(y, c, rate):
    return st.nbinom.logpmf(y, c, rate / (1.0 + rate))


def _zero_inflate(lp, y, log_gate, log_1m):
    """The zero-inflated log mass from the base's, in float64, without forming 1 - gate."""
    return np.where(y == 0, np.logaddexp(log_gate, log_1m + lp), log_1m + lp)


def _gate(t):
    return np.log(t["gate"]), np.log1p(-t["gate"])


def _gate_logits(t):
    return -np.logaddexp(0.0, -t["gl"]), -np.logaddexp(0.0, t["gl"])


MassCase = collections.namedtuple("MassCase", "name kinds grid make law")
# name -> (parameter kinds, grid of values per parameter, distribution of a dict of parameters,
# float64 log mass by scipy at (dict of [S, 1] arrays, y [N]))
_C = (0.3, 7.5, 2e3)
_M = (0.5, 40.0)
_P = (0.02, 0.4, 0.97)
_L = (-3.0, 0.5, 4.0)
MASS_CASES = [
    MassCase("gamma_poisson", {"c": "pos", "r": "pos"}, {"c": _C, "r": (0.05, 3.0)},
             lambda t: dist.GammaPoisson(t["c"], t["r"]), lambda t, y: _log_nb(y, t["c"], t["r"])),
    MassCase("nb2", {"m": "pos", "c": "pos"}, {"m": _M, "c": _C},
             lambda t: dist.NegativeBinomial2(t["m"], t["c"]), lambda t, y: _log_nb(y, t["c"], t["c"] / t["m"])),
    MassCase("nb_probs", {"n": "pos", "p": "unit"}, {"n": _C, "p": _P},
             lambda t: dist.NegativeBinomial(t["n"], probs=t["p"]), lambda t, y: st.nbinom.logpmf(y, t["n"], 1.0 - t["p"])),
    MassCase("nb_logits", {"n": "pos", "l": "real"}, {"n": _C, "l": _L},
             lambda t: dist.NegativeBinomial(t["n"], logits=t["l"]),
             lambda t, y: st.nbinom.logpmf(y, t["n"], sigmoid(-t["l"]))),
    MassCase("beta_binomial", {"a": "pos", "b": "pos"}, {"a": (0.1, 5.0, 1e4), "b": (0.1, 5.0, 1e4)},
             lambda t: dist.BetaBinomial(t["a"], t["b"], TOTAL), lambda t, y: st.betabinom.logpmf(y, TOTAL, t["a"], t["b"])),
    MassCase("geometric_probs", {"p": "unit"}, {"p": _P},
             lambda t: dist.Geometric(probs=t["p"]), lambda t, y: st.geom.logpmf(y + 1.0, t["p"])),
    MassCase("geometric_logits", {"l": "real"}, {"l": _L},
             lambda t: dist.Geometric(logits=t["l"]), lambda t, y: st.geom.logpmf(y + 1.0, sigmoid(t["l"]))),
    # ---- zero-inflated: every base of the list, the gate as a probability or as logits
    MassCase("zi_poisson", {"gate": "unit", "r": "pos"}, {"gate": GATES, "r": (0.05, 3.0, 40.0)},
             lambda t: dist.ZeroInflatedPoisson(t["gate"], t["r"]),
             lambda t, y: _zero_inflate(st.poisson.logpmf(y, t["r"]), y, *_gate(t))),
    MassCase("zi_poisson_logits", {"gl": "real", "r": "pos"}, {"gl": GATE_LOGITS, "r": (0.05, 40.0)},
             lambda t: dist.ZeroInflatedDistribution(dist.Poisson(t["r"]), gate_logits=t["gl"]),
             lambda t, y: _zero_inflate(st.poisson.logpmf(y, t["r"]), y, *_gate_logits(t))),
    MassCase("zi_nb2", {"gate": "unit", "m": "pos", "c": "pos"}, {"gate": GATES, "m": _M, "c": _C},
             lambda t: dist.ZeroInflatedNegativeBinomial2(t["m"], t["c"], gate=t["gate"]),
             lambda t, y: _zero_inflate(_log_nb(y, t["c"], t["c"] / t["m"]), y, *_gate(t))),
    MassCase("zi_nb2_logits", {"gl": "real", "m": "pos", "c": "pos"}, {"gl": GATE_LOGITS, "m": _M, "c": _C},
             lambda t: dist.ZeroInflatedNegativeBinomial2(t["m"], t["c"], gate_logits=t["gl"]),
             lambda t, y: _zero_inflate(_log_nb(y, t["c"], t["c"] / t["m"]), y, *_gate_logits(t))),
    MassCase("zi_gamma_poisson", {"gate": "unit", "c": "pos", "r": "pos"}, {"gate": GATES, "c": _C, "r": (0.05, 3.0)},
             lambda t: dist.ZeroInflatedDistribution(dist.GammaPoisson(t["c"], t["r"]), gate=t["gate"]),
             lambda t, y: _zero_inflate(_log_nb(y, t["c"], t["r"]), y, *_gate(t))),
    MassCase("zi_nb_probs", {"gl": "real", "n": "pos", "p": "unit"}, {"gl": GATE_LOGITS, "n": _C, "p": _P},
             lambda t: dist.ZeroInflatedDistribution(dist.NegativeBinomialProbs(t["n"], t["p"]), gate_logits=t["gl"]),
             lambda t, y: _zero_inflate(st.nbinom.logpmf(y, t["n"], 1.0 - t["p"]), y, *_gate_logits(t))),
    MassCase("zi_nb_logits", {"gate": "unit", "n": "pos", "l": "real"}, {"gate": GATES, "n": _C, "l": _L},
             lambda t: dist.ZeroInflatedDistribution(dist.NegativeBinomialLogits(t["n"], t["l"]), gate=t["gate"]),
             lambda t, y: _zero_inflate(st.nbinom.logpmf(y, t["n"], sigmoid(-t["l"])), y, *_gate(t))),
    MassCase("zi_geometric_probs", {"gate": "unit", "p": "unit"}, {"gate": GATES, "p": _P},
             lambda t: dist.ZeroInflatedDistribution(dist.GeometricProbs(t["p"]), gate=t["gate"]),
             lambda t, y: _zero_inflate(st.geom.logpmf(y + 1.0, t["p"]), y, *_gate(t))),
    MassCase("zi_geometric_logits", {"gl": "real", "l": "real"}, {"gl": GATE_LOGITS, "l": _L},
             lambda t: dist.ZeroInflatedDistribution(dist.GeometricLogits(t["l"]), gate_logits=t["gl"]),
             lambda t, y: _zero_inflate(st.geom.logpmf(y + 1.0, sigmoid(t["l"])), y, *_gate_logits(t))),
    MassCase("zi_binomial_probs", {"gate": "unit", "p": "unit"}, {"gate": GATES, "p": _P},
             lambda t: dist.ZeroInflatedDistribution(dist.Binomial(TOTAL, probs=t["p"]), gate=t["gate"]),
             lambda t, y: _zero_inflate(st.binom.logpmf(y, TOTAL, t["p"]), y, *_gate(t))),
    MassCase("zi_binomial_logits", {"gl": "real", "l": "real"}, {"gl": GATE_LOGITS, "l": _L},
             lambda t: dist.ZeroInflatedDistribution(dist.Binomial(TOTAL, logits=t["l"]), gate_logits=t["gl"]),
             lambda t, y: _zero_inflate(st.binom.logpmf(y, TOTAL, sigmoid(t["l"])), y, *_gate_logits(t))),
    MassCase("zi_beta_binomial", {"gate": "unit", "a": "pos", "b": "pos"},
             {"gate": GATES, "a": (0.1, 5.0, 1e4), "b": (0.1, 1e4)},
             lambda t: dist.ZeroInflatedDistribution(dist.BetaBinomial(t["a"], t["b"], TOTAL), gate=t["gate"]),
             lambda t, y: _zero_inflate(st.betabinom.logpmf(y, TOTAL, t["a"], t["b"]), y, *_gate(t))),
]
MASS = {c.name: c for c in MASS_CASES}
assert len(MASS) == len(MASS_CASES)


def mass_model(case):
    """Every parameter a latent site (sorted by name, as the compilers lay them out), y observed."""
    def model(y):
        t = {k: numpyro.sample(k, _PRIOR[kind]()) for k, kind in sorted(case.kinds.items())}
        numpyro.sample("y", case.make(t), obs=y)
    model.__name__ = f"{case.name}_model"
    return model


def mass_grid(case):
    """{parameter: [S] float64} of the full grid of the case's parameter values."""
    names = sorted(case.grid)
    mesh = np.meshgrid(*[np.asarray(case.grid[k], np.float64) for k in names], indexing="ij")
    return {k: m.reshape(-1) for k, m in zip(names, mesh)}


def mass_reference(case, samples):
    """[S, N] float64 log mass of Y by scipy.stats at the samples {parameter: [S]}."""
    with np.errstate(all="ignore"):
        return np.asarray(case.law({k: np.asarray(v, np.float64)[:, None] for k, v in samples.items()}, Y), np.float64)


def mass_reference_rounding(case, samples):
    """[S, 1] bound of the rounding of scipy's own log masses: they are sums of gammaln / betaln
    values of the concentrations plus the counts, 8 ulp of the largest of which is allowed (at
    concentrations of 1e4 the terms are 1e5 and a beta-binomial log mass can be -1e-5: measured
    against 50-digit arithmetic scipy is 2e-6 off there in relative terms, the interpreter 4e-12)."""
    top = sum(np.asarray(samples[k], np.float64) for k, kind in case.kinds.items() if kind == "pos") \
        if "pos" in case.kinds.values() else np.zeros(1)
    return (8.0 * np.finfo(np.float64).eps * sp.gammaln(top + max(Y.max(), TOTAL.max()) + 2.0))[:, None]


def unconstrain(case, samples):
    """Z [S, dim] of the samples, the sites in sorted order."""
    return np.stack([_UNCONSTRAIN[case.kinds[k]](np.asarray(samples[k], np.float64)) for k in sorted(case.kinds)], 1)


def moderate(case, S=6, seed=0):
    """S random parameter rows away from the extremes (the gradient test)."""
    rs = np.random.RandomState(seed + sum(map(ord, case.name)))
    draw = {"pos": lambda: np.exp(rs.uniform(-1.5, 3.0, S)), "unit": lambda: rs.uniform(0.05, 0.95, S),
            "real": lambda: rs.uniform(-3.0, 3.0, S)}
    return {k: draw[case.kinds[k]]() for k in sorted(case.kinds)}


# ------------------------------------------------------------------------------ 4, 7: the float32 corners
Y1000 = np.array([0.0, 1.0, 3.0, 10.0, 30.0, 100.0, 300.0, 1000.0])  # N = 8, counts up to 1000
Y30 = np.array([0.0, 0.0, 1.0, 2.0, 3.0, 7.0, 12.0, 30.0])
# The concentrations at which the float32 restatement meets U_TOL / G_TOL with counts up to 1000.  The
# issue's grid starts at 0.05 and 1; there the terms y log(mu) and (phi + y) log1p(mu / phi) are 6000
# each at y = 1000 against a U of 60, and their float32 roundings alone (3e-4 each) pass U_TOL's 7e-4
# (DESIGN.md "Count likelihoods"): no float32 sum of such terms can meet it, and at phi = 5 the
# restatement still misses it at N = 65 (1.05e-2 against 9.3e-3 at U = 920).  Those two corners move
# to the data with counts up to 30 (PHIS_SMALL), the bottom of this grid is 10, the others stay.
PHIS = (10.0, 30.0, 1e3, 1e5)
PHIS_SMALL = (0.05, 1.0)
INTERCEPTS = (1.0, 3.0, 4.5, 6.0)
BB_CONCENTRATIONS = (0.1, 5.0, 1e4)
# totals up to 100: at a concentration c of 0.1 a rising factorial over n steps is n log(n / c), and
# one float32 rounding of such a term must stay below U_TOL's 1e-4: 6e-8 x 100 log(1000) = 4e-5,
# while n = 300 gives 1.4e-4 per term, three of which make up an observation
BB_TOTAL = np.array([1.0, 5.0, 5.0, 40.0, 40.0, 100.0, 100.0, 100.0])
BB_Y = np.array([0.0, 0.0, 3.0, 17.0, 40.0, 35.0, 0.0, 64.0])


def nb_regression(y):
    b = numpyro.sample("b", dist.Normal(3.0, 2.0))
    phi = numpyro.sample("phi", dist.LogNormal(3.0, 3.0))
    numpyro.sample("y", dist.NegativeBinomial2(jnp.exp(b), phi), obs=y)


def beta_binomial_model(n, y):
    a = numpyro.sample("a", dist.LogNormal(1.0, 3.0))
    b = numpyro.sample("b", dist.LogNormal(1.0, 3.0))
    numpyro.sample("y", dist.BetaBinomial(a, b, n), obs=y)


def zi_poisson_model(y):
    b = numpyro.sample("b", dist.Normal(1.0, 2.0))
    gate = numpyro.sample("gate", dist.Beta(1.0, 1.0))
    numpyro.sample("y", dist.ZeroInflatedPoisson(gate, jnp.exp(b)), obs=y)


def zi_nb2_logits_model(y):
    b = numpyro.sample("b", dist.Normal(1.0, 2.0))
    gl = numpyro.sample("gl", dist.Normal(0.0, 50.0))
    phi = numpyro.sample("phi", dist.LogNormal(1.0, 2.0))
    numpyro.sample("y", dist.ZeroInflatedNegativeBinomial2(jnp.exp(b), phi, gate_logits=gl), obs=y)


def _logit(p):
    return math.log(p) - math.log1p(-p)


Corner = collections.namedtuple("Corner", "name model args Z")


@functools.lru_cache(maxsize=None)
def corners():
    """The corner rows of item 4, per model: Z [rows, dim] of float32 numbers, sites in sorted order."""
    nb = [[b, math.log(phi)] for phi in PHIS for b in INTERCEPTS]
    nb_small = [[b, math.log(phi)] for phi in PHIS_SMALL for b in (-1.0, 1.0, 3.0)]
    bb = [[math.log(a), math.log(b)] for a in BB_CONCENTRATIONS for b in BB_CONCENTRATIONS]
    zip_ = [[b, _logit(g)] for g in GATES for b in (-1.0, 1.0, 3.0)]
    zinb = [[b, gl, math.log(phi)] for gl in GATE_LOGITS for b in (-1.0, 2.0) for phi in (0.5, 50.0)]
    return (Corner("nb_regression", nb_regression, (Y1000,), f32(nb)),
            Corner("nb_regression_small_phi", nb_regression, (Y30,), f32(nb_small)),
            Corner("beta_binomial", beta_binomial_model, (BB_TOTAL, BB_Y), f32(bb)),
            Corner("zi_poisson", zi_poisson_model, (Y30,), f32(zip_)),
            Corner("zi_nb2_logits", zi_nb2_logits_model, (Y30,), f32(zinb)))


def random_rows(corner, n=64, seed=5):
    """n rows of U(-2, 2) around the middle of the corner rows, as float32 numbers."""
    rs = np.random.RandomState(seed)
    return f32(np.median(corner.Z, 0)[None, :] + rs.uniform(-2.0, 2.0, (n, corner.Z.shape[1])))


def observed_at(corner, N):
    """The corner's model with observed vectors of N elements: the data cycled from its fifth
    observation, a middle count, which is the one observation of N = 1 (the first is a zero, which
    folds the rising factorial away; the last, 1000 alone, is a U of 10 made of terms of 6000, beyond
    float32 at U_TOL for the reason given at PHIS).  A wave's lane edge is crossed at N = 65."""
    return tuple(np.resize(np.roll(a, -4), N) for a in corner.args)


# ------------------------------------------------------------------------------ 3, 8: the two ops alone
OP_SIZES = (1, 63, 64, 65, 130)
RISING_A = (1e-3, 0.5, 1.0, 7.5, 50.0, 1e3, 1e5, 1e7)
RISING_K = (0.0, 1.0, 2.0, 9.0, 100.0, 1e4, 1e6)
LAE_GAPS = (0.0, 1e-3, 20.0, 200.0, np.inf)  # inf: the partner is -inf


def rising_reference(a, k):
    """lgamma(a + k) - lgamma(a) - k log(a) by scipy.special.gammaln in float64, and the bound of
    that difference's own rounding: 4 ulp of each of its three terms (gammaln is good to an ulp or
    two; at a = 1e7 the terms are 1.5e8 and the value can be 1e-7)."""
    a, k = np.asarray(a, np.float64), np.asarray(k, np.float64)
    t = (sp.gammaln(a + k), sp.gammaln(a), k * np.log(a))
    return t[0] - t[1] - t[2], 4.0 * np.finfo(np.float64).eps * (np.abs(t[0]) + np.abs(t[1]) + np.abs(t[2]))


def _values_slot(A, values):
    """A computed value holding `values` [ROWS, n]: 0.5 * z with z = 2 values (exact in float32)."""
    values = np.asarray(values, np.float64)
    return A.ew("mul", A.z(values.shape[1], None, values=2.0 * values), A.const([0.5], 0))


def _special(A, name, a, b, n, fn):
    return A._emit(name, a.ref, b.ref, n, a.stride, b.stride, 0, n, fn)


def rising_values(n):
    """(a [ROWS, n], k [n]) walking the grid: k by element, a by element block and row, so that
    from n = 7 on the 16 rows meet every pair."""
    i = np.arange(n)
    k = np.asarray(RISING_K)[(i + n) % len(RISING_K)]
    a = np.asarray(RISING_A)[(i[None, :] // len(RISING_K) + np.arange(OC.ROWS)[:, None]) % len(RISING_A)]
    return f32(a), f32(k)


RISING_LAYOUTS = ("slot-cvec", "slot-cscalar", "z3-cvec", "sslot-cvec", "zs-cscalar")
LAE_LAYOUTS = ("slot-slot", "slot-cvec", "slot-cscalar", "cvec-slot", "sslot-slot", "z3-slot")


def rising_case(layout, n):
    """lrising(a, k) in one operand layout; ``expect`` is the weighted sum of the scipy reference
    and its rounding bound."""
    ka, kb = layout.split("-")
    A = OC.Asm(f"lrising.{layout}.n{n}", "special")
    a_val, k_val = rising_values(n)
    if ka in ("sslot", "zs"):
        a_val = a_val[:, :1]
    if kb == "cscalar":
        k_val = k_val[:1]
    if ka in ("z3", "zs"):
        A.pad()
    if ka == "slot":
        a = _values_slot(A, a_val)
    elif ka == "sslot":
        a = _values_slot(A, a_val).broadcast()
    else:
        a = A.z(a_val.shape[1], None, stride=int(ka == "z3"), values=a_val)
    k = A.const(k_val, int(kb == "cvec"))
    case = A.case(_special(A, "lrising", a, k, n, None))
    ref, err = rising_reference(a_val, k_val[None, :])
    w = OC.weights(n)[None, :]
    case.expect = ((w * ref).sum(1), (w * err).sum(1))
    return case


def rising_slot_k(n=5):
    """lrising with k in a slot: nmx_program_check must refuse it."""
    A = OC.Asm("lrising.slot-slot", "refused")
    a = _values_slot(A, np.full((OC.ROWS, n), 2.0))
    k = _values_slot(A, np.full((OC.ROWS, n), 3.0))
    return A.case(_special(A, "lrising", a, k, n, None))


def lae_values(n):
    """(x, y) [ROWS, n]: x in [-3, 3], y = x - gap with the gaps by element and row; every other
    element swapped; (-inf, -inf) where the gap is inf and the element is a multiple of 5."""
    i = np.arange(n)[None, :]
    r = np.arange(OC.ROWS)[:, None]
    x = np.linspace(-3.0, 3.0, OC.ROWS * max(n, 2)).reshape(max(n, 2), OC.ROWS).T[:, :n].copy()
    gap = np.asarray(LAE_GAPS)[(i + r) % len(LAE_GAPS)]
    y = x - gap
    x = np.where(np.isinf(gap) & ((i + r) % 2 == 0) & (i % 5 == 0), -np.inf, x)
    swap = (i + r // len(LAE_GAPS)) % 2 == 1
    return f32(np.where(swap, y, x)), f32(np.where(swap, x, y))


def lae_case(layout, n):
    """exp(logaddexp(x, y)) in one operand layout (the exp keeps a -inf result out of the weighted
    sum and carries the zero adjoint of a (-inf, -inf) pair); ``expect`` by np.logaddexp."""
    ka, kb = layout.split("-")
    A = OC.Asm(f"logaddexp.{layout}.n{n}", "special")
    x_val, y_val = lae_values(n)
    if ka == "sslot":
        x_val = x_val[:, :1]
    if ka == "cvec":
        x_val = x_val[:1]
    if kb == "cvec":
        y_val = y_val[:1]
    if kb == "cscalar":
        y_val = y_val[:1, :1]
    if ka == "z3":
        A.pad()

    def operand(kind, val):
        if kind == "slot":
            return _values_slot(A, val)
        if kind == "sslot":
            return _values_slot(A, val).broadcast()
        if kind == "z3":
            return A.z(val.shape[1], None, values=val)
        return A.const(val[0], int(kind == "cvec"))

    x = operand(ka, x_val)
    y = operand(kb, y_val)
    case = A.case(A.ew("exp", _special(A, "logaddexp", x, y, n, None)))
    with np.errstate(all="ignore"):
        ref = np.exp(np.logaddexp(np.broadcast_to(x_val, (OC.ROWS, n)), np.broadcast_to(y_val, (OC.ROWS, n))))
    case.expect = ((OC.weights(n)[None, :] * ref).sum(1), 0.0)
    return case


@functools.lru_cache(maxsize=None)
def op_cases():
    return tuple([rising_case(lay, n) for n in OP_SIZES for lay in RISING_LAYOUTS] +
                 [lae_case(lay, n) for n in OP_SIZES for lay in LAE_LAYOUTS])


# ------------------------------------------------------------------------------ 5: the draws and their laws
class ZeroInflatedLaw:
    """The pieces of a frozen scipy law that draw_cases.chi_square reads, for gate + (1 - gate) base."""

    def __init__(self, base, gate):
        self.base, self.gate = base, float(gate)

    def support(self):
        return self.base.support()

    def pmf(self, k):
        k = np.asarray(k, np.float64)
        return (1.0 - self.gate) * self.base.pmf(k) + self.gate * (k == 0)

    def cdf(self, k):
        k = np.asarray(k, np.float64)
        return np.where(k >= 0, self.gate + (1.0 - self.gate) * self.base.cdf(k), 0.0)

    def ppf(self, q):
        q = np.asarray(q, np.float64)
        inner = np.clip((q - self.gate) / (1.0 - self.gate), 0.0, 1.0)
        return np.where(q <= self.gate, 0.0, np.maximum(self.base.ppf(inner), 0.0))


def _nb2_law(mean, c):
    return st.nbinom(c, c / (c + mean))


_D = "discrete"
DRAW_CASES = [
    DC.Case("nb2_0p3", "count", "count", lambda: dist.NegativeBinomial2(4.0, 0.3), _nb2_law(4.0, 0.3), _D, False),
    DC.Case("nb2_50", "count", "count", lambda: dist.NegativeBinomial2(30.0, 50.0), _nb2_law(30.0, 50.0), _D, False),
    DC.Case("gamma_poisson", "count", "count", lambda: dist.GammaPoisson(2.5, 0.5), st.nbinom(2.5, 0.5 / 1.5), _D, False),
    DC.Case("nb_probs", "count", "count", lambda: dist.NegativeBinomial(5.0, probs=0.4), st.nbinom(5.0, 0.6), _D, False),
    DC.Case("nb_logits", "count", "count", lambda: dist.NegativeBinomial(5.0, logits=_logit(0.4)), st.nbinom(5.0, 0.6),
            _D, False),
    DC.Case("geometric_0p02", "count", "count", lambda: dist.Geometric(probs=0.02), st.geom(0.02, loc=-1), _D, False),
    DC.Case("geometric_logits", "count", "count", lambda: dist.Geometric(logits=_logit(0.3)), st.geom(0.3, loc=-1), _D,
            False),
    DC.Case("beta_binomial_1", "count", "count", lambda: dist.BetaBinomial(0.7, 1.5, 1), st.betabinom(1, 0.7, 1.5), _D,
            False),
    DC.Case("beta_binomial_40", "count", "count", lambda: dist.BetaBinomial(2.0, 3.0, 40), st.betabinom(40, 2.0, 3.0), _D,
            False),
    # rates on both sides of POISSON_PTRS_RATE = 10
    DC.Case("zi_poisson_3", "count", "count", lambda: dist.ZeroInflatedPoisson(0.3, 3.0),
            ZeroInflatedLaw(st.poisson(3.0), 0.3), _D, False),
    DC.Case("zi_poisson_40", "count", "count", lambda: dist.ZeroInflatedPoisson(0.3, 40.0),
            ZeroInflatedLaw(st.poisson(40.0), 0.3), _D, False),
    DC.Case("zi_nb2_logits", "count", "count",
            lambda: dist.ZeroInflatedNegativeBinomial2(12.0, 2.0, gate_logits=_logit(0.2)),
            ZeroInflatedLaw(_nb2_law(12.0, 2.0), 0.2), _D, False),
    DC.Case("zi_beta_binomial", "count", "count",
            lambda: dist.ZeroInflatedDistribution(dist.BetaBinomial(2.0, 3.0, 40), gate=0.25),
            ZeroInflatedLaw(st.betabinom(40, 2.0, 3.0), 0.25), _D, False),
]
DRAW_UPPER = {"beta_binomial_1": 1, "beta_binomial_40": 40, "zi_beta_binomial": 40}


def draw_model():
    with numpyro.plate("n", DC.ELEMENTS):
        for c in DRAW_CASES:
            numpyro.sample(c.name, c.make())


@functools.lru_cache(maxsize=None)
def host_draws(seed, dtype):
    """{site: [SAMPLES, ELEMENTS]} of draw_model on the host interpreter in `dtype`."""
    import predictive_cases as PC
    from numpyro_amd.predictive_program import compile_predictive

    prog = compile_predictive(draw_model, (), {}, [])
    assert prog.dim == 0 and prog.native_check() == (0, ""), prog.native_check()
    assert all(o.integer for o in prog.outputs)
    out = prog.run_host(DC.SAMPLES, seed, PC.words, dtype=dtype)
    for v in out.values():
        v.setflags(write=False)
    return out


def check_draws(draws_at, log=print):
    """draw_cases.check_family's decision rule over DRAW_CASES: a case misses when its p-value is
    at or below DC.LEVEL at both seeds; a NaN draw is a miss.  Every draw is whole, non-negative and
    at most its total_count."""
    missed = []
    for case in DRAW_CASES:
        ps = []
        for seed in DC.SEEDS:
            x = np.asarray(draws_at(seed)[case.name], np.float64)
            text, p, nan = DC.case_pvalue(case, x)
            log(f"{case.name} seed {seed}: {text}, p = {p:.3g}" + (f", NaN share {nan:.2e}" if nan else ""))
            ok = bool(np.all(x == np.floor(x)) and x.min() >= 0 and x.max() <= DRAW_UPPER.get(case.name, np.inf))
            if nan or not ok:
                missed.append((case.name, "NaN share" if nan else "outside the support", nan))
            ps.append(p)
            if p > DC.LEVEL:
                break
        else:
            missed.append((case.name, ps))
    assert not missed, missed
