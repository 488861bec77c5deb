"""Models with bounded-support latents and Binomial likelihoods for the program potential's and
the predictive programs' tests, in the style of tests/program_zoo.py: each model is written
twice, with numpyro_amd's primitives and independently as a hand-written torch potential of the
unconstrained coordinates (textbook densities and bijections, no use of the compiler; gradients
by autograd).  The four models of the reference's examples/baseball.py are cases, on the 18
players of Efron and Morris (1975), and a scale with a Uniform prior is the fifth.

Site lists are [(name, shape, transform code)] in sorted order, as every Potential.sites."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import numpyro_amd as numpyro
from numpyro_amd import distributions as dist
from numpyro_amd import jnp
from numpyro_amd.potentials import LOWER, POSITIVE, REAL, UNIT
from program_zoo import Case

# Efron and Morris (1975), Table 1: the first 45 at bats of the 1970 season (Clemente ... Alvis)
AT_BATS = np.full(18, 45.0)
HITS = np.array([18, 17, 16, 15, 14, 14, 13, 12, 11, 11, 10, 10, 10, 10, 10, 9, 8, 7], np.float64)

_HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)


# ---- log densities and log-Jacobians, written out
def _log_binomial(k, n, log_p, log_1mp):
    return (torch.lgamma(n + 1.0) - torch.lgamma(k + 1.0) - torch.lgamma(n - k + 1.0)
            + k * log_p + (n - k) * log_1mp)


def _log_beta(log_x, log_1mx, a, b):
    return (a - 1.0) * log_x + (b - 1.0) * log_1mx + torch.lgamma(a + b) - torch.lgamma(a) - torch.lgamma(b)


def _sigmoid_site(u):
    """(log x, log(1 - x), log|dx/du|) of x = sigmoid(u)."""
    lx, l1 = F.logsigmoid(u), F.logsigmoid(-u)
    return lx, l1, lx + l1


# ---- the four models of examples/baseball.py
def fully_pooled(at_bats, hits=None):
    phi = numpyro.sample("phi", dist.Uniform(0, 1))
    with numpyro.plate("num_players", at_bats.shape[0]):
        return numpyro.sample("obs", dist.Binomial(at_bats, probs=phi), obs=hits)


def _fully_pooled_u(s, d):
    lx, l1, jac = _sigmoid_site(s["phi"])  # Uniform(0, 1): log density 0
    return -(_log_binomial(d["hits"], d["at_bats"], lx, l1).sum() + jac)


def not_pooled(at_bats, hits=None):
    with numpyro.plate("num_players", at_bats.shape[0]):
        phi = numpyro.sample("phi", dist.Uniform(0, 1))
        return numpyro.sample("obs", dist.Binomial(at_bats, probs=phi), obs=hits)


def _not_pooled_u(s, d):
    lx, l1, jac = _sigmoid_site(s["phi"])
    return -(_log_binomial(d["hits"], d["at_bats"], lx, l1).sum() + jac.sum())


def partially_pooled(at_bats, hits=None):
    m = numpyro.sample("m", dist.Uniform(0, 1))
    kappa = numpyro.sample("kappa", dist.Pareto(1, 1.5))
    with numpyro.plate("num_players", at_bats.shape[0]):
        phi = numpyro.sample("phi", dist.Beta(m * kappa, (1 - m) * kappa))
        return numpyro.sample("obs", dist.Binomial(at_bats, probs=phi), obs=hits)


def _partially_pooled_u(s, d):
    lm, l1m, jac_m = _sigmoid_site(s["m"])
    m = torch.exp(lm)
    kappa = 1.0 + torch.exp(s["kappa"])  # Pareto(1, 1.5): 1.5 * 1^1.5 / kappa^2.5, log|J| = u
    lp = math.log(1.5) - 2.5 * torch.log(kappa) + s["kappa"] + jac_m
    lx, l1, jac = _sigmoid_site(s["phi"])
    one_minus_m = torch.exp(l1m)  # 1 - sigmoid(u) = sigmoid(-u), exact where the subtraction cancels
    lp = lp + (_log_beta(lx, l1, m * kappa, one_minus_m * kappa) + jac).sum()
    return -(lp + _log_binomial(d["hits"], d["at_bats"], lx, l1).sum())


def partially_pooled_with_logit(at_bats, hits=None):
    loc = numpyro.sample("loc", dist.Normal(-1, 1))
    scale = numpyro.sample("scale", dist.HalfCauchy(1))
    with numpyro.plate("num_players", at_bats.shape[0]):
        alpha = numpyro.sample("alpha", dist.Normal(loc, scale))
        return numpyro.sample("obs", dist.Binomial(at_bats, logits=alpha), obs=hits)


def _with_logit_u(s, d):
    scale = torch.exp(s["scale"])
    lp = -0.5 * (s["loc"] + 1.0) ** 2 - _HALF_LOG_2PI
    lp = lp + math.log(2.0 / math.pi) - torch.log1p(scale ** 2) + s["scale"]
    a = s["alpha"]
    lp = lp + (-0.5 * ((a - s["loc"]) / scale) ** 2 - torch.log(scale) - _HALF_LOG_2PI).sum()
    return -(lp + _log_binomial(d["hits"], d["at_bats"], F.logsigmoid(a), F.logsigmoid(-a)).sum())


# ---- a scale with a Uniform prior
SIGMA_LOW, SIGMA_HIGH = 0.5, 6.0
Y_SIGMA = np.random.RandomState(11).normal(1.0, 2.0, 20)


def uniform_sigma(y=None):
    sigma = numpyro.sample("sigma", dist.Uniform(SIGMA_LOW, SIGMA_HIGH))
    with numpyro.plate("n", 20):
        numpyro.sample("y", dist.Normal(1.0, sigma), obs=y)


def _uniform_sigma_u(s, d):
    width = SIGMA_HIGH - SIGMA_LOW
    _, _, jac = _sigmoid_site(s["sigma"])
    sigma = SIGMA_LOW + width * torch.sigmoid(s["sigma"])
    lp = -math.log(width) + jac + math.log(width)  # prior density, log|J| of lo + width sigmoid(u)
    return -(lp + (-0.5 * ((d["y"] - 1.0) / sigma) ** 2 - torch.log(sigma) - _HALF_LOG_2PI).sum())


_BASEBALL = {"at_bats": AT_BATS, "hits": HITS}
CASES = {
    "fully_pooled": lambda: Case("fully_pooled", fully_pooled, (AT_BATS, HITS), [("phi", (), UNIT)],
                                 _fully_pooled_u, _BASEBALL),
    "not_pooled": lambda: Case("not_pooled", not_pooled, (AT_BATS, HITS), [("phi", (18,), UNIT)],
                               _not_pooled_u, _BASEBALL),
    "partially_pooled": lambda: Case("partially_pooled", partially_pooled, (AT_BATS, HITS),
                                     [("kappa", (), LOWER), ("m", (), UNIT), ("phi", (18,), UNIT)],
                                     _partially_pooled_u, _BASEBALL),
    "partially_pooled_with_logit": lambda: Case("partially_pooled_with_logit", partially_pooled_with_logit,
                                                (AT_BATS, HITS),
                                                [("alpha", (18,), REAL), ("loc", (), REAL), ("scale", (), POSITIVE)],
                                                _with_logit_u, _BASEBALL),
    "uniform_sigma": lambda: Case("uniform_sigma", uniform_sigma, (Y_SIGMA,), [("sigma", (), UNIT)],
                                  _uniform_sigma_u, {"y": Y_SIGMA}),
}
# the affine part (lo, width) each case's potential must carry
AFFINE = {"fully_pooled": {"phi": (0.0, 1.0)}, "not_pooled": {"phi": (0.0, 1.0)},
          "partially_pooled": {"m": (0.0, 1.0), "kappa": (1.0, 1.0)}, "partially_pooled_with_logit": {},
          "uniform_sigma": {"sigma": (SIGMA_LOW, SIGMA_HIGH - SIGMA_LOW)}}

EDGE_U = (-30.0, -17.0, 0.0, 17.0, 30.0)


def edge_rows(case, seed=3):
    """Rows with every unit site's coordinates at each of EDGE_U in turn, the other coordinates
    uniform in (-2, 2): [len(EDGE_U) * number of unit sites, dim]."""
    rs = np.random.RandomState(seed)
    rows, o = [], 0
    for _, shape, code in case.sites:
        n = int(np.prod(shape))
        if code == UNIT:
            for u in EDGE_U:
                z = rs.uniform(-2, 2, case.dim)
                z[o:o + n] = u
                rows.append(z)
        o += n
    return np.asarray(rows).reshape(-1, case.dim)


# ---- predictive programs: the Binomial draw with every kind of operand, on both sides of the
# switch between the inversion and BTRS (n q = 10)
PLATE_SIZES = (1, 63, 64, 65, 129)
PLATE_SEED = 5
OPERAND_KINDS = ("scalar", "vector", "broadcast", "constant")


def binomial_plate_model(n, kind):
    """Site "probs" varies the probability's operand kind, site "count" the total count's.  The
    given sites feed the slot operands: s, q, ks are scalars, v and kv vectors of the plate's
    size; ks and kv hold whole numbers (Poisson sites)."""
    def model(counts, probs):
        s = numpyro.sample("s", dist.HalfNormal(1.0))
        q = numpyro.sample("q", dist.Beta(2.0, 2.0))
        ks = numpyro.sample("ks", dist.Poisson(30.0))
        v = numpyro.sample("v", dist.Normal(np.zeros(n), np.ones(n)))
        kv = numpyro.sample("kv", dist.Poisson(np.full(n, 30.0)))
        with numpyro.plate("n", n):
            numpyro.sample("uniform", dist.Uniform(-1.0, 3.0))
            numpyro.sample("pareto", dist.Pareto(2.0, 1.0 + s))
            numpyro.sample("beta", dist.Beta(0.5 + s, jnp.exp(0.5 * v) + 0.3))
            if kind == "scalar":  # one computed slot, written by lane 0 and read by every lane
                numpyro.sample("probs", dist.Binomial(counts, probs=s / (1.0 + s)))
                numpyro.sample("count", dist.Binomial(ks * 2.0, probs=probs))
            elif kind == "vector":  # a computed slot per element
                numpyro.sample("probs", dist.Binomial(counts, probs=jnp.expit(v)))
                numpyro.sample("count", dist.Binomial(kv + 1.0, logits=v))
            elif kind == "broadcast":  # a given scalar site's own slot
                numpyro.sample("probs", dist.Binomial(counts, probs=q))
                numpyro.sample("count", dist.Binomial(ks, probs=probs))
            else:  # constants in the pool
                numpyro.sample("probs", dist.Binomial(counts, probs=probs))
                numpyro.sample("count", dist.Binomial(40, probs=0.26))

    return model


def binomial_plate_inputs(n):
    """(samples of one draw, args): total counts 1 ... 200 and probabilities 0.02 ... 0.98 across
    the plate, so both the inversion and BTRS run, mirrored and not."""
    rs = np.random.RandomState(n)
    samples = {"s": (0.5 + np.abs(rs.randn(1))).astype(np.float32), "q": rs.uniform(0.1, 0.9, 1).astype(np.float32),
               "ks": rs.poisson(30.0, 1).astype(np.float32), "v": rs.randn(1, n).astype(np.float32),
               "kv": rs.poisson(30.0, (1, n)).astype(np.float32)}
    counts = np.round(np.linspace(1.0, 200.0, n)) if n > 1 else np.array([40.0])
    probs = np.linspace(0.02, 0.98, n) if n > 1 else np.array([0.26])
    return samples, (counts, probs)


PLATE_RULES = {"uniform": "exact", "pareto": "monotone", "beta": "calibrated", "probs": "discrete",
               "count": "discrete"}
