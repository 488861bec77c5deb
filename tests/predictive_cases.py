"""Shared pieces of the predictive-program tests (tests/test_predictive_program.py on the host
interpreter, tests/test_gpu_predictive_program.py on the device): the oracle's Philox as the
interpreter's word source, the zoo models with their observed arguments removed, the comparison
rules of device against host, and the moment checks with their analytic moments."""
import math

import numpy as np

import numpyro_amd as numpyro
from numpyro_amd import distributions as dist
from oracle import philox


def words(seed, sample, stream, element, attempt):
    """The device's predictive stream (csrc/nmx_program.h): nmx_rng(seed, sample, stream, EV_PREDICT, element, attempt)."""
    return philox.rng(seed, sample, stream, philox.EV_PREDICT, element, attempt)


# positions of the observed arguments in Case.args
OBSERVED_ARGS = {"robust8": (2,), "poisson": (2,), "treg": (1,), "logit": (1,), "edge": (2, 3)}
# drawn site -> how its device draws are compared with the float64 host run (compare below)
SITE_RULE = {"robust8": {"obs": "calibrated"}, "poisson": {"y": "discrete"}, "treg": {"y": "calibrated"},
             "logit": {"y": "discrete"}, "edge": {"y1": "monotone", "y2": "monotone"}}


def unobserved_args(case):
    return tuple(None if i in OBSERVED_ARGS[case.name] else a for i, a in enumerate(case.args))


def posterior_like(case, S, seed=0):
    """Constrained values [S, *shape] of every latent site, float32: positive sites in [0.5, ~3]."""
    rs = np.random.RandomState(seed)
    out = {}
    for name, shape, positive in case.sites:
        z = rs.randn(S, *shape)
        out[name] = ((0.5 + np.abs(z) + (2.0 if name == "nu" else 0.0)) if positive else z).astype(np.float32)
    return out


def eight_schools_model(J, sigma, y=None):
    """README.md:47-55."""
    mu = numpyro.sample("mu", dist.Normal(0, 5))
    tau = numpyro.sample("tau", dist.HalfCauchy(5))
    with numpyro.plate("J", J):
        theta = numpyro.sample("theta", dist.Normal(mu, tau))
        numpyro.sample("obs", dist.Normal(theta, sigma), obs=y)


def host_runs(prog, samples, seed):
    """(float64 outputs, float32 outputs, {site: elements whose accept / reject decision differs
    between the two runs}) of the host interpreter."""
    i64, i32 = {}, {}
    r64 = prog.run_host(samples, seed, words, info=i64)
    r32 = prog.run_host(samples, seed, words, dtype=np.float32, info=i32)
    flipped = {}
    for o in prog.outputs:
        f = np.zeros(r64[o.name].shape, bool).reshape(r64[o.name].shape[0], -1)
        for k in o.streams:
            f |= i64[k] != i32[k]
        flipped[o.name] = f.reshape(r64[o.name].shape)
    return r64, r32, flipped


def compare(name, rule, dev, r64, r32, flipped, log=print):
    """Device draws of one site against the float64 host run.
    discrete: equal except a share <= 1e-3.
    monotone (a monotone map of one normal or exponential): |dev - ref| <= 1e-4 (1 + |ref|).
    calibrated (gamma-based and Cauchy sites): |dev - ref| <= 4 x the largest deviation of the
      float32 host run from the float64 one on the same inputs (the factor covers another
      float32 libm), over the elements whose accept / reject decisions agree in both host runs;
      the excluded share must be <= 1e-3."""
    dev, ref = np.asarray(dev, np.float64), np.asarray(r64, np.float64)
    assert dev.shape == ref.shape, (name, dev.shape, ref.shape)
    if rule == "discrete":
        ref = np.where(np.isnan(ref), -1.0, ref)
        share = float((dev != ref).mean())
        log(f"{name}: discrete mismatch share {share:.2e}")
        assert share <= 1e-3, (name, share)
    elif rule == "monotone":
        err = np.abs(dev - ref) / (1.0 + np.abs(ref))
        log(f"{name}: max |dev - ref| / (1 + |ref|) = {err.max():.3e}")
        assert np.all(err <= 1e-4), (name, err.max())
    else:
        keep = ~flipped
        assert 1.0 - keep.mean() <= 1e-3, (name, "accept / reject decisions differ", 1.0 - keep.mean())
        cal = float(np.abs(np.asarray(r32, np.float64) - ref)[keep].max())
        err = float(np.abs(dev - ref)[keep].max())
        log(f"{name}: float32 host deviation {cal:.3e}, device deviation {err:.3e} (bound {4 * cal:.3e}), "
            f"excluded share {1.0 - keep.mean():.2e}")
        assert err <= 4.0 * cal, (name, err, cal)


# ---------------------------------------------------------------------------- moments
MOMENT_SAMPLES, MOMENT_ELEMENTS = 64, 512


def moments_model():
    with numpyro.plate("n", MOMENT_ELEMENTS):
        numpyro.sample("normal", dist.Normal(1.5, 2.0))
        numpyro.sample("lognormal", dist.LogNormal(0.2, 0.5))
        numpyro.sample("halfnormal", dist.HalfNormal(1.5))
        numpyro.sample("exponential", dist.Exponential(2.5))
        numpyro.sample("gamma_below1", dist.Gamma(0.5, 2.0))
        numpyro.sample("gamma_above1", dist.Gamma(3.0, 0.5))
        numpyro.sample("studentt", dist.StudentT(9.0, 1.0, 2.0))
        numpyro.sample("poisson_inversion", dist.Poisson(3.0))
        numpyro.sample("poisson_ptrs", dist.Poisson(40.0))
        numpyro.sample("bernoulli", dist.Bernoulli(probs=0.3))
        numpyro.sample("bernoulli_logits", dist.Bernoulli(logits=-0.4))
        numpyro.sample("cauchy", dist.Cauchy(1.0, 2.0))
        numpyro.sample("halfcauchy", dist.HalfCauchy(3.0))


def _central4(m1, m2, m3, m4):
    return m4 - 4 * m1 * m3 + 6 * m1 ** 2 * m2 - 3 * m1 ** 4


def _analytic():
    """site -> (mean, variance, fourth central moment)."""
    w = math.exp(0.5 ** 2)
    ln_var = (w - 1.0) * math.exp(2 * 0.2 + 0.5 ** 2)
    s, c = 1.5, math.sqrt(2.0 / math.pi)
    t_var = 2.0 ** 2 * 9.0 / 7.0
    p, pl = 0.3, 1.0 / (1.0 + math.exp(0.4))
    return {
        "normal": (1.5, 4.0, 3 * 16.0),
        "lognormal": (math.exp(0.2 + 0.125), ln_var, ln_var ** 2 * (w ** 4 + 2 * w ** 3 + 3 * w ** 2 - 3)),
        "halfnormal": (s * c, s * s * (1 - 2 / math.pi), _central4(s * c, s * s, 2 * c * s ** 3, 3 * s ** 4)),
        "exponential": (1 / 2.5, 1 / 2.5 ** 2, 9 / 2.5 ** 4),
        "gamma_below1": (0.25, 0.5 / 4, (3 * 0.25 + 6 * 0.5) / 2.0 ** 4),
        "gamma_above1": (6.0, 12.0, (3 * 9.0 + 6 * 3.0) / 0.5 ** 4),
        "studentt": (1.0, t_var, (3 + 6 / (9.0 - 4)) * t_var ** 2),
        "poisson_inversion": (3.0, 3.0, 3.0 * (1 + 9.0)),
        "poisson_ptrs": (40.0, 40.0, 40.0 * (1 + 120.0)),
        "bernoulli": (p, p * (1 - p), p * (1 - p) * (1 - 3 * p * (1 - p))),
        "bernoulli_logits": (pl, pl * (1 - pl), pl * (1 - pl) * (1 - 3 * pl * (1 - pl))),
    }


def check_moments(draws, log=print):
    """Sample mean within 5 standard errors of the analytic mean, sample variance within 5
    standard errors (from the fourth central moment: Var(s^2) ~ (mu4 - var^2) / N) of the analytic
    variance; for Cauchy / HalfCauchy the share of draws within one scale of the location is 0.5
    within 5 binomial standard errors."""
    N = MOMENT_SAMPLES * MOMENT_ELEMENTS
    for name, (mean, var, mu4) in _analytic().items():
        x = np.asarray(draws[name], np.float64)
        assert x.shape == (MOMENT_SAMPLES, MOMENT_ELEMENTS) and np.all(np.isfinite(x)), name
        zm = (x.mean() - mean) / math.sqrt(var / N)
        zv = (x.var() - var) / math.sqrt((mu4 - var ** 2) / N)
        log(f"{name}: mean {x.mean():.5f} ({zm:+.2f} se), variance {x.var():.5f} ({zv:+.2f} se)")
        assert abs(zm) <= 5.0 and abs(zv) <= 5.0, (name, zm, zv)
    for name, loc, scale in (("cauchy", 1.0, 2.0), ("halfcauchy", 0.0, 3.0)):
        x = np.asarray(draws[name], np.float64)
        assert x.shape == (MOMENT_SAMPLES, MOMENT_ELEMENTS) and np.all(np.isfinite(x)), name
        z = ((np.abs(x - loc) < scale).mean() - 0.5) / math.sqrt(0.25 / N)
        log(f"{name}: share within one scale {0.5 + z * math.sqrt(0.25 / N):.5f} ({z:+.2f} se)")
        assert abs(z) <= 5.0, (name, z)
    assert np.all(np.asarray(draws["halfcauchy"]) >= 0) and np.all(np.asarray(draws["halfnormal"]) >= 0)
