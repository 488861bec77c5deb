"""Shared pieces of the draw-op distribution tests (tests/test_draws.py on the host interpreter,
tests/test_gpu_draws.py on the device): one table of draw sites with constant parameters and their
exact laws (frozen scipy.stats distributions), the models that hold them over a plate of 512, and
the exact tests: Pearson's chi-square against the pmf, Kolmogorov-Smirnov against the cdf, the
correlations between and within sites, the ranges the word maps give and the share of gamma draws
that underflow to zero.

Nothing here compares a draw with another implementation of the same algorithm: the host
interpreter restates the kernel's constants and formulas, so a wrong one agrees with itself there.
"""
import collections
import functools
import math

import numpy as np
import scipy.stats as st

import numpyro_amd as numpyro
import predictive_cases as PC
from numpyro_amd import distributions as dist
from numpyro_amd import native
from test_bounded import BINOMIAL_CASES

SAMPLES, ELEMENTS = 196, PC.MOMENT_ELEMENTS  # 100 352 draws per case
SEEDS = (23, 24)
LEVEL = 1e-3  # a case misses when its p-value is at or below this at both seeds (1e-6 by chance)
MAX_COUNT = native.BINOMIAL_MAX_COUNT - 1
MAX_RATE = float(native.POISSON_MAX_RATE)
BELOW_MAX_RATE = float(np.nextafter(np.float32(MAX_RATE), np.float32(0)))

Case = collections.namedtuple("Case", "name model family make law kind underflow")
CASES = []


def _case(name, model, family, make, law, kind, underflow=False):
    CASES.append(Case(name, model, family, make, law, kind, underflow))


def _num(x):
    return f"{x:g}".replace("-", "m").replace(".", "p").replace("+", "")


def _build():
    c, d = "continuous", "discrete"
    # ---- base draws; the twins differ from their sites in the stream id alone (independence below)
    _case("normal", "base", "normal", lambda: dist.Normal(0.0, 1.0), st.norm(), c)
    _case("normal_twin", "base", "normal", lambda: dist.Normal(0.0, 1.0), st.norm(), c)
    _case("normal_1p5_2", "base", "normal", lambda: dist.Normal(1.5, 2.0), st.norm(1.5, 2.0), c)
    _case("exponential", "base", "exponential", lambda: dist.Exponential(1.0), st.expon(), c)
    _case("exponential_2p5", "base", "exponential", lambda: dist.Exponential(2.5), st.expon(scale=1 / 2.5), c)
    _case("cauchy", "base", "cauchy", lambda: dist.Cauchy(1.0, 2.0), st.cauchy(1.0, 2.0), c)
    _case("uniform", "base", "uniform", lambda: dist.Uniform(-1.0, 3.0), st.uniform(-1.0, 4.0), c)
    _case("uniform01", "base", "uniform", lambda: dist.Uniform(0.0, 1.0), st.uniform(), c)
    _case("bernoulli_0p3", "base", "bernoulli", lambda: dist.Bernoulli(probs=0.3), st.bernoulli(0.3), d)
    _case("bernoulli_0p001", "base", "bernoulli", lambda: dist.Bernoulli(probs=1e-3), st.bernoulli(1e-3), d)
    _case("bernoulli_logits", "base", "bernoulli", lambda: dist.Bernoulli(logits=-0.4),
          st.bernoulli(1.0 / (1.0 + math.exp(0.4))), d)
    _case("gamma_3", "base", "gamma", lambda: dist.Gamma(3.0, 1.0), st.gamma(3.0), c)
    _case("gamma_3_twin", "base", "gamma", lambda: dist.Gamma(3.0, 1.0), st.gamma(3.0), c)
    # ---- gamma: the boost below 1, both sides of 1, and c = 1 / sqrt(9 d) from 0.4 down to 3e-4
    for a in (0.02, 0.05, 0.5, 0.999, 1.0, 1.001, 100.0, 1e4, 1e6):
        _case(f"gamma_{_num(a)}", "gamma", "gamma", lambda a=a: dist.Gamma(a, 1.0), st.gamma(a), c, a < 0.1)
    _case("gamma_3_rate2p5", "gamma", "gamma", lambda: dist.Gamma(3.0, 2.5), st.gamma(3.0, scale=1 / 2.5), c)
    # ---- poisson: both sides of NMX_POISSON_PTRS_RATE, then up to the guard
    for r in (0.05, 3.0, 9.99, 10.0, 10.5, 40.0, 1e3, 1e4, 1e5, 1e6, 4e6, 1e7, MAX_RATE / 2, BELOW_MAX_RATE):
        _case(f"poisson_{_num(r)}", "poisson", "poisson", lambda r=r: dist.Poisson(r), st.poisson(r), d)
    # ---- binomial: both sides of n q = 10, the mirror branch, then up to the largest count
    pairs = list(BINOMIAL_CASES) + [(1000, 0.99), (10 ** 5, 0.5), (10 ** 6, 0.5), (10 ** 6, 0.25), (10 ** 7, 0.001)]
    pairs += [(MAX_COUNT, p) for p in (1e-6, 0.01, 0.25, 0.5, 0.9)]
    for n, p in pairs:
        _case(f"binomial_{_num(n)}_{_num(p)}", "binomial", "binomial", lambda n=n, p=p: dist.Binomial(n, probs=p),
              st.binom(n, p), d)
    _case("binomial_logits", "binomial", "binomial", lambda: dist.Binomial(1000, logits=math.log(0.3 / 0.7)),
          st.binom(1000, 0.3), d)
    # ---- derived samplers (predictive_program._DRAW)
    _case("studentt_3", "derived", "derived", lambda: dist.StudentT(3.0, 0.0, 1.0), st.t(3.0), c)
    _case("studentt_9", "derived", "derived", lambda: dist.StudentT(9.0, 1.0, 2.0), st.t(9.0, 1.0, 2.0), c)
    _case("halfnormal", "derived", "derived", lambda: dist.HalfNormal(1.5), st.halfnorm(scale=1.5), c)
    _case("halfcauchy", "derived", "derived", lambda: dist.HalfCauchy(3.0), st.halfcauchy(scale=3.0), c)
    _case("lognormal", "derived", "derived", lambda: dist.LogNormal(0.2, 0.5), st.lognorm(0.5, scale=math.exp(0.2)), c)
    _case("pareto", "derived", "derived", lambda: dist.Pareto(2.0, 10.0), st.pareto(10.0, scale=2.0), c)
    _case("beta_2_3", "derived", "derived", lambda: dist.Beta(2.0, 3.0), st.beta(2.0, 3.0), c)
    _case("beta_0p5_0p7", "derived", "derived", lambda: dist.Beta(0.5, 0.7), st.beta(0.5, 0.7), c)


_build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
MODELS = ("base", "gamma", "poisson", "binomial", "derived")
FAMILIES = tuple(dict.fromkeys(c.family for c in CASES))
INTEGER_SITES = tuple(c.name for c in CASES if c.kind == "discrete")

# a Dirichlet site is one vector: its draws are SAMPLES x ELEMENTS samples of 4 components, and
# component i of Dirichlet(a) is Beta(a_i, sum(a) - a_i)
DIRICHLET = (0.5, 1.0, 2.5, 4.0)
DIRICHLET_LAWS = tuple(st.beta(a, sum(DIRICHLET) - a) for a in DIRICHLET)
INDEPENDENT = ("normal", "normal_twin", "exponential", "uniform01", "gamma_3", "gamma_3_twin")


def model(name):
    """The model function of one group of cases, a site per case over plate("n", ELEMENTS)."""
    def fn():
        with numpyro.plate("n", ELEMENTS):
            for c in CASES:
                if c.model == name:
                    numpyro.sample(c.name, c.make())
    fn.__name__ = f"{name}_draws"
    return fn


def dirichlet_model():
    numpyro.sample("dirichlet", dist.Dirichlet(np.asarray(DIRICHLET)))


def limit_model():
    with numpyro.plate("n", ELEMENTS):
        numpyro.sample("beta_0p05", dist.Beta(0.05, 0.05))
        numpyro.sample("studentt_0p1", dist.StudentT(0.1, 0.0, 1.0))


# ------------------------------------------------------------------------------ host draws
_HOST_FLOOR = {}


def host_floor(name, seed, dtype):
    """The underflow threshold in force when host_draws(name, seed, dtype) ran."""
    host_draws(name, seed, dtype)
    return _HOST_FLOOR[name, seed, dtype]


@functools.lru_cache(maxsize=None)
def host_draws(name, seed, dtype):
    """{site: [SAMPLES, ELEMENTS] float64} of one model on the host interpreter in `dtype`."""
    from numpyro_amd.predictive_program import compile_predictive

    if name == "dirichlet":
        fn, S = dirichlet_model, SAMPLES * ELEMENTS
    else:
        fn, S = (limit_model if name == "limit" else model(name)), SAMPLES
    prog = compile_predictive(fn, (), {}, [])
    assert prog.dim == 0 and prog.native_check() == (0, "")
    floor = host_float32_floor()
    out = prog.run_host(S, seed, PC.words, dtype=dtype)
    assert host_float32_floor() == floor
    _HOST_FLOOR[name, seed, dtype] = floor if dtype is np.float32 else 0.0  # float64 does not underflow here
    for v in out.values():
        v.setflags(write=False)
    return out


# ------------------------------------------------------------------------------ statistics
def chi_square(x, law):
    """(statistic, degrees of freedom, p-value) of Pearson's chi-square of whole-number draws
    against a discrete law; a draw outside the support gives p = 0.  One cell per value where the
    support between the 1e-7 and 1 - 1e-7 quantiles has at most 400 points (cells expected below 5,
    and everything outside, pooled into one); else 40 cells cut at the law's own quantiles."""
    x = np.asarray(x, np.float64).reshape(-1)
    lo_s, hi_s = law.support()
    if not (np.all(x == np.floor(x)) and x.min() >= lo_s and x.max() <= hi_s):
        return math.inf, 0, 0.0
    N = x.size
    lo, hi = int(law.ppf(1e-7)), int(law.ppf(1.0 - 1e-7))
    lo = max(lo, int(lo_s))
    if hi - lo + 1 <= 400:
        values = np.arange(lo, hi + 1)
        expected = law.pmf(values) * N
        inside = (x >= lo) & (x <= hi)
        observed = np.bincount((x[inside] - lo).astype(np.int64), minlength=values.size).astype(np.float64)
        big = expected >= 5.0
        obs = np.append(observed[big], observed[~big].sum() + (~inside).sum())
        exp = np.append(expected[big], N - expected[big].sum())
        if exp[-1] < 1e-9 * N and obs[-1] == 0.0:  # nothing left to pool (the two cells of a Bernoulli)
            obs, exp = obs[:-1], exp[:-1]
    else:
        edges = np.unique(law.ppf(np.linspace(0.0, 1.0, 41)))  # cells (e_i, e_i+1]; ppf(0) = support - 1
        exp = np.diff(law.cdf(edges)) * N
        obs = np.bincount(np.searchsorted(edges, x, side="left") - 1, minlength=exp.size).astype(np.float64)
        assert obs.size == exp.size and obs.sum() == N
    assert exp.size >= 2 and exp.min() > 0.0, exp
    stat = float(((obs - exp) ** 2 / exp).sum())
    return stat, exp.size - 1, float(st.chi2.sf(stat, exp.size - 1))


def ks(x, law, floor=0.0):
    """(statistic, p-value) of the one-sample Kolmogorov-Smirnov test over every draw.  `floor`
    is the underflow threshold of a gamma below concentration 1 (zero_share below): a draw below
    it is held at it, the law of max(G, floor), whose cdf is 0 below `floor` and the law's own
    from it on: the atom's share is compared at `floor` and the rest of the steps as usual."""
    x = np.asarray(x, np.float64).reshape(-1)
    if not floor:
        r = st.kstest(x, law.cdf)
        return float(r.statistic), float(r.pvalue)
    x = np.sort(np.maximum(x, floor))
    N, k = x.size, int((x <= floor).sum())
    F = law.cdf(x[k:])
    above = np.arange(k, N)
    D = max(abs(k / N - float(law.cdf(floor))), float(((above + 1) / N - F).max()), float((F - above / N).max()))
    return D, float(st.kstwo.sf(D, N))


def case_pvalue(case, x, floor=0.0):
    """(text, p-value, NaN share) of one case's draws; NaN draws are the only ones left out."""
    x = np.asarray(x, np.float64).reshape(-1)
    nan = np.isnan(x)
    x = x[~nan]
    if case.kind == "discrete":
        stat, df, p = chi_square(x, case.law)
        text = f"chi2 {stat:.2f} on {df} df"
    else:
        stat, p = ks(x, case.law, floor if case.underflow else 0.0)
        text = f"KS D {stat:.5f}"
    return text, p, float(nan.mean())


def check_family(family, draws_at, floor_at=lambda model, seed: 0.0, log=print):
    """Every case of one family under the decision rule: `draws_at(model, seed)` -> {site: draws},
    `floor_at(model, seed)` -> the underflow threshold of those draws (ks above); the second seed
    is drawn only for a case at or below the level at the first.  Asserts once, naming every case
    that misses; a NaN draw is a miss."""
    missed = []
    for case in (c for c in CASES if c.family == family):
        ps = []
        for seed in SEEDS:
            text, p, nan = case_pvalue(case, draws_at(case.model, seed)[case.name],
                                       floor_at(case.model, seed) if case.underflow else 0.0)
            log(f"{case.name} seed {seed}: {text}, p = {p:.3g}" + (f", NaN share {nan:.2e}" if nan else ""))
            ps.append(p)
            if nan:
                missed.append((case.name, "NaN share", nan))
            if p > LEVEL:
                break
        else:
            missed.append((case.name, ps))
    assert not missed, missed


def check_dirichlet(draws_at, log=print):
    missed = []
    for i, law in enumerate(DIRICHLET_LAWS):
        ps = []
        for seed in SEEDS:
            x = np.asarray(draws_at("dirichlet", seed)["dirichlet"], np.float64)
            assert x.shape == (SAMPLES * ELEMENTS, len(DIRICHLET)) and not np.isnan(x).any()
            np.testing.assert_allclose(x.sum(1), 1.0, atol=1e-6)
            stat, p = ks(x[:, i], law)
            log(f"dirichlet[{i}] seed {seed}: KS D {stat:.5f}, p = {p:.3g}")
            ps.append(p)
            if p > LEVEL:
                break
        else:
            missed.append((i, ps))
    assert not missed, missed


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


def check_independence(draws, log=print):
    """Pearson correlations within 5 / sqrt(N): between every pair of INDEPENDENT sites at equal
    (sample, element), and at lag 1 along the elements and along the samples within each.  A
    reused stream id, or an index dropped from the counter, gives a correlation of 1."""
    x = {k: np.asarray(draws[k], np.float64) for k in INDEPENDENT}
    missed = []

    def check(what, r, n):
        log(f"{what}: r = {r:+.5f} (bound {5 / math.sqrt(n):.5f})")
        if not abs(r) <= 5.0 / math.sqrt(n):
            missed.append((what, r))

    for i, a in enumerate(INDEPENDENT):
        for b in INDEPENDENT[i + 1:]:
            check(f"{a} x {b}", _corr(x[a].ravel(), x[b].ravel()), x[a].size)
        e0, e1 = x[a][:, :-1].ravel(), x[a][:, 1:].ravel()
        check(f"{a} lag 1 along elements", _corr(e0, e1), e0.size)
        s0, s1 = x[a][:-1].ravel(), x[a][1:].ravel()
        check(f"{a} lag 1 along samples", _corr(s0, s1), s0.size)
    assert not missed, missed


# a float32 result may sit a few ulp past the real-number bound of its word map
_ULPS = 1.0 + 4 * 2.0 ** -23


def check_ranges(draws):
    """The ranges of the word maps (include/numpyro_amd.h): u01 in [0, 1), u01_open0 in (0, 1]."""
    u = np.asarray(draws["uniform01"])
    assert u.min() >= 0.0 and u.max() < 1.0, (u.min(), u.max())
    u = np.asarray(draws["uniform"])
    assert u.min() >= -1.0 and u.max() < 3.0, (u.min(), u.max())
    z = np.asarray(draws["normal"])
    assert np.abs(z).max() <= math.sqrt(48 * math.log(2)) * _ULPS, np.abs(z).max()
    # -log u01_open0 is 0 at the one word in 2^24 that maps to 1: not among these draws at the fixed seeds
    e = np.asarray(draws["exponential"])
    assert e.min() > 0.0 and e.max() <= 24 * math.log(2) * _ULPS, (e.min(), e.max())
    assert np.all(np.isfinite(np.asarray(draws["cauchy"])))


def check_integer_sites(draws, device):
    for name, x in draws.items():
        if name in INTEGER_SITES:
            x = np.asarray(x)
            if device:
                assert x.dtype == np.int32, (name, x.dtype)
            assert not np.isnan(x).any() and np.array_equal(x, np.floor(x)) and x.min() >= 0, name


# ------------------------------------------------------------------------------ the gamma underflow
DENORMALS_KEPT, DENORMALS_FLUSHED = 2.0 ** -150, 2.0 ** -126  # what rounds to 0 in float32


def host_float32_floor():
    """The threshold of this process's float32 NumPy arithmetic: 2^-150, NumPy's rounding, unless
    the thread runs with flush-to-zero on.  Loading a library linked with -ffast-math, as the CPU
    oracle's (oracle/build.py) is, turns it on for the rest of the process, so the threshold depends on
    which tests ran before; the draws and the threshold are always taken in the same state
    (host_draws asserts it)."""
    return DENORMALS_FLUSHED if float(np.float32(2.0 ** -126) * np.float32(0.5)) == 0.0 else DENORMALS_KEPT


def zero_share(x, a, thresholds, log=print):
    """A Gamma(a) draw below concentration 1 is d v exp(log(U) / a), and in float32 the exp
    underflows to exactly 0: the share of exact zeros must lie within 5 binomial standard errors
    of P(Gamma(a) < t) for one t of `thresholds`.  Returns that t."""
    x = np.asarray(x).reshape(-1)
    share = float((x == 0).mean())
    found = None
    for t in thresholds:
        want = float(st.gamma(a).cdf(t))
        se = math.sqrt(want * (1 - want) / x.size)
        z = (share - want) / se
        log(f"Gamma({a:g}): zero share {share:.5f}; P(G < 2^{math.log2(t):.0f}) = {want:.5f} ({z:+.2f} se)")
        if found is None and abs(share - want) <= 5 * se:
            found = t
    assert found is not None, (a, share)
    return found


def limit_shares(draws, log=print):
    """Beta(0.05, 0.05) and StudentT(0.1): the docs promise values in [0, 1] or NaN for the Beta
    and nothing on finiteness for the StudentT; the shares are printed for DESIGN.md."""
    b = np.asarray(draws["beta_0p05"], np.float64).reshape(-1)
    t = np.asarray(draws["studentt_0p1"], np.float64).reshape(-1)
    nan = np.isnan(b)
    log(f"Beta(0.05, 0.05): NaN share {nan.mean():.5f}, exact 0 or 1 share {((b == 0) | (b == 1)).mean():.5f}")
    log(f"StudentT(0.1): non-finite share {(~np.isfinite(t)).mean():.5f}, NaN share {np.isnan(t).mean():.5f}")
    assert np.all((b[~nan] >= 0.0) & (b[~nan] <= 1.0))
