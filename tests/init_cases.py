"""Chain start-up cases shared by tests/test_init.py (CPU: every prediction and bound holds for the
references alone) and tests/test_gpu_init.py (the same predictions on the device's arena).

* draws: the init_to_uniform stream restated by oracle/philox.py.  nuts.hip is built with
  -ffp-contract=off, so the oracle's multiply-then-subtract is the kernel's arithmetic at any
  radius and a start is identified BITWISE (attempt_of);
* verdicts: what a float64 evaluation of the model says about a draw -- VALID when U and the
  largest gradient entry are clearly inside float32 range, INVALID when either is clearly outside
  it or not finite, AMBIGUOUS within a factor BAND of FLT_MAX;
* plain float32 restatements of the two fused kernels that the retry tests run, to show on the
  CPU that a float32 evaluation never contradicts a verdict and meets the standing tolerances at
  the accepted points.

BAND.  The float32 form of the oracle (oracle/potentials.py, dtype=np.float32) evaluates in
float64 and rounds once, so it contradicts no band above 1 + 2^-24: it cannot tighten the band
(tests/test_init.py shows this over the ladder 2, 4, ..., 2^14 at the seeds used here).  What a
band has to absorb is an intermediate of a float32 evaluation leaving the range before the result
does: both kernels square before they halve (0.5 v^2 with v^2 formed first; 0.5 e^-y sum x^2),
a factor 2, and BAND = 4 doubles that.  The plain float32 restatements below, which do overflow in
their intermediates, never contradict it either."""
from __future__ import annotations

import functools

import numpy as np

from numpyro_amd import datasets
from oracle import philox
from oracle import potentials as OP

FLT_MAX = float(np.finfo(np.float32).max)
BAND = 4.0
VALID, AMBIGUOUS, INVALID = "valid", "ambiguous", "invalid"
AMBIGUOUS_CAP = 0.10  # of all evaluated draws

# the retry cases of the fused kernels: (seed, chain_offset, C, radius)
SCHOOLS_CASE = dict(seed=1, chain_offset=0, C=130, radius=100.0)
FUNNEL_CASE = dict(seed=1, chain_offset=7, C=130, radius=100.0, dim=300)
# the exactly predicted retries of a torch potential_fn: C, D, radius; the seed is chosen by
# pick_retry_seed (tests/test_init.py pins the value)
GATE_CASE = dict(C=130, D=5, radius=2.0, seed=0)
GATE_EDGE_CHAINS = (0, 63, 64, 129)


# ---------------------------------------------------------------- draws
def draw(seed, chain, attempt, D, radius):
    return philox.init_uniform(seed, chain, attempt, D, radius)


@functools.lru_cache(maxsize=None)
def draws(seed, chain_offset, C, attempt, D, radius):
    """[C, D] float32: attempt `attempt` of chains chain_offset .. chain_offset + C - 1 (read-only)."""
    out = np.stack([draw(seed, chain_offset + c, attempt, D, radius) for c in range(C)])
    out.setflags(write=False)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def attempt_of(z, seed, chain, D, radius, max_attempts):
    """The attempt a for which z is bitwise philox.init_uniform(seed, chain, a, D, radius), else None."""
    zb = bits(np.asarray(z, np.float32).reshape(-1))
    if zb.shape != (D,):
        return None
    for a in range(max_attempts):
        if np.array_equal(zb, bits(draw(seed, chain, a, D, radius))):
            return a
    return None


# ---------------------------------------------------------------- verdicts
def verdict(pe, g, band=BAND):
    """VALID / AMBIGUOUS / INVALID of one draw from its float64 (U, grad U)."""
    pe, g = float(pe), np.asarray(g, np.float64)
    if not (np.isfinite(pe) and np.isfinite(g).all()):
        return INVALID
    m = max(abs(pe), float(np.abs(g).max()))
    if m < FLT_MAX / band:
        return VALID
    if m > FLT_MAX * band:
        return INVALID
    return AMBIGUOUS


def contradicts(v, pe32, g32):
    """Does a float32 evaluation (accepted iff all of it is finite) contradict verdict v?"""
    ok = bool(np.isfinite(np.float32(pe32)) and np.isfinite(np.asarray(g32, np.float32)).all())
    return (v == VALID and not ok) or (v == INVALID and ok)


def schools_oracle(dtype=np.float64):
    return OP.EightSchools(datasets.EIGHT_SCHOOLS_Y, datasets.EIGHT_SCHOOLS_SIGMA, dtype=dtype)


def funnel_oracle(dim, dtype=np.float64):
    return OP.Funnel(dim, dtype=dtype)


def as_f32(oracle_cls_instance, z):
    """The oracle's float32 form at z (rounds the float64 result once; overflow -> inf)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return oracle_cls_instance.pe_grad(np.asarray(z, np.float64))


def eval64(oracle, z):
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        pe, g = oracle.pe_grad(np.asarray(z, np.float64))
    return float(pe), np.asarray(g, np.float64)


# ---------------------------------------------------------------- plain float32 restatements
def schools_plain_f32(z, guarded=True):
    """nmx_small_models.h NmxEightSchools restated in NumPy float32 (libm exp / log / log1p), one
    chain: (U, grad) as float32.  guarded=False: without the kernel's u > 40 branch, i.e. with
    log1p((tau / 5)^2), 2 q / (1 + q) and log(sqrt(2 pi) tau) formed from tau = e^u at every u."""
    f = np.float32
    y, sigma = datasets.EIGHT_SCHOOLS_Y.astype(f), datasets.EIGHT_SCHOOLS_SIGMA.astype(f)
    z = np.asarray(z, f)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        mu, u, th = z[0], z[1], z[2:]
        tau = np.exp(u)
        tau2 = tau * tau
        big = bool(guarded) and u > f(40.0)
        log5, hl2pi = f(1.6094379124341003), f(0.9189385332046727)

        def nlpN(x, loc, scale):
            v = (x - loc) / scale
            return f(0.5) * v * v + np.log(f(2.5066282746310002) * scale)

        x5 = tau / f(5.0)
        l1p = f(2.0) * (u - log5) if big else np.log1p(x5 * x5)
        U = nlpN(mu, f(0.0), f(5.0)) + (f(1.1447298858494002) + log5 + l1p - f(0.6931471805599453)) - u
        dt = th - mu
        v = dt / tau
        nl_th = f(0.5) * v * v + (hl2pi + u) if big else nlpN(th, mu, tau)
        for j in range(len(y)):
            U = U + (nl_th[j] + nlpN(y[j], th[j], sigma[j]))
        g = np.empty_like(z)
        g_mu = mu / f(25.0)
        g_u = (f(2.0) if big else (f(2.0) * tau2 / f(25.0)) / (f(1.0) + tau2 / f(25.0))) - f(1.0)
        for j in range(len(y)):
            g_mu = g_mu - dt[j] / tau2
            g_u = g_u - (dt[j] * dt[j] / tau2 - f(1.0))
        g[0], g[1] = g_mu, g_u
        g[2:] = dt / tau2 + (th - y) / (sigma * sigma)
    return f(U), g


def funnel_plain_f32(z):
    """nmx_wide_models.h NmxWideFunnel restated in NumPy float32, one chain."""
    f = np.float32
    z = np.asarray(z, f)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        x, y, K = z[:-1], z[-1], f(z.size - 1)
        e, S = np.exp(-y), (x * x).sum(dtype=f)
        g = np.concatenate([x * e, [y / f(9) + f(0.5) * K - f(0.5) * e * S]]).astype(f)
        pe = y * y / f(18) + f(2.0175508218727822) + f(0.5) * e * S + K * (f(0.5) * y + f(0.9189385332046727))
    return f(pe), g


# ---------------------------------------------------------------- the standing tolerances
def check_schools(pe, g, ref):
    """tests/test_gpu_potentials.py test_eight_schools_matches_oracle's tolerances, one chain."""
    np.testing.assert_allclose(pe, ref[0], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(g, ref[1], rtol=1e-4, atol=1e-4)


def check_funnel(pe, g, ref):
    """tests/potential_cases.py check_funnel_outer (centred), one chain."""
    np.testing.assert_allclose(pe, ref[0], rtol=2e-5)
    np.testing.assert_allclose(g, ref[1], rtol=1e-4, atol=1e-3 * max(1.0, np.abs(ref[1]).max() * 1e-2))


def check_diag(pe, g, ref):
    """tests/test_gpu_potentials.py test_diag_normal's tolerances, one chain."""
    np.testing.assert_allclose(pe, ref[0], rtol=1e-5)
    np.testing.assert_allclose(g, ref[1], rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------- predicted retries
class Retry:
    """The retry loop of C chains replayed on the CPU: chain c draws attempts 0, 1, ... until
    `accepts(z)`; per chain the accepted attempt, and the float64 verdict of every draw evaluated."""

    def __init__(self, seed, chain_offset, C, D, radius, accepts, oracle64, max_attempts, band=BAND):
        self.accepted = np.full(C, -1, np.int64)
        self.verdicts = [[] for _ in range(C)]  # per chain: verdict of attempt 0 .. accepted
        self.refs = [None] * C                  # float64 (U, grad) at the accepted draw
        self.z = np.zeros((C, D), np.float32)
        for c in range(C):
            for a in range(max_attempts):
                z = draws(seed, chain_offset, C, a, D, radius)[c]
                pe, g = eval64(oracle64, z)
                self.verdicts[c].append(verdict(pe, g, band))
                if accepts(z):
                    self.accepted[c], self.refs[c], self.z[c] = a, (pe, g), z
                    break

    @property
    def retrying(self):
        return int((self.accepted > 0).sum())

    @property
    def most_redraws(self):
        return int(self.accepted.max())

    @property
    def evaluated(self):
        return sum(len(v) for v in self.verdicts)

    @property
    def ambiguous(self):
        return sum(v.count(AMBIGUOUS) for v in self.verdicts)


def _finite32(fn):
    def accepts(z):
        pe, g = fn(z)
        return bool(np.isfinite(np.float32(pe)) and np.isfinite(np.asarray(g, np.float32)).all())
    return accepts


@functools.lru_cache(maxsize=None)
def schools_retry(which="oracle32", band=BAND, max_attempts=100):
    """Eight schools at SCHOOLS_CASE, accepted by the float32 oracle or by the plain restatement."""
    k = SCHOOLS_CASE
    o32 = schools_oracle(np.float32)
    fn = (lambda z: as_f32(o32, z)) if which == "oracle32" else schools_plain_f32
    return Retry(k["seed"], k["chain_offset"], k["C"], 10, k["radius"], _finite32(fn), schools_oracle(),
                 max_attempts, band)


@functools.lru_cache(maxsize=None)
def funnel_retry(which="oracle32", band=BAND, max_attempts=100):
    k = FUNNEL_CASE
    o32 = funnel_oracle(k["dim"], np.float32)
    fn = (lambda z: as_f32(o32, z)) if which == "oracle32" else funnel_plain_f32
    return Retry(k["seed"], k["chain_offset"], k["C"], k["dim"], k["radius"], _finite32(fn),
                 funnel_oracle(k["dim"]), max_attempts, band)


def check_accepted(z, seed, chain_offset, D, radius, oracle64, max_attempts, band=BAND):
    """The retry properties of final positions z [C, D] against the float64 verdicts: each z is
    bitwise one attempt's draw, that draw is not INVALID, and no earlier draw of the chain is VALID.
    Returns (accepted attempt per chain, evaluated draws, ambiguous draws, refs at accepted)."""
    C = z.shape[0]
    acc, evaluated, ambiguous, refs = np.zeros(C, np.int64), 0, 0, []
    for c in range(C):
        a = attempt_of(z[c], seed, chain_offset + c, D, radius, max_attempts)
        assert a is not None, f"chain {c}: its start is no attempt's draw"
        acc[c] = a
        for k in range(a + 1):
            zk = draws(seed, chain_offset, C, k, D, radius)[c]
            pe, g = eval64(oracle64, zk)
            v = verdict(pe, g, band)
            evaluated += 1
            ambiguous += v == AMBIGUOUS
            if k < a:
                assert v != VALID, f"chain {c}: attempt {k} is valid (U {pe:.3g}, max|g| {np.abs(g).max():.3g}) " \
                                   f"but attempt {a} was accepted"
            else:
                assert v != INVALID, f"chain {c}: accepted attempt {a} is invalid (U {pe:.3g})"
                refs.append((pe, g, v))
    return acc, evaluated, ambiguous, refs


# ---------------------------------------------------------------- the gated torch potential
def gate_threshold(radius):
    return np.float32(radius / 2)


def gate_first_valid(seed, C, D, radius, max_attempts=100):
    """First attempt of each chain whose draw has z[0] <= radius / 2 (the gated potential_fn is
    valid exactly there): an exact function of the draws."""
    t = gate_threshold(radius)
    out = np.full(C, -1, np.int64)
    for c in range(C):
        for a in range(max_attempts):
            if draws(seed, 0, C, a, D, radius)[c, 0] <= t:
                out[c] = a
                break
    return out


def gate_seed_ok(first):
    edge = first[list(GATE_EDGE_CHAINS)]
    return bool(first.max() >= 3 and first.min() >= 0 and len(set(edge.tolist())) > 1 and (first == 0).any())


def pick_retry_seed(C, D, radius, limit=50):
    """The smallest seed at which some chain needs 3 or more redraws and chains 0, 63, 64 and 129
    do not all accept at the same attempt."""
    for seed in range(limit):
        if gate_seed_ok(gate_first_valid(seed, C, D, radius)):
            return seed
    raise AssertionError("no seed found")


def diag_params(D):
    """(mu, sd) of the diag_normal arena cases, float32, a function of D alone."""
    d = np.arange(D, dtype=np.float64)
    return (np.sin(0.7 * d) * 1.5).astype(np.float32), (0.5 + 1.5 * ((d * 0.37) % 1.0)).astype(np.float32)


def imm_diag(D):
    """A non-trivial diagonal inverse mass matrix, float32."""
    d = np.arange(D, dtype=np.float64)
    return (0.25 + ((d * 0.61) % 1.0) * 3.0).astype(np.float32)
