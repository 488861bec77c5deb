"""Shared pieces of the PSIS-LOO tests (tests/test_psis.py on the host, tests/test_gpu_psis.py on
the device): NumPy restatements of the arithmetic of include/numpyro_amd.h "PSIS-LOO", written from
that statement, and the tables the tests run on.

* ``psis64(table, M)``: the log ratios r in float32 with one rounding, as stated (every discrete
  decision is taken on them), everything after in float64.
* ``psis32(table, M)``: the same with every operation and every sum in float32; its deviation from
  psis64 calibrates the device's bound (loglik_cases.calibrated_bound).
* ``normal_table``: a one-parameter normal model whose prior spread sets the tail's shape.
* ``conjugate_normal``: a conjugate normal model with exact posterior draws and the closed-form
  leave-one-out predictive density.
"""
import math

import numpy as np

LOG_FLT_MIN = np.float32(-87.33655)  # NMX_PSIS_LOG_FLT_MIN
K_ZERO = 1e-10  # NMX_PSIS_K_ZERO


def tail_length(S, reff=1.0):
    """M = ceil(min(S / 5, 3 sqrt(S / reff)))."""
    return int(math.ceil(min(S / 5.0, 3.0 * math.sqrt(S / reff))))


def gpd_fit(e, F=np.float64):
    """(k, sigma) of the exceedances e (ascending, > 0) by Zhang and Stephens (2009) with the weak
    prior of the loo package, in the number format F."""
    e = np.asarray(e, F)
    T = e.size
    fT = F(T)
    with np.errstate(all="ignore"):
        q = e[(T + 2) // 4 - 1]  # floor(T / 4 + 0.5) - 1
        J = 30 + math.isqrt(T)
        j = np.arange(1, J + 1).astype(F)
        b_j = (F(1) - np.sqrt(F(J) / (j - F(0.5)))) / (F(3) * q) + F(1) / e[-1]
        kappa_j = np.log1p(-b_j[:, None] * e[None, :]).sum(1, dtype=F) / fT
        L = fT * (np.log(-b_j / kappa_j) - kappa_j - F(1))
        w = np.exp(L - L.max())
        w = w / w.sum(dtype=F)
        b = (b_j * w).sum(dtype=F)
        kappa = np.log1p(-b * e).sum(dtype=F) / fT
        sigma = -kappa / b
        k = (fT * kappa + F(5)) / (fT + F(10))
    assert np.asarray(k).dtype == F and np.asarray(sigma).dtype == F
    return k, sigma


def psis_column(x, M, F=np.float64):
    """(elpd_loo, pareto_k, lw, t) of one column x [S] (float32) with the tail length M: lw the log
    weights of the tail after smoothing and t the sorted tail (None for a non-finite column)."""
    x = np.asarray(x, np.float32)
    S = x.size
    assert 1 <= M < S
    if not np.all(np.isfinite(x)):
        return F(np.nan), F(np.nan), None, None
    with np.errstate(all="ignore"):
        neg = -x
        m = neg.max()
        r = neg - m  # float32, one rounding, <= 0
        assert r.dtype == np.float32
        cut = max(np.sort(r)[S - 1 - M], LOG_FLT_MIN)  # the (M+1)-th largest, floored
        in_tail = r > cut
        t = np.sort(r[in_tail]).astype(F)
        T = t.size
        assert T <= M
        body = np.exp(r[~in_tail].astype(F)).sum(dtype=F)
        expcut = np.exp(F(cut))
        k, lw = F(np.inf), t
        if T > 4:
            k, sigma = gpd_fit(np.exp(t) - expcut, F)
            if np.isfinite(k) and np.isfinite(sigma):
                p = (np.arange(T).astype(F) + F(0.5)) / F(T)
                l1 = np.log1p(-p)
                g = -sigma * l1 if abs(k) < K_ZERO else sigma * np.expm1(-k * l1) / k
                lw = np.fmin(np.log(g + expcut), F(0))
        den = body + np.exp(lw).sum(dtype=F)
        num = F(S - T) + np.exp(lw - t).sum(dtype=F)
        elpd = (np.log(num) - F(m)) - np.log(den)
    assert np.asarray(elpd).dtype == F and np.asarray(lw).dtype == F
    return elpd, k, lw, t


def _psis(table, M, F):
    table = np.asarray(table, np.float32)
    table = table.reshape(table.shape[0], -1)
    cols = [psis_column(table[:, c], M, F)[:2] for c in range(table.shape[1])]
    return np.array([c[0] for c in cols], F), np.array([c[1] for c in cols], F)


def psis64(table, M):
    """(elpd_loo [N], pareto_k [N]) of table [S, N]: float32 log ratios, then float64."""
    return _psis(table, M, np.float64)


def psis32(table, M):
    """(elpd_loo [N], pareto_k [N]) of table [S, N] with every operation and sum in float32."""
    return _psis(table, M, np.float32)


def is_loo(x, F=np.float64):
    """elpd_loo of one column by plain importance sampling: log(S) - logsumexp(-x)."""
    x = np.asarray(x, np.float32)
    neg = -x
    m = neg.max()
    r = (neg - m).astype(F)
    return (np.log(F(x.size)) - F(m)) - np.log(np.exp(r).sum(dtype=F))


def normal_table(S, N, spread, seed=0, ties=False):
    """float32 table [S, N] of the model y_i ~ N(mu, 1) at S draws mu_s ~ N(0, spread) and N
    observations on linspace(-3, 3, N); ``ties`` rounds the log likelihood to one decimal.  The
    spreads 0.2, 0.7 and 1.5 give k of about 0 - 0.4, 0.4 - 1.2 and 1.4 - 4."""
    rs = np.random.RandomState(seed)
    mu = rs.normal(0.0, spread, S)
    y = np.linspace(-3.0, 3.0, N)
    ll = -0.5 * (y[None, :] - mu[:, None]) ** 2 - 0.5 * math.log(2.0 * math.pi)
    if ties:
        ll = np.round(ll, 1)
    return ll.astype(np.float32)


def conjugate_normal(S=40000, N=40, seed=3):
    """y_i ~ N(mu, 1), mu ~ N(0, 10^2), N observations of which the last is an outlier at 4.5.
    Returns (table [S, N] float32 at S exact posterior draws, exact leave-one-out log predictive
    density [N], exact in-sample log posterior predictive density [N])."""
    rs = np.random.RandomState(seed)
    y = np.concatenate([rs.normal(0.0, 1.0, N - 1), [4.5]])
    prec = 1.0 / 100.0 + N
    mean = y.sum() / prec
    mu = mean + rs.normal(0.0, 1.0, S) / math.sqrt(prec)
    table = (-0.5 * (y[None, :] - mu[:, None]) ** 2 - 0.5 * math.log(2.0 * math.pi)).astype(np.float32)

    def normal_logpdf(v, loc, var):
        return -0.5 * (v - loc) ** 2 / var - 0.5 * np.log(2.0 * math.pi * var)

    prec_i = 1.0 / 100.0 + (N - 1)
    loo = normal_logpdf(y, (y.sum() - y) / prec_i, 1.0 + 1.0 / prec_i)
    lppd = normal_logpdf(y, mean, 1.0 + 1.0 / prec)
    return table, loo, lppd


def same_nonfinite(a, b):
    """Whether a and b are non-finite at the same entries, in the same way (NaN, +inf, -inf)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b))
                and np.array_equal(np.isneginf(a), np.isneginf(b)))
