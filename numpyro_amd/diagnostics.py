"""Posterior diagnostics over [chains, draws, ...] arrays (host NumPy, float64), with the
semantics of numpyro/diagnostics.py: split Gelman-Rubin (:64-80), Geyer initial
monotone sequence ESS from FFT autocovariance (:101-203), HPDI (:206-231), summary and
print_summary tables (:234-342).  Accepts torch tensors as well as arrays."""
from __future__ import annotations

from collections import OrderedDict
import math
from itertools import product

import numpy as np

__all__ = ["autocorrelation", "autocovariance", "effective_sample_size", "gelman_rubin", "hpdi",
           "split_gelman_rubin", "summary", "print_summary", "print_summary_table", "lppd", "waic",
           "loo", "pareto_k"]


def _np(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def _chain_variances(x):
    """(within-chain variance W, pooled estimator var+) for x [C, N, ...]."""
    C, N = x.shape[:2]
    w = x.var(axis=1, ddof=1).mean(axis=0)
    est = w * (N - 1) / N
    if C > 1:
        est = est + x.mean(axis=1).var(axis=0, ddof=1)
    else:
        w = est
    return w, est


def gelman_rubin(x):
    x = _np(x)
    assert x.ndim >= 2 and x.shape[0] >= 2 and x.shape[1] >= 2
    w, est = _chain_variances(x)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(est / w)


def split_gelman_rubin(x):
    x = _np(x)
    assert x.ndim >= 2 and x.shape[1] >= 4
    half = x.shape[1] // 2
    return gelman_rubin(np.concatenate([x[:, :half], x[:, -half:]], axis=0))


def _next_fast_len(n):
    if n <= 2:
        return n
    while True:
        m = n
        for p in (2, 3, 5):
            while m % p == 0:
                m //= p
        if m == 1:
            return n
        n += 1


def autocorrelation(x, axis=0, bias=True):
    x = _np(x)
    n = x.shape[axis]
    m2 = 2 * _next_fast_len(n)
    y = np.swapaxes(x, axis, -1)
    y = y - y.mean(axis=-1, keepdims=True)
    f = np.fft.rfft(y, n=m2, axis=-1)
    ac = np.fft.irfft(f * np.conjugate(f), n=m2, axis=-1)[..., :n]
    if not bias:
        ac = ac / np.arange(n, 0.0, -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        ac = (ac / ac[..., :1]).astype(np.float64)
    return np.swapaxes(ac, axis, -1)


def autocovariance(x, axis=0, bias=True):
    x = _np(x)
    return autocorrelation(x, axis, bias) * x.var(axis=axis, keepdims=True)


def effective_sample_size(x, bias=True):
    x = _np(x).astype(np.float64)
    assert x.ndim >= 2 and x.shape[1] >= 2
    gamma = autocovariance(x, axis=1, bias=bias)
    w, est = _chain_variances(x)
    rho = 1.0 - (w - gamma.mean(axis=0)) / est
    rho[0] = 1.0
    pairs = rho[:-1:2, ...] + rho[1::2, ...]  # Geyer initial positive sequence
    mono = np.concatenate([pairs[:1], np.minimum.accumulate(np.clip(pairs[1:, ...], 0, None), axis=0)],
                          axis=0)
    tau = -1.0 + 2.0 * mono.sum(axis=0)
    return np.prod(x.shape[:2]) / tau


def hpdi(x, prob=0.90, axis=0):
    x = np.swapaxes(_np(x), axis, 0)
    xs = np.sort(x, axis=0)
    mass = x.shape[0]
    k = int(prob * mass)
    width = xs[k:] - xs[:mass - k]
    start = width.argmin(axis=0)
    lo = np.take_along_axis(xs, start[None, ...], axis=0)
    hi = np.take_along_axis(xs, (start + k)[None, ...], axis=0)
    return np.concatenate([np.swapaxes(lo, axis, 0), np.swapaxes(hi, axis, 0)], axis=axis)


def summary(samples, prob=0.90, group_by_chain=True):
    if not isinstance(samples, dict):
        samples = {"Param:0": samples}
    out = {}
    for name, value in samples.items():
        value = _np(value)
        if not group_by_chain:
            value = value[None, ...]
        if value.size == 0:
            continue
        value = value.astype(np.float64)
        flat = value.reshape((-1,) + value.shape[2:])
        h = hpdi(flat, prob=prob)
        out[name] = OrderedDict([
            ("mean", flat.mean(axis=0)),
            ("std", flat.std(axis=0, ddof=1)),
            ("median", np.median(flat, axis=0)),
            ("{:.1f}%".format(50 * (1 - prob)), h[0]),
            ("{:.1f}%".format(50 * (1 + prob)), h[1]),
            ("n_eff", effective_sample_size(value)),
            ("r_hat", split_gelman_rubin(value)),
        ])
    return out


def print_summary(samples, prob=0.90, group_by_chain=True):
    if not isinstance(samples, dict):
        samples = {"Param:0": samples}
    if not group_by_chain:
        samples = {k: _np(v)[None, ...] for k, v in samples.items()}
    print_summary_table(summary(samples, prob, group_by_chain=True), prob)


def print_summary_table(table, prob=0.90):
    """Print a {site: OrderedDict(stat -> array)} table as numpyro's print_summary does."""
    if not table:
        return
    table = {k: OrderedDict((s, _np(v)) for s, v in st.items()) for k, st in table.items()}
    width = max(max(len(k) + 2 + 3 * st["mean"].ndim for k, st in table.items()), 10)
    name_fmt = "{:>" + str(width) + "}"
    cols = [""] + list(next(iter(table.values())).keys())
    print()
    print((name_fmt + " {:>9}" * 7).format(*cols))
    row_fmt = name_fmt + " {:>9.2f}" * 7
    for name, stats in table.items():
        shape = stats["mean"].shape
        if len(shape) == 0:
            print(row_fmt.format(name, *[float(v) for v in stats.values()]))
        else:
            for idx in product(*map(range, shape)):
                label = name + "[{}]".format(",".join(map(str, idx)))
                print(row_fmt.format(label, *[float(v[idx]) for v in stats.values()]))
    print()


# ----------------------------------------------------------------------------- predictive accuracy
def _pointwise(log_lik):
    """(lppd_i, p_waic_i) float32 device tensors of a table [S, ...] or a dict of such tables."""
    from .pointwise import reduce_table

    if isinstance(log_lik, dict):
        if not log_lik:
            raise ValueError("an empty dict of log-likelihood tables")
        parts = {k: reduce_table(v) for k, v in log_lik.items()}
        return {k: v[0] for k, v in parts.items()}, {k: v[1] for k, v in parts.items()}
    return reduce_table(log_lik)


def lppd(log_lik):
    """Log pointwise predictive density per observation of a log-likelihood table [S, ...] (the
    result of infer.log_likelihood; a dict of tables gives a dict): logsumexp over the S samples
    minus log S, reduced by the pointwise HIP kernels (numpyro_amd/pointwise.py).  A float32 tensor
    of the table's trailing shape on the current GPU."""
    return _pointwise(log_lik)[0]


def waic(log_lik):
    """Widely applicable information criterion of a log-likelihood table [S, ...] or a dict of
    tables (their observations pooled), on the log score scale (Watanabe 2010; Vehtari, Gelman and
    Gabry 2017, eqs. 11-13): elpd_i = lppd_i - p_waic_i with p_waic_i the variance over samples
    (S - 1) of the log likelihood of observation i.  Returns {"elpd_waic": sum elpd_i, "p_waic":
    sum p_waic_i, "lppd": sum lppd_i, "se": sqrt(n var(elpd_i))} (the population variance over the n
    observations) as float64 tensors; the per-observation figures come from the pointwise HIP
    kernels, the sums over observations are torch."""
    import torch

    lp, pw = _pointwise(log_lik)
    if isinstance(lp, dict):
        lp = torch.cat([v.reshape(-1) for v in lp.values()])
        pw = torch.cat([v.reshape(-1) for v in pw.values()])
    lp, pw = lp.reshape(-1).double(), pw.reshape(-1).double()
    elpd = lp - pw
    n = elpd.numel()
    return {"elpd_waic": elpd.sum(), "p_waic": pw.sum(), "lppd": lp.sum(),
            "se": torch.sqrt(n * elpd.var(unbiased=False))}


def _rows(table):
    shape = tuple(table.shape) if hasattr(table, "shape") else np.shape(table)
    return int(shape[0]) if shape else 0


def _psis(log_lik, reff):
    """(elpd_loo_i, pareto_k_i) float32 device tensors of a table [S, ...] or a dict of such
    tables, and S."""
    from . import psis

    if isinstance(log_lik, dict):
        if not log_lik:
            raise ValueError("an empty dict of log-likelihood tables")
        rows = {k: _rows(v) for k, v in log_lik.items()}
        if len(set(rows.values())) != 1:
            raise ValueError(f"the log-likelihood tables of one model hold the same samples, got {rows} rows")
        parts = {k: psis.psis_loo_table(v, reff) for k, v in log_lik.items()}
        return {k: v[0] for k, v in parts.items()}, {k: v[1] for k, v in parts.items()}, next(iter(rows.values()))
    elpd, k = psis.psis_loo_table(log_lik, reff)
    return elpd, k, _rows(log_lik)


def pareto_k(log_lik, reff=1.0):
    """The Pareto-k diagnostic per observation of a log-likelihood table [S, ...] (a dict of tables
    gives a dict): the shape of the generalised Pareto distribution fitted to the largest
    leave-one-out importance ratios of the observation, by the PSIS HIP kernel
    (numpyro_amd/psis.py).  +inf where the tail is too short to fit (at most 4 ratios above the
    cutoff), NaN for a column that holds a non-finite entry.  A float32 tensor of the table's
    trailing shape on the current GPU."""
    return _psis(log_lik, reff)[1]


def loo(log_lik, reff=1.0):
    """Pareto-smoothed importance-sampling leave-one-out cross-validation of a log-likelihood table
    [S, ...] or a dict of tables (their observations pooled), on the log score scale (Vehtari,
    Gelman and Gabry 2017): elpd_loo_i from the importance ratios 1 / p(y_i | theta_s), their
    M = ceil(min(S / 5, 3 sqrt(S / reff))) largest replaced by the order statistics of a fitted
    generalised Pareto distribution, whose shape k_i is the diagnostic: above k_threshold =
    min(1 - 1 / log10(S), 0.7) the estimate of that observation is not to be trusted, and a
    UserWarning says how many there are.  ``reff`` is the relative efficiency of the draws (MCMC
    effective sample size / S).  Returns {"elpd_loo": sum elpd_loo_i, "p_loo": sum (lppd_i -
    elpd_loo_i), "lppd": sum lppd_i, "se": sqrt(n var(elpd_loo_i))} (the population variance over
    the n observations, as waic) as float64 tensors, "elpd_loo_i" and "pareto_k" per observation
    (float32, shaped like the table's trailing dimensions; dicts for a dict), "k_threshold" and
    "n_bad".  The per-observation figures come from the PSIS and pointwise HIP kernels, the sums over
    observations are torch."""
    import warnings

    import torch

    elpd_i, k_i, S = _psis(log_lik, reff)
    lp_i = _pointwise(log_lik)[0]
    if isinstance(elpd_i, dict):
        elpd = torch.cat([v.reshape(-1) for v in elpd_i.values()])
        k = torch.cat([v.reshape(-1) for v in k_i.values()])
        lp = torch.cat([v.reshape(-1) for v in lp_i.values()])
    else:
        elpd, k, lp = elpd_i, k_i, lp_i
    elpd, k, lp = elpd.reshape(-1).double(), k.reshape(-1), lp.reshape(-1).double()
    n = elpd.numel()
    k_threshold = min(1.0 - 1.0 / math.log10(S), 0.7)
    n_bad = int((k > k_threshold).sum())
    if n_bad > 0:
        warnings.warn(f"PSIS-LOO: {n_bad} of {n} observations have a Pareto k above {k_threshold:.2f}; elpd_loo of "
                      "these observations is unreliable", UserWarning, stacklevel=2)
    return {"elpd_loo": elpd.sum(), "p_loo": (lp - elpd).sum(), "lppd": lp.sum(),
            "se": torch.sqrt(n * elpd.var(unbiased=False)), "elpd_loo_i": elpd_i, "pareto_k": k_i,
            "k_threshold": k_threshold, "n_bad": n_bad}
