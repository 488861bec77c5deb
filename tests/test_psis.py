"""PSIS-LOO without a GPU: the NumPy oracle of tests/psis_cases.py against exact results (the
generalised Pareto fit on exact quantiles, a conjugate model's closed-form leave-one-out density),
its branches, the argument checks of nmx_psis_loo, and the host logic of diagnostics.loo with the
kernel calls replaced by the oracle."""
import math
import warnings

import numpy as np
import pytest

import psis_cases as PC


# ------------------------------------------------------------------------------ the oracle
def test_gpd_fit_recovers_shape():
    """Sorted exact GPD quantiles (sigma = 1, T = 4000 uniform draws each, one stream of seed 0):
    the fit gives 0.128, 0.491 and 0.892 for k = 0.1, 0.5 and 0.9."""
    rs = np.random.RandomState(0)
    for k in (0.1, 0.5, 0.9):
        u = np.sort(rs.uniform(size=4000))
        e = ((1.0 - u) ** -k - 1.0) / k
        k_hat, sigma_hat = PC.gpd_fit(e)
        print(f"k = {k}: k_hat = {k_hat:.4f}, sigma_hat = {sigma_hat:.4f}")
        assert abs(k_hat - k) <= 0.05
        assert abs(sigma_hat - 1.0) <= 0.1


def test_exact_loo_conjugate_normal():
    """y_i ~ N(mu, 1), mu ~ N(0, 10^2), N = 40 with one outlier at 4.5, S = 40000 exact posterior
    draws (psis_cases.conjugate_normal, seed 3): the oracle's largest |elpd_loo_i - exact_i| was
    measured as 2.31e-3 (at the outlier, where exact lppd_i - loo_i = 0.521); the bound is 4 x that,
    and it must stay below a tenth of the gap, so that the test tells LOO from the in-sample lppd."""
    table, loo, lppd = PC.conjugate_normal()
    elpd, k = PC.psis64(table, PC.tail_length(table.shape[0]))
    err = float(np.abs(elpd - loo).max())
    gap = float((lppd - loo)[-1])
    print(f"largest error {err:.3e}, gap at the outlier {gap:.4f}, largest k {k.max():.3f}")
    assert err < 4 * 2.31e-3
    assert err < gap / 10
    assert np.all(elpd <= lppd + 4 * 2.31e-3)
    assert np.all(k < 0.7)


def test_short_tail_is_plain_importance_sampling():
    table = PC.normal_table(20, 9, 0.7)
    assert PC.tail_length(20) == 4
    for F in (np.float64, np.float32):
        for c in range(table.shape[1]):
            elpd, k, lw, t = PC.psis_column(table[:, c], 4, F)
            assert k == np.inf and t.size <= 4 and np.array_equal(lw, t)
            ref = PC.is_loo(table[:, c])
            assert abs(elpd - ref) <= 1e-5 * (1 + abs(ref))
    elpd, k = PC.psis64(table, 4)
    assert np.all(np.isposinf(k)) and np.all(np.isfinite(elpd))


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_nonfinite_column_is_nan(value):
    table = PC.normal_table(65, 3, 0.7)
    table[17, 1] = value
    for fn in (PC.psis64, PC.psis32):
        elpd, k = fn(table, PC.tail_length(65))
        assert np.isnan(elpd[1]) and np.isnan(k[1])
        assert np.all(np.isfinite(elpd[[0, 2]])) and np.all(np.isfinite(k[[0, 2]]))


@pytest.mark.parametrize("spread", [0.2, 0.7, 1.5])
@pytest.mark.parametrize("S", [26, 257, 4097])
def test_smoothed_weights_are_nonpositive_and_ascending(S, spread):
    table = PC.normal_table(S, 9, spread)
    M = PC.tail_length(S)
    for c in range(table.shape[1]):
        elpd, k, lw, t = PC.psis_column(table[:, c], M)
        assert np.isfinite(k) and 4 < t.size <= M
        assert np.all(lw <= 0.0) and np.all(np.diff(lw) >= 0.0)
        assert not np.array_equal(lw, t)  # smoothed


def test_constant_and_floored_columns():
    """A constant column has no tail (k = +inf, elpd_loo = the constant); ratios that span more
    than e^87 put the floor log FLT_MIN at the cutoff, so that T < M."""
    S, M = 65, 13
    const = np.full(S, -1.25, np.float32)
    elpd, k, lw, t = PC.psis_column(const, M)
    assert t.size == 0 and k == np.inf and abs(elpd + 1.25) < 1e-12
    wide = np.full(S, 100.0, np.float32)
    wide[:6] = [-3.0, -2.5, -2.0, -1.0, 0.0, 0.5]  # six ratios within e^87 of the largest
    elpd, k, lw, t = PC.psis_column(wide, M)
    assert t.size == 6 < M and np.isfinite(k) and np.isfinite(elpd)


def test_float32_restatement_takes_the_same_decisions():
    for S in (20, 26, 257):
        table = PC.normal_table(S, 9, 1.5, ties=True)
        M = PC.tail_length(S)
        e64, k64 = PC.psis64(table, M)
        e32, k32 = PC.psis32(table, M)
        assert e32.dtype == np.float32 and k32.dtype == np.float32
        assert PC.same_nonfinite(k32, k64) and PC.same_nonfinite(e32, e64)


# ------------------------------------------------------------------------------ the C ABI
def test_invalid_arguments_report_errors():
    import ctypes

    from numpyro_amd import native

    lib = native.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = native.PSIS_MAX_TAIL + 1
    #        table rows ld  cols tail work elpd k     names
    cases = [(None, 8, 4, 4, 2, p, p, p, [b"table"]),
             (p, 1, 4, 4, 1, p, p, p, [b"num_rows"]),
             (p, 8, 4, 4, 0, p, p, p, [b"tail"]),
             (p, 8, 4, 4, 8, p, p, p, [b"tail", b"num_rows"]),
             (p, 8, 4, 4, 9, p, p, p, [b"tail"]),
             (p, 4 * big, 4, 4, big, p, p, p, [b"tail", b"NMX_PSIS_MAX_TAIL"]),
             (p, native.PSIS_MAX_ROWS + 1, 4, 4, 2, p, p, p, [b"num_rows", b"NMX_PSIS_MAX_ROWS"]),
             (p, 8, 3, 4, 2, p, p, p, [b"ld"]),
             (p, 8, 4, 0, 2, p, p, p, [b"num_columns"]),
             (p, 8, 4, 4, 2, None, p, p, [b"workspace"]),
             (p, 8, 4, 4, 2, p, None, None, [b"elpd_loo", b"pareto_k"])]
    for table, rows, ld, cols, tail, work, elpd, k, names in cases:
        st = lib.nmx_psis_loo(table, rows, ld, cols, tail, work, elpd, k, None)
        msg = lib.nmx_last_error()
        assert st == 1, (rows, ld, cols, tail)
        assert all(n in msg for n in names), msg


def test_workspace_bytes_and_limits():
    from numpyro_amd import native, psis

    lib = native.lib()
    assert lib.nmx_psis_workspace_bytes(1000, 7) == 4 * 7000
    assert lib.nmx_psis_workspace_bytes(1 << 20, 4096) == 4 << 32  # past 2^32: size_t arithmetic
    assert native.PSIS_MAX_TAIL >= 8192
    assert psis.tail_length(1 << 22) <= native.PSIS_MAX_TAIL  # S = 2^22 at the default M
    for S in (5, 20, 26, 4097, 70001):
        assert psis.tail_length(S) == PC.tail_length(S)
    assert [psis.tail_length(S) for S in (5, 20, 26, 1025, 4097, 70001)] == [1, 4, 6, 97, 193, 794]
    assert psis.tail_length(4096, reff=0.25) == 384
    with pytest.raises(NotImplementedError, match="NMX_PSIS_MAX_TAIL"):
        psis.check_sizes(1 << 24, psis.tail_length(1 << 24))
    with pytest.raises(NotImplementedError, match="NMX_PSIS_MAX_ROWS"):
        psis.check_sizes((1 << 24) + 1, 100)
    with pytest.raises(ValueError, match="at least 2"):
        psis.check_sizes(1, 1)
    with pytest.raises(ValueError, match="reff"):
        psis.tail_length(100, reff=0.0)


def test_header_constants_match_native():
    import os
    import re

    from numpyro_amd import native

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "numpyro_amd.h")).read()
    assert int(re.search(r"#define NMX_PSIS_MAX_TAIL (\d+)", src).group(1)) == native.PSIS_MAX_TAIL
    assert int(re.search(r"#define NMX_PSIS_MAX_ROWS (\d+)", src).group(1)) == native.PSIS_MAX_ROWS
    assert np.float32(re.search(r"#define NMX_PSIS_LOG_FLT_MIN (-[\d.]+)f", src).group(1)) == PC.LOG_FLT_MIN
    assert float(re.search(r"#define NMX_PSIS_K_ZERO (\S+)", src).group(1)) == PC.K_ZERO
    assert abs(float(PC.LOG_FLT_MIN) - math.log(float(np.finfo(np.float32).tiny))) < 4e-6  # a float32 ulp at 87


# ------------------------------------------------------------------------------ diagnostics.loo on the host
@pytest.fixture
def host_kernels(monkeypatch):
    """psis.psis_loo_table and pointwise.reduce_table replaced by float64 NumPy on the host."""
    import torch

    from numpyro_amd import pointwise, psis
    from loglik_cases import pointwise64

    def loo_table(table, reff=1.0):
        t = np.asarray(table, np.float32)
        elpd, k = PC.psis64(t, psis.tail_length(t.shape[0], reff))
        return (torch.from_numpy(elpd.astype(np.float32)).reshape(t.shape[1:]),
                torch.from_numpy(k.astype(np.float32)).reshape(t.shape[1:]))

    def reduce_table(table):
        t = np.asarray(table, np.float32)
        lppd, p_waic = pointwise64(t.reshape(t.shape[0], -1))
        return (torch.from_numpy(lppd.astype(np.float32)).reshape(t.shape[1:]),
                torch.from_numpy(p_waic.astype(np.float32)).reshape(t.shape[1:]))

    monkeypatch.setattr(psis, "psis_loo_table", loo_table)
    monkeypatch.setattr(pointwise, "reduce_table", reduce_table)


def test_diagnostics_loo_host_logic(host_kernels):
    from loglik_cases import pointwise64
    from numpyro_amd import diagnostics as D

    S, N = 257, 12
    table = PC.normal_table(S, N, 0.2).reshape(S, 3, 4)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # k stays below the threshold: no warning
        out = D.loo(table)
    elpd, k = PC.psis64(table, PC.tail_length(S))
    elpd, k = elpd.astype(np.float32).astype(np.float64), k.astype(np.float32)
    lppd = pointwise64(table.reshape(S, N))[0].astype(np.float32).astype(np.float64)
    assert out["elpd_loo"].dtype == out["se"].dtype == out["p_loo"].dtype == out["lppd"].dtype
    assert str(out["elpd_loo"].dtype) == "torch.float64"
    assert abs(float(out["elpd_loo"]) - elpd.sum()) < 1e-12 * N * 10
    assert abs(float(out["lppd"]) - lppd.sum()) < 1e-12 * N * 10
    assert abs(float(out["p_loo"]) - (lppd - elpd).sum()) < 1e-12 * N * 10
    assert abs(float(out["se"]) - math.sqrt(N * elpd.var())) < 1e-12 * N * 10
    assert out["k_threshold"] == min(1.0 - 1.0 / math.log10(S), 0.7) and out["k_threshold"] < 0.7
    assert out["n_bad"] == 0 == int((k > out["k_threshold"]).sum())
    assert tuple(out["pareto_k"].shape) == tuple(out["elpd_loo_i"].shape) == (3, 4)
    assert np.array_equal(out["pareto_k"].numpy().reshape(-1), k)
    assert np.array_equal(D.pareto_k(table).numpy(), out["pareto_k"].numpy())
    assert float(out["p_loo"]) > 0


def test_diagnostics_loo_warns_and_pools(host_kernels):
    from numpyro_amd import diagnostics as D

    S, N = 4097, 9
    table = PC.normal_table(S, N, 1.5)
    k = PC.psis64(table, PC.tail_length(S))[1].astype(np.float32)
    with pytest.warns(UserWarning, match=r"9 of 9 observations .* above 0\.70") as rec:
        whole = D.loo(table)
    assert len(rec) == 1
    assert whole["k_threshold"] == 0.7 and whole["n_bad"] == int((k > 0.7).sum()) == 9
    with pytest.warns(UserWarning, match="9 of 9"):
        parts = D.loo({"a": table[:, :4], "b": table[:, 4:]})
    for key in ("elpd_loo", "p_loo", "lppd", "se"):
        assert abs(float(parts[key]) - float(whole[key])) <= 1e-12 * (1 + abs(float(whole[key])))
    assert parts["n_bad"] == whole["n_bad"] and parts["k_threshold"] == whole["k_threshold"]
    assert set(parts["pareto_k"]) == set(parts["elpd_loo_i"]) == {"a", "b"}
    assert np.array_equal(parts["pareto_k"]["b"].numpy(), k[4:])
    assert set(D.pareto_k({"a": table[:, :4], "b": table[:, 4:]})) == {"a", "b"}
    with pytest.raises(ValueError, match="same samples"):
        D.loo({"a": table[:, :4], "b": table[:100, 4:]})
    with pytest.raises(ValueError, match="empty"):
        D.loo({})
    # a short tail (k = +inf) counts as bad
    with pytest.warns(UserWarning, match="9 of 9"):
        assert D.loo(PC.normal_table(20, 9, 0.2))["n_bad"] == 9
