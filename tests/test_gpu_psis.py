"""PSIS-LOO on the device (csrc/psis.hip): k_psis_transpose / k_psis_column against the NumPy
oracle of tests/psis_cases.py over the sizes at which the kernel takes another path, explicit tail
lengths through the C ABI, column counts and layouts, determinism, the special columns, and
infer.loo / diagnostics.loo end to end.

Tolerance everywhere is the project's calibration rule (loglik_cases.calibrated_bound): the
device's largest |d| / (1 + |ref|) over the finite entries may be at most 4 x the deviation of the
float32 restatement (psis32) from the float64 one (psis64) on the same table, plus 16 x 2^-24;
the non-finite entries (k = +inf of a short tail, NaN of a non-finite column) must be equal."""
import functools
import math
import warnings

import numpy as np
import pytest
import torch

import loglik_cases as LC
import psis_cases as PC
from numpyro_amd import diagnostics, native
from numpyro_amd.infer import log_likelihood, loo
from numpyro_amd.psis import psis_loo_columns, psis_loo_table, tail_length

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(S, spread, ties=False, N=9, M=None):
    """(table, M, psis32, psis64), computed once and shared (read only)."""
    table = PC.normal_table(S, N, spread, ties=ties)
    M = PC.tail_length(S) if M is None else M
    table.setflags(write=False)
    return table, M, PC.psis32(table, M), PC.psis64(table, M)


def _check(label, dev, r32, r64):
    """dev, r32, r64: (elpd_loo, pareto_k) triples of arrays."""
    for name, d, a, b in zip(("elpd_loo", "pareto_k"), dev, r32, r64):
        d, a, b = (np.asarray(v, np.float64).reshape(-1) for v in (d, a, b))
        assert PC.same_nonfinite(d, b), (label, name, d, b)
        assert PC.same_nonfinite(a, b), (label, name, "the float32 restatement took another decision")
        fin = np.isfinite(b)
        if not fin.any():
            continue
        err, bound = LC.scaled_error(d[fin], b[fin]), LC.calibrated_bound(a[fin], b[fin])
        print(f"{label}.{name}: float32 host deviation {LC.scaled_error(a[fin], b[fin]):.3e}, device deviation "
              f"{err:.3e} (bound {bound:.3e})")
        assert err <= bound, (label, name, err, bound)


def _native(table, M, num_columns=None, fill=None, outputs=(True, True)):
    """nmx_psis_loo on a device tensor [S, ld]; ``fill``: the byte the workspace holds before."""
    S, ld = table.shape[0], table.stride(0)
    N = table.shape[1] if num_columns is None else num_columns
    lib = native.lib()
    work = torch.empty(lib.nmx_psis_workspace_bytes(S, N), dtype=torch.uint8, device=table.device)
    if fill is not None:
        work.fill_(fill)
    elpd = torch.full((N,), -7.0, device=table.device) if outputs[0] else None
    k = torch.full((N,), -7.0, device=table.device) if outputs[1] else None
    native.check(lib.nmx_psis_loo(native.ptr(table), S, ld, N, M, native.ptr(work), native.ptr(elpd), native.ptr(k),
                                  native.stream_ptr()), "nmx_psis_loo")
    torch.cuda.synchronize()
    return elpd, k


def _np(pair):
    return tuple(v.cpu().numpy() for v in pair)


# ------------------------------------------------------------------ 1. against the oracle
SIZES = (5, 20, 26, 63, 64, 65, 257, 1025, 4097, 70001)
REGIMES = [(0.2, False), (0.7, False), (1.5, False), (0.7, True)]


@pytest.mark.parametrize("spread,ties", REGIMES, ids=["k0.2", "k0.7", "k1.5", "ties"])
@pytest.mark.parametrize("S", SIZES)
def test_against_oracle(S, spread, ties, device):
    table, M, r32, r64 = _case(S, spread, ties)
    assert M == tail_length(S)
    dev = psis_loo_table(torch.tensor(table).to(device))
    assert all(v.dtype == torch.float32 and tuple(v.shape) == (9,) and v.device.type == "cuda" for v in dev)
    _check(f"S={S} spread={spread} ties={ties}", _np(dev), r32, r64)
    if S == 20:
        assert np.all(np.isposinf(r64[1]))  # the T <= 4 branch
    if S >= 26 and not ties:
        assert np.all(np.isfinite(r64[1]))  # a smoothed tail


@pytest.mark.parametrize("S,M", [(65, 64), (65, 1), (4097, 1), (4097, 2048)])
def test_explicit_tail_through_the_native_call(S, M, device):
    table, _, r32, r64 = _case(S, 0.7, M=M)
    dev = _native(torch.tensor(table).to(device), M)
    _check(f"S={S} M={M}", _np(dev), r32, r64)
    if M == 2048:
        assert np.all(np.isfinite(r64[1]))


def test_either_output_may_be_absent(device):
    table, M, _, _ = _case(257, 0.7)
    t = torch.tensor(table).to(device)
    elpd, k = _native(t, M)
    only_elpd, none = _native(t, M, outputs=(True, False))
    none2, only_k = _native(t, M, outputs=(False, True))
    assert none is None and none2 is None
    assert torch.equal(only_elpd, elpd) and torch.equal(only_k, k)


# ------------------------------------------------------------------ 2. column counts and layout
@pytest.mark.parametrize("N", [1, 18, 65, 129])
def test_columns_are_independent_of_the_table(N, device):
    S = 257
    table, M, r32, r64 = _case(S, 0.7, N=N)
    t = torch.tensor(table).to(device)
    elpd, k = _native(t, M)
    _check(f"N={N}", _np((elpd, k)), r32, r64)
    for c in sorted({0, N // 2, N - 1}):  # the column alone, in a table of its own: the same bits
        e1, k1 = _native(t[:, c:c + 1].contiguous(), M)
        assert torch.equal(e1, elpd[c:c + 1]) and torch.equal(k1, k[c:c + 1]), c
    # ld > N, NaN in the padding columns
    wide = torch.full((S, N + 5), float("nan"), device=device)
    wide[:, :N] = t
    e2, k2 = _native(wide, M, num_columns=N)
    assert torch.equal(e2, elpd) and torch.equal(k2, k)
    e3, k3 = psis_loo_columns(wide, N, M)
    assert torch.equal(e3, elpd) and torch.equal(k3, k)


def test_non_contiguous_tables(device):
    table, M, _, _ = _case(257, 0.7, N=18)
    t = torch.tensor(table).to(device)
    ref = psis_loo_table(t)
    tt = t.T.contiguous().T  # [S, N] with unit row stride
    assert tt.stride(1) != 1
    got = psis_loo_table(tt)  # psis_loo_table makes its own contiguous copy
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    with pytest.raises(ValueError, match="PSIS table"):
        psis_loo_columns(tt, 18, M)
    with pytest.raises(ValueError, match="PSIS table"):
        psis_loo_columns(t.double(), 18, M)
    with pytest.raises(ValueError, match="PSIS table"):
        psis_loo_columns(t, 19, M)
    # trailing dimensions come back; arrays are accepted
    e, k = psis_loo_table(np.array(table).reshape(257, 3, 6))
    assert tuple(e.shape) == tuple(k.shape) == (3, 6)
    assert torch.equal(e.reshape(-1), ref[0]) and torch.equal(k.reshape(-1), ref[1])


# ------------------------------------------------------------------ 3. determinism and the workspace
@pytest.mark.parametrize("S", [65, 70001])
def test_two_launches_are_bitwise_equal_whatever_the_workspace_held(S, device):
    table, M, _, _ = _case(S, 0.7)
    t = torch.tensor(table).to(device)
    a = _native(t, M, fill=0)
    b = _native(t, M, fill=0)
    c = _native(t, M, fill=0xFF)
    for x, y in ((a, b), (a, c)):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])


# ------------------------------------------------------------------ 4. special columns
@pytest.mark.parametrize("S", [65, 1025])
def test_special_columns(S, device):
    base, M, _, _ = _case(S, 0.7)
    table = np.array(base[:, [0, 1, 2, 3, 4, 5, 6, 7, 8, 0, 1]])  # 11 columns; the odd ones become special
    table[S // 3, 1] = np.nan
    table[S - 1, 3] = np.inf
    table[0, 5] = -np.inf
    table[:, 7] = -1.25                      # constant: T = 0
    table[:, 9] = 100.0                      # ratios spanning more than e^87: the floor is the cutoff
    table[:6, 9] = [-3.0, -2.5, -2.0, -1.0, 0.0, 0.5]
    r32, r64 = PC.psis32(table, M), PC.psis64(table, M)
    assert np.isnan(r64[0][[1, 3, 5]]).all() and np.isnan(r64[1][[1, 3, 5]]).all()
    assert np.isposinf(r64[1][7]) and abs(r64[0][7] + 1.25) < 1e-12
    assert PC.psis_column(table[:, 9], M)[3].size == 6 < M and np.isfinite(r64[1][9])
    dev = psis_loo_table(torch.tensor(table).to(device))
    _check(f"special S={S}", _np(dev), r32, r64)
    # the finite neighbours are what they are in the table without the special columns
    ref = psis_loo_table(torch.tensor(base).to(device))
    for c, b in ((0, 0), (2, 2), (4, 4), (6, 6), (8, 8), (10, 1)):
        assert torch.equal(dev[0][c], ref[0][b]) and torch.equal(dev[1][c], ref[1][b]), c


# ------------------------------------------------------------------ 5. end to end
def _f32(samples):
    return {k: torch.as_tensor(np.asarray(v, np.float32)) for k, v in samples.items()}


def _loo_numpy(elpd, lppd):
    elpd, lppd = np.asarray(elpd, np.float64), np.asarray(lppd, np.float64)
    return {"elpd_loo": elpd.sum(), "p_loo": (lppd - elpd).sum(), "lppd": lppd.sum(),
            "se": math.sqrt(elpd.size * elpd.var())}


def test_partially_pooled_end_to_end(device):
    S = 512
    case = LC.CASES["partially_pooled"]()
    samples = _f32(case.samples(S))
    ll = log_likelihood(case.model, samples, *case.args)["obs"]
    assert tuple(ll.shape) == (S, 18)
    M = tail_length(S)
    table = ll.cpu().numpy()
    r32, r64 = PC.psis32(table, M), PC.psis64(table, M)
    direct = psis_loo_table(ll)
    _check("psis_loo_table", _np(direct), r32, r64)
    # infer.loo recomputes the table: the same kernels on the same inputs, the same bits
    site = loo(case.model, samples, *case.args)["obs"]
    assert sorted(site) == ["elpd_loo", "lppd", "pareto_k"]
    assert torch.equal(site["elpd_loo"], direct[0]) and torch.equal(site["pareto_k"], direct[1])
    assert torch.equal(site["lppd"], diagnostics.lppd(ll))
    assert torch.equal(diagnostics.pareto_k(ll), direct[1])
    assert torch.equal(diagnostics.pareto_k({"obs": ll})["obs"], direct[1])
    # diagnostics.loo against the oracle's sums
    l32, _ = LC.pointwise32(table.astype(np.float64))
    l64, _ = LC.pointwise64(table.astype(np.float64))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        out = diagnostics.loo(ll)
        both = diagnostics.loo({"a": ll[:, :7], "b": ll[:, 7:]})
    w32, w64 = _loo_numpy(r32[0], l32), _loo_numpy(r64[0], l64)
    for key, ref_value in w64.items():
        assert out[key].dtype == torch.float64
        err, bound = LC.scaled_error(float(out[key]), ref_value), LC.calibrated_bound(w32[key], ref_value)
        print(f"loo.{key}: device {float(out[key]):.6f}, float64 {ref_value:.6f}, deviation {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (key, err, bound)
    assert out["k_threshold"] == min(1.0 - 1.0 / math.log10(S), 0.7)
    assert out["n_bad"] == int((r64[1] > out["k_threshold"]).sum())
    assert torch.equal(out["elpd_loo_i"], direct[0]) and torch.equal(out["pareto_k"], direct[1])
    # a dict of tables pools their observations: a column's elpd_loo is the same bits in any table
    # (the lppd of the pointwise kernels merges in another order at another column count)
    assert float(both["elpd_loo"]) == float(out["elpd_loo"]) and float(both["se"]) == float(out["se"])
    for key in w64:
        assert abs(float(both[key]) - float(out[key])) <= 1e-5 * (1.0 + abs(float(out[key]))), key
    assert both["n_bad"] == out["n_bad"]
    assert torch.equal(torch.cat([both["pareto_k"]["a"], both["pareto_k"]["b"]]), direct[1])
    assert float(out["p_loo"]) > 0
    assert bool((out["elpd_loo_i"] <= site["lppd"]).all())


def test_loo_refuses_a_table_above_the_limit(device, monkeypatch):
    from numpyro_amd.infer import loglik as LL

    case = LC.CASES["partially_pooled"]()
    samples = _f32(case.samples(64))
    monkeypatch.setattr(LL, "MAX_LOO_BYTES", 2 * 4 * 64 * 18 - 1)
    with pytest.raises(NotImplementedError, match=r"S = 64 .* N = 18 .* 9216 bytes.*thin"):
        loo(case.model, samples, *case.args)
    monkeypatch.setattr(LL, "MAX_LOO_BYTES", 2 * 4 * 64 * 18)
    assert tuple(loo(case.model, samples, *case.args)["obs"]["pareto_k"].shape) == (18,)


def test_conjugate_normal_against_exact_loo(device):
    """The table of test_psis.test_exact_loo_conjugate_normal (S = 40000): the device is within the
    calibrated bound of the oracle, and so within that test's bound (4 x 2.31e-3) of exact LOO."""
    table, exact, lppd = PC.conjugate_normal()
    M = PC.tail_length(table.shape[0])
    r32, r64 = PC.psis32(table, M), PC.psis64(table, M)
    dev = _np(psis_loo_table(table))
    _check("conjugate normal", dev, r32, r64)
    err = float(np.abs(dev[0].astype(np.float64) - exact).max())
    print(f"largest |elpd_loo_i - exact_i| on the device: {err:.3e}")
    assert err < 4 * 2.31e-3 and err < float((lppd - exact)[-1]) / 10
