"""Log-likelihood programs and the pointwise reductions on the device (csrc/loglik_program.hip):
k_program_loglik against the float64 host interpreter, the output plumbing, the reduce kernels
against float64 NumPy on synthetic tables, and log_likelihood / pointwise_predictive / lppd / waic
end to end.

Tolerance everywhere is the project's calibration rule (loglik_cases.calibrated_bound): the
device's largest |d| / (1 + |ref|) may be at most 4 x the deviation of the same arithmetic run in
float32 NumPy from the float64 run on the same inputs, plus 16 x 2^-24."""
import math

import numpy as np
import pytest
import torch

import bounded_zoo as BZ
import loglik_cases as LC
import numpyro_amd as numpyro
import predictive_cases as PC
from numpyro_amd import diagnostics
from numpyro_amd import distributions as dist
from numpyro_amd.infer import MCMC, NUTS, log_likelihood, pointwise_predictive
from numpyro_amd.infer import loglik as LL
from numpyro_amd.loglik_program import compile_log_likelihood
from numpyro_amd.pointwise import PointwiseReducer

pytestmark = pytest.mark.gpu


def _f32(samples):
    return {k: torch.as_tensor(np.asarray(v, np.float32)) for k, v in samples.items()}


def _check_calibrated(label, dev, r32, r64):
    err, bound = LC.scaled_error(dev, r64), LC.calibrated_bound(r32, r64)
    print(f"{label}: float32 host deviation {LC.scaled_error(r32, r64):.3e}, device deviation {err:.3e} "
          f"(bound {bound:.3e})")
    assert err <= bound, (label, err, bound)


# ------------------------------------------------------------------ 1. device against the interpreter
@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_device_against_float64_interpreter_whole_and_chunked(name, device, monkeypatch):
    S = 65
    case = LC.CASES[name]()
    samples = case.samples(S)
    prog = compile_log_likelihood(case.model, case.args, {}, given=samples)
    r64, r32 = prog.run_host(samples), prog.run_host(samples, dtype=np.float32)
    whole = log_likelihood(case.model, _f32(samples), *case.args)
    assert sorted(whole) == sorted(r64)
    for site, ref in r64.items():
        assert whole[site].dtype == torch.float32 and tuple(whole[site].shape) == ref.shape, (name, site)
        _check_calibrated(f"{name}.{site}", whole[site].cpu().numpy(), r32[site], ref)
    # chunks of 20 samples (20, 20, 20, 5): the device against itself, bitwise
    monkeypatch.setattr(LL, "MAX_WORKSPACE_BYTES", 20 * 4 * prog.num_slots)
    run = LL._Run(case.model, _f32(samples), case.args, {}, 1, "test")
    assert [m for _, m in run.chunks()] == [20, 20, 20, 5]
    chunked = log_likelihood(case.model, _f32(samples), *case.args)
    for site in whole:
        assert torch.equal(chunked[site], whole[site]), (name, site)
    # the streamed reduction of the same chunks, against float64 NumPy on the device's own table
    streamed = pointwise_predictive(case.model, _f32(samples), *case.args)
    for site in r64:
        table = whole[site].cpu().numpy().reshape(S, -1)
        d32, d64 = LC.pointwise32(table, chunks=[20, 20, 20, 5]), LC.pointwise64(table)
        for key, a, b in zip(("lppd", "p_waic"), d32, d64):
            _check_calibrated(f"{name}.{site}.{key} streamed", streamed[site][key].cpu().numpy().reshape(-1), a, b)


# ------------------------------------------------------------------ 2. output plumbing
def _plumbing_model(y63, y66, ys, y1, y64, y129, yc, y7):
    mu = numpyro.sample("mu", dist.Normal(0.0, 1.0))
    sd = numpyro.sample("sd", dist.HalfNormal(1.0))
    with numpyro.plate("a", 63):
        numpyro.sample("y63", dist.Normal(mu, sd), obs=y63)
    with numpyro.plate("b", 66):
        numpyro.sample("y66", dist.StudentT(4.0, mu, sd), obs=y66)
    numpyro.sample("ys", dist.Normal(mu, 2.0), obs=ys)  # a scalar site
    with numpyro.plate("p1", 1):
        numpyro.sample("y1", dist.Normal(mu, sd), obs=y1)
    with numpyro.plate("p64", 64):
        numpyro.sample("y64", dist.Normal(mu, sd), obs=y64)
    with numpyro.plate("p129", 129):
        numpyro.sample("y129", dist.Cauchy(mu, sd), obs=y129)
    numpyro.sample("yc", dist.Normal(0.5, 2.0), obs=yc)  # no latent: a host constant
    with numpyro.plate("p7", 7):
        numpyro.sample("y7", dist.Uniform(0.0, 1.0 + sd), obs=y7)  # one value under 7 elements


def test_output_plumbing(device):
    rs = np.random.RandomState(7)
    args = tuple(rs.randn(n) for n in (63, 66)) + (np.float64(0.3),) + tuple(rs.randn(n) for n in (1, 64, 129)) + \
        (rs.randn(3), rs.uniform(0.05, 0.95, 7))
    S = 5
    samples = {"mu": rs.randn(S).astype(np.float32).astype(np.float64),
               "sd": (0.5 + np.abs(rs.randn(S))).astype(np.float32).astype(np.float64)}
    prog = compile_log_likelihood(_plumbing_model, args, {}, given=samples)
    by = {o.name: o for o in prog.outputs}
    assert [(o.name, o.n, o.column) for o in prog.outputs] == [
        ("y63", 63, 0), ("y66", 66, 63), ("ys", 1, 129), ("y1", 1, 130), ("y64", 64, 131), ("y129", 129, 195),
        ("y7", 1, 324)], prog.outputs
    assert by["y7"].shape == (7,) and by["ys"].shape == () and list(prog.constant_outputs) == ["yc"]
    r64, r32 = prog.run_host(samples), prog.run_host(samples, dtype=np.float32)
    got = log_likelihood(_plumbing_model, _f32(samples), *args)
    assert list(got) == ["y63", "y66", "ys", "y1", "y64", "y129", "y7", "yc"]
    for site, ref in r64.items():
        assert tuple(got[site].shape) == ref.shape and got[site].is_contiguous(), (site, got[site].shape, ref.shape)
        _check_calibrated(f"plumbing.{site}", got[site].cpu().numpy(), r32[site], ref)
    assert torch.equal(got["y7"], got["y7"][:, :1].expand(S, 7))
    assert torch.equal(got["yc"].cpu(), torch.as_tensor(r32["yc"]))
    pw = pointwise_predictive(_plumbing_model, _f32(samples), *args)
    for site, ref in r64.items():
        lppd64, _ = LC.pointwise64(ref.reshape(S, -1))
        assert tuple(pw[site]["lppd"].shape) == ref.shape[1:] == tuple(pw[site]["p_waic"].shape), site
        err = LC.scaled_error(pw[site]["lppd"].cpu().numpy().reshape(-1), lppd64)
        assert err <= 1e-5, (site, err)  # plumbing only: the reductions are held to their bound below
    assert torch.equal(pw["yc"]["p_waic"].cpu(), torch.zeros(3))
    # two leading batch dimensions, and none
    two = log_likelihood(_plumbing_model, {k: v.reshape(1, S) for k, v in _f32(samples).items()}, *args,
                         batch_ndims=2)
    assert tuple(two["y66"].shape) == (1, S, 66) and torch.equal(two["y66"][0], got["y66"])
    none = log_likelihood(_plumbing_model, {k: v[2] for k, v in _f32(samples).items()}, *args, batch_ndims=0)
    assert tuple(none["y66"].shape) == (66,) and torch.equal(none["y66"], got["y66"][2])
    assert tuple(none["ys"].shape) == () and tuple(none["yc"].shape) == (3,)


# ------------------------------------------------------------------ 3. the reduce kernels
ROWS = (1, 2, 63, 64, 65, 257)
COLUMNS = (1, 18, 63, 64, 65, 129)


def _reduce(table, chunks=None):
    """(lppd, p_waic) float32 NumPy of a device table [S, >= C] through the reduce kernels."""
    red = PointwiseReducer(table.shape[1], table.device)
    r = 0
    for rows in (chunks or [table.shape[0]]):
        red.accumulate(table[r:r + rows])
        r += rows
    lppd, p_waic = red.finish()
    return lppd.cpu().numpy(), p_waic.cpu().numpy()


def _check_reduction(label, dev, r32, r64):
    for key, d, a, b in zip(("lppd", "p_waic"), dev, r32, r64):
        if np.all(np.isnan(b)):  # S = 1: no variance
            assert np.all(np.isnan(d)) and np.all(np.isnan(a)), (label, key)
            continue
        _check_calibrated(f"{label}.{key}", d, a, b)


@pytest.mark.parametrize("S", ROWS)
def test_reduce_kernels_against_numpy(S, device):
    rs = np.random.RandomState(S)
    for C in COLUMNS:
        t = rs.normal(-50.0, 30.0, (S, C)).astype(np.float32)
        r64, r32 = LC.pointwise64(t), LC.pointwise32(t)
        dt = torch.from_numpy(t).to(device)
        dev = _reduce(dt)
        _check_reduction(f"S{S}xC{C}", dev, r32, r64)
        again = _reduce(dt)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(dev, again)), (S, C, "two launches differ")
        # ld larger than the column count: the same columns inside a wider table
        wide = torch.full((S, C + 5), float("nan"), device=device)
        wide[:, :C] = dt
        red = PointwiseReducer(C, device)
        red.accumulate(wide)
        strided = [x.cpu().numpy() for x in red.finish()]
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(dev, strided)), (S, C, "ld > columns differs")
        assert np.array_equal(diagnostics.lppd(dt).cpu().numpy(), dev[0], equal_nan=True)


@pytest.mark.parametrize("C", (18, 129))
def test_reduce_in_chunks_matches_one_pass(C, device):
    S, chunks = 257, [100, 100, 57]
    t = np.random.RandomState(C).normal(-50.0, 30.0, (S, C)).astype(np.float32)
    r64 = LC.pointwise64(t)
    dt = torch.from_numpy(t).to(device)
    _check_reduction(f"one pass C{C}", _reduce(dt), LC.pointwise32(t), r64)
    dev = _reduce(dt, chunks)
    _check_reduction(f"chunks of 100 C{C}", dev, LC.pointwise32(t, chunks), r64)
    again = _reduce(dt, chunks)
    assert all(np.array_equal(a, b) for a, b in zip(dev, again))


@pytest.mark.parametrize("S,C", ((65, 18), (65, 129), (257, 64), (2, 5)))
def test_reduce_special_columns(S, C, device):
    """Column 0 all -inf, column 1 one -inf, column 2 one NaN, column 3 one +inf; the others finite."""
    rs = np.random.RandomState(S + C)
    t = rs.normal(-50.0, 30.0, (S, C)).astype(np.float32)
    t[:, 0] = -np.inf
    t[S // 2, 1] = -np.inf
    t[S - 1, 2] = np.nan
    t[0, 3] = np.inf
    lppd, p_waic = _reduce(torch.from_numpy(t).to(device))
    l32, p32 = LC.pointwise32(t)
    l64, p64 = LC.pointwise64(t)
    assert lppd[0] == -np.inf and np.isnan(p_waic[0])
    assert np.isfinite(lppd[1]) and np.isnan(p_waic[1])
    assert np.isnan(lppd[2]) and np.isnan(p_waic[2])
    assert lppd[3] == np.inf and np.isnan(p_waic[3])
    assert np.all(np.isfinite(lppd[4:])) and np.all(np.isfinite(p_waic[4:]))
    _check_calibrated(f"special S{S}xC{C}.lppd", lppd[[1, *range(4, C)]], l32[[1, *range(4, C)]],
                      l64[[1, *range(4, C)]])
    _check_calibrated(f"special S{S}xC{C}.p_waic", p_waic[4:], p32[4:], p64[4:])


def test_one_sample_has_no_variance(device):
    t = torch.tensor([[-1.5, -2.5, float("-inf")]], device=device)
    lppd, p_waic = _reduce(t)
    assert np.array_equal(lppd, np.array([-1.5, -2.5, -np.inf], np.float32)) and np.all(np.isnan(p_waic))


# ------------------------------------------------------------------ 4. end to end
def _waic_numpy(table):
    lppd, p = LC.pointwise64(table)
    elpd = lppd - p
    return {"elpd_waic": elpd.sum(), "p_waic": p.sum(), "lppd": lppd.sum(), "se": math.sqrt(elpd.size * elpd.var())}


def test_partially_pooled_end_to_end(device):
    S = 512
    case = LC.CASES["partially_pooled"]()
    samples = _f32(case.samples(S))
    ll = log_likelihood(case.model, samples, *case.args, parallel=True)["obs"]
    assert tuple(ll.shape) == (S, 18) and ll.dtype == torch.float32 and ll.device.type == "cuda"
    table = ll.cpu().numpy().astype(np.float64)
    ref = (torch.logsumexp(ll.double(), 0) - math.log(S)).cpu().numpy()
    l64, p64 = LC.pointwise64(table)
    np.testing.assert_allclose(ref, l64, rtol=1e-12)
    l32, p32 = LC.pointwise32(table)
    pw = pointwise_predictive(case.model, samples, *case.args)["obs"]
    # pointwise_predictive recomputes the table: the same kernel on the same inputs, the same bits
    _check_calibrated("pointwise_predictive.lppd", pw["lppd"].cpu().numpy(), l32, ref)
    _check_calibrated("pointwise_predictive.p_waic", pw["p_waic"].cpu().numpy(), p32, p64)
    _check_calibrated("diagnostics.lppd", diagnostics.lppd(ll).cpu().numpy(), l32, ref)
    assert torch.equal(diagnostics.lppd(ll), pw["lppd"]) and torch.equal(diagnostics.lppd({"obs": ll})["obs"], pw["lppd"])
    # the printed figure of examples/baseball.py
    total = (torch.logsumexp(ll, 0) - math.log(ll.shape[0])).sum()
    assert abs(float(total) - l64.sum()) <= 1e-4 * (1.0 + abs(l64.sum()))
    w, w64 = diagnostics.waic(ll), _waic_numpy(table)
    e32 = l32.astype(np.float64) - p32.astype(np.float64)
    w32 = {"elpd_waic": e32.sum(), "p_waic": p32.astype(np.float64).sum(), "lppd": l32.astype(np.float64).sum(),
           "se": math.sqrt(e32.size * e32.var())}
    assert sorted(w) == sorted(w64)
    for key, ref_value in w64.items():
        _check_calibrated(f"waic.{key}", float(w[key]), w32[key], ref_value)
    # a dict of tables pools their observations (other column counts: other merge orders)
    both = diagnostics.waic({"a": ll[:, :7], "b": ll[:, 7:]})
    for key in w:
        assert abs(float(both[key]) - float(w[key])) <= 1e-4 * (1.0 + abs(float(w[key]))), key


@pytest.mark.parametrize("name", ["fully_pooled", "not_pooled", "partially_pooled", "partially_pooled_with_logit"])
def test_baseball_predict_runs_on_mcmc_draws(name, device):
    """The last lines of examples/baseball.py predict(), with numpyro_amd's names."""
    case = BZ.CASES[name]()
    at_bats, hits = case.args
    mcmc = MCMC(NUTS(case.model), num_warmup=50, num_samples=20, num_chains=16, progress_bar=False)
    mcmc.run(0, at_bats, hits)
    z = mcmc.get_samples()
    post_loglik = log_likelihood(case.model, z, at_bats, hits)["obs"]
    assert tuple(post_loglik.shape) == (320, 18) and bool(torch.isfinite(post_loglik).all())
    exp_log_density = (torch.logsumexp(post_loglik, 0) - math.log(post_loglik.shape[0])).sum()
    assert math.isfinite(float(exp_log_density))
    host = {k: v.cpu().numpy().astype(np.float64) for k, v in z.items()}
    prog = compile_log_likelihood(case.model, case.args, {}, given=host)
    r64, r32 = prog.run_host(host)["obs"], prog.run_host(host, dtype=np.float32)["obs"]
    _check_calibrated(f"{name} on MCMC draws", post_loglik.cpu().numpy(), r32, r64)
    grouped = log_likelihood(case.model, mcmc.get_samples(group_by_chain=True), at_bats, hits, batch_ndims=2)["obs"]
    assert tuple(grouped.shape) == (16, 20, 18) and torch.equal(grouped.reshape(320, 18), post_loglik)
    lppd = pointwise_predictive(case.model, z, at_bats, hits)["obs"]["lppd"]
    assert abs(float(lppd.sum()) - float(exp_log_density)) <= 1e-4 * (1.0 + abs(float(exp_log_density)))


def test_model_function_that_nuts_maps_to_a_fused_kernel(device):
    """Eight schools written with numpyro_amd.sample: NUTS runs it on the fused kernel, log_likelihood
    traces it the program way."""
    from numpyro_amd import datasets

    sigma = np.asarray(datasets.EIGHT_SCHOOLS_SIGMA, np.float64)
    y = np.asarray(datasets.EIGHT_SCHOOLS_Y, np.float64)
    rs = np.random.RandomState(3)
    S = 33
    samples = {"mu": rs.randn(S), "tau": 0.5 + np.abs(rs.randn(S)), "theta": 5.0 * rs.randn(S, 8)}
    samples = {k: v.astype(np.float32).astype(np.float64) for k, v in samples.items()}
    got = log_likelihood(PC.eight_schools_model, _f32(samples), 8, sigma, y=y)["obs"]
    ref = torch.distributions.Normal(torch.as_tensor(samples["theta"]), torch.as_tensor(sigma)).log_prob(torch.as_tensor(y))
    assert tuple(got.shape) == (S, 8)
    assert LC.scaled_error(got.cpu().numpy(), ref.numpy()) <= 1e-5
