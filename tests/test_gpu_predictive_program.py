"""Predictive on the program path on the GPU (numpyro_amd.infer.Predictive for a traced model
function, csrc/predictive_program.hip) against the oracle's predictive draws and the float64 host
interpreter on the same Philox words (PredictiveProgram.run_host), plus distribution checks.
The comparison rules are predictive_cases.compare's: discrete sites equal except a share of
1e-3, sites that are a monotone map of one normal or exponential within 1e-4 (1 + |ref|), gamma-
based and Cauchy sites within 4 x the float32 host run's own deviation from the float64 run."""
import numpy as np
import pytest
import torch

import numpyro_amd as numpyro
import predictive_cases as PC
import program_zoo as Zoo
from numpyro_amd import datasets
from numpyro_amd import distributions as dist
from numpyro_amd import jnp
from numpyro_amd.infer import MCMC, NUTS, Predictive
from numpyro_amd.predictive_program import compile_predictive
from oracle import predictive as OPred

pytestmark = pytest.mark.gpu


def _torch(samples):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in samples.items()}


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


# ------------------------------------------------------------------ 1, 2: against the oracle
def test_eight_schools_function_matches_oracle(device):
    """The README's eight schools written as a model function: Predictive draws obs ~ Normal(theta,
    sigma) on the program kernel, on the words of nmx_predict_normal."""
    J, S = 8, 40
    sigma = np.asarray(datasets.EIGHT_SCHOOLS_SIGMA, np.float64)
    rs = np.random.RandomState(4)
    samples = {"mu": rs.randn(S).astype(np.float32), "tau": (np.abs(rs.randn(S)) + 0.1).astype(np.float32),
               "theta": (5 * rs.randn(S, J)).astype(np.float32)}
    out = Predictive(PC.eight_schools_model, _torch(samples))(11, J, sigma)
    assert set(out) == {"obs"} and out["obs"].shape == (S, J) and out["obs"].dtype == torch.float32
    ref = OPred.predict_normal(samples["theta"].astype(np.float64), sigma, 11)
    np.testing.assert_allclose(out["obs"].cpu().numpy(), ref, rtol=1e-4, atol=1e-4 * np.max(sigma))


@pytest.mark.parametrize("N", [25, 65])
def test_logit_model_matches_oracle(device, N):
    S = 40
    case = Zoo.logit(N=N)
    samples = PC.posterior_like(case, S, seed=N)
    out = Predictive(case.model, _torch(samples))(9, *PC.unobserved_args(case))["y"]
    assert out.shape == (S, N) and out.dtype == torch.int32
    X1 = np.concatenate([np.ones((N, 1)), case.args[0]], 1)
    coefs = np.concatenate([samples["b0"][:, None], samples["b"]], 1).astype(np.float64)
    ref, p, u = OPred.predict_logreg(X1, coefs, 9)
    mismatch = out.cpu().numpy() != ref
    print(f"logit N={N}: mismatch share {mismatch.mean():.2e}")
    assert mismatch.mean() <= 1e-3
    assert np.all(np.abs(u[mismatch] - p[mismatch]) < 1e-5)


# ------------------------------------------------------------------ 3: device vs host interpreter
@pytest.mark.parametrize("name", sorted(Zoo.CASES))
def test_zoo_models_match_the_host_interpreter(device, name):
    S, seed = 7, 21
    case = Zoo.CASES[name]()
    samples = PC.posterior_like(case, S, seed=1)
    args = PC.unobserved_args(case)
    out = _np(Predictive(case.model, _torch(samples))(seed, *args))
    prog = compile_predictive(case.model, args, {}, samples)
    r64, r32, flipped = PC.host_runs(prog, samples, seed)
    assert set(out) == set(PC.SITE_RULE[name]) == set(r64)
    for site, rule in PC.SITE_RULE[name].items():
        assert out[site].dtype == (np.int32 if rule == "discrete" else np.float32)
        PC.compare(f"{name}.{site}", rule, out[site], r64[site], r32[site], flipped[site])


# ------------------------------------------------------------------ 4: the lane mapping
def _plate_model(n, vector_parameters):
    def model(loc, rate):
        s = numpyro.sample("s", dist.HalfNormal(1.0))  # scalar, given
        v = numpyro.sample("v", dist.Normal(np.zeros(n), np.ones(n)))  # vector, given
        with numpyro.plate("n", n):
            if vector_parameters:
                numpyro.sample("normal", dist.Normal(v + loc, jnp.exp(0.3 * v)))
                numpyro.sample("gamma", dist.Gamma(jnp.exp(0.5 * v) + 0.2, rate))
                numpyro.sample("poisson", dist.Poisson(jnp.exp(v) * rate))
                numpyro.sample("bernoulli", dist.Bernoulli(logits=v))
            else:
                numpyro.sample("normal", dist.Normal(s, s))
                numpyro.sample("gamma", dist.Gamma(s, 2.0))
                numpyro.sample("poisson", dist.Poisson(s * 8.0))
                numpyro.sample("bernoulli", dist.Bernoulli(probs=s / (1.0 + s)))
                numpyro.sample("exponential", dist.Exponential(s))

    return model


@pytest.mark.parametrize("vector_parameters", [False, True], ids=["scalar_parameters", "vector_parameters"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_plate_sizes_around_the_wave(device, n, vector_parameters):
    """One sample (S = 1); a plate of fewer, exactly, and more elements than the 64 lanes; scalar
    parameters broadcast to the site (a barrier before the draw) and per-element parameters."""
    rs = np.random.RandomState(n)
    samples = {"s": (0.5 + np.abs(rs.randn(1))).astype(np.float32), "v": rs.randn(1, n).astype(np.float32)}
    args = (np.linspace(-1.0, 1.0, n), np.linspace(1.0, 12.0, n))  # rates on both sides of the PTRS threshold
    model = _plate_model(n, vector_parameters)
    out = _np(Predictive(model, _torch(samples))(5, *args))
    prog = compile_predictive(model, args, {}, samples)
    r64, r32, flipped = PC.host_runs(prog, samples, 5)
    rules = {"normal": "monotone", "gamma": "calibrated", "poisson": "discrete", "bernoulli": "discrete",
             "exponential": "monotone"}
    assert set(out) == set(r64)
    for site in r64:  # at these sizes the shares of 1e-3 allow no mismatch and no excluded element
        assert out[site].shape == (1, n)
        PC.compare(f"n={n}.{site}", rules[site], out[site], r64[site], r32[site], flipped[site])


# ------------------------------------------------------------------ 5, 6: chunking, determinism, layout
def test_chunks_draw_what_the_whole_call_draws(device):
    case = Zoo.CASES["treg"]()
    samples = _torch(PC.posterior_like(case, 5))
    args = PC.unobserved_args(case)
    whole = Predictive(case.model, samples)(3, *args)["y"]
    slots = compile_predictive(case.model, args, {}, samples).num_slots
    chunked = Predictive(case.model, samples, max_workspace_bytes=2 * slots * 4 + 4)(3, *args)["y"]
    assert torch.equal(whole, chunked)
    with pytest.raises(NotImplementedError, match="max_workspace_bytes"):
        Predictive(case.model, samples, max_workspace_bytes=slots * 4 - 4)(3, *args)


def test_determinism_layout_and_returned_sites(device):
    def model(X, y=None):
        b = numpyro.sample("b", dist.Normal(np.zeros(3), np.ones(3)))
        eta = numpyro.deterministic("eta", jnp.matmul(X, b))
        y = numpyro.sample("y", dist.Poisson(jnp.exp(eta)), obs=y)
        if not isinstance(y, np.ndarray):
            numpyro.deterministic("total", jnp.sum(y))

    rs = np.random.RandomState(0)
    X = 0.5 * rs.randn(10, 3)
    b = rs.randn(4, 6, 3).astype(np.float32)
    flat = {"b": torch.from_numpy(b.reshape(24, 3))}
    one = Predictive(model, flat)(3, X)
    two = Predictive(model, flat)(3, X)
    assert set(one) == {"y", "eta", "total"} and all(torch.equal(one[k], two[k]) for k in one)
    assert one["y"].dtype == torch.int32 and one["eta"].dtype == torch.float32 and one["total"].shape == (24,)
    assert torch.equal(one["total"], one["y"].sum(1).to(torch.float32))  # whole numbers: exact in f32
    np.testing.assert_allclose(one["eta"].cpu().numpy(), b.reshape(24, 3) @ X.T.astype(np.float32), rtol=1e-4, atol=1e-5)
    assert not torch.equal(one["y"], Predictive(model, flat)(4, X)["y"])  # another key, other draws
    # batch_ndims = 2 is the flattened call
    nested = Predictive(model, {"b": torch.from_numpy(b)}, batch_ndims=2)(3, X)
    assert nested["y"].shape == (4, 6, 10) and nested["total"].shape == (4, 6) and nested["eta"].shape == (4, 6, 10)
    assert all(torch.equal(nested[k].reshape(one[k].shape), one[k]) for k in one)
    # observed data passed is returned as given
    y = rs.poisson(2.0, 10).astype(np.float64)
    kept = Predictive(model, flat)(3, X, y)
    assert set(kept) == {"y", "eta"}
    assert torch.equal(kept["y"].cpu(), torch.from_numpy(y.astype(np.int32)).expand(24, 10))
    # return_sites: a given latent comes back as given, with a deterministic site
    some = Predictive(model, flat, return_sites=["b", "eta", "total"])(3, X)
    assert set(some) == {"b", "eta", "total"} and torch.equal(some["b"].cpu(), flat["b"])
    assert torch.equal(some["total"], one["total"]) and torch.equal(some["eta"], one["eta"])


# ------------------------------------------------------------------ 7: moments on the device
def test_device_draws_have_the_distributions_moments(device):
    out = _np(Predictive(PC.moments_model, num_samples=PC.MOMENT_SAMPLES)(17))
    PC.check_moments(out)
    for name in ("poisson_inversion", "poisson_ptrs", "bernoulli", "bernoulli_logits"):
        assert out[name].dtype == np.int32 and out[name].min() >= 0


# ------------------------------------------------------------------ 8: prior predictive
def test_prior_predictive_of_a_hierarchical_model(device):
    S, seed = 64, 3
    sigma = np.asarray(datasets.EIGHT_SCHOOLS_SIGMA, np.float64)
    out = _np(Predictive(Zoo.robust8_model, num_samples=S)(seed, 8, sigma))
    assert {k: v.shape for k, v in out.items()} == {"mu": (S,), "tau": (S,), "theta": (S, 8), "obs": (S, 8)}
    prog = compile_predictive(Zoo.robust8_model, (8, sigma), {}, [])
    r64, r32, flipped = PC.host_runs(prog, S, seed)
    for site, rule in (("mu", "monotone"), ("tau", "calibrated"), ("theta", "calibrated"), ("obs", "calibrated")):
        PC.compare(f"prior.{site}", rule, out[site], r64[site], r32[site], flipped[site])


# ------------------------------------------------------------------ 9: out-of-support inputs
def test_out_of_support_inputs_give_nan_and_touch_nothing_else(device):
    """The guard of the draw ops (no loop is entered): a negative concentration / rate and a NaN
    coefficient give NaN (-1 at an integer site) at the elements that depend on them."""
    def model(X):
        sigma_a = numpyro.sample("sigma_a", dist.HalfNormal(1.0))
        b = numpyro.sample("b", dist.Normal(np.zeros(3), np.ones(3)))
        with numpyro.plate("n", X.shape[0]):
            numpyro.sample("g", dist.Gamma(sigma_a, 2.0))
            numpyro.sample("y", dist.Poisson(sigma_a * jnp.exp(jnp.matmul(X, b))))
            numpyro.sample("z", dist.Normal(0.0, 1.0))

    rs = np.random.RandomState(2)
    X = rs.randn(70, 3)
    good = {"sigma_a": (0.5 + np.abs(rs.randn(6))).astype(np.float32), "b": (0.5 * rs.randn(6, 3)).astype(np.float32)}
    # a seventh sample whose rates are all at or above NMX_POISSON_MAX_RATE in the bad inputs
    good = {"sigma_a": np.append(good["sigma_a"], np.float32(1.0)),
            "b": np.vstack([good["b"], np.zeros((1, 3), np.float32)])}
    bad = {k: v.copy() for k, v in good.items()}
    bad["sigma_a"][1] = -1.0
    bad["b"][4, 0] = np.nan
    bad["sigma_a"][6] = 2.0 ** 24
    ref = _np(Predictive(model, _torch(good))(8, X))
    out = _np(Predictive(model, _torch(bad))(8, X))
    assert np.all(np.isfinite(ref["g"])) and ref["y"].min() >= 0
    assert np.all(np.isnan(out["g"][1])) and np.all(out["y"][1] == -1) and np.all(out["y"][4] == -1)
    assert np.all(out["y"][6] == -1) and np.all(np.isfinite(out["g"][6]))
    assert np.array_equal(out["g"][4], ref["g"][4])  # the NaN coefficient does not reach g
    others = [0, 2, 3, 5]
    for site in ("g", "y"):
        assert np.array_equal(out[site][others], ref[site][others]), site
    assert np.array_equal(out["z"], ref["z"])


# ------------------------------------------------------------------ 10: end to end
def test_posterior_predictive_after_nuts_on_the_program_kernel(device):
    case = Zoo.CASES["poisson"]()
    X, group, y, G = case.args
    mcmc = MCMC(NUTS(case.model), num_warmup=100, num_samples=100, num_chains=4, progress_bar=False)
    mcmc.run(0, X, group, y, G)
    samples = mcmc.get_samples()
    out = Predictive(case.model, samples)(5, X, group, None, G)["y"]
    assert out.shape == (400, 40) and out.dtype == torch.int32
    a, b = samples["a"].cpu().numpy().astype(np.float64), samples["b"].cpu().numpy().astype(np.float64)
    rate = np.exp(a[:, group] + b @ X.T)  # [400, 40]
    # y_s ~ Poisson(rate_s): mean of the draws has variance (sum_s rate_s) / S^2 around mean(rate)
    se = np.sqrt(rate.mean(0) / rate.shape[0])
    z = (out.cpu().numpy().astype(np.float64).mean(0) - rate.mean(0)) / se
    print("end to end: largest |z| of the per-observation means", np.abs(z).max())
    assert np.all(np.abs(z) <= 5.0)
