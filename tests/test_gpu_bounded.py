"""Bounded-support latents and Binomial likelihoods on the GPU: the program kernel on the cases of
tests/bounded_zoo.py against the float64 interpreter (far out on the sigmoid sites too),
posteriors with known answers (they fail if a Jacobian term is wrong), every public route to
constrained draws, the new draw ops against the host interpreter, and the baseball example end
to end.  Tolerances and comparison rules are the existing ones (tests/test_gpu_program.py U_TOL /
G_TOL / _check_posterior, predictive_cases.compare)."""
import functools

import numpy as np
import pytest
import torch

import bounded_zoo as BZ
import numpyro_amd as numpyro
import predictive_cases as PC
from numpyro_amd import distributions as dist
from numpyro_amd.infer import HMC, MCMC, NUTS, Predictive
from numpyro_amd.predictive_program import compile_predictive
from numpyro_amd.program import ProgramPotential, compile_model
from test_gpu_program import G_TOL, U_TOL, _check_posterior, _launch

pytestmark = pytest.mark.gpu


def _torch(samples):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in samples.items()}


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


# ------------------------------------------------------------------ 1: kernel vs the interpreter
@pytest.mark.parametrize("name", sorted(BZ.CASES))
def test_kernel_matches_the_float64_interpreter(device, name):
    """64 random rows and the rows with every unit site at u = -30, -17, 0, 17, 30."""
    case = BZ.CASES[name]()
    pot = compile_model(case.model, case.args)
    Z = np.concatenate([np.random.RandomState(1).uniform(-2, 2, (64, case.dim)), BZ.edge_rows(case)]).astype(np.float32)
    U, G = pot.program.run_host(Z.astype(np.float64))
    pe, g = _launch(pot, Z, device)
    print(name, "max |dU|", np.abs(pe - U).max(), "max |dG|", np.abs(g - G).max())
    assert np.all(np.isfinite(pe)) and np.all(np.isfinite(g))
    np.testing.assert_allclose(pe, U, **U_TOL)
    np.testing.assert_allclose(g, G, **G_TOL)


# ------------------------------------------------------------------ 2: posteriors with known answers
_N_BETA = np.array([10.0, 12.0, 8.0])
_K_BETA = np.array([3.0, 5.0, 2.0])


def _beta_binomial_model(n, k):
    phi = numpyro.sample("phi", dist.Beta(2.0, 3.0))
    numpyro.sample("k", dist.Binomial(n, probs=phi), obs=k)


def _pareto_model():
    numpyro.sample("kappa", dist.Pareto(2.0, 6.0))


def _beta_moments(a, b):
    return a / (a + b), a * b / ((a + b) ** 2 * (a + b + 1.0))


@pytest.mark.parametrize("which", ["uniform_binomial", "beta_binomial", "pareto"])
def test_posteriors_with_known_answers(device, which):
    if which == "uniform_binomial":  # Beta(1 + k, 1 + n - k): the sigmoid's Jacobian
        model, args, site = BZ.fully_pooled, (BZ.AT_BATS, BZ.HITS), "phi"
        mean, var = _beta_moments(1.0 + BZ.HITS.sum(), 1.0 + (BZ.AT_BATS - BZ.HITS).sum())
    elif which == "beta_binomial":  # Beta(2 + k, 3 + n - k)
        model, args, site = _beta_binomial_model, (_N_BETA, _K_BETA), "phi"
        mean, var = _beta_moments(2.0 + _K_BETA.sum(), 3.0 + (_N_BETA - _K_BETA).sum())
    else:  # log(kappa / 2) ~ Exponential(6): the lower bound and its Jacobian
        model, args, site = _pareto_model, (), "kappa"
        mean, var = 1.0 / 6.0, 1.0 / 36.0
    mcmc = MCMC(NUTS(model), num_warmup=300, num_samples=200, num_chains=256, progress_bar=False)
    mcmc.run(0, *args)
    assert isinstance(mcmc.sampler._potential, ProgramPotential)
    x = mcmc.get_samples(group_by_chain=True)[site].cpu().numpy().astype(np.float64)
    if which == "pareto":
        assert x.min() > 2.0
        x = np.log(x / 2.0)
    else:
        assert x.min() > 0.0 and x.max() < 1.0
    _check_posterior(x, mean, var)


# ------------------------------------------------------------------ 3: every route constrains
def test_every_route_returns_constrained_draws(device):
    """sigma ~ Uniform(0.5, 6): inside (0.5, 6) by every route, and the routes that share a seed
    and a mass matrix give the same draws."""
    case = BZ.CASES["uniform_sigma"]()
    C, S, W, seed = 8, 10, 20, 4

    def inside(x):
        x = x.cpu()
        return bool((x > BZ.SIGMA_LOW).all() and (x < BZ.SIGMA_HIGH).all())

    def run(kernel=None, extra_fields=(), **kw):
        mcmc = MCMC(kernel or NUTS(case.model), num_warmup=W, num_samples=S, num_chains=C, progress_bar=False, **kw)
        mcmc.run(seed, *case.args, extra_fields=extra_fields)
        return mcmc

    default = run()
    flat = default.get_samples()["sigma"]
    grouped = default.get_samples(group_by_chain=True)["sigma"]
    assert flat.shape == (C * S,) and grouped.shape == (C, S) and torch.equal(grouped.reshape(-1), flat)
    assert inside(flat)
    default.print_summary()
    dense = run(NUTS(case.model, dense_mass=True)).get_samples()["sigma"]
    assert dense.shape == (C * S,) and inside(dense)
    with_grad = run(extra_fields=("z_grad",))
    assert torch.equal(with_grad.get_samples()["sigma"], flat)
    assert with_grad.get_extra_fields()["z_grad"]["sigma"].shape == (C * S,)
    post = run(postprocess_fn=NUTS(case.model).postprocess_fn(case.args, {})).get_samples()["sigma"]
    assert torch.equal(post, flat)
    # the functional surface
    kern = HMC(case.model, trajectory_length=1.0)
    st = kern.init(seed, 5, model_args=case.args, num_chains=C)
    for _ in range(8):
        st = kern.sample(st, case.args, {})
    stepped = kern.postprocess_fn(case.args, {})(st.z)["sigma"]
    assert stepped.shape == (C,) and inside(stepped)
    u = st.z["sigma"].to(torch.float64)
    np.testing.assert_allclose(stepped.cpu().numpy(), (BZ.SIGMA_LOW + 5.5 * torch.sigmoid(u)).cpu().numpy(), rtol=1e-6)


def test_gather_samples_returns_constrained_draws(device):
    case = BZ.CASES["partially_pooled"]()
    mcmc = MCMC(NUTS(case.model), num_warmup=20, num_samples=5, num_chains=8, progress_bar=False)
    mcmc.run(1, *case.args)
    local = mcmc.get_samples(group_by_chain=True)
    gathered = mcmc.gather_samples(group_by_chain=True)
    for k in ("m", "kappa", "phi"):
        assert torch.equal(gathered[k].cpu(), local[k].cpu()), k
    assert local["kappa"].min() > 1.0 and 0.0 < local["phi"].min() and local["phi"].max() < 1.0
    assert 0.0 < local["m"].min() and local["m"].max() < 1.0


# ------------------------------------------------------------------ 4: the draw ops against the host
@pytest.mark.parametrize("kind", BZ.OPERAND_KINDS)
@pytest.mark.parametrize("n", BZ.PLATE_SIZES)
def test_draws_match_the_host_interpreter(device, n, kind):
    """One sample; plates below, at and above the 64 lanes; total_count and probs each as a
    computed scalar slot (a barrier), a slot per element, a given site's own slot and a
    constant.  At this seed the float32 host run shows no mismatch (tests/test_bounded.py), so
    the share of 1e-3 allows none here either at these sizes."""
    samples, args = BZ.binomial_plate_inputs(n)
    model = BZ.binomial_plate_model(n, kind)
    out = _np(Predictive(model, _torch(samples))(BZ.PLATE_SEED, *args))
    prog = compile_predictive(model, args, {}, samples)
    r64, r32, flipped = PC.host_runs(prog, samples, BZ.PLATE_SEED)
    assert set(out) == set(r64) == set(BZ.PLATE_RULES)
    for site, rule in BZ.PLATE_RULES.items():
        assert out[site].shape == (1, n)
        assert out[site].dtype == (np.int32 if rule == "discrete" else np.float32)
        if rule == "exact":
            assert np.array_equal(out[site], r32[site]) and np.array_equal(out[site].astype(np.float64), r64[site])
        else:
            PC.compare(f"n={n}.{kind}.{site}", rule, out[site], r64[site], r32[site], flipped[site])
    assert np.all(out["probs"] >= 0) and np.all(out["probs"] <= args[0])


def test_chunks_draw_what_the_whole_call_draws(device):
    samples = {"m": np.linspace(0.2, 0.8, 5, dtype=np.float32), "kappa": np.linspace(1.5, 40.0, 5, dtype=np.float32)}
    args = (BZ.AT_BATS,)
    whole = Predictive(BZ.partially_pooled, _torch(samples))(3, *args)
    slots = compile_predictive(BZ.partially_pooled, args, {}, samples).num_slots
    chunked = Predictive(BZ.partially_pooled, _torch(samples), max_workspace_bytes=2 * slots * 4 + 4)(3, *args)
    assert set(whole) == {"phi", "obs"} and all(torch.equal(whole[k], chunked[k]) for k in whole)
    assert whole["obs"].dtype == torch.int32 and whole["obs"].min() >= 0 and whole["obs"].max() <= 45


def test_binomial_guards_give_minus_one_and_touch_nothing_else(device):
    def model():
        n = numpyro.sample("n", dist.Normal(np.zeros(70), np.ones(70)))
        p = numpyro.sample("p", dist.Normal(np.zeros(70), np.ones(70)))
        numpyro.sample("k", dist.Binomial(n, probs=p))
        numpyro.sample("z", dist.Uniform(np.zeros(70), np.ones(70)))

    rs = np.random.RandomState(3)
    good = {"n": rs.randint(1, 80, (12, 70)).astype(np.float32), "p": rs.uniform(0.05, 0.95, (12, 70)).astype(np.float32)}
    bad = {k: v.copy() for k, v in good.items()}
    nan = np.nan
    cases = [("p", nan, -1), ("p", -0.1, -1), ("p", 1.1, -1), ("n", -1.0, -1), ("n", 2.5, -1), ("n", nan, -1),
             ("n", 2.0 ** 24, -1), ("p", 0.0, 0), ("p", 1.0, None), ("n", 0.0, 0)]
    for row, (site, value, _) in enumerate(cases):
        bad[site][row, 5] = value
    ref = _np(Predictive(model, _torch(good))(8))
    out = _np(Predictive(model, _torch(bad))(8))
    assert ref["k"].dtype == np.int32 and ref["k"].min() >= 0 and np.all(ref["k"] <= good["n"])
    for row, (site, value, want) in enumerate(cases):
        assert out["k"][row, 5] == (good["n"][row, 5] if want is None else want), (row, site, value)
    touched = np.zeros(good["n"].shape, bool)
    touched[:len(cases), 5] = True
    assert np.array_equal(out["k"][~touched], ref["k"][~touched]) and np.array_equal(out["z"], ref["z"])


# ------------------------------------------------------------------ 5: the baseball example end to end
@functools.lru_cache(maxsize=None)
def _baseball_run(name):
    case = BZ.CASES[name]()
    mcmc = MCMC(NUTS(case.model), num_warmup=100, num_samples=50, num_chains=64, progress_bar=False)
    mcmc.run(0, *case.args)
    assert isinstance(mcmc.sampler._potential, ProgramPotential)
    return case, mcmc.get_samples()


@pytest.mark.parametrize("name", ["partially_pooled", "partially_pooled_with_logit"])
def test_baseball_posterior_predictive_after_nuts(device, name):
    case, samples = _baseball_run(name)
    if name == "partially_pooled":
        phi = samples["phi"].cpu().numpy().astype(np.float64)
        assert phi.min() > 0.0 and phi.max() < 1.0 and samples["kappa"].min() > 1.0
        assert 0.0 < samples["m"].min() and samples["m"].max() < 1.0
    else:
        phi = 1.0 / (1.0 + np.exp(-samples["alpha"].cpu().numpy().astype(np.float64)))
    assert phi.shape == (64 * 50, 18)
    out = Predictive(case.model, samples)(5, BZ.AT_BATS)["obs"]
    assert out.shape == (64 * 50, 18) and out.dtype == torch.int32
    hits = out.cpu().numpy().astype(np.float64)
    assert hits.min() >= 0 and np.all(hits <= BZ.AT_BATS)
    # hits_s ~ Binomial(n, phi_s): the mean over draws has variance sum_s n phi_s (1 - phi_s) / S^2
    # around the mean of n phi_s
    rate = BZ.AT_BATS * phi
    se = np.sqrt((rate * (1.0 - phi)).mean(0) / phi.shape[0])
    z = (hits.mean(0) - rate.mean(0)) / se
    print(name, "largest |z| of the per-player means", np.abs(z).max())
    assert np.all(np.abs(z) <= 5.0)


@pytest.mark.parametrize("name", ["partially_pooled", "partially_pooled_with_logit"])
def test_baseball_prior_predictive_runs(device, name):
    case = BZ.CASES[name]()
    out = _np(Predictive(case.model, num_samples=64)(2, BZ.AT_BATS))
    assert set(out) == {n for n, _, _ in case.sites} | {"obs"}
    assert out["obs"].shape == (64, 18) and out["obs"].dtype == np.int32
    assert out["obs"].min() >= 0 and out["obs"].max() <= 45  # a NaN draw would come back as -1
    if name == "partially_pooled":
        assert out["kappa"].min() >= 1.0 and 0.0 <= out["m"].min() and out["m"].max() < 1.0
        assert np.all(np.isfinite(out["phi"])) and out["phi"].min() >= 0.0 and out["phi"].max() <= 1.0
