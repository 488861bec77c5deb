"""The program potential on the GPU (csrc/potential_program.hip through nmx_pe_program): the
kernel against the hand-written float64 potentials of tests/program_zoo.py, the shapes where it
can go wrong, bitwise invariances, NUTS against the oracle, and posteriors with known answers.

Tolerances of the kernel tests are the eight-schools ones (tests/test_gpu_potentials.py
test_eight_schools_matches_oracle): U rtol 1e-5 / atol 1e-4, gradient rtol 1e-4 / atol 1e-4."""
import functools

import numpy as np
import pytest
import torch

import numpyro_amd as numpyro
import program_zoo as Zoo
from numpyro_amd import diagnostics, native
from numpyro_amd import distributions as dist
from numpyro_amd.infer import HMC, MCMC, NUTS
from numpyro_amd.program import Program, ProgramPotential, compile_model
from oracle import hmc_ref as H
from oracle import philox

pytestmark = pytest.mark.gpu

U_TOL = dict(rtol=1e-5, atol=1e-4)
G_TOL = dict(rtol=1e-4, atol=1e-4)


def _launch(pot, Z, device, C=None, ldc=None, phase=None, idx=None):
    """U [C], dU [C, D] of a batch (NaN where the launch wrote nothing): every chain, the
    chains with phase >= PH_LEAF, or the compacted list idx."""
    C = Z.shape[0] if C is None else C
    D = Z.shape[1]
    ldc = (C + 63) // 64 * 64 if ldc is None else ldc
    pot.bind(C, ldc, device)
    z = torch.zeros(D, ldc, device=device)
    z[:, :C] = torch.from_numpy(np.ascontiguousarray(Z[:C].T.astype(np.float32))).to(device)
    g = torch.full((D, ldc), float("nan"), device=device)
    pe = torch.full((ldc,), float("nan"), device=device)
    kw = {}
    keep = []
    if phase is not None:
        ph = torch.zeros(ldc, dtype=torch.int32, device=device)
        ph[:C] = torch.from_numpy(phase.astype(np.int32)).to(device)
        keep.append(ph)
        kw["phase"] = native.ptr(ph)
    if idx is not None:
        lst = torch.zeros(ldc, dtype=torch.int32, device=device)
        lst[:len(idx)] = torch.from_numpy(np.asarray(idx, np.int32)).to(device)
        cnt = torch.tensor([len(idx)], dtype=torch.int32, device=device)
        keep += [lst, cnt]
        kw.update(active_idx=native.ptr(lst), active_count=native.ptr(cnt))
    ev = native.EvalBatch(z=native.ptr(z), grad=native.ptr(g), pe=native.ptr(pe), num_chains=C, ldc=ldc, **kw)
    pot.evaluate(ev, native.stream_ptr())
    torch.cuda.synchronize()
    return pe[:C].cpu().numpy().astype(np.float64), g[:, :C].cpu().numpy().T.astype(np.float64)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(case, potential, Z [300, D] float32, float64 reference of its first 100 rows)."""
    case = Zoo.CASES[name]()
    pot = compile_model(case.model, case.args)
    Z = np.random.RandomState(1).uniform(-2, 2, (300, case.dim)).astype(np.float32)
    U, G = case.pe_grad64(Z[:100].astype(np.float64))
    return case, pot, Z, (U, G)


# ------------------------------------------------------------------------------ 6: kernel vs float64
@pytest.mark.parametrize("name", sorted(Zoo.CASES))
def test_kernel_matches_float64(device, name):
    case, pot, Z, (U, G) = _case(name)
    pe, g = _launch(pot, Z[:100], device)
    print(name, "max |dU|", np.abs(pe - U).max(), "max |dG|", np.abs(g - G).max())
    np.testing.assert_allclose(pe, U, **U_TOL)
    np.testing.assert_allclose(g, G, **G_TOL)


# ------------------------------------------------------------------------------ 7: shapes
@pytest.mark.parametrize("C", [1, 63, 64, 65, 300])
def test_chain_counts_are_bitwise_rows_of_one_batch(device, C):
    """Every chain count (ldc padded to 64) gives, chain by chain, bitwise what the 300-chain
    batch gives, and matches float64."""
    case, pot, Z, (U, G) = _case("poisson")
    pe_all, g_all = _launch(pot, Z, device)
    pe, g = _launch(pot, Z, device, C=C)
    np.testing.assert_array_equal(pe, pe_all[:C])
    np.testing.assert_array_equal(g, g_all[:C])
    n = min(C, 100)
    np.testing.assert_allclose(pe[:n], U[:n], **U_TOL)
    np.testing.assert_allclose(g[:n], G[:n], **G_TOL)
    # a wider leading dimension changes nothing
    pe_w, g_w = _launch(pot, Z, device, C=C, ldc=(C + 63) // 64 * 64 + 128)
    np.testing.assert_array_equal(pe_w, pe)
    np.testing.assert_array_equal(g_w, g)


def test_phase_mask_skips_inactive_chains(device):
    case, pot, Z, _ = _case("poisson")
    pe_all, g_all = _launch(pot, Z, device)
    phase = np.random.RandomState(2).randint(0, 6, 300)
    on = phase >= native.PH_LEAF
    assert on.any() and (~on).any()
    pe, g = _launch(pot, Z, device, phase=phase)
    np.testing.assert_array_equal(pe[on], pe_all[on])
    np.testing.assert_array_equal(g[on], g_all[on])
    assert np.all(np.isnan(pe[~on])) and np.all(np.isnan(g[~on]))


@pytest.mark.parametrize("name", ["poisson", "treg"])
def test_compacted_active_list_is_bitwise_equal_to_dense(device, name):
    """77 of 300 chains in arbitrary order, as the NUTS step lists them: bitwise the dense
    results, the other chains untouched."""
    case, pot, Z, _ = _case(name)
    pe_all, g_all = _launch(pot, Z, device)
    chosen = np.random.RandomState(9).permutation(300)[:77]
    pe, g = _launch(pot, Z, device, ldc=320, idx=chosen)
    np.testing.assert_array_equal(pe[chosen], pe_all[chosen])
    np.testing.assert_array_equal(g[chosen], g_all[chosen])
    others = np.setdiff1d(np.arange(300), chosen)
    assert np.all(np.isnan(pe[others])) and np.all(np.isnan(g[others]))


def test_large_likelihood(device):
    """The poisson shape at N = 2000, G = 50, K = 8: vectors of many elements per lane, the
    wave-per-row adjoint of the matvec, long gather segments."""
    case = Zoo.poisson_large()
    pot = compile_model(case.model, case.args)
    Z = np.random.RandomState(4).uniform(-2, 2, (64, case.dim)).astype(np.float32)
    U, G = case.pe_grad64(Z.astype(np.float64))
    pe, g = _launch(pot, Z, device)
    extra = 1e-6 * np.abs(U).max()
    print("max |U|", np.abs(U).max(), "max |dU|", np.abs(pe - U).max(), "max |dG|", np.abs(g - G).max(),
          "max |G|", np.abs(G).max())
    np.testing.assert_allclose(pe, U, rtol=U_TOL["rtol"], atol=U_TOL["atol"] + extra)
    np.testing.assert_allclose(g, G, rtol=G_TOL["rtol"], atol=G_TOL["atol"] + extra)


def test_nonfinite_rows_are_contained(device):
    """A NaN and an inf row give a non-finite U for their chains, leave the others bitwise
    unchanged, and raise nothing."""
    case, pot, Z, _ = _case("poisson")
    pe_all, g_all = _launch(pot, Z[:100], device)
    Zb = Z[:100].copy()
    Zb[17, :] = np.nan
    Zb[64, 2] = np.inf
    pe, g = _launch(pot, Zb, device)
    assert not np.isfinite(pe[17]) and not np.isfinite(pe[64])
    ok = np.setdiff1d(np.arange(100), [17, 64])
    np.testing.assert_array_equal(pe[ok], pe_all[ok])
    np.testing.assert_array_equal(g[ok], g_all[ok])


# ------------------------------------------------------------------------------ 8: lgamma / digamma
def test_lgamma_op_and_its_digamma_adjoint(device):
    """A one-op program, U = lgamma(z), so dU/dz = digamma(z), over x in [0.02, 60] against
    torch in float64: float32-level error."""
    prog = Program([[native.OPCODE["lgamma"], 1, 0, 0, 1, 1, 0, 0]], [0.0], [], num_slots=2, dim=1)
    pot = ProgramPotential(prog, [("x", (), 0)])
    x = np.geomspace(0.02, 60.0, 500).astype(np.float32)
    pe, g = _launch(pot, x[:, None], device)
    x64 = torch.from_numpy(x.astype(np.float64))
    lg, dg = torch.lgamma(x64).numpy(), torch.special.digamma(x64).numpy()
    print("lgamma max err", np.abs(pe - lg).max(), "digamma max err", np.abs(g[:, 0] - dg).max())
    np.testing.assert_allclose(pe, lg, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(g[:, 0], dg, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------ 9: NUTS vs the oracle
def _oracle_states(case, seed, chain, num_warmup, num_iters, **kw):
    """The oracle's NUTS on the float64 potential wrapped to float32."""
    def pe_grad(z):
        u, g = case.pe_grad_one(np.asarray(z, np.float64))
        return np.float32(u), np.asarray(g, np.float32)

    o = H.NUTSOracle(pe_grad, case.dim, num_warmup, **kw)
    s = o.init(philox.init_uniform(seed, chain, 0, case.dim), seed, chain)
    out = []
    for _ in range(num_iters):
        s = o.sample(s)
        out.append(s)
    return out


@pytest.mark.parametrize("leg", ["fixed", "adaptive"])
@pytest.mark.parametrize("name", ["poisson", "treg"])
def test_nuts_matches_oracle(device, name, leg):
    """First 4 transitions of 32 chains: every chain's first tree size equals the oracle's, at
    least 0.9 C chains reproduce all four, and those chains' draws agree to 2e-3."""
    seed, C, T0 = 7, 32, 4
    case = Zoo.CASES[name]()
    fields = ("num_steps",)
    if leg == "fixed":
        kw = dict(step_size=0.1, adapt_step_size=False, adapt_mass_matrix=False)
        mcmc = MCMC(NUTS(case.model, **kw), num_warmup=0, num_samples=T0, num_chains=C, progress_bar=False)
        mcmc.run(seed, *case.args, extra_fields=fields)
        W = 0
    else:
        kw, W = {}, 30
        mcmc = MCMC(NUTS(case.model), num_warmup=W, num_samples=T0, num_chains=C, progress_bar=False)
        mcmc.warmup(seed, *case.args, collect_warmup=True, extra_fields=fields)
    assert isinstance(mcmc.sampler._potential, ProgramPotential)
    ns_dev = mcmc.get_extra_fields(group_by_chain=True)["num_steps"].cpu().numpy()
    draws = {k: v.cpu().numpy() for k, v in mcmc.get_samples(group_by_chain=True).items()}
    match = 0
    for c in range(C):
        states = _oracle_states(case, seed, c, W, T0, **kw)
        ns = np.array([s.num_steps for s in states])
        assert ns[0] == ns_dev[c, 0], (c, ns, ns_dev[c, :T0])
        if np.array_equal(ns, ns_dev[c, :T0]):
            match += 1
            for t, s in enumerate(states):
                for site, val in case.unflatten(np.asarray(s.z, np.float64)).items():
                    positive = dict((n, p) for n, _, p in case.sites)[site]
                    np.testing.assert_allclose(draws[site][c, t], np.exp(val) if positive else val,
                                               rtol=2e-3, atol=2e-3)
    assert match >= 29, f"only {match}/{C} chains reproduced the oracle path"


# ------------------------------------------------------------------------------ 10: known posteriors
_Y_NORMAL = np.random.RandomState(21).normal(1.5, 2.0, 20)
_Y_COUNTS = np.random.RandomState(22).poisson(3.0, 15).astype(np.float64)


def normal_mean_model(y):
    mu = numpyro.sample("mu", dist.Normal(0.0, 10.0))
    numpyro.sample("y", dist.Normal(mu, 2.0), obs=y)


def gamma_poisson_model(y):
    lam = numpyro.sample("lam", dist.Gamma(2.0, 1.0))
    numpyro.sample("y", dist.Poisson(lam), obs=y)


def _normal_posterior():
    prec = 1.0 / 100.0 + _Y_NORMAL.size / 4.0
    return _Y_NORMAL.sum() / 4.0 / prec, 1.0 / prec


def _check_posterior(x, mean, var):
    """x [chains, draws]: mean within 0.05 sd, variance within 10 %, split R-hat < 1.05."""
    print("posterior mean", x.mean(), "expected", mean, "var", x.var(), "expected", var)
    assert abs(x.mean() - mean) < 0.05 * np.sqrt(var)
    assert abs(x.var() / var - 1.0) < 0.10
    assert float(np.max(diagnostics.split_gelman_rubin(x))) < 1.05


@pytest.mark.parametrize("which", ["normal", "gamma_poisson"])
def test_posteriors_with_known_answers(device, which):
    if which == "normal":
        model, y, site = normal_mean_model, _Y_NORMAL, "mu"
        mean, var = _normal_posterior()
    else:  # Gamma(2 + sum y, 1 + n): checks the positive transform's Jacobian
        model, y, site = gamma_poisson_model, _Y_COUNTS, "lam"
        a, b = 2.0 + _Y_COUNTS.sum(), 1.0 + _Y_COUNTS.size
        mean, var = a / b, a / b ** 2
    mcmc = MCMC(NUTS(model), num_warmup=300, num_samples=200, num_chains=256, progress_bar=False)
    mcmc.run(0, y)
    assert isinstance(mcmc.sampler._potential, ProgramPotential)
    _check_posterior(mcmc.get_samples(group_by_chain=True)[site].cpu().numpy().astype(np.float64), mean, var)


# ------------------------------------------------------------------------------ 11: invariances
def test_chain_sharding_is_bitwise_invariant(device):
    """Chains keyed by global id: two shards of 32 reproduce the 64-chain run exactly."""
    case = Zoo.CASES["poisson"]()

    def run(C, offset):
        m = MCMC(NUTS(case.model), num_warmup=40, num_samples=20, num_chains=C, progress_bar=False,
                 chain_offset=offset)
        m.run(5, *case.args)
        return {k: v.cpu().numpy() for k, v in m.get_samples(group_by_chain=True).items()}

    full, lo, hi = run(64, None), run(32, 0), run(32, 32)
    for k in full:
        np.testing.assert_array_equal(full[k][:32], lo[k])
        np.testing.assert_array_equal(full[k][32:], hi[k])


def test_hmc_runs(device):
    case = Zoo.CASES["logit"]()
    mcmc = MCMC(HMC(case.model, trajectory_length=1.0), num_warmup=50, num_samples=20, num_chains=16,
                progress_bar=False)
    mcmc.run(3, *case.args)
    s = mcmc.get_samples()
    assert s["b"].shape == (16 * 20, 4) and torch.isfinite(s["b"]).all() and torch.isfinite(s["b0"]).all()


def test_dense_mass_recovers_the_normal_posterior(device):
    mean, var = _normal_posterior()
    mcmc = MCMC(NUTS(normal_mean_model, dense_mass=True), num_warmup=300, num_samples=200, num_chains=256,
                progress_bar=False)
    mcmc.run(1, _Y_NORMAL)
    x = mcmc.get_samples()["mu"].cpu().numpy().astype(np.float64)
    print("dense-mass posterior mean", x.mean(), "expected", mean)
    assert abs(x.mean() - mean) < 0.05 * np.sqrt(var)


# ------------------------------------------------------------------------------ 12: the feature
def test_model_without_a_fused_kernel_samples(device):
    """Eight schools with another prior constant and a StudentT likelihood has no fused
    kernel: NUTS samples it through the program potential."""
    case = Zoo.CASES["robust8"]()
    mcmc = MCMC(NUTS(case.model), num_warmup=100, num_samples=50, num_chains=32, progress_bar=False)
    mcmc.run(0, *case.args)
    s = mcmc.get_samples()
    assert set(s) == {"mu", "tau", "theta"}
    assert s["mu"].shape == (1600,) and s["tau"].shape == (1600,) and s["theta"].shape == (1600, 8)
    assert bool((s["tau"] > 0).all()) and all(bool(torch.isfinite(v).all()) for v in s.values())
