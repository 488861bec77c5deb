"""The cumsum / logsumexp / concat ops of the program kernel (csrc/nmx_program.h) and the models
built on them, on the device: the hand-assembled cases of tests/simplex_cases.py against their
float64 torch references, the log-sum-exp of a row of -inf, bitwise repeatability and stale
workspace contents, the compiled simplex / Categorical / mixture models near and far from the
mode, a posterior with a known answer (the stick-breaking Jacobian end to end), a marginalised
mixture under NUTS, and the prior predictive of a Dirichlet.

Tolerances are the project's (tests/test_gpu_program.py U_TOL / G_TOL); far from the mode the
rule of tests/test_gpu_program_ops.py: 4 x the scaled error of the float32 NumPy restatement
(simplex_cases.run_host_f32) + 16 x 2^-24, no row excluded."""
import functools

import numpy as np
import pytest
import torch

import numpyro_amd as numpyro
import simplex_cases as SC
from numpyro_amd import diagnostics
from numpyro_amd import distributions as dist
from numpyro_amd import jnp
from numpyro_amd.infer import MCMC, NUTS, Predictive
from numpyro_amd.program import ProgramPotential, compile_model
from test_gpu_program import G_TOL, U_TOL, _check_posterior, _launch
from test_gpu_program_ops import _evaluate_bound, _share

pytestmark = pytest.mark.gpu
OC = SC.OC


# ------------------------------------------------------------------ 1: every case against torch
@pytest.mark.parametrize("family", SC.FAMILIES)
def test_cases_match_the_float64_reference(device, family):
    """Every case of the family, then one assertion naming the cases that miss."""
    bad, worst_u, worst_g, share, at = [], 0.0, 0.0, 0.0, ""
    for c in SC.cases(family):
        U64, G64 = c.reference()
        pe, g = _launch(c.pot, c.Z, device)
        eU, eG = OC.scaled_errors(pe, g, U64, G64)
        u_tol, g_tol = c.tolerances(U_TOL, G_TOL)
        ok = bool(np.all(np.isfinite(pe)) and np.all(np.isfinite(g)))
        s = max(_share(pe, U64, **u_tol), _share(g, G64, **g_tol)) if ok else np.inf
        if not (ok and s <= 1.0):
            bad.append(f"{c.name}: scaled error of U {np.nanmax(eU):.3e}, of the gradient {np.nanmax(eG):.3e}, "
                       f"max |dU| {np.nanmax(np.abs(pe - U64)):.3e}, max |dG| {np.nanmax(np.abs(g - G64)):.3e}")
        else:
            worst_u, worst_g = max(worst_u, eU.max()), max(worst_g, eG.max())
            share, at = max((share, at), (s, c.name))
    print(f"{family}: {len(SC.cases(family))} cases, largest scaled error of U {worst_u:.3e}, of the gradient "
          f"{worst_g:.3e}, largest share of a tolerance {share:.3f} at {at}")
    assert not bad, f"{len(bad)} of {len(SC.cases(family))} cases:\n" + "\n".join(bad[:40])


def test_a_row_of_minus_inf(device):
    """log-sum-exp of a row that is all -inf is -inf: U = sum w (-lse) is +inf, the row's adjoint
    exactly 0, no NaN anywhere, the other rows' gradient the float64 one."""
    pot, Z, (rows, cols), dead, G64 = SC.all_inf_row()
    pe, g = _launch(pot, Z, device)
    assert np.all(pe == np.inf), pe
    assert not np.isnan(g).any()
    assert np.all(g[:, dead * cols:(dead + 1) * cols] == 0.0)
    np.testing.assert_allclose(g, G64, **G_TOL)


# ------------------------------------------------------------------ 2: determinism, the workspace
@pytest.mark.parametrize("family,name", SC.ONE_PER_OP)
def test_two_launches_are_bitwise_equal(device, family, name):
    c = SC.case(family, name)
    one, two = _launch(c.pot, c.Z, device), _launch(c.pot, c.Z, device)
    np.testing.assert_array_equal(one[0], two[0])
    np.testing.assert_array_equal(one[1], two[1])


@pytest.mark.parametrize("family,name", SC.ONE_PER_OP)
def test_nothing_leaks_from_the_workspace(device, family, name):
    """With every byte of the workspace 0xff (NaN) before the launch, the results are bitwise those
    of a zeroed workspace."""
    c = SC.case(family, name)
    c.pot.bind(OC.ROWS, 64, device)
    c.pot.workspace.zero_()
    clean = _evaluate_bound(c.pot, c.Z, device)
    assert np.all(np.isfinite(clean[0])) and np.all(np.isfinite(clean[1]))
    c.pot.workspace.fill_(0xFF)
    assert bool(torch.isnan(c.pot.workspace.view(torch.float32)).all())
    poisoned = _evaluate_bound(c.pot, c.Z, device)
    np.testing.assert_array_equal(poisoned[0], clean[0])
    np.testing.assert_array_equal(poisoned[1], clean[1])


# ------------------------------------------------------------------ 3: compiled models
@functools.lru_cache(maxsize=None)
def _model(name, R):
    m = SC.MODELS[name]()
    pot = compile_model(m.model, m.args)
    Z = SC.wide_rows(m.dim, R)
    return m, pot, Z, m.logspace_reference(Z)


@pytest.mark.parametrize("R", [2, 8])
@pytest.mark.parametrize("name", sorted(SC.MODELS))
def test_compiled_models_match_float64(device, name, R):
    """Z ~ U(-R, R), 200 rows, against the float64 log-space statement (held to torch.distributions
    by tests/test_simplex.py) under U_TOL / G_TOL."""
    m, pot, Z, (U64, G64) = _model(name, R)
    pe, g = _launch(pot, Z, device)
    eU, eG = OC.scaled_errors(pe, g, U64, G64)
    print(f"{name} R={R}: scaled error of U {eU.max():.3e}, of the gradient {eG.max():.3e}, max |dU| "
          f"{np.abs(pe - U64).max():.3e}, max |dG| {np.abs(g - G64).max():.3e}, max |U| {np.abs(U64).max():.3e}")
    np.testing.assert_allclose(pe, U64, **U_TOL)
    np.testing.assert_allclose(g, G64, **G_TOL)


@pytest.mark.parametrize("name", sorted(SC.MODELS))
def test_wide_range_stays_at_float32_level(device, name):
    """Z ~ U(-16, 16), 200 rows, none excluded: reference and kernel finite on every row, and the
    kernel's scaled errors within 4 x the float32 restatement's + 16 x 2^-24."""
    m, pot, Z, (U64, G64) = _model(name, 16)
    U32, G32 = SC.run_host_f32(pot.program, Z)
    assert np.all(np.isfinite(U64)) and np.all(np.isfinite(G64))
    assert np.all(np.isfinite(U32)) and np.all(np.isfinite(G32))
    pe, g = _launch(pot, Z, device)
    assert np.all(np.isfinite(pe)) and np.all(np.isfinite(g)), (int((~np.isfinite(pe)).sum()), "rows not finite")
    eU32, eG32 = OC.scaled_errors(U32, G32, U64, G64)
    eU, eG = OC.scaled_errors(pe, g, U64, G64)
    bU, bG = 4.0 * eU32.max() + 16 * 2.0 ** -24, 4.0 * eG32.max() + 16 * 2.0 ** -24
    print(f"wide {name} R=16: U device {eU.max():.3e} float32 {eU32.max():.3e} bound {bU:.3e}; gradient device "
          f"{eG.max():.3e} float32 {eG32.max():.3e} bound {bG:.3e}")
    assert eU.max() <= bU, (eU.max(), bU)
    assert eG.max() <= bG, (eG.max(), bG)


# ------------------------------------------------------------------ 4: a known posterior
_A = np.array([1.5, 0.8, 2.0, 1.2])
_Y_CAT = np.random.RandomState(41).choice(4, 30, p=[0.4, 0.1, 0.3, 0.2])


def dirichlet_categorical_model(y):
    w = numpyro.sample("w", dist.Dirichlet(_A))
    numpyro.sample("y", dist.Categorical(probs=w), obs=y)


def test_dirichlet_categorical_posterior(device):
    """w ~ Dirichlet(a), y ~ Categorical(w): the posterior is Dirichlet(a + counts).  Every
    component by test_gpu_program._check_posterior's rule: the stick-breaking Jacobian end to end."""
    post = _A + np.bincount(_Y_CAT, minlength=4)
    total = post.sum()
    mcmc = MCMC(NUTS(dirichlet_categorical_model), num_warmup=300, num_samples=200, num_chains=256,
                progress_bar=False)
    mcmc.run(0, _Y_CAT)
    assert isinstance(mcmc.sampler._potential, ProgramPotential)
    w = mcmc.get_samples(group_by_chain=True)["w"].cpu().numpy().astype(np.float64)
    assert w.shape == (256, 200, 4)
    assert np.abs(w.sum(-1) - 1.0).max() < 1e-5 and w.min() > 0.0
    for k in range(4):
        _check_posterior(w[..., k], post[k] / total, post[k] * (total - post[k]) / (total ** 2 * (total + 1.0)))


# ------------------------------------------------------------------ 5: a marginalised mixture
_MIX_LOC, _MIX_SCALE = np.array([-3.0, 0.0, 4.0]), np.array([1.0, 0.5, 1.5])
_rs = np.random.RandomState(43)
_MIX_K = _rs.choice(3, 50, p=[0.5, 0.2, 0.3])
_Y_MIX = _MIX_LOC[_MIX_K] + _MIX_SCALE[_MIX_K] * _rs.randn(50)


def mixture_weights_model(y):
    w = numpyro.sample("w", dist.Dirichlet(np.ones(3)))
    numpyro.sample("y", dist.MixtureSameFamily(dist.Categorical(probs=w), dist.Normal(_MIX_LOC, _MIX_SCALE)), obs=y)


def test_mixture_weights_run(device):
    """Component locations and scales constant, the weights latent: draws finite and on the
    simplex, split R-hat of every weight below 1.05."""
    mcmc = MCMC(NUTS(mixture_weights_model), num_warmup=200, num_samples=100, num_chains=64, progress_bar=False)
    mcmc.run(1, _Y_MIX)
    pot = mcmc.sampler._potential
    assert isinstance(pot, ProgramPotential)
    assert "logsumexp" in [ln.split()[1] for ln in pot.program.describe()]
    w = mcmc.get_samples(group_by_chain=True)["w"]
    assert w.shape == (64, 100, 3) and bool(torch.isfinite(w).all())
    w = w.cpu().numpy().astype(np.float64)
    assert np.abs(w.sum(-1) - 1.0).max() < 1e-5
    rhat = [float(np.max(diagnostics.split_gelman_rubin(w[..., k]))) for k in range(3)]
    print("mixture weights: posterior mean", w.mean((0, 1)), "split R-hat", rhat)
    assert max(rhat) < 1.05


# ------------------------------------------------------------------ 6: predictive programs
def test_prior_predictive_of_a_dirichlet(device):
    """Normalised gamma draws: the sample means within 5 standard errors of a / sum(a), the
    standard error from the Dirichlet's variance."""
    a = np.array([0.7, 2.0, 1.3, 4.0, 1.0])

    def model():
        numpyro.sample("w", dist.Dirichlet(a))

    S = 4096
    w = Predictive(model, num_samples=S)(5)["w"]
    assert w.shape == (S, 5) and w.dtype == torch.float32 and bool(torch.isfinite(w).all())
    w = w.cpu().numpy().astype(np.float64)
    assert np.abs(w.sum(1) - 1.0).max() < 1e-5 and w.min() >= 0.0
    A = a.sum()
    mean, var = a / A, a * (A - a) / (A ** 2 * (A + 1.0))
    z = (w.mean(0) - mean) / np.sqrt(var / S)
    print("prior predictive Dirichlet: z-scores of the means", z, "variance ratio", w.var(0) / var)
    assert np.abs(z).max() < 5.0


def test_predictive_kernel_runs_the_three_ops(device):
    """k_program_predict shares NmxProgram::forward: a deterministic site of a drawn site through
    cumsum (two chunks), concat and logsumexp, against float64 NumPy of the g the device returned."""
    n = 70

    def model():
        g = numpyro.sample("g", dist.Normal(np.zeros(n), np.ones(n)))
        numpyro.deterministic("d", jnp.concatenate([jnp.cumsum(g), np.ones(3)]) - jnp.logsumexp(g))

    out = Predictive(model, num_samples=OC.ROWS)(3)
    g = out["g"].cpu().numpy().astype(np.float64)
    assert g.shape == (OC.ROWS, n) and g.std() > 0.5
    lse = np.log(np.exp(g - g.max(1, keepdims=True)).sum(1)) + g.max(1)
    ref = np.concatenate([np.cumsum(g, 1), np.ones((OC.ROWS, 3))], 1) - lse[:, None]
    np.testing.assert_allclose(out["d"].cpu().numpy(), ref, rtol=1e-5, atol=1e-4)
