"""The dense ops of the program kernel (cholesky, trisolve; csrc/nmx_program.h) and the
MultivariateNormal models built on them, on the device: the cases of tests/linalg_op_cases.py
against their float64 torch references, bitwise repeatability and stale workspace contents, chain
counts, an indefinite matrix in one row, log_likelihood, and NUTS on the Gaussian-process model.

The float32 error of a factorisation depends on the matrix, so the tolerance is measured, by the
rule of tests/test_gpu_program_ops.py test_wide_range_stays_at_float32_level: the device's scaled
error (program_op_cases.scaled_errors) within 4 x that of a float32 restatement of the same
computation on the same rows (torch on the CPU in float32, with autograd) + 16 x 2^-24, no row
excluded."""
import numpy as np
import pytest
import torch

import linalg_op_cases as LC
import program_op_cases as OC
from numpyro_amd import diagnostics
from numpyro_amd.infer import MCMC, NUTS, log_likelihood
from numpyro_amd.program import Program, ProgramPotential
from test_gpu_program import _launch, _oracle_states
from test_gpu_program_ops import _evaluate_bound

pytestmark = pytest.mark.gpu
assert LC.ROWS == OC.ROWS
_ONE_PER_OP = (("cholesky", 65), ("tri.Ls_bs", 65))


def _check_float32_level(label, got, f32, f64):
    """got, f32, f64: (U [C], G [C, D]) of the device, the float32 restatement and the reference."""
    (pe, g), (U32, G32), (U64, G64) = got, f32, f64
    assert np.all(np.isfinite(U64)) and np.all(np.isfinite(G64)), label
    assert np.all(np.isfinite(U32)) and np.all(np.isfinite(G32)), label
    assert np.all(np.isfinite(pe)) and np.all(np.isfinite(g)), (label, int((~np.isfinite(pe)).sum()), "rows not finite")
    eU32, eG32 = OC.scaled_errors(U32, G32, U64, G64)
    eU, eG = OC.scaled_errors(pe, g, U64, G64)
    bU, bG = 4.0 * eU32.max() + 16 * 2.0 ** -24, 4.0 * eG32.max() + 16 * 2.0 ** -24
    print(f"{label}: U device {eU.max():.3e} float32 {eU32.max():.3e} bound {bU:.3e} ratio "
          f"{eU.max() / max(eU32.max(), 2.0 ** -24):.2f}; gradient device {eG.max():.3e} float32 {eG32.max():.3e} "
          f"bound {bG:.3e} ratio {eG.max() / max(eG32.max(), 2.0 ** -24):.2f}")
    assert eU.max() <= bU, (label, eU.max(), bU)
    assert eG.max() <= bG, (label, eG.max(), bG)


# ------------------------------------------------------------------ 1: the ops against torch
@pytest.mark.parametrize("n", LC.SIZES)
@pytest.mark.parametrize("kind", LC.KINDS)
def test_ops_stay_at_float32_level(device, kind, n):
    c = LC.op_case(kind, n)
    _check_float32_level(c.name, _launch(c.pot, c.Z, device), c.float32, c.reference)


def test_cholesky_writes_exact_zeros_above_the_diagonal(device):
    """U = sum(L * L) over all n * n elements of the factor, from a workspace of NaN bytes: the
    trace of A, which a stale element above the diagonal would spoil."""
    n = 65
    c = LC.op_case("cholesky", n)
    rows = c.program.ops.copy()
    rows[1] = [rows[1][0], rows[1][1], n * n, n * n, n * n, 1, 1, 0]  # mul: L * L
    pot = ProgramPotential(Program(rows, c.program.consts64, [], c.program.num_slots, c.dim), [("z", (c.dim,), 0)])
    pot.bind(LC.ROWS, 64, device)
    pot.workspace.fill_(0xFF)
    pe, _ = _evaluate_bound(pot, c.Z, device)
    trace = c.Z.reshape(LC.ROWS, n, n).diagonal(axis1=1, axis2=2).sum(1)
    np.testing.assert_allclose(pe, trace, rtol=1e-5)


# ------------------------------------------------------------------ 2: determinism, the workspace
@pytest.mark.parametrize("kind,n", _ONE_PER_OP)
def test_two_launches_are_bitwise_equal(device, kind, n):
    c = LC.op_case(kind, n)
    one, two = _launch(c.pot, c.Z, device), _launch(c.pot, c.Z, device)
    np.testing.assert_array_equal(one[0], two[0])
    np.testing.assert_array_equal(one[1], two[1])


@pytest.mark.parametrize("kind,n", _ONE_PER_OP)
def test_nothing_leaks_from_the_workspace(device, kind, n):
    """With every byte of the workspace 0xff (NaN) before the launch, the results are bitwise those
    of a zeroed workspace."""
    c = LC.op_case(kind, n)
    c.pot.bind(LC.ROWS, 64, device)
    c.pot.workspace.zero_()
    clean = _evaluate_bound(c.pot, c.Z, device)
    assert np.all(np.isfinite(clean[0])) and np.all(np.isfinite(clean[1]))
    c.pot.workspace.fill_(0xFF)
    assert bool(torch.isnan(c.pot.workspace.view(torch.float32)).all())
    poisoned = _evaluate_bound(c.pot, c.Z, device)
    np.testing.assert_array_equal(poisoned[0], clean[0])
    np.testing.assert_array_equal(poisoned[1], clean[1])


def test_an_indefinite_matrix_is_contained(device):
    """One row of 16 is [[1, 2], [2, 1]]: a NaN U for that chain only, the other rows bitwise
    unchanged, nothing raised."""
    c = LC.op_case("mvn", 2)
    pe_all, g_all = _launch(c.pot, c.Z, device)
    Z = c.Z.copy()
    Z[5] = [1.0, 2.0, 2.0, 1.0]
    pe, g = _launch(c.pot, Z, device)
    assert np.isnan(pe[5])
    ok = np.setdiff1d(np.arange(LC.ROWS), [5])
    assert np.all(np.isfinite(pe[ok]))
    np.testing.assert_array_equal(pe[ok], pe_all[ok])
    np.testing.assert_array_equal(g[ok], g_all[ok])


# ------------------------------------------------------------------ 3: compiled models
@pytest.mark.parametrize("name", ["gp", "latent_f"])
def test_models_stay_at_float32_level(device, name):
    c = LC.gp_case() if name == "gp" else LC.latent_f_case()
    _check_float32_level(name, _launch(c.pot, c.Z, device), c.float32, c.reference)


@pytest.mark.parametrize("C", [1, 63, 64, 65])
def test_chain_counts_are_bitwise_rows_of_one_batch(device, C):
    c = LC.gp_case()
    Z = np.random.RandomState(13).uniform(-1, 1, (128, c.dim)).astype(np.float32)
    pe_all, g_all = _launch(c.pot, Z, device)
    assert np.all(np.isfinite(pe_all)) and np.all(np.isfinite(g_all))
    pe, g = _launch(c.pot, Z, device, C=C)
    np.testing.assert_array_equal(pe, pe_all[:C])
    np.testing.assert_array_equal(g, g_all[:C])


def test_log_likelihood_of_the_gp(device):
    """One observation per posterior sample: shape [5], at float32 level against float64."""
    c = LC.gp_case()
    Z = c.Z[:5]
    names = [n for n, _, _ in c.sites]
    samples = {n: torch.as_tensor(np.exp(Z[:, i]).astype(np.float32)) for i, n in enumerate(names)}
    got = log_likelihood(c.model, samples, *c.args)
    assert sorted(got) == ["Y"] and tuple(got["Y"].shape) == (5,)
    dev = got["Y"].cpu().numpy().astype(np.float64)

    def restated(dtype):
        X, Y = (torch.tensor(a, dtype=dtype) for a in c.args)
        out = []
        for r in range(5):
            length, noise, var = (samples[n][r].to(dtype) for n in names)
            out.append(float(LC._mvn_logp(Y, torch.zeros_like(Y), LC._sq_exp(X, var, length, noise, dtype))))
        return np.array(out)

    r64, r32 = restated(torch.float64), restated(torch.float32)
    scale = np.maximum(1.0, np.abs(r64))
    e, e32 = np.abs(dev - r64) / scale, np.abs(r32 - r64) / scale
    bound = 4.0 * e32.max() + 16 * 2.0 ** -24
    print(f"gp log_likelihood: device {e.max():.3e} float32 {e32.max():.3e} bound {bound:.3e}")
    assert np.all(np.isfinite(dev)) and e.max() <= bound, (e.max(), bound)


# ------------------------------------------------------------------ 4: NUTS on the Gaussian process
def test_nuts_matches_oracle(device):
    """test_gpu_program.test_nuts_matches_oracle's fixed leg on the GP model: the first 4 transitions
    of 32 chains; every chain's first tree size equals the oracle's, at least 29 chains reproduce all
    four, and those chains' draws agree to 2e-3."""
    seed, C, T0 = 7, 32, 4
    case = LC.gp_case()
    kw = dict(step_size=0.1, adapt_step_size=False, adapt_mass_matrix=False)
    mcmc = MCMC(NUTS(case.model, **kw), num_warmup=0, num_samples=T0, num_chains=C, progress_bar=False)
    mcmc.run(seed, *case.args, extra_fields=("num_steps",))
    assert isinstance(mcmc.sampler._potential, ProgramPotential)
    ns_dev = mcmc.get_extra_fields(group_by_chain=True)["num_steps"].cpu().numpy()
    draws = {k: v.cpu().numpy() for k, v in mcmc.get_samples(group_by_chain=True).items()}
    match = 0
    for c in range(C):
        states = _oracle_states(case, seed, c, 0, T0, **kw)
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


def test_gp_hyperparameters_converge(device):
    """64 chains x 200 + 200 transitions: finite draws, split R-hat < 1.05 on the draws of the three
    sites as get_samples returns them (the figure of their logs is printed beside it)."""
    case = LC.gp_case()
    mcmc = MCMC(NUTS(case.model), num_warmup=200, num_samples=200, num_chains=64, progress_bar=False)
    mcmc.run(0, *case.args)
    assert isinstance(mcmc.sampler._potential, ProgramPotential)
    s = {k: v.cpu().numpy().astype(np.float64) for k, v in mcmc.get_samples(group_by_chain=True).items()}
    assert sorted(s) == ["kernel_length", "kernel_noise", "kernel_var"]
    for name, x in s.items():
        assert x.shape == (64, 200) and np.all(np.isfinite(x)) and np.all(x > 0), name
        rhat = float(np.max(diagnostics.split_gelman_rubin(x)))
        rhat_log = float(np.max(diagnostics.split_gelman_rubin(np.log(x))))
        print(name, "posterior mean", x.mean(), "max", x.max(), "split R-hat", rhat, "of the log", rhat_log)
    for name, x in s.items():
        rhat = float(np.max(diagnostics.split_gelman_rubin(x)))
        assert rhat < 1.05, (name, rhat)


def test_chain_sharding_is_bitwise_invariant(device):
    """Chains keyed by global id: two shards of 16 reproduce the 32-chain run exactly."""
    case = LC.gp_case()

    def run(C, offset):
        m = MCMC(NUTS(case.model), num_warmup=40, num_samples=20, num_chains=C, progress_bar=False,
                 chain_offset=offset)
        m.run(5, *case.args)
        return {k: v.cpu().numpy() for k, v in m.get_samples(group_by_chain=True).items()}

    full, lo, hi = run(32, None), run(16, 0), run(16, 16)
    for k in full:
        np.testing.assert_array_equal(full[k][:16], lo[k])
        np.testing.assert_array_equal(full[k][16:], hi[k])
