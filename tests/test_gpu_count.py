"""The count likelihoods on the GPU: the potential kernel against the float64 interpreter at the
corner rows of tests/count_cases.py, the two special ops (lrising, logaddexp) alone from a NaN-filled
workspace, log_likelihood and loo, Predictive, two posteriors with known answers, one SVI run and
the debug build.

Tolerances are the project's: U_TOL / G_TOL of tests/test_gpu_program.py for the kernel, the rule of
tests/test_gpu_program_ops.py for the op programs (4 x the scaled error of the float32 host
restatement + 16 x 2^-24), loglik_cases.calibrated_bound for the tables, predictive_cases.compare for
the draws and test_gpu_program._check_posterior for the posteriors.

Observed on one MI355X, for the record (every test prints its own figures; "share" is the largest
error as a share of its tolerance, device / float32 restatement):

  kernel, N = 65      share of U_TOL      share of G_TOL      max |dU|   max |dG|
    nb_regression       0.21 / 0.28         0.77 / 0.24        7.3e-03    4.0e-03
    small phi           0.12 / 0.12         0.51 / 0.76        2.8e-04    8.4e-05
    beta_binomial       0.45 / 0.41         0.43 / 0.54        1.0e-03    4.4e-04
    zi_poisson          0.02 / 0.03         0.21 / 0.16        1.2e-04    6.3e-05
    zi_nb2_logits       0.10 / 0.07         0.27 / 0.18        2.1e-04    7.3e-05
  kernel, N = 1: every share below 0.11
  op programs, scaled error of U / gradient: lrising 1.6e-07 / 1.7e-07 (float32 1.4e-07 / 1.7e-07),
    logaddexp 1.8e-07 / 1.5e-07 (float32 1.5e-07 / 1.8e-07)
  log_likelihood: device deviation equal to the float32 host run's (2.2e-05 and 1.7e-06, bounds 8.7e-05 and
    7.7e-06); Pareto-k in [-0.12, 7.8] and [-0.16, 0.13]
  Predictive: no mismatch in 2 x 4 sites of 64 x 65 draws
  posteriors: mean 0.29312 (0.29333), variance 2.744e-3 (2.727e-3); mean 0.41118 (0.41135), variance
    1.712e-3 (1.705e-3)
  SVI: loss 2507.0 -> 837.5 in 20 steps"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import numpyro_amd as numpyro
import count_cases as CC
import loglik_cases as LC
import predictive_cases as PC
import program_op_cases as OC
from numpyro_amd import distributions as dist
from numpyro_amd import jnp, native, optim
from numpyro_amd.infer import MCMC, NUTS, SVI, Predictive, Trace_ELBO, log_likelihood, loo
from numpyro_amd.infer.autoguide import AutoNormal
from numpyro_amd.loglik_program import compile_log_likelihood
from numpyro_amd.potentials import POSITIVE, REAL
from numpyro_amd.predictive_program import compile_predictive
from numpyro_amd.program import ProgramPotential, compile_model
from test_gpu_program import G_TOL, U_TOL, _check_posterior, _launch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _share(x, ref, rtol, atol):
    return float(np.max(np.abs(x - ref) / (atol + rtol * np.abs(ref))))


# ------------------------------------------------------------------------------ 7: kernel vs float64
@pytest.mark.parametrize("N", [1, 65])
@pytest.mark.parametrize("corner", CC.corners(), ids=lambda c: c.name)
def test_kernel_matches_the_float64_interpreter(device, corner, N):
    """64 random rows and the corner rows, observed vectors of N elements: finite, within U_TOL / G_TOL."""
    pot = compile_model(corner.model, CC.observed_at(corner, N))
    Z = np.concatenate([CC.random_rows(corner), corner.Z])
    U, G = pot.program.run_host(Z)
    U32, G32 = pot.program.run_host(Z, dtype=np.float32)
    pe, g = _launch(pot, Z, device)
    assert np.all(np.isfinite(pe)) and np.all(np.isfinite(g))
    print(f"{corner.name} N={N}: device share of U_TOL {_share(pe, U, **U_TOL):.3f}, of G_TOL {_share(g, G, **G_TOL):.3f}; "
          f"float32 restatement {_share(U32, U, **U_TOL):.3f}, {_share(G32, G, **G_TOL):.3f}; max |dU| "
          f"{np.abs(pe - U).max():.3e}, max |dG| {np.abs(g - G).max():.3e}")
    np.testing.assert_allclose(pe, U, **U_TOL)
    np.testing.assert_allclose(g, G, **G_TOL)


# ------------------------------------------------------------------------------ 8: the op programs
def _evaluate_from_nan_workspace(pot, Z, device):
    """U, dU of the rows of Z from a workspace whose every byte is 0xff (NaN) before the launch."""
    C, D = Z.shape
    ldc = 64
    pot.bind(C, ldc, device)
    pot.workspace.fill_(0xFF)
    z = torch.zeros(D, ldc, device=device)
    z[:, :C] = torch.from_numpy(np.ascontiguousarray(Z.T.astype(np.float32))).to(device)
    g = torch.full((D, ldc), float("nan"), device=device)
    pe = torch.full((ldc,), float("nan"), device=device)
    ev = native.EvalBatch(z=native.ptr(z), grad=native.ptr(g), pe=native.ptr(pe), num_chains=C, ldc=ldc)
    pot.evaluate(ev, native.stream_ptr())
    torch.cuda.synchronize()
    return pe[:C].cpu().numpy().astype(np.float64), g[:, :C].cpu().numpy().T.astype(np.float64)


@pytest.mark.parametrize("op", ["lrising", "logaddexp"])
def test_op_programs_match_the_float64_interpreter(device, op):
    """Every layout and size of the op's hand-assembled programs, values and adjoints: the device's
    scaled errors within 4 x the float32 restatement's + 16 x 2^-24; then one assertion naming the
    cases that miss."""
    bad, worst = [], (0.0, 0.0, 0.0, 0.0)
    cases = [c for c in CC.op_cases() if c.name.startswith(op)]
    assert len(cases) >= 25
    for c in cases:
        U64, G64 = c.program.run_host(c.Z)
        U32, G32 = c.program.run_host(c.Z, dtype=np.float32)
        pe, g = _evaluate_from_nan_workspace(c.pot, c.Z, device)
        eU32, eG32 = OC.scaled_errors(U32, G32, U64, G64)
        eU, eG = OC.scaled_errors(pe, g, U64, G64)
        bU, bG = 4.0 * eU32.max() + 16 * 2.0 ** -24, 4.0 * eG32.max() + 16 * 2.0 ** -24
        ok = bool(np.all(np.isfinite(pe)) and np.all(np.isfinite(g))) and eU.max() <= bU and eG.max() <= bG
        if not ok:
            bad.append(f"{c.name}: U {np.nanmax(eU):.3e} (bound {bU:.3e}), gradient {np.nanmax(eG):.3e} (bound {bG:.3e})")
        else:
            worst = tuple(max(a, b) for a, b in zip(worst, (eU.max(), eU32.max(), eG.max(), eG32.max())))
    print(f"{op}: {len(cases)} cases, largest scaled error of U device {worst[0]:.3e} float32 {worst[1]:.3e}, of the "
          f"gradient device {worst[2]:.3e} float32 {worst[3]:.3e}")
    assert not bad, f"{len(bad)} of {len(cases)} cases:\n" + "\n".join(bad)


# ------------------------------------------------------------------------------ 9: log_likelihood and loo
def _constrained(corner, Z):
    """{site: [S] float32 numbers} of the rows of Z (scalar sites in sorted order): real sites as they
    are, positive ones exp, unit ones sigmoid."""
    pot = compile_model(corner.model, corner.args)
    out = {}
    for i, (name, _, code) in enumerate(pot.sites):
        u = Z[:, i]
        out[name] = CC.f32(u if code == REAL else np.exp(u) if code == POSITIVE else CC.sigmoid(u))
    return out


@pytest.mark.parametrize("which", ["nb_regression", "zi_nb2_logits"])
def test_log_likelihood_table_and_loo(device, which):
    corner = next(c for c in CC.corners() if c.name == which)
    args = CC.observed_at(corner, 65)
    samples = _constrained(corner, CC.random_rows(corner, 65))
    prog = compile_log_likelihood(corner.model, args, {}, given=samples)
    r64, r32 = prog.run_host(samples)["y"], prog.run_host(samples, dtype=np.float32)["y"]
    f32 = {k: torch.from_numpy(v.astype(np.float32)) for k, v in samples.items()}
    dev = log_likelihood(corner.model, f32, *args)["y"]
    assert tuple(dev.shape) == (65, 65) and dev.dtype == torch.float32
    err, bound = LC.scaled_error(dev.cpu().numpy(), r64), LC.calibrated_bound(r32, r64)
    print(f"{which}: float32 host deviation {LC.scaled_error(r32, r64):.3e}, device deviation {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    # loo on draws that look like a posterior: 256 rows within 0.02 of one point (rows spread as widely
    # as the ones above leave columns with fewer than five tail ratios, whose Pareto-k is inf by definition)
    cloud = CC.f32(np.median(corner.Z, 0)[None, :] + 0.02 * np.random.RandomState(8).randn(256, corner.Z.shape[1]))
    post = {k: torch.from_numpy(v.astype(np.float32)) for k, v in _constrained(corner, cloud).items()}
    site = loo(corner.model, post, *args)["y"]
    print(f"{which}: elpd_loo sum {float(site['elpd_loo'].sum()):.2f}, Pareto-k in [{float(site['pareto_k'].min()):.3f}, "
          f"{float(site['pareto_k'].max()):.3f}]")
    assert bool(torch.isfinite(site["elpd_loo"]).all()) and bool(torch.isfinite(site["pareto_k"]).all())
    assert tuple(site["elpd_loo"].shape) == (65,) and tuple(site["pareto_k"].shape) == (65,)


# ------------------------------------------------------------------------------ 10: Predictive
def _predictive_model(N):
    def model(y=None):
        b = numpyro.sample("b", dist.Normal(1.0, 1.0))
        phi = numpyro.sample("phi", dist.LogNormal(1.0, 1.0))
        g = numpyro.sample("g", dist.Beta(2.0, 5.0))
        with numpyro.plate("n", N):
            numpyro.sample("y", dist.NegativeBinomial2(jnp.exp(b), phi), obs=y)
            numpyro.sample("zy", dist.ZeroInflatedNegativeBinomial2(jnp.exp(b), phi, gate=g))
            numpyro.sample("bb", dist.BetaBinomial(phi, 2.0, 40))
            numpyro.sample("geo", dist.Geometric(probs=g))
    return model


_INT_SITES = ("y", "zy", "bb", "geo")


def test_predictive_posterior_and_prior(device):
    """Device draws against the float64 host interpreter under predictive_cases.compare's discrete
    rule; integer dtype as for the existing integer sites."""
    N, S, seed = 65, 64, 4
    model = _predictive_model(N)
    rs = np.random.RandomState(3)
    samples = {"b": rs.normal(1.0, 1.0, S).astype(np.float32), "phi": np.exp(rs.normal(1.0, 1.0, S)).astype(np.float32),
               "g": rs.beta(2.0, 5.0, S).astype(np.float32)}
    out = Predictive(model, {k: torch.from_numpy(v) for k, v in samples.items()})(seed)
    prog = compile_predictive(model, (), {}, samples)
    r64, r32, flipped = PC.host_runs(prog, samples, seed)
    assert set(out) == set(_INT_SITES) == set(r64)
    for site in _INT_SITES:
        x = out[site].cpu().numpy()
        assert x.dtype == np.int32 and x.shape == (S, N) and x.min() >= 0, site
        PC.compare(f"posterior.{site}", "discrete", x, r64[site], r32[site], flipped[site])
    assert out["bb"].max() <= 40
    prior = Predictive(model, num_samples=S)(seed)
    prog = compile_predictive(model, (), {}, [])
    r64, r32, flipped = PC.host_runs(prog, S, seed)
    for site in _INT_SITES:
        x = prior[site].cpu().numpy()
        assert x.dtype == np.int32 and x.shape == (S, N), site
        PC.compare(f"prior.{site}", "discrete", x, r64[site], r32[site], flipped[site])


# ------------------------------------------------------------------------------ 11: posteriors with known answers
_RS = np.random.RandomState(12)
_Y_GEOMETRIC = _RS.geometric(0.3, 20).astype(np.float64) - 1.0
_R = 4.0
_Y_NEGBIN = _RS.negative_binomial(_R, 0.6, 20).astype(np.float64)  # numpy's p is the chance that ends the count


def _geometric_model(y):
    p = numpyro.sample("p", dist.Beta(2.0, 3.0))
    numpyro.sample("y", dist.GeometricProbs(p), obs=y)


def _negbin_model(y):
    p = numpyro.sample("p", dist.Beta(2.0, 3.0))
    numpyro.sample("y", dist.NegativeBinomialProbs(_R, p), obs=y)


@pytest.mark.parametrize("which", ["geometric", "negative_binomial"])
def test_posteriors_with_known_answers(device, which):
    """p ~ Beta(2, 3).

    GeometricProbs(p) has mass (1 - p)^y p, so N observations multiply the prior by p^N (1 - p)^(sum y):
    the posterior is Beta(2 + N, 3 + sum y).

    NegativeBinomialProbs(r, p) is GammaPoisson(r, rate = 1 / p - 1), whose mass is
    C(y + r - 1, y) (rate / (1 + rate))^r (1 / (1 + rate))^y.  With rate = (1 - p) / p, 1 + rate = 1 / p, so
    rate / (1 + rate) = 1 - p and 1 / (1 + rate) = p: the mass is C(y + r - 1, y) (1 - p)^r p^y, p the chance
    of the events that are counted.  N observations multiply the prior by p^(sum y) (1 - p)^(N r): the
    posterior is Beta(2 + sum y, 3 + N r)."""
    if which == "geometric":
        model, y = _geometric_model, _Y_GEOMETRIC
        a, b = 2.0 + y.size, 3.0 + y.sum()
    else:
        model, y = _negbin_model, _Y_NEGBIN
        a, b = 2.0 + y.sum(), 3.0 + y.size * _R
    mcmc = MCMC(NUTS(model), num_warmup=300, num_samples=200, num_chains=256, progress_bar=False)
    mcmc.run(0, y)
    assert isinstance(mcmc.sampler._potential, ProgramPotential)
    mean, var = a / (a + b), a * b / ((a + b) ** 2 * (a + b + 1.0))
    _check_posterior(mcmc.get_samples(group_by_chain=True)["p"].cpu().numpy().astype(np.float64), mean, var)


# ------------------------------------------------------------------------------ 12: SVI
def test_svi_runs_on_the_negative_binomial_regression(device):
    corner = CC.corners()[0]
    svi = SVI(corner.model, AutoNormal(corner.model), optim.Adam(0.05), Trace_ELBO(64))
    res = svi.run(5, 20, *corner.args, device=device)
    losses = res.losses.cpu().numpy()
    print("losses", losses[0], "->", losses[-1])
    assert losses.shape == (20,) and np.all(np.isfinite(losses)) and losses[-1] < losses[0]


# ------------------------------------------------------------------------------ 13: the debug build
DEBUG_SCRIPT = r"""
import sys
sys.path.insert(0, "tests")
import numpy as np, torch
import count_cases as CC
from numpyro_amd import native
from numpyro_amd.infer import log_likelihood
from numpyro_amd.program import compile_model
from test_gpu_program import _launch
from test_gpu_count import _constrained
assert native.LIB_PATH.endswith("libnumpyro_amd_debug.so"), native.LIB_PATH
device = torch.device("cuda", 0)
for corner in CC.corners():
    for N in (1, 65):
        args = CC.observed_at(corner, N)
        pot = compile_model(corner.model, args)
        pe, g = _launch(pot, np.concatenate([CC.random_rows(corner), corner.Z]), device)
        assert np.all(np.isfinite(pe)) and np.all(np.isfinite(g)), (corner.name, N)
        if corner.name in ("nb_regression", "zi_nb2_logits"):
            samples = _constrained(corner, CC.random_rows(corner, 65))
            ll = log_likelihood(corner.model, {k: torch.from_numpy(v.astype(np.float32)) for k, v in samples.items()},
                                *args)["y"]
            assert bool(torch.isfinite(ll).all()), (corner.name, N)
torch.cuda.synchronize()
print("count debug build ok")
"""


def test_debug_build_runs_the_count_programs_without_a_failed_check():
    """The kernel test and the log-likelihood tables at N = 1 and 65 under the NMX_DCHECK build."""
    lib = os.path.join(ROOT, "numpyro_amd", "_lib", "libnumpyro_amd_debug.so")
    if not os.path.exists(lib):
        pytest.fail("debug library missing: run numpyro_amd.build(debug=True) (done by __graft_entry__.build())")
    env = dict(os.environ, NUMPYRO_AMD_DEBUG="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", DEBUG_SCRIPT], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=110)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "NMX_DCHECK failed" not in out, out[-3000:]
    assert "count debug build ok" in out
