"""The D-blocked logistic-regression potential for 65 to 1024 features
(csrc/potential_logreg_wide.hip through potentials.LogisticRegression) against the float64 oracle.

Tolerances: potential_cases.check_logreg, and (the convention of tests/test_gpu_softmax.py) the
float32 oracle's largest deviation from the float64 one on the same case, times 4 for the different
summation order; U and dU each have their own.  Every case prints both numbers; one MI355X run, for
the record (max |x - float64|: "f32" the float32 oracle, whose 4-fold is the tolerance, "dev" the
device):

  D, N, C [regime]: U f32 / dev; dU f32 / dev
    65,   1,   1: 2.7e-07 / 2.7e-07; 1.9e-07 / 1.9e-07     128,  33, 129: 1.4e-05 / 1.1e-05; 3.4e-06 / 3.0e-06
   129, 513, 300: 1.4e-04 / 7.8e-05; 4.5e-05 / 1.4e-05     256,  33, 300: 3.7e-05 / 2.2e-05; 5.1e-06 / 3.8e-06
   257, 513,  65: 2.1e-04 / 9.3e-05; 2.6e-05 / 1.4e-05     512,   1, 300: 2.6e-05 / 1.8e-05; 9.7e-07 / 1.7e-06
   513,  33,  33: 4.9e-05 / 3.1e-05; 4.3e-06 / 3.5e-06    1023, 513, 300: 4.0e-04 / 2.3e-04; 2.9e-05 / 1.7e-05
  1024,   1,  33: 4.3e-05 / 3.1e-05; 8.0e-07 / 6.6e-07    1024, 513,   1: 2.0e-04 / 4.6e-05; 1.5e-05 / 1.2e-05
    65, 513, 300: 9.8e-05 / 4.1e-05; 3.6e-05 / 1.5e-05     512, 513,  65: 2.2e-04 / 1.1e-04; 2.1e-05 / 1.4e-05
   257, 513,  65 saturated: 0.12 / 0.032; 2.9e-04 / 1.2e-04 (max |U| 2.4e6, max |dU| 484)
  1023,  33, 300 saturated: 0.60 / 0.25; 1.3e-04 / 1.1e-04 (max |U| 7.4e6, max |dU| 423)
  Largest dev / f32 ratio 1.71 (dU at D = 512, N = 1).  End to end: the two runs' posterior means differ by at
  most 1.14 combined standard errors.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import numpyro_amd as numpyro
import potential_cases as K
from numpyro_amd import diagnostics, jnp, native
from numpyro_amd import distributions as dist, potentials as P
from numpyro_amd.infer import MCMC, NUTS, Predictive
from oracle import potentials as OP
from oracle import predictive as OPred

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def evaluate(device, X, y, Z, phase=None, active=None):
    """(U [ldc], dU [ldc, D]) of a NaN-filled arena after one launch over the chains Z [C, D]."""
    C, ldc = len(Z), (len(Z) + 63) // 64 * 64 + 64
    pot = P.LogisticRegression(X, y)
    pot.bind(C, ldc, device)
    z, g = (torch.full((pot.dim, ldc), float("nan"), device=device) for _ in range(2))
    z[:, :C] = torch.from_numpy(Z.T.copy()).to(device)
    pe = torch.full((ldc,), float("nan"), device=device)
    keep = []
    ev = native.EvalBatch(z=native.ptr(z), grad=native.ptr(g), pe=native.ptr(pe), num_chains=C, ldc=ldc)
    if phase is not None:
        keep.append(torch.from_numpy(np.pad(phase, (0, ldc - C)).astype(np.int32)).to(device))
        ev.phase = native.ptr(keep[-1])
    if active is not None:
        keep.append(torch.from_numpy(np.pad(active, (0, ldc - len(active))).astype(np.int32)).to(device))
        keep.append(torch.tensor([len(active)], dtype=torch.int32, device=device))
        ev.active_idx, ev.active_count = native.ptr(keep[-2]), native.ptr(keep[-1])
    pot.evaluate(ev, native.stream_ptr())
    torch.cuda.synchronize()
    return pe.cpu().numpy(), g.cpu().numpy().T


def chains_of(D, kind):
    """1 chain, one workgroup's chains + 1 (32 per chain tile, 4 / 4 / 2 / 1 tiles by D), 300."""
    tiles = 4 if D <= 256 else 2 if D <= 512 else 1
    return (1, 32 * tiles + 1, 300)[kind]


# every shape class (D <= 128, 256, 512, 1024), its first and last width, a partial last k-block and
# d-tile; one tile, two tiles and several row splits with tiles; the chain counts of chains_of
SHAPES = [(65, 1, 0), (128, 33, 1), (129, 513, 2), (256, 33, 2), (257, 513, 1), (512, 1, 2), (513, 33, 1),
          (1023, 513, 2), (1024, 1, 1), (1024, 513, 0), (65, 513, 2), (512, 513, 1)]


@pytest.mark.parametrize("D,N,kind,regime", [s + ("unit",) for s in SHAPES] + [(257, 513, 1, "saturated"),
                                                                               (1023, 33, 2, "saturated")])
def test_potential_and_gradient_match_float64(device, D, N, kind, regime):
    C = chains_of(D, kind)
    X, y, Z, (U64, G64) = K.logreg_reference(N, D, C, regime)
    U, G = evaluate(device, X, y, Z)
    assert np.isnan(U[C:]).all() and np.isnan(G[C:]).all()
    K.check_logreg(U[:C], G[:C], X, y, Z, (U64, G64), label=f"D={D} N={N} C={C} {regime}")
    f32 = OP.LogisticRegression(X, y, dtype=np.float32)
    U32, G32 = (np.array(v, np.float64) for v in zip(*(f32.pe_grad(z) for z in Z)))
    for what, dev, r64, r32 in (("U", U[:C], U64, U32), ("dU", G[:C], G64, G32)):
        spread, err = np.abs(r32 - r64).max(), np.abs(dev - r64).max()
        print(f"D={D} N={N} C={C} {regime} {what}: float32 vs float64 {spread:.3g}, device vs float64 {err:.3g}, "
              f"max |{what}| {np.abs(r64).max():.3g}")
        assert err <= 4 * spread


@pytest.mark.parametrize("D", [100, 200, 400, 1000])
def test_a_chain_does_not_depend_on_its_batch(device, D):
    """Alone, one of 300, at another position, under a phase mask and in a scrambled list: the same bits."""
    C, (X, y, Z, _) = 300, K.logreg_reference(513, D, 300, "unit")
    U, G = evaluate(device, X, y, Z)
    for c in (0, 7, 299):
        U1, G1 = evaluate(device, X, y, Z[c:c + 1])
        np.testing.assert_array_equal(U1[0], U[c])
        np.testing.assert_array_equal(G1[0], G[c])
    Ur, Gr = evaluate(device, X, y, np.roll(Z, 37, axis=0))
    np.testing.assert_array_equal(Ur[:C], np.roll(U[:C], 37))
    np.testing.assert_array_equal(Gr[:C], np.roll(G[:C], 37, axis=0))
    rs = np.random.RandomState(1)
    on = rs.rand(C) < 0.3
    on[128:256] = False  # workgroups without a chain, in every shape class
    Up, Gp = evaluate(device, X, y, Z, phase=np.where(on, native.PH_LEAF, native.PH_WAIT))
    listed = rs.permutation(np.flatnonzero(rs.rand(C) < 0.4))
    Ua, Ga = evaluate(device, X, y, Z, active=listed)
    for Us, Gs, chains in ((Up, Gp, np.flatnonzero(on)), (Ua, Ga, listed)):
        assert 0 < len(chains) < C
        np.testing.assert_array_equal(Us[chains], U[chains])
        np.testing.assert_array_equal(Gs[chains], G[chains])
        rest = np.setdiff1d(np.arange(len(Us)), chains)
        assert np.all(np.isnan(Us[rest])) and np.all(np.isnan(Gs[rest]))


DEBUG_SCRIPT = r"""
import sys
sys.path.insert(0, "tests")
import numpy as np, torch
from numpyro_amd import native
import potential_cases as K
import test_gpu_logreg_wide as T
assert native.LIB_PATH.endswith("libnumpyro_amd_debug.so"), native.LIB_PATH
for D in (100, 200, 400, 1000):
    X, y, Z = K.logreg_case(70, D, 70)
    U, G = T.evaluate(torch.device("cuda:0"), X, y, Z)
    Ua, Ga = T.evaluate(torch.device("cuda:0"), X, y, Z, active=np.array([69, 3, 40]))
    assert np.isfinite(U[:70]).all() and np.isfinite(G[:70]).all() and np.isfinite(Ua).sum() == 3
print("wide logreg debug build ok")
"""


def test_debug_build_runs_the_kernels_without_a_failed_check():
    env = dict(os.environ, NUMPYRO_AMD_DEBUG="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", DEBUG_SCRIPT], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=110)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "NMX_DCHECK failed" not in out and "wide logreg debug build ok" in out, out[-3000:]


def model(X, y):
    beta = numpyro.sample("beta", dist.Normal(0.0, 1.0).expand([72]))
    numpyro.sample("obs", dist.Bernoulli(logits=jnp.matmul(X, beta)), obs=y)


def torch_potential(X, y, beta):
    logits = X @ beta
    return (torch.nn.functional.softplus(logits) - y * logits).sum() + 0.5 * beta.pow(2).sum()


def test_nuts_matches_the_torch_potential(device):
    rs = np.random.RandomState(5)
    X = np.concatenate([rs.randn(400, 71), np.ones((400, 1))], 1).astype(np.float32)
    y = (rs.rand(400) < 1 / (1 + np.exp(-X @ (0.5 * rs.randn(72))))).astype(np.float32)
    Xd, yd = torch.from_numpy(X).to(device), torch.from_numpy(y).to(device)
    runs = []
    for kernel, args, kw in ((NUTS(model), (X, y), {}),
                             (NUTS(potential_fn=lambda s: torch_potential(Xd, yd, s["beta"])), (),
                              {"init_params": {"beta": torch.zeros(64, 72)}})):
        mcmc = MCMC(kernel, num_warmup=150, num_samples=150, num_chains=64, progress_bar=False)
        mcmc.run(3, *args, **kw)
        x = mcmc.get_samples(group_by_chain=True)["beta"].cpu().numpy().reshape(64, 150, 72).astype(np.float64)
        ess = diagnostics.effective_sample_size(x)
        runs.append((x.mean((0, 1)), x.var((0, 1), ddof=1) / ess, kernel))
    assert type(runs[0][2]._potential) is P.LogisticRegression
    (m0, v0, _), (m1, v1, _) = runs
    print("largest mean difference / combined standard error", (np.abs(m0 - m1) / np.sqrt(v0 + v1)).max())
    assert np.all(np.abs(m0 - m1) <= 5 * np.sqrt(v0 + v1))


def test_predictive_matches_oracle(device):
    rs = np.random.RandomState(0)
    N, D, S = 3000, 100, 40
    X = rs.randn(N, D).astype(np.float32) * 0.3
    coefs = rs.randn(S, D).astype(np.float32)
    out = Predictive(P.logistic_regression, {"coefs": torch.from_numpy(coefs)})(7, torch.from_numpy(X).to(device), None)["obs"]
    assert out.shape == (S, N) and out.dtype == torch.int32
    got = out.cpu().numpy()
    ref, p, u = OPred.predict_logreg(X, coefs, 7)
    mismatch = got != ref
    assert mismatch.mean() <= 1e-3
    assert np.all(np.abs(u[mismatch] - p[mismatch]) < 1e-5)
    np.testing.assert_allclose(got.mean(), p.mean(), atol=0.01)
