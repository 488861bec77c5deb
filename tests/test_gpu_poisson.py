"""Poisson regression on the D-blocked kernel (csrc/potential_logreg_wide.hip with the Poisson policy,
through potentials.PoissonRegression) against a NumPy float64 restatement of U and dU.

Tolerance (the convention of tests/test_gpu_softmax.py and tests/test_gpu_logreg_wide.py): the device's
largest deviation from float64 is at most 4 times that of the same NumPy function run in float32, for
U and for dU separately; every case prints both numbers.  One MI355X run, for the record: the device's
deviation was 0.06 to 1.2 times the float32 restatement's (largest: dU at D = 1024, N = 1, 1.13e-05
against 9.72e-06; large rates, max |U| 3.4e6: U 0.77 against 12.8, dU 1.06 against 1.57); end to end the
fused and the torch runs' posterior means differ by at most 1.9 combined standard errors.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import numpyro_amd as numpyro
from numpyro_amd import diagnostics, jnp, native
from numpyro_amd import distributions as dist, potentials as P
from numpyro_amd.infer import MCMC, NUTS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference(X, y, off, Z, dtype):
    """(U [C], dU [C, D]) of the chains Z [C, D], every operation in `dtype`."""
    X, Z, y = X.astype(dtype), Z.astype(dtype), y.astype(dtype)
    eta = X @ Z.T + (0 if off is None else off.astype(dtype)[:, None])
    mu = np.exp(eta)
    const = dtype(sum(math.lgamma(v + 1) for v in y.astype(np.float64)) + 0.5 * X.shape[1] * math.log(2 * math.pi))
    return (mu - y[:, None] * eta).sum(0) + dtype(0.5) * (Z * Z).sum(1) + const, (mu - y[:, None]).T @ X + Z


def case(N, D, C, offset, seed=0):
    """eta of order 1 (coefficients of order 1 / sqrt(D)); offset: None, "unit" or "large" (eta up to
    about 10, rates up to about 1e5; the test asserts that the float32 reference stays finite)."""
    rs = np.random.RandomState(seed + 7 * D + N)
    X = rs.randn(N, D).astype(np.float32)
    Z = (rs.randn(C, D) / np.sqrt(D)).astype(np.float32)
    off = {None: None, "unit": rs.randn(N), "large": rs.uniform(6, 9, N)}[offset]
    off = None if off is None else off.astype(np.float32)
    y = rs.poisson(np.exp(X @ (rs.randn(D) / np.sqrt(D)) + (0 if off is None else off))).astype(np.float32)
    return X, y, off, Z


def evaluate(device, X, y, off, Z, phase=None, active=None):
    """(U [ldc], dU [ldc, D]) of a NaN-filled arena after one launch over the chains Z [C, D]."""
    C, ldc = len(Z), (len(Z) + 63) // 64 * 64 + 64
    pot = P.PoissonRegression(X, y, off)
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


# every shape class and class edge (D <= 32 and 64: the 4 x 1 class with one and two d-tiles; 128, 256, 512,
# 1024); N = one tile, two tiles, several row splits with tiles; C = 1, one workgroup's chains + 1 (32 per
# chain tile, 4 / 2 / 1 tiles by D) and 300; with and without an offset; large rates through the offset
CASES = [(1, 1, 300, None), (32, 513, 129, "unit"), (33, 33, 300, None), (64, 513, 1, "unit"), (65, 33, 129, "unit"),
         (128, 513, 300, None), (129, 1, 129, "unit"), (257, 513, 65, None), (513, 33, 300, "unit"),
         (1024, 513, 1, None), (1024, 1, 33, "unit"), (50, 513, 300, "large"), (300, 513, 65, "large")]


@pytest.mark.parametrize("D,N,C,offset", CASES)
def test_potential_and_gradient_match_float64(device, D, N, C, offset):
    X, y, off, Z = case(N, D, C, offset)
    U64, G64 = reference(X, y, off, Z, np.float64)
    U32, G32 = reference(X, y, off, Z, np.float32)
    assert np.isfinite(U32).all() and np.isfinite(G32).all()
    U, G = evaluate(device, X, y, off, Z)
    assert np.isnan(U[C:]).all() and np.isnan(G[C:]).all()
    for what, dev, r64, r32 in (("U", U[:C], U64, U32), ("dU", G[:C], G64, G32)):
        spread, err = np.abs(r32 - r64).max(), np.abs(dev - r64).max()
        print(f"D={D} N={N} C={C} offset={offset} {what}: float32 vs float64 {spread:.3g}, device vs float64 "
              f"{err:.3g}, max |{what}| {np.abs(r64).max():.3g}")
        assert err <= 4 * spread


@pytest.mark.parametrize("D", [20, 50, 100, 200, 400, 1000])
def test_a_chain_does_not_depend_on_its_batch(device, D):
    """Alone, one of 300, at another position, under a phase mask and in a scrambled list: the same bits."""
    C, (X, y, off, Z) = 300, case(513, D, 300, "unit")
    U, G = evaluate(device, X, y, off, Z)
    assert np.isfinite(U[:C]).all() and np.isfinite(G[:C]).all()
    for c in (0, 7, 299):
        U1, G1 = evaluate(device, X, y, off, Z[c:c + 1])
        np.testing.assert_array_equal(U1[0], U[c])
        np.testing.assert_array_equal(G1[0], G[c])
    Ur, Gr = evaluate(device, X, y, off, np.roll(Z, 37, axis=0))
    np.testing.assert_array_equal(Ur[:C], np.roll(U[:C], 37))
    np.testing.assert_array_equal(Gr[:C], np.roll(G[:C], 37, axis=0))
    rs = np.random.RandomState(1)
    on = rs.rand(C) < 0.3
    on[128:256] = False  # workgroups without a chain, in every shape class
    Up, Gp = evaluate(device, X, y, off, Z, phase=np.where(on, native.PH_LEAF, native.PH_WAIT))
    listed = rs.permutation(np.flatnonzero(rs.rand(C) < 0.4))
    Ua, Ga = evaluate(device, X, y, off, Z, active=listed)
    for Us, Gs, chains in ((Up, Gp, np.flatnonzero(on)), (Ua, Ga, listed)):
        assert 0 < len(chains) < C
        np.testing.assert_array_equal(Us[chains], U[chains])
        np.testing.assert_array_equal(Gs[chains], G[chains])
        rest = np.setdiff1d(np.arange(len(Us)), chains)
        assert np.all(np.isnan(Us[rest])) and np.all(np.isnan(Gs[rest]))


@pytest.mark.parametrize("D", [20, 400])
def test_an_overflowing_chain_gets_infinite_energy_and_touches_no_other(device, D):
    X, y, off, Z = case(70, D, 70, "unit")
    U, G = evaluate(device, X, y, off, Z)
    Zo = Z.copy()
    Zo[5] = 40.0 * np.sign(X[3])  # eta of row 3 = 40 sum |x|: past float32's exp range, every product finite
    Uo, Go = evaluate(device, X, y, off, Zo)
    assert Uo[5] == np.inf
    others = np.arange(70) != 5
    np.testing.assert_array_equal(Uo[:70][others], U[:70][others])
    np.testing.assert_array_equal(Go[:70][others], G[:70][others])


DEBUG_SCRIPT = r"""
import sys
sys.path.insert(0, "tests")
import numpy as np, torch
from numpyro_amd import native
import test_gpu_poisson as T
assert native.LIB_PATH.endswith("libnumpyro_amd_debug.so"), native.LIB_PATH
for D in (20, 50, 80, 128, 160, 256, 300, 512, 700, 1024):  # one per instantiation of the Poisson policy
    X, y, off, Z = T.case(70, D, 70, "unit")
    U, G = T.evaluate(torch.device("cuda:0"), X, y, off, Z)
    Ua, Ga = T.evaluate(torch.device("cuda:0"), X, y, off, Z, active=np.array([69, 3, 40]))
    assert np.isfinite(U[:70]).all() and np.isfinite(G[:70]).all() and np.isfinite(Ua).sum() == 3
print("poisson debug build ok")
"""


def test_debug_build_runs_the_kernels_without_a_failed_check():
    env = dict(os.environ, NUMPYRO_AMD_DEBUG="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", DEBUG_SCRIPT], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=110)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "NMX_DCHECK failed" not in out and "poisson debug build ok" in out, out[-3000:]


def traced_model(X, y, log_exposure):
    beta = numpyro.sample("beta", dist.Normal(0.0, 1.0).expand([X.shape[1]]))
    numpyro.sample("obs", dist.Poisson(jnp.exp(jnp.matmul(X, beta) + log_exposure)), obs=y)


@pytest.mark.parametrize("D,T", [(5, 100), (72, 30)])  # T warm-up and T sampling transitions (three runs each)
def test_nuts_fused_and_traced_agree_and_match_the_torch_potential(device, D, T):
    rs = np.random.RandomState(5)
    X = np.concatenate([0.5 * rs.randn(300, D - 1), np.ones((300, 1))], 1).astype(np.float32)
    off = rs.uniform(-1, 1, 300).astype(np.float32)
    y = rs.poisson(np.exp(X @ (0.5 * rs.randn(D)) + off)).astype(np.float32)
    Xd, yd, od = (torch.from_numpy(v).to(device) for v in (X, y, off))

    def torch_potential(s):
        eta = Xd @ s["beta"] + od
        return (torch.exp(eta) - yd * eta).sum() + 0.5 * s["beta"].pow(2).sum()

    runs = []
    for kernel, args, kw, site in ((NUTS(P.poisson_regression), (X, y, off), {}, "coefs"),
                                   (NUTS(traced_model), (X, y, off), {}, "beta"),
                                   (NUTS(potential_fn=torch_potential), (), {"init_params": {"beta": torch.zeros(64, D)}},
                                    "beta")):
        mcmc = MCMC(kernel, num_warmup=T, num_samples=T, num_chains=64, progress_bar=False)
        mcmc.run(3, *args, **kw)
        runs.append(mcmc.get_samples(group_by_chain=True)[site].cpu().numpy().reshape(64, T, D))
        if args:
            assert type(kernel._potential) is P.PoissonRegression
    np.testing.assert_array_equal(runs[0], runs[1])
    stats = []
    for x in (runs[0].astype(np.float64), runs[2].astype(np.float64)):
        stats.append((x.mean((0, 1)), x.var((0, 1), ddof=1) / diagnostics.effective_sample_size(x)))
    (m0, v0), (m1, v1) = stats
    print("largest mean difference / combined standard error", (np.abs(m0 - m1) / np.sqrt(v0 + v1)).max())
    assert np.all(np.abs(m0 - m1) <= 5 * np.sqrt(v0 + v1))
