"""Horseshoe-prior regression on the D-blocked kernel (csrc/potential_logreg_wide.hip with the horseshoe prior
policy, through potentials.HorseshoeRegression) against a NumPy float64 restatement of U and its gradient.

Tolerance (the convention of tests/test_gpu_poisson.py): the device's largest deviation from float64 is at
most 4 times that of the same NumPy function run in float32, for U, dU/dz, dU/dul and dU/dut separately;
every case prints both numbers.  One MI355X run, for the record: the device's deviation was 0.20 to 1.06 times
the float32 restatement's in 51 of the 52 comparisons; the other is dU/dut of the single chain at D = 1024,
N = 513 (Bernoulli), 5.98e-06 against 1.65e-06 at |dU/dut| = 101: 3.6 times, where the restatement's one sample
happens to sit within half an ulp of float32.  End to end the fused and the torch runs' posterior means of
betas differ by at most 1.8 combined standard errors.
"""
import math

import numpy as np
import pytest
import torch

from numpyro_amd import diagnostics, native, potentials as P
from numpyro_amd.infer import MCMC, NUTS
from test_horseshoe import model

pytestmark = pytest.mark.gpu


def reference(X, y, off, A, likelihood, dtype):
    """[C, 2 D + 2] = (dU/dul | dU/dut | dU/dz | U) of the chains A [C, 2 D + 1] = (ul | ut | z), all in `dtype`."""
    D = X.shape[1]
    X, y, A = X.astype(dtype), y.astype(dtype)[:, None], A.astype(dtype)
    ul, ut, z = A[:, :D], A[:, D:D + 1], A[:, D + 1:]
    s = np.exp(ut + ul)
    beta = s * z
    eta = X @ beta.T + (0 if off is None else off.astype(dtype)[:, None])
    if likelihood == "bernoulli":
        L, res = (np.maximum(eta, 0) + np.log1p(np.exp(-np.abs(eta))) - y * eta).sum(0), 1 / (1 + np.exp(-eta)) - y
    else:
        L = (np.exp(eta) - y * eta).sum(0) + dtype(sum(math.lgamma(v + 1) for v in y[:, 0].astype(np.float64)))
        res = np.exp(eta) - y
    G = res.T @ X
    l2c = lambda u: (np.abs(u) + np.log1p(np.exp(-2 * np.abs(u)))).sum(1)  # noqa: E731
    const = dtype((D + 1) * math.log(math.pi / 2) + 0.5 * D * math.log(2 * math.pi))
    U = L + l2c(ul) + l2c(ut) + dtype(0.5) * (z * z).sum(1) + const
    dut = (beta * G).sum(1, keepdims=True) + np.tanh(ut)
    return np.concatenate([beta * G + np.tanh(ul), dut, s * G + z, U[:, None]], 1)


def case(N, D, C, likelihood, offset=False):
    """z of order 1, ul and ut ~ N(0, 0.5), then ut shifted per chain to |beta| = 1: X @ beta has unit variance."""
    rs = np.random.RandomState(7 * D + N)
    X = rs.randn(N, D).astype(np.float32)
    A = np.concatenate([0.5 * rs.randn(C, D), 0.5 * rs.randn(C, 1), rs.randn(C, D)], 1)
    A[:, D] -= np.log(np.linalg.norm(np.exp(A[:, D:D + 1] + A[:, :D]) * A[:, D + 1:], axis=1))
    off = rs.randn(N).astype(np.float32) if offset else None
    eta = X @ (rs.randn(D) / np.sqrt(D)) + (0 if off is None else off)
    y = rs.poisson(np.exp(eta)) if likelihood == "poisson" else rs.rand(N) < 1 / (1 + np.exp(-eta))
    return X, y.astype(np.float32), off, A.astype(np.float32), likelihood


def evaluate(device, X, y, off, A, likelihood, phase=None, active=None):
    """[ldc, 2 D + 2] = (dU | U) of a NaN-filled arena after one launch over the chains A [C, 2 D + 1]."""
    C, ldc = len(A), (len(A) + 63) // 64 * 64 + 64
    pot = P.HorseshoeRegression(X, y, likelihood, off)
    pot.bind(C, ldc, device)
    z, g = (torch.full((pot.dim, ldc), float("nan"), device=device) for _ in range(2))
    z[:, :C] = torch.from_numpy(A.T.copy()).to(device)
    pe = torch.full((ldc,), float("nan"), device=device)
    ev = native.EvalBatch(z=native.ptr(z), grad=native.ptr(g), pe=native.ptr(pe), num_chains=C, ldc=ldc)
    i32 = lambda v: torch.from_numpy(np.pad(v, (0, ldc - len(v))).astype(np.int32)).to(device)  # noqa: E731
    if phase is not None:
        keep = i32(phase)
        ev.phase = native.ptr(keep)
    if active is not None:
        keep = i32(active), torch.tensor([len(active)], dtype=torch.int32, device=device)
        ev.active_idx, ev.active_count = native.ptr(keep[0]), native.ptr(keep[1])
    pot.evaluate(ev, native.stream_ptr())
    torch.cuda.synchronize()
    return torch.cat([g, pe[None]]).cpu().numpy().T


# D: the 4 x 1 class with one and two d-tiles, then each class edge; N: one tile, two tiles, several row splits
# with tiles; C: 1, one workgroup's chains + 1 and several workgroups
CASES = [(1, 33, 300, "bernoulli", False), (33, 513, 129, "poisson", True), (33, 33, 300, "bernoulli", False),
         (64, 1, 300, "bernoulli", False), (64, 513, 1, "poisson", False), (65, 33, 129, "bernoulli", False),
         (129, 513, 300, "poisson", True), (257, 33, 129, "bernoulli", False), (257, 513, 1, "poisson", False),
         (513, 1, 300, "bernoulli", False), (513, 33, 129, "poisson", True), (1024, 513, 1, "bernoulli", False),
         (1024, 33, 129, "poisson", False)]


@pytest.mark.parametrize("D,N,C,likelihood,offset", CASES)
def test_potential_and_gradient_match_float64(device, D, N, C, likelihood, offset):
    args = case(N, D, C, likelihood, offset)
    R64, R32, R = reference(*args, np.float64), reference(*args, np.float32), evaluate(device, *args)
    assert np.isfinite(R32).all() and np.isnan(R[C:]).all()
    rows = {"U": np.s_[:, -1], "dU/dul": np.s_[:, :D], "dU/dut": np.s_[:, D], "dU/dz": np.s_[:, D + 1:-1]}
    for what, at in rows.items():
        dev, r64, r32 = R[:C][at], R64[at], R32[at]
        spread, err = np.abs(r32 - r64).max(), np.abs(dev - r64).max()
        print(f"D={D} N={N} C={C} {likelihood} offset={offset} {what}: float32 vs float64 {spread:.3g}, device vs "
              f"float64 {err:.3g}, max |{what}| {np.abs(r64).max():.3g}")
        assert err <= 4 * spread


@pytest.mark.parametrize("D,likelihood", [(20, "bernoulli"), (200, "poisson"), (1000, "bernoulli")])
def test_a_chain_does_not_depend_on_its_batch(device, D, likelihood):
    """Alone, one of 300, at another position, under a phase mask and in a scrambled list: the same bits."""
    C, (X, y, off, A, _) = 300, case(513, D, 300, likelihood, likelihood == "poisson")
    R = evaluate(device, X, y, off, A, likelihood)
    assert np.isfinite(R[:C]).all()
    for c in (0, 7, 299):
        np.testing.assert_array_equal(evaluate(device, X, y, off, A[c:c + 1], likelihood)[0], R[c])
    rolled = evaluate(device, X, y, off, np.roll(A, 37, axis=0), likelihood)
    np.testing.assert_array_equal(rolled[:C], np.roll(R[:C], 37, axis=0))
    rs = np.random.RandomState(1)
    on = rs.rand(C) < 0.3
    on[128:256] = False  # workgroups without a chain, in every shape class
    masked = evaluate(device, X, y, off, A, likelihood, phase=np.where(on, native.PH_LEAF, native.PH_WAIT))
    listed = rs.permutation(np.flatnonzero(rs.rand(C) < 0.4))
    scrambled = evaluate(device, X, y, off, A, likelihood, active=listed)
    for some, chains in ((masked, np.flatnonzero(on)), (scrambled, listed)):
        assert 0 < len(chains) < C
        np.testing.assert_array_equal(some[chains], R[chains])
        assert np.all(np.isnan(np.delete(some, chains, axis=0)))


@pytest.mark.parametrize("D", [20, 400])
def test_an_overflowing_chain_gets_its_own_energy_and_touches_no_other(device, D):
    X, y, off, A, lk = case(70, D, 70, "bernoulli")
    R = evaluate(device, X, y, off, A, lk)
    A[5, D] = 100.0  # ut: exp(ut + ul) is past float32's range
    Ro = evaluate(device, X, y, off, A, lk)
    assert not np.isfinite(Ro[5, -1])
    np.testing.assert_array_equal(np.delete(Ro[:70], 5, axis=0), np.delete(R[:70], 5, axis=0))


def test_nuts_on_the_traced_model_matches_the_torch_potential(device):
    N, D, T, C = 200, 16, 40, 64  # T warm-up and T sampling transitions, trees of depth <= 5 (two runs)
    rs = np.random.RandomState(0)
    X = rs.randn(N, D).astype(np.float32)
    Y = (rs.rand(N) < 1 / (1 + np.exp(-X[:, :3] @ np.array([2.0, -1.0, 0.5])))).astype(np.float32)
    Xd, yd = torch.from_numpy(X).to(device), torch.from_numpy(Y).to(device)

    def torch_potential(s):
        eta = Xd @ (torch.exp(s["ut"] + s["ul"]) * s["z"])
        u = torch.cat([s["ul"], s["ut"]]).abs()
        prior = (u + torch.log1p(torch.exp(-2 * u))).sum() + 0.5 * s["z"].pow(2).sum()
        return (torch.nn.functional.softplus(eta) - yd * eta).sum() + prior

    kernel = NUTS(model, max_tree_depth=5)
    mcmc = MCMC(kernel, num_warmup=T, num_samples=T, num_chains=C, progress_bar=False)
    mcmc.run(3, X, Y)
    assert type(kernel._potential) is P.HorseshoeRegression
    flat = mcmc.get_samples()
    shapes = {"lambdas": (D,), "tau": (1,), "unscaled_betas": (D,), "betas": (D,)}
    assert {k: tuple(v.shape[1:]) for k, v in flat.items()} == shapes
    torch.testing.assert_close(flat["betas"], flat["tau"] * flat["lambdas"] * flat["unscaled_betas"], rtol=1e-6, atol=0)
    runs = [mcmc.get_samples(group_by_chain=True)["betas"].cpu().numpy().reshape(C, T, D)]
    mcmc = MCMC(NUTS(potential_fn=torch_potential, max_tree_depth=5), num_warmup=T, num_samples=T, num_chains=C,
                progress_bar=False)
    mcmc.run(3, init_params={"ul": torch.zeros(C, D), "ut": torch.zeros(C, 1), "z": torch.zeros(C, D)})
    s = {k: v.cpu().numpy() for k, v in mcmc.get_samples(group_by_chain=True).items()}
    runs.append((np.exp(s["ut"] + s["ul"]) * s["z"]).reshape(C, T, D))
    (m0, v0), (m1, v1) = ((x.mean((0, 1)), x.var((0, 1), ddof=1) / diagnostics.effective_sample_size(x))
                          for x in (r.astype(np.float64) for r in runs))
    print("largest mean difference / combined standard error", (np.abs(m0 - m1) / np.sqrt(v0 + v1)).max())
    assert np.all(np.abs(m0 - m1) <= 5 * np.sqrt(v0 + v1))
