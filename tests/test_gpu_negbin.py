"""Negative-binomial regression on the D-blocked kernel (csrc/potential_logreg_wide.hip, lk_negbin and k_negbin_rising,
through potentials.NegativeBinomialRegression) against a NumPy float64 restatement of U and its gradient.

Tolerance (the convention of tests/test_gpu_poisson.py): the device's largest deviation from float64 is at most 4
times that of the same NumPy function run in float32, for U, dU/db and dU/du separately; every case prints both.
The float32 run takes R(phi, y) and its derivative as rising sums below y = 64 and from scipy in float64, cast,
above: the difference of two float32 gammaln values would inflate the yardstick.  A case with C = 1 launches eight
chains, each alone: one chain is one sample of a float32 rounding (first MI355X run, D = 64, N = 513: U = 974 off by
5.89e-05, 0.97 ulp, on the device where the float32 restatement happened to land 2.15e-06 from float64).  One run,
for the record: device over float32 deviation 0.005 to 1.01 (U), 0.18 to 1.59 (dU/db), 0.04 to 1.02 (dU/du).
"""
import numpy as np
import pytest
import scipy.special as sp
import torch

from numpyro_amd import diagnostics, native, potentials as P
from numpyro_amd.infer import MCMC, NUTS, log_likelihood
from test_negbin import model

pytestmark = pytest.mark.gpu
PRIOR = (2.0, 0.5)


def reference(X, y, off, A, dtype):
    """[C, D + 2] = (dU/db | dU/du | U) of the chains A [C, D + 1] = (b | u = log phi), all in `dtype`."""
    D, (a, b) = X.shape[1], PRIOR
    X, A, yc = X.astype(dtype), A.astype(dtype), y.astype(dtype)[:, None]
    B, u, phi = A[:, :D], A[:, D], np.exp(A[:, D])
    Rs, dRs = np.zeros_like(phi), np.zeros_like(phi)  # sum_n R(phi, y_n) and its phi-derivative
    for v, m in zip(*np.unique(y, return_counts=True)):
        if v < 64:
            j = np.arange(v, dtype=dtype)[:, None]
            r, d = np.log(phi + j).sum(0), (1 / (phi + j)).sum(0)
        else:
            p64 = phi.astype(np.float64)
            r, d = sp.gammaln(p64 + v) - sp.gammaln(p64), sp.digamma(p64 + v) - sp.digamma(p64)
        Rs, dRs = Rs + dtype(m) * r.astype(dtype), dRs + dtype(m) * d.astype(dtype)
    l = X @ B.T + (0 if off is None else off.astype(dtype)[:, None]) - u
    e = np.exp(-np.abs(l))
    spl, p = np.maximum(l, 0) + np.log1p(e), np.where(l >= 0, 1, e) / (1 + e)
    res = (phi + yc) * p - yc
    const = dtype(sp.gammaln(y.astype(np.float64) + 1).sum() + 0.5 * D * np.log(2 * np.pi) + sp.gammaln(a) - a * np.log(b))
    U = (phi * spl.sum(0) + (yc * spl).sum(0) - (yc * l).sum(0) - Rs + dtype(0.5) * (B * B).sum(1)
         - (dtype(a) * u - dtype(b) * phi) + const)
    du = phi * spl.sum(0) - res.sum(0) - phi * dRs - dtype(a) + dtype(b) * phi
    return np.concatenate([res.T @ X + B, du[:, None], U[:, None]], 1)


def case(N, D, C, offset=False, kind="plain"):
    """u ~ N(0, 1.5); "poisson-limit": phi = 1e4, dU/du cancels; "wide": > 300 distinct counts up to about 1e5."""
    rs = np.random.RandomState(7 * D + N)
    X = rs.randn(N, D).astype(np.float32)
    A = np.concatenate([rs.randn(C, D) / np.sqrt(D), 1.5 * rs.randn(C, 1)], 1)
    if kind == "poisson-limit":
        A[:, D] = np.log(1e4)
    off = (rs.uniform(0, 11.5, N) if kind == "wide" else rs.randn(N)).astype(np.float32) if offset else None
    mu = np.exp(X @ (rs.randn(D) / np.sqrt(D)) + (0 if off is None else off))
    y = rs.poisson(rs.gamma(2.0, mu / 2.0))
    assert kind != "wide" or (len(np.unique(y)) > 300 and y.max() > 3e4)
    return X, y.astype(np.float32), off, A.astype(np.float32)


def evaluate(device, X, y, off, A, phase=None, active=None):  # [ldc, D + 2] = (dU | U) of a NaN-filled arena
    C, ldc = len(A), (len(A) + 63) // 64 * 64 + 64
    pot = P.NegativeBinomialRegression(X, y, off, PRIOR)
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


def within_four_times_float32(R, args, chains=np.s_[:]):
    with np.errstate(over="ignore"):
        R64, R32 = reference(*args, np.float64), reference(*args, np.float32)
    assert np.isfinite(R32[chains]).all()
    for what, at in {"U": np.s_[:, -1], "dU/db": np.s_[:, :-2], "dU/du": np.s_[:, -2]}.items():
        dev, r64, r32 = R[chains][at], R64[chains][at], R32[chains][at]
        spread, err = np.abs(r32 - r64).max(), np.abs(dev - r64).max()
        print(f"{what}: float32 vs float64 {spread:.3g}, device vs float64 {err:.3g}, max |{what}| {np.abs(r64).max():.3g}")
        assert err <= 4 * spread


# D: the 4 x 1 class with one and two d-tiles, then each class edge; N: one, two and 17 tiles; C: 1, 129, 300
CASES = [(1, 33, 300, False, "plain"), (33, 513, 129, True, "plain"), (33, 1, 300, False, "plain"),
         (64, 33, 129, True, "plain"), (64, 513, 1, False, "plain"), (65, 33, 129, False, "plain"),
         (129, 513, 300, True, "plain"), (257, 33, 1, False, "plain"), (257, 513, 129, True, "plain"),
         (513, 1, 300, False, "plain"), (513, 513, 129, True, "plain"), (1024, 33, 129, True, "plain"),
         (1024, 513, 1, False, "plain"), (33, 513, 129, True, "poisson-limit"), (65, 513, 129, True, "wide")]


@pytest.mark.parametrize("D,N,C,offset,kind", CASES)
def test_potential_and_gradient_match_float64(device, D, N, C, offset, kind):
    args = case(N, D, 8 if C == 1 else C, offset, kind)
    A = args[3]  # C = 1: eight chains, each launched alone (see the docstring)
    Rs = [evaluate(device, *args[:3], A[i:i + 1]) for i in range(8)] if C == 1 else [evaluate(device, *args)]
    assert all(np.isnan(R[C:]).all() for R in Rs)
    within_four_times_float32(np.concatenate([R[:C] for R in Rs]), args)


@pytest.mark.parametrize("D", [20, 200, 1000])
def test_a_chain_does_not_depend_on_its_batch(device, D):  # alone, rolled, masked, listed, beside edge chains
    C, (X, y, off, A) = 300, case(513, D, 300, True)
    R = evaluate(device, X, y, off, A)
    assert np.isfinite(R[:C]).all()
    for c in (0, 7, 299):
        np.testing.assert_array_equal(evaluate(device, X, y, off, A[c:c + 1])[0], R[c])
    rolled = evaluate(device, X, y, off, np.roll(A, 37, axis=0))
    np.testing.assert_array_equal(rolled[:C], np.roll(R[:C], 37, axis=0))
    rs = np.random.RandomState(1)
    on = rs.rand(C) < 0.3
    on[128:256] = False  # workgroups without a chain, in every shape class
    masked = evaluate(device, X, y, off, A, phase=np.where(on, native.PH_LEAF, native.PH_WAIT))
    listed = rs.permutation(np.flatnonzero(rs.rand(C) < 0.4))
    scrambled = evaluate(device, X, y, off, A, active=listed)
    for some, chains in ((masked, np.flatnonzero(on)), (scrambled, listed)):
        assert 0 < len(chains) < C
        np.testing.assert_array_equal(some[chains], R[chains])
        assert np.all(np.isnan(np.delete(some, chains, axis=0)))
    # edges: u past float32's exp range in chain 5, eta reaching +-200 in chain 9; every other chain keeps its bits
    A[5, D] = 100.0
    A[9, :D] *= 200.0 / np.abs(X @ A[9, :D]).max()
    Ro = evaluate(device, X, y, off, A)
    assert not np.isfinite(Ro[5, -1]) and np.isfinite(Ro[9]).all()
    np.testing.assert_array_equal(np.delete(Ro[:C], [5, 9], axis=0), np.delete(R[:C], [5, 9], axis=0))
    within_four_times_float32(Ro[:C], (X, y, off, A), chains=np.s_[9:10])


def test_nuts_on_the_traced_model_matches_the_torch_potential(device):
    N, D, T, C = 200, 16, 40, 64  # T warm-up and T sampling transitions, trees of depth <= 5 (two runs)
    X, Y, _, _ = case(N, D, 1)
    Xd, yd = torch.from_numpy(X).to(device), torch.from_numpy(Y).to(device)

    def torch_potential(s):
        u, phi = s["u"], torch.exp(s["u"])
        l = Xd @ s["b"] - u
        nll = (phi + yd) * torch.nn.functional.softplus(l) - yd * l - torch.lgamma(phi + yd) + torch.lgamma(phi)
        return nll.sum() + 0.5 * s["b"].pow(2).sum() - (PRIOR[0] * u - PRIOR[1] * phi).sum()

    mcmc = MCMC(NUTS(model, max_tree_depth=5), num_warmup=T, num_samples=T, num_chains=C, progress_bar=False)
    mcmc.run(3, X, Y)
    assert type(mcmc.sampler._potential) is P.NegativeBinomialRegression
    flat = mcmc.get_samples()
    assert {k: tuple(v.shape[1:]) for k, v in flat.items()} == {"coefs": (D,), "phi": ()}
    ll = log_likelihood(model, flat, X, Y)["obs"]
    assert tuple(ll.shape) == (C * T, N) and bool(torch.isfinite(ll).all())
    s = {k: v.cpu().numpy() for k, v in mcmc.get_samples(group_by_chain=True).items()}
    runs = [np.concatenate([s["coefs"], np.log(s["phi"])[..., None]], -1)]
    mcmc = MCMC(NUTS(potential_fn=torch_potential, max_tree_depth=5), num_warmup=T, num_samples=T, num_chains=C,
                progress_bar=False)
    mcmc.run(3, init_params={"b": torch.zeros(C, D), "u": torch.zeros(C, 1)})
    s = {k: v.cpu().numpy() for k, v in mcmc.get_samples(group_by_chain=True).items()}
    runs.append(np.concatenate([s["b"], s["u"]], -1))
    (m0, v0), (m1, v1) = ((x.mean((0, 1)), x.var((0, 1), ddof=1) / diagnostics.effective_sample_size(x))
                          for x in (r.astype(np.float64).reshape(C, T, D + 1) for r in runs))
    print("largest mean difference / combined standard error", (np.abs(m0 - m1) / np.sqrt(v0 + v1)).max())
    assert np.all(np.abs(m0 - m1) <= 5 * np.sqrt(v0 + v1))
