"""The fused softmax-regression potential (csrc/potential_softmax.hip through
potentials.SoftmaxRegression) against plain torch float64 with autograd on the CPU.

Tolerance (the convention of tests/test_gpu_svi.py): the same expression in torch float32 on the
CPU, its largest deviation from float64 on the same inputs, times 4 for the different summation
order; U and dU each have their own.  Every case prints both numbers; one MI355X run, for the
record (max |x - float64|: "f32" the float32 expression, whose 4-fold is the tolerance, "dev" the
device):

  K, D, N, C [x scale]: U f32 / dev; dU f32 / dev
   2,  1,   1, 65: 3.3e-07 / 3.3e-07; 8.8e-08 / 8.8e-08      3, 16,  31,  9: 1.9e-05 / 8.5e-06; 2.5e-06 / 1.8e-06
   7, 55, 513, 17: 6.3e-04 / 3.1e-04; 3.8e-05 / 1.0e-05      8, 17,  33,  5: 3.2e-05 / 1.8e-05; 2.3e-06 / 1.2e-06
   9, 64,  33,  1: 6.7e-05 / 5.5e-05; 3.3e-06 / 2.1e-06     32, 55,  31,  5: 1.9e-04 / 7.8e-05; 5.1e-06 / 2.3e-06
  32,  1, 513,  2: 9.6e-05 / 9.6e-05; 1.8e-05 / 1.7e-06      7, 64,   1,  1: 1.6e-05 / 1.6e-05; 9.2e-07 / 1.2e-06
   2, 17, 513, 17: 1.7e-04 / 1.5e-04; 6.8e-05 / 1.4e-05      3, 55,  33, 33: 6.5e-05 / 2.3e-05; 5.2e-06 / 3.9e-06
   9, 16,  31,  9: 1.5e-05 / 1.5e-05; 2.4e-06 / 1.6e-06      8, 64, 513,  1: 3.1e-04 / 1.8e-04; 3.2e-05 / 7.5e-06
   7, 55, 513, 17 x 30: 3.7e-02 / 1.7e-02; 1.4e-04 / 7.2e-05 (max |U| 3.6e5, max |dU| 160)
  Largest dev / f32 ratio 1.32 (dU at N = 1).  End to end: the two runs' posterior means differ by at most 0.55
  combined standard errors; SVI loss 681.2 -> 155.8.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import numpyro_amd as numpyro
from numpyro_amd import diagnostics, jnp, native, optim
from numpyro_amd import distributions as dist, potentials as P
from numpyro_amd.infer import MCMC, NUTS, SVI, Trace_ELBO
from numpyro_amd.infer.autoguide import AutoNormal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def potential_energy(X, y, W):
    """U of one chain, W [D, K]: the reference expression."""
    D, K = W.shape
    logits = X @ W
    return (torch.logsumexp(logits, 1).sum() - logits[torch.arange(X.shape[0]), y].sum() + 0.5 * W.pow(2).sum()
            + D * K / 2 * math.log(2 * math.pi))


def reference(X, y, W, dtype):
    """(U [C], dU [C, D K]) of the chains W [C, D, K] in `dtype` on the CPU, as float64."""
    Xt, Wt = torch.from_numpy(X).to(dtype), torch.from_numpy(W).to(dtype).requires_grad_(True)
    yt = torch.from_numpy(y).long()
    U = torch.stack([potential_energy(Xt, yt, w) for w in Wt])
    (G,) = torch.autograd.grad(U.sum(), Wt)
    return U.detach().double().numpy(), G.double().reshape(len(W), -1).numpy()


def data(N, D, K, C, scale=1.0):
    rs = np.random.RandomState(N + 1000 * D + 100000 * K)
    return (rs.randn(N, D).astype(np.float32), rs.randint(0, K, N),
            (scale * rs.randn(C, D, K)).astype(np.float32))


def evaluate(device, X, y, K, W, phase=None, active=None):
    """(U [ldc], dU [ldc, D K]) of a NaN-filled arena after one launch over the chains W."""
    C, ldc = len(W), (len(W) + 63) // 64 * 64 + 64
    pot = P.SoftmaxRegression(X, y, K)
    pot.bind(C, ldc, device)
    z, g = (torch.full((pot.dim, ldc), float("nan"), device=device) for _ in range(2))
    z[:, :C] = torch.from_numpy(W.reshape(C, -1).T.copy()).to(device)
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


def chains_of(K, kind):
    """1 chain, a partial second column tile, a second workgroup (32 / KP chains per tile, 4 tiles)."""
    per_tile = 32 // (1 << (K - 1).bit_length())
    return (1, per_tile + 1, 4 * per_tile + 1)[kind]


# every K, D, N and chain count the kernel treats differently, crossed a few at a time
SHAPES = [(2, 1, 1, 2), (3, 16, 31, 1), (7, 55, 513, 2), (8, 17, 33, 1), (9, 64, 33, 0), (32, 55, 31, 2),
          (32, 1, 513, 1), (7, 64, 1, 0), (2, 17, 513, 1), (3, 55, 33, 2), (9, 16, 31, 2), (8, 64, 513, 0)]


@pytest.mark.parametrize("K,D,N,kind,scale", [s + (1.0,) for s in SHAPES] + [(7, 55, 513, 2, 30.0)])
def test_potential_and_gradient_match_float64(device, K, D, N, kind, scale):
    C = chains_of(K, kind)
    X, y, W = data(N, D, K, C, scale)
    U, G = evaluate(device, X, y, K, W)
    assert np.isnan(U[C:]).all() and np.isnan(G[C:]).all() and np.isfinite(U[:C]).all() and np.isfinite(G[:C]).all()
    (U64, G64), (U32, G32) = reference(X, y, W, torch.float64), reference(X, y, W, torch.float32)
    for what, dev, f64, f32 in (("U", U[:C], U64, U32), ("dU", G[:C], G64, G32)):
        spread, err = np.abs(f32 - f64).max(), np.abs(dev - f64).max()
        print(f"K={K} D={D} N={N} C={C} scale={scale} {what}: float32 vs float64 {spread:.3g}, device vs float64 "
              f"{err:.3g}, max |{what}| {np.abs(f64).max():.3g}")
        assert err <= 4 * spread


@pytest.mark.parametrize("K,D,N", [(7, 55, 513), (32, 17, 33)])
def test_a_chain_does_not_depend_on_its_batch(device, K, D, N):
    """Alone, one of 300, at another position, under a phase mask and in a scrambled list: the same bits."""
    C, (X, y, W) = 300, data(N, D, K, 300)
    U, G = evaluate(device, X, y, K, W)
    for c in (0, 7, 299):
        U1, G1 = evaluate(device, X, y, K, W[c:c + 1])
        np.testing.assert_array_equal(U1[0], U[c])
        np.testing.assert_array_equal(G1[0], G[c])
    Ur, Gr = evaluate(device, X, y, K, np.roll(W, 37, axis=0))
    np.testing.assert_array_equal(Ur[:C], np.roll(U[:C], 37))
    np.testing.assert_array_equal(Gr[:C], np.roll(G[:C], 37, axis=0))
    rs = np.random.RandomState(1)
    on = rs.rand(C) < 0.3
    on[128:256] = False  # a workgroup without a chain
    Up, Gp = evaluate(device, X, y, K, W, phase=np.where(on, native.PH_LEAF, native.PH_WAIT))
    listed = rs.permutation(np.flatnonzero(rs.rand(C) < 0.4))
    Ua, Ga = evaluate(device, X, y, K, W, active=listed)
    for Us, Gs, chains in ((Up, Gp, np.flatnonzero(on)), (Ua, Ga, listed)):
        assert 0 < len(chains) < C
        np.testing.assert_array_equal(Us[chains], U[chains])
        np.testing.assert_array_equal(Gs[chains], G[chains])
        rest = np.setdiff1d(np.arange(len(Us)), chains)
        assert np.all(np.isnan(Us[rest])) and np.all(np.isnan(Gs[rest]))


def test_a_label_outside_the_classes_is_refused_naming_the_row(device):
    X, y, _ = data(33, 3, 3, 1)
    pot = P.SoftmaxRegression(X, np.where(np.arange(33) == 21, 3, y), 3)
    with pytest.raises(native.NativeError, match=r"row 21 .*\[0, 3\)"):
        pot.bind(1, 64, device)


DEBUG_SCRIPT = r"""
import sys
sys.path.insert(0, "tests")
import numpy as np, torch
from numpyro_amd import native
import test_gpu_softmax as T
assert native.LIB_PATH.endswith("libnumpyro_amd_debug.so"), native.LIB_PATH
for K in (3, 32):
    for D in (1, 55):
        X, y, W = T.data(33, D, K, 70)
        U, G = T.evaluate(torch.device("cuda:0"), X, y, K, W)
        Ua, Ga = T.evaluate(torch.device("cuda:0"), X, y, K, W, active=np.array([69, 3, 40]))
        assert np.isfinite(U[:70]).all() and np.isfinite(G[:70]).all() and np.isfinite(Ua).sum() == 3
print("softmax debug build ok")
"""


def test_debug_build_runs_the_kernels_without_a_failed_check():
    env = dict(os.environ, NUMPYRO_AMD_DEBUG="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", DEBUG_SCRIPT], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=110)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "NMX_DCHECK failed" not in out and "softmax debug build ok" in out, out[-3000:]


def model(X, y):
    W = numpyro.sample("coefs", dist.Normal(0.0, 1.0).expand([3, 3]))
    numpyro.sample("obs", dist.Categorical(logits=jnp.matmul(X, W)), obs=y)


def end_to_end_data(rs=np.random.RandomState(5)):
    X = rs.randn(200, 3).astype(np.float32)
    return X, np.argmax(X @ rs.randn(3, 3) + rs.gumbel(size=(200, 3)), 1)


def test_nuts_matches_the_torch_potential(device):
    X, y = end_to_end_data()
    Xd, yd = torch.from_numpy(X).to(device), torch.from_numpy(y).to(device)
    runs = []
    for kernel, args, kw in ((NUTS(model), (X, y), {}),
                             (NUTS(potential_fn=lambda s: potential_energy(Xd, yd, s["coefs"])), (),
                              {"init_params": {"coefs": torch.zeros(64, 3, 3)}})):
        mcmc = MCMC(kernel, num_warmup=200, num_samples=200, num_chains=64, progress_bar=False)
        mcmc.run(3, *args, **kw)
        x = mcmc.get_samples(group_by_chain=True)["coefs"].cpu().numpy().reshape(64, 200, 9).astype(np.float64)
        ess = diagnostics.effective_sample_size(x)
        runs.append((x.mean((0, 1)), x.var((0, 1), ddof=1) / ess, kernel))
    assert type(runs[0][2]._potential) is P.SoftmaxRegression
    (m0, v0, _), (m1, v1, _) = runs
    print("mean difference / combined standard error", np.abs(m0 - m1) / np.sqrt(v0 + v1))
    assert np.all(np.abs(m0 - m1) <= 5 * np.sqrt(v0 + v1))


def test_svi_lowers_the_loss(device):
    X, y = end_to_end_data()
    res = SVI(model, AutoNormal(model), optim.Adam(0.05), Trace_ELBO(64)).run(2, 50, X, y, device=device)
    losses = res.losses.cpu().numpy()
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0]
