"""The softmax-regression log-likelihood table and predictive draws (csrc/predictive_softmax.hip through
softmax_predictive.SoftmaxPredictive, infer.log_likelihood / pointwise_predictive / loo and
infer.Predictive) against plain torch float64 on the CPU.

Tolerance (the convention of tests/test_gpu_softmax.py): the same expression in torch float32 on the
CPU, its largest deviation from float64 over the table, times 4.  Every case prints both numbers.
One MI355X run, for the record (max |x - float64|: "f32" the float32 expression, "dev" the device):

  K, D, N, S [x scale]: f32 / dev
   2,  1,   1, 65: 7.6e-08 / 9.7e-08      3, 16,  31,  9: 1.8e-06 / 1.3e-06      7, 55, 513, 17: 1.0e-05 / 8.4e-06
   8, 17,  33,  5: 1.7e-06 / 1.7e-06      9, 64,  33,  1: 4.7e-06 / 4.9e-06     16, 55,  31,  9: 5.7e-06 / 5.1e-06
  17,  1, 513,  2: 1.0e-06 / 1.0e-06     32, 55,  31,  5: 5.7e-06 / 5.6e-06     32, 64, 513,  1: 9.1e-06 / 1.1e-05
   7, 64,   1, 17: 3.8e-06 / 3.1e-06      2, 17, 513,  1: 1.9e-06 / 1.4e-06      3, 55,  33, 33: 6.8e-06 / 6.6e-06
   7, 55, 513, 17 x 30: 2.9e-04 / 2.2e-04 (max |ll| 1.4e3)
  Largest dev / f32 ratio 1.29 (K = 2, D = 1, N = 1).  Draws: every frequency inside its bound by at least 1.2e-4.
  End to end (200 x 3, K = 3, S = 200): table 5.7e-07 / 6.2e-07, lppd 5.6e-07 / 7.3e-07, p_waic 9.6e-08 / 1.8e-07.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from numpyro_amd import potentials as P
from numpyro_amd.infer import Predictive, log_likelihood, loo, pointwise_predictive
from numpyro_amd.softmax_predictive import SoftmaxPredictive
from test_gpu_softmax import end_to_end_data, model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def data(N, D, K, S, scale=1.0):
    rs = np.random.RandomState(N + 1000 * D + 100000 * K)
    return (rs.randn(N, D).astype(np.float32), rs.randint(0, K, N).astype(np.int32),
            (scale * rs.randn(S, D, K)).astype(np.float32))


def reference(X, y, W, dtype):
    """log_softmax(X @ W_s)[n, y_n] [S, N] in `dtype` on the CPU, as float64."""
    l = torch.log_softmax(torch.from_numpy(X).to(dtype) @ torch.from_numpy(W).to(dtype), -1)
    return l[:, torch.arange(len(y)), torch.from_numpy(y).long()].double().numpy()


# every KP mapping and its pad, k-block count, row count and sample count (kind: 1 sample, one more
# than a tile's 32 / KP, one more than a workgroup's), crossed a few at a time
SHAPES = [(2, 1, 1, 2), (3, 16, 31, 1), (7, 55, 513, 2), (8, 17, 33, 1), (9, 64, 33, 0), (16, 55, 31, 2),
          (17, 1, 513, 1), (32, 55, 31, 2), (32, 64, 513, 0), (7, 64, 1, 2), (2, 17, 513, 0), (3, 55, 33, 2)]


@pytest.mark.parametrize("K,D,N,kind,scale", [s + (1.0,) for s in SHAPES] + [(7, 55, 513, 2, 30.0)])
def test_table_matches_float64(device, K, D, N, kind, scale):
    per_tile = 32 // (1 << (K - 1).bit_length())
    S = (1, per_tile + 1, 4 * per_tile + 1)[kind]
    X, y, W = data(N, D, K, S, scale)
    kernel = SoftmaxPredictive(X, device)
    # two launches at a sample offset into a wider NaN-filled table
    table = torch.full((S + 2, N + 5), float("nan"), device=device)
    for s0, s1 in ((0, S // 2), (S // 2, S)):
        if s1 > s0:
            kernel.log_likelihood(y, W[s0:s1], table[s0:])
    table = table.cpu().numpy()
    assert np.isnan(table[S:]).all() and np.isnan(table[:, N:]).all()
    r64, r32 = reference(X, y, W, torch.float64), reference(X, y, W, torch.float32)
    spread, err = np.abs(r32 - r64).max(), np.abs(table[:S, :N] - r64).max()
    print(f"K={K} D={D} N={N} S={S} scale={scale}: float32 vs float64 {spread:.3g}, device vs float64 {err:.3g}, "
          f"max |ll| {np.abs(r64).max():.3g}")
    assert err <= 4 * spread


@pytest.mark.parametrize("K,D,N", [(7, 55, 513), (32, 17, 33)])
def test_a_sample_does_not_depend_on_its_batch(device, K, D, N):
    X, y, W = data(N, D, K, 300)
    kernel = SoftmaxPredictive(X, device)
    full = kernel.log_likelihood(y, W)
    for s in (0, 7, 299):
        assert torch.equal(kernel.log_likelihood(y, W[s:s + 1])[0], full[s])
    assert torch.equal(kernel.log_likelihood(y, np.roll(W, 37, axis=0)), torch.roll(full, 37, 0))


@pytest.mark.parametrize("K", [8, 7, 32])
def test_draws_follow_the_softmax(device, K):
    S, N, D = 4096, 33, 17
    X, _, W = data(N, D, K, 300)
    kernel = SoftmaxPredictive(X, device)
    draws = kernel.draw(np.broadcast_to(W[0], (S, D, K)).copy(), 11).cpu().numpy()
    assert draws.dtype == np.int32 and draws.shape == (S, N) and draws.min() >= 0 and draws.max() < K
    p = torch.softmax(torch.from_numpy(X).double() @ torch.from_numpy(W[0]).double(), -1).numpy()
    freq = (draws[:, :, None] == np.arange(K)).mean(0)
    excess = np.abs(freq - p) - (5 * np.sqrt(p * (1 - p) / S) + 1 / S)
    print(f"K={K}: largest |frequency - p| over its bound {excess.max():.3g} (<= 0 passes)")
    assert (excess <= 0).all()
    assert torch.equal(kernel.draw(W, 11)[:5], kernel.draw(W[:5], 11))


def test_public_interface_end_to_end(device):
    X, y = end_to_end_data()
    S, N = 200, len(y)
    W = (0.5 * np.random.RandomState(3).randn(S, 3, 3)).astype(np.float32)
    samples = {"coefs": torch.from_numpy(W)}
    r64, r32 = reference(X, y.astype(np.int32), W, torch.float64), reference(X, y.astype(np.int32), W, torch.float32)

    ll = log_likelihood(model, samples, X, y)["obs"]
    assert ll.dtype == torch.float32 and tuple(ll.shape) == (S, N)
    spread, err = np.abs(r32 - r64).max(), np.abs(ll.cpu().numpy() - r64).max()
    print(f"log_likelihood: float32 vs float64 {spread:.3g}, device vs float64 {err:.3g}")
    assert err <= 4 * spread

    def reduced(t):  # (lppd, p_waic) in the table's dtype
        return torch.logsumexp(t, 0) - math.log(S), t.var(0)

    pw = pointwise_predictive(model, samples, X, y)["obs"]
    t64 = torch.from_numpy(r64)
    spreads = {}
    for key, v64, v32 in zip(("lppd", "p_waic"), reduced(t64), reduced(torch.from_numpy(r32).float())):
        spreads[key] = (v32.double() - v64).abs().max().item()
        err = (pw[key].cpu().double() - v64).abs().max().item()
        print(f"{key}: float32 vs float64 {spreads[key]:.3g}, device vs float64 {err:.3g}")
        assert tuple(pw[key].shape) == (N,) and err <= 4 * spreads[key]

    cv = loo(model, samples, X, y)["obs"]
    elpd, k = cv["elpd_loo"].cpu().double(), cv["pareto_k"].cpu()
    assert tuple(elpd.shape) == tuple(k.shape) == (N,) and torch.isfinite(elpd).all() and torch.isfinite(k).all()
    assert (elpd <= reduced(t64)[0] + 4 * spreads["lppd"]).all()

    by_model = Predictive(model, samples)(5, X, None)["obs"]
    by_fused = Predictive(P.softmax_regression, samples)(5, X, None)["obs"]
    assert by_model.dtype == torch.int32 and tuple(by_model.shape) == (S, N) and by_model.is_cuda
    assert torch.equal(by_model, by_fused)
    kept = Predictive(model, samples)(5, X, y)["obs"]
    assert kept.dtype == torch.int32 and torch.equal(kept.cpu(), torch.from_numpy(y).int().expand(S, N))


DEBUG_SCRIPT = r"""
import sys
sys.path.insert(0, "tests")
import numpy as np, torch
from numpyro_amd import native
from numpyro_amd.softmax_predictive import SoftmaxPredictive
import test_gpu_softmax_predictive as T
assert native.LIB_PATH.endswith("libnumpyro_amd_debug.so"), native.LIB_PATH
for K in (3, 32):
    for D in (1, 55):
        X, y, W = T.data(33, D, K, 70)
        kernel = SoftmaxPredictive(X, torch.device("cuda:0"))
        ll, draws = kernel.log_likelihood(y, W), kernel.draw(W, 3)
        torch.cuda.synchronize()
        assert torch.isfinite(ll).all() and int(draws.min()) >= 0 and int(draws.max()) < K
print("softmax predictive debug build ok")
"""


def test_debug_build_runs_the_kernels_without_a_failed_check():
    env = dict(os.environ, NUMPYRO_AMD_DEBUG="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", DEBUG_SCRIPT], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=110)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "NMX_DCHECK failed" not in out and "softmax predictive debug build ok" in out, out[-3000:]
