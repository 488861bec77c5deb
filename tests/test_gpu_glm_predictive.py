"""The logistic / Poisson regression log-likelihood table and Poisson predictive counts
(csrc/predictive_glm.hip, through GlmPredictive and the public functions) against torch float64 on the CPU.
Tolerance (tests/test_gpu_softmax_predictive.py's): the same torch.distributions log_prob in float32, its
largest deviation from float64 over the table, times 4; every case prints both.  One MI355X run: the largest
device / float32 ratio was 3.2 (Poisson, D = 1024), every draw frequency inside its bound by 9e-5."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import numpyro_amd as numpyro
from numpyro_amd import distributions as dist, jnp
from numpyro_amd import potentials as P
from numpyro_amd.glm_predictive import GlmPredictive
from numpyro_amd.infer import Predictive, log_likelihood, loglik, loo, pointwise_predictive
from program_zoo import logit_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def data(family, N, D, S, scale=1.0, offset=False):  # y from the model at W[0], its log rate capped at 10
    rs = np.random.RandomState(N + 1000 * D + (family == "poisson"))
    X, W = rs.randn(N, D).astype(np.float32), (scale * rs.randn(S, D) / math.sqrt(D)).astype(np.float32)
    off = rs.uniform(-1, 1, N).astype(np.float32) if offset else None
    eta = X.astype(np.float64) @ W[0] + (0 if off is None else off)
    y = rs.poisson(np.exp(np.minimum(eta, 10))) if family == "poisson" else rs.rand(N) < 1 / (1 + np.exp(-eta))
    return X, y.astype(np.float32), off, W


def reference(family, X, y, off, W, dtype):
    eta = torch.from_numpy(W).to(dtype) @ torch.from_numpy(X).to(dtype).T
    if off is not None:
        eta = eta + torch.from_numpy(off).to(dtype)
    d = (torch.distributions.Bernoulli(logits=eta, validate_args=False) if family == "bernoulli" else
         torch.distributions.Poisson(eta.exp(), validate_args=False))
    return d.log_prob(torch.from_numpy(y).to(dtype)).double().numpy()


def check_table(tag, table, r64, r32):
    # the criterion on the entries finite in float32 in both references; -inf where float64 is -inf as float32
    with np.errstate(over="ignore"):
        r64f = r64.astype(np.float32)
    assert not np.isnan(table).any()
    assert (table[np.isneginf(r64f)] == -np.inf).all() and np.isfinite(table[np.isfinite(r64f)]).all()
    m = np.isfinite(r64f) & np.isfinite(r32)
    spread, err = np.abs(r32 - r64)[m].max(), np.abs(table - r64)[m].max()
    print(f"{tag}: float32 vs float64 {spread:.3g}, device vs float64 {err:.3g}, max |ll| {np.abs(r64[m]).max():.3g}, "
          f"-inf entries {int(np.isneginf(r64f).sum())}")
    assert m.sum() >= 32 and spread > 0 and err <= 4 * spread


# (D, N, kind) round the 16-deep chunk, the 32-row tile and 128-row block; S = 1, a wave's 64 + 1, a block's 128 + 1
SHAPES = [(1, 1, 2), (16, 31, 1), (17, 33, 0), (64, 513, 1), (65, 127, 2), (1024, 129, 1), (33, 128, 0), (17, 513, 2)]


@pytest.mark.parametrize("family", ["bernoulli", "poisson"])
@pytest.mark.parametrize("D,N,kind,scale", [s + (1.0,) for s in SHAPES] + [(65, 129, 1, 30.0)])
def test_table_matches_float64(device, family, D, N, kind, scale):
    S = (1, 65, 129)[kind]
    X, y, off, W = data(family, N, D, S, scale, offset=family == "poisson" and D % 2 == 1)
    kernel = GlmPredictive(X, device, family, y=y, offset=off)
    table = torch.full((S + 2, N + 5), float("nan"), device=device)
    for s0, s1 in ((0, S // 2), (S // 2, S)):  # two launches at a sample offset into the wider NaN-filled table
        if s1 > s0:
            kernel.log_likelihood(W[s0:s1], table[s0:])
    table = table.cpu().numpy()
    assert np.isnan(table[S:]).all() and np.isnan(table[:, N:]).all()
    check_table(f"{family} D={D} N={N} S={S} scale={scale}", table[:S, :N],
                reference(family, X, y, off, W, torch.float64), reference(family, X, y, off, W, torch.float32))


@pytest.mark.parametrize("family,D,N", [("poisson", 70, 256), ("poisson", 17, 333), ("bernoulli", 70, 333)])
def test_a_sample_does_not_depend_on_its_batch(device, family, D, N):
    X, y, off, W = data(family, N, D, 300, offset=family == "poisson")
    kernel = GlmPredictive(X, device, family, y=y, offset=off)
    full = kernel.log_likelihood(W)
    for s in (0, 7, 299):
        assert torch.equal(kernel.log_likelihood(W[s:s + 1])[0], full[s])
    assert torch.equal(kernel.log_likelihood(np.roll(W, 37, axis=0)), torch.roll(full, 37, 0))
    if family == "poisson":
        draws = kernel.draw(W, 11)
        assert torch.equal(draws[:5], kernel.draw(W[:5], 11))
        assert torch.equal(draws[5:], kernel.draw(W[5:], 11, sample0=5))


def test_draws_follow_the_poisson(device):
    S, N, D = 4096, 33, 17
    X, _, _, W = data("poisson", N, D, 1)
    off = np.linspace(math.log(0.5), math.log(60.0), N).astype(np.float32)  # inversion below a rate of 10, PTRS above
    draws = GlmPredictive(X, device, "poisson", offset=off).draw(np.broadcast_to(W[0], (S, D)).copy(), 11).cpu().numpy()
    assert draws.dtype == np.int32 and draws.shape == (S, N) and draws.min() >= 0
    rate = np.exp(X.astype(np.float64) @ W[0] + off)
    assert rate.min() < 5 and rate.max() > 20
    k = torch.arange(int(rate.max() * 3 + 30), dtype=torch.float64)
    p = torch.distributions.Poisson(torch.from_numpy(rate)[:, None]).log_prob(k).exp().numpy()  # [N, K]
    tested = np.cumsum(p, 1) - p < 1 - 1e-6  # the counts up to the 1 - 1e-6 quantile
    freq = (draws[:, :, None] == np.arange(p.shape[1])).mean(0)
    excess = (np.abs(freq - p) - (5 * np.sqrt(p * (1 - p) / S) + 1 / S))[tested]
    print(f"rates {rate.min():.3g} .. {rate.max():.3g}: largest |frequency - pmf| over its bound {excess.max():.3g}")
    assert (excess <= 0).all()


def logistic_model(X, y):
    b = numpyro.sample("b", dist.Normal(0.0, 1.0).expand([X.shape[1]]))
    numpyro.sample("obs", dist.Bernoulli(logits=jnp.matmul(X, b)), obs=y)


def poisson_model(X, y, off):
    b = numpyro.sample("b", dist.Normal(0.0, 1.0).expand([X.shape[1]]))
    numpyro.sample("obs", dist.Poisson(jnp.exp(jnp.matmul(X, b) + off)), obs=y)


@pytest.mark.parametrize("family", ["bernoulli", "poisson"])
def test_public_interface_end_to_end(device, family):
    S, N, D = 200, 300, 70
    X, y, off, W = data(family, N, D, S, offset=family == "poisson")
    model, args = (logistic_model, (X, y)) if family == "bernoulli" else (poisson_model, (X, y, off))
    samples = {"b": torch.from_numpy(W)}
    r64, r32 = reference(family, X, y, off, W, torch.float64), reference(family, X, y, off, W, torch.float32)
    assert isinstance(loglik._run(model, samples, args, {}, 1, "test"), loglik._GlmRun)
    ll = log_likelihood(model, samples, *args)["obs"]
    assert ll.dtype == torch.float32 and tuple(ll.shape) == (S, N)
    check_table(f"log_likelihood {family}", ll.cpu().numpy(), r64, r32)
    by4 = log_likelihood(model, {"b": samples["b"].reshape(4, 50, D)}, *args, batch_ndims=2)["obs"]
    assert torch.equal(by4, ll.reshape(4, 50, N))
    lppd = pointwise_predictive(model, samples, *args)["obs"]["lppd"].cpu().double()
    want = torch.logsumexp(ll.cpu().double(), 0) - math.log(S)
    assert torch.isfinite(lppd).all() and ((lppd - want).abs() <= 1e-5 * want.abs()).all()
    assert torch.isfinite(loo(model, samples, *args)["obs"]["elpd_loo"]).all()


def test_poisson_predictive_and_the_program_route(device):
    S, N, D = 200, 300, 70
    X, y, off, W = data("poisson", N, D, S, offset=True)
    samples = {"coefs": torch.from_numpy(W)}
    draws = Predictive(P.poisson_regression, samples)(5, X, None, off)["obs"]
    assert draws.dtype == torch.int32 and tuple(draws.shape) == (S, N) and draws.is_cuda
    rate = np.exp(W.astype(np.float64) @ X.T.astype(np.float64) + off)
    assert abs(draws.double().mean().item() - rate.mean()) <= 5 * math.sqrt(rate.mean() / (S * N))
    kept = Predictive(P.poisson_regression, samples)(5, X, y, off)["obs"]
    assert kept.dtype == torch.int32 and torch.equal(kept.cpu(), torch.from_numpy(y).int().expand(S, N))
    Xb, yb, _, Wb = data("bernoulli", 40, 5, 9)
    run = loglik._run(logit_model, {"b0": torch.zeros(9), "b": torch.from_numpy(Wb)}, (Xb, yb), {}, 1, "test")
    assert type(run) is loglik._Run


DEBUG_SCRIPT = r"""
import sys
sys.path.insert(0, "tests")
import torch
from numpyro_amd import native
import test_gpu_glm_predictive as T
assert native.LIB_PATH.endswith("libnumpyro_amd_debug.so"), native.LIB_PATH
for family, N, D, S in (("bernoulli", 33, 1, 70), ("poisson", 130, 70, 130)):
    X, y, off, W = T.data(family, N, D, S, offset=family == "poisson")
    kernel = T.GlmPredictive(X, torch.device("cuda:0"), family, y=y, offset=off)
    ll, draws = kernel.log_likelihood(W), kernel.draw(W, 3) if family == "poisson" else torch.zeros(1)
    torch.cuda.synchronize()
    assert torch.isfinite(ll).all() and int(draws.min()) >= 0
print("glm predictive debug build ok")
"""


def test_debug_build_runs_the_kernels_without_a_failed_check():
    env = dict(os.environ, NUMPYRO_AMD_DEBUG="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", DEBUG_SCRIPT], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=110)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "NMX_DCHECK failed" not in out and "glm predictive debug build ok" in out, out[-3000:]
