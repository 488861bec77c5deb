"""Softmax regression off the GPU: the front end's matcher, the size functions and the refusals that
the C ABI makes before any launch (csrc/potential_softmax.hip)."""
import numpy as np
import pytest

import numpyro_amd as numpyro
from numpyro_amd import distributions as dist
from numpyro_amd import jnp, native
from numpyro_amd import potentials as P
from numpyro_amd.frontend import _match_softmax, potential_from_model, trace_model

N, D, K = 12, 3, 4
X, Y = np.random.RandomState(0).randn(N, D).astype(np.float32), np.arange(N) % K


def _model(prior=None, event=False, intercept=False, likelihood="categorical"):
    def model(X, y):
        d = prior or dist.Normal(0.0, 1.0).expand([D, K])
        W = numpyro.sample("weights", d.to_event(2) if event else d)
        logits = jnp.matmul(X, W)
        if intercept:
            logits = logits + numpyro.sample("b", dist.Normal(0.0, 1.0).expand([K]))
        if likelihood == "bernoulli":
            numpyro.sample("obs", dist.Bernoulli(logits=logits), obs=np.zeros((N, K)))
        else:
            numpyro.sample("obs", dist.Categorical(logits=logits), obs=y)
    return model


@pytest.mark.parametrize("event", [False, True])
def test_the_model_traces_to_the_fused_potential(event):
    pot = potential_from_model(_model(event=event), (X, Y))
    assert type(pot) is P.SoftmaxRegression
    assert pot.sites == [("weights", (D, K), P.REAL)] and pot.dim == D * K and (pot.N, pot.K) == (N, K)
    built = P.softmax_regression.potential(X, Y)  # num_classes = max(labels) + 1
    assert type(built) is P.SoftmaxRegression and built.K == K and built.sites[0][0] == "coefs"


@pytest.mark.parametrize("kw,y", [
    (dict(prior=dist.Normal(0.0, 2.0).expand([D, K])), Y), (dict(intercept=True), Y), (dict(likelihood="bernoulli"), Y),
    (dict(), np.where(Y == 0, K, Y)), (dict(), Y.astype(np.float32)),  # a label == K; labels that are not integers
], ids=["scale2", "intercept", "bernoulli", "label_K", "float_labels"])
def test_other_models_do_not_match(kw, y):
    assert _match_softmax(trace_model(_model(**kw), (X, y))) is None


def test_sizes_are_positive_and_monotone():
    pb, wb = native.lib().nmx_softmax_packed_bytes, native.lib().nmx_softmax_workspace_bytes
    assert 0 < pb(1, 1, 2) <= pb(33, 1, 2) <= pb(33, 17, 2) <= pb(33, 64, 32) < pb(100000, 64, 32)
    assert (0 < wb(1, 1, 2, 1) <= wb(1, 1, 2, 65) <= wb(1, 2, 2, 65) <= wb(1, 2, 3, 65) <= wb(10 ** 6, 2, 3, 65)
            < wb(10 ** 6, 64, 32, 4096))


@pytest.mark.parametrize("d,k,number", [(65, 3, "dim = 65"), (3, 33, "num_classes = 33"), (0, 3, "dim = 0"),
                                        (3, 1, "num_classes = 1")])
def test_shapes_outside_the_kernel_are_refused_by_name(d, k, number):
    L = native.lib()
    ev = native.EvalBatch(num_chains=1, ldc=64)
    for status in (L.nmx_softmax_pack(0, 0, 10, d, k, 0, 0), L.nmx_softmax_pe_grad(0, 10, d, k, ev, 0, 0)):
        assert status != 0 and number in L.nmx_last_error().decode()
    assert L.nmx_softmax_packed_bytes(10, d, k) == 0
    with pytest.raises(ValueError, match=rf"\(got {d if not 1 <= d <= 64 else k}\)"):
        P.SoftmaxRegression(np.zeros((10, d), np.float32), np.zeros(10, np.int64), k)
