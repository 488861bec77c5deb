"""Horseshoe regression off the GPU: what the front end maps onto potentials.HorseshoeRegression, what it
leaves to the program path, and what the constructor refuses."""
import numpy as np
import pytest
import torch

import numpyro_amd as numpyro
from numpyro_amd import distributions as dist, jnp, potentials as P
from numpyro_amd.frontend import potential_from_model


def model(X, Y, offset=None, tau_scale=1.0, intercept=False):
    """examples/horseshoe_regression.py model_bernoulli_likelihood; with an offset the Poisson form."""
    D_X = X.shape[1]
    lambdas = numpyro.sample("lambdas", dist.HalfCauchy(jnp.ones(D_X)))
    tau = numpyro.sample("tau", dist.HalfCauchy(tau_scale * jnp.ones(1)))
    unscaled_betas = numpyro.sample("unscaled_betas", dist.Normal(0.0, jnp.ones(D_X)))
    scaled_betas = numpyro.deterministic("betas", tau * lambdas * unscaled_betas)
    mean_function = jnp.dot(X, scaled_betas)
    if intercept:
        mean_function = mean_function + numpyro.sample("b0", dist.Normal(0.0, 1.0))
    if offset is None:
        numpyro.sample("Y", dist.Bernoulli(logits=mean_function), obs=Y)
    else:
        numpyro.sample("Y", dist.Poisson(jnp.exp(mean_function + offset)), obs=Y)


def case(D=5, N=12):
    rs = np.random.RandomState(D)
    return rs.randn(N, D).astype(np.float32), (rs.rand(N) < 0.5).astype(np.int64), rs.randn(N).astype(np.float32)


def test_the_reference_model_maps_onto_the_fused_potential():
    X, Y, off = case()
    for args, likelihood in (((X, Y), "bernoulli"), ((X, 3 * Y, off), "poisson")):
        pot = potential_from_model(model, args)
        assert type(pot) is P.HorseshoeRegression and pot.likelihood == likelihood and pot.dim == 11
        assert (pot.o_in is not None) == (likelihood == "poisson")
        assert pot.sites == [("lambdas", (5,), P.POSITIVE), ("tau", (1,), P.POSITIVE), ("unscaled_betas", (5,), P.REAL)]
        draw = {"lambdas": torch.rand(4, 5), "tau": torch.rand(4, 1), "unscaled_betas": torch.randn(4, 5)}
        det = pot.deterministic(draw)
        assert list(det) == ["betas"]
        torch.testing.assert_close(det["betas"], draw["tau"] * draw["lambdas"] * draw["unscaled_betas"])

    def renamed(X, Y):  # other names, another order and association, a scalar tau, no deterministic site
        z = numpyro.sample("z", dist.Normal(0.0, 1.0).expand([X.shape[1]]))
        t = numpyro.sample("t", dist.HalfCauchy(1.0))
        lam = numpyro.sample("lam", dist.HalfCauchy(jnp.ones(X.shape[1])))
        numpyro.sample("obs", dist.Bernoulli(logits=jnp.matmul(X, z * (lam * t))), obs=Y)

    pot = potential_from_model(renamed, (X, Y))
    assert pot.sites == [("lam", (5,), P.POSITIVE), ("t", (), P.POSITIVE), ("z", (5,), P.REAL)]
    assert pot.deterministic({"lam": torch.rand(4, 5), "t": torch.rand(4), "z": torch.randn(4, 5)}) == {}


@pytest.mark.parametrize("args,kwargs", [
    (case()[:2], {"tau_scale": 2.0}), (case()[:2], {"intercept": True}), (case(D=1025, N=2)[:2], {}),
    ((case()[0], case()[1] + 0.5, case()[2]), {})], ids=["HalfCauchy(2)", "intercept", "D=1025", "non-integer count"])
def test_other_structures_are_not_matched(args, kwargs):
    with pytest.raises(NotImplementedError, match="no fused kernel"):
        potential_from_model(model, args, kwargs)


@pytest.mark.parametrize("D,likelihood,offset", [(0, "bernoulli", False), (1025, "bernoulli", False),
                                                 (5, "bernoulli", True), (5, "probit", False)])
def test_the_constructor_refuses(D, likelihood, offset):
    X, Y, off = case(D, 4)
    with pytest.raises(ValueError):
        P.HorseshoeRegression(X, Y, likelihood, off if offset else None)
    assert type(P.horseshoe_regression.potential(*case()[:2])) is P.HorseshoeRegression
