"""Models for the program potential's tests (numpyro_amd/program.py), each written twice: with
numpyro_amd's primitives, and independently as a hand-written torch potential of the
unconstrained site values (no use of the compiler; gradients by autograd).  ``CASES[name]()``
builds a Case; ``Case.pe_grad64(Z)`` is the float64 reference over rows of Z (sites in sorted
order, as every Potential.sites), ``Case.torch_fn(dtype, device)`` the potential_fn of one chain's
site dict, the generic path NUTS(potential_fn=...) offers without the compiler."""
import math

import numpy as np
import torch

import numpyro_amd as numpyro
from numpyro_amd import datasets
from numpyro_amd import distributions as dist
from numpyro_amd import jnp

_LOG_PI = math.log(math.pi)
_HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)


# ---- log densities, written out (numpyro/distributions/continuous.py, discrete.py)
def _normal(x, loc, scale):
    return -0.5 * ((x - loc) / scale) ** 2 - torch.log(torch.as_tensor(scale, dtype=x.dtype)) - _HALF_LOG_2PI


def _half_cauchy(x, scale):
    return math.log(2.0) - _LOG_PI - math.log(scale) - torch.log1p((x / scale) ** 2)


def _cauchy(x, loc, scale):
    return -_LOG_PI - math.log(scale) - torch.log1p(((x - loc) / scale) ** 2)


def _half_normal(x, scale):
    return -0.5 * (x / scale) ** 2 - math.log(scale) + 0.5 * math.log(2.0 / math.pi)


def _log_normal(x, loc, scale):
    return _normal(torch.log(x), loc, scale) - torch.log(x)


def _student_t(x, df, loc, scale):
    df = torch.as_tensor(df, dtype=x.dtype)
    y = (x - loc) / scale
    return (torch.lgamma(0.5 * (df + 1.0)) - torch.lgamma(0.5 * df) - 0.5 * torch.log(df) - 0.5 * _LOG_PI
            - torch.log(torch.as_tensor(scale, dtype=x.dtype)) - 0.5 * (df + 1.0) * torch.log1p(y * y / df))


def _gamma(x, conc, rate):
    return conc * math.log(rate) - math.lgamma(conc) + (conc - 1.0) * torch.log(x) - rate * x


def _exponential(x, rate):
    return math.log(rate) - rate * x


class Case:
    def __init__(self, name, model, args, sites, potential, data):
        self.name, self.model, self.args = name, model, args
        self.sites = sites  # [(name, shape, positive)] in sorted order
        self.potential = potential  # (site dict of one chain, data dict of tensors) -> U
        self.data = data  # name -> NumPy array
        self.dim = int(sum(int(np.prod(s)) for _, s, _ in sites))

    def torch_fn(self, dtype=torch.float64, device="cpu"):
        data = {k: torch.as_tensor(v, device=device).to(dtype if np.asarray(v).dtype.kind == "f" else torch.long)
                for k, v in self.data.items()}
        return lambda s: self.potential(s, data)

    def unflatten(self, z):
        out, o = {}, 0
        for name, shape, _ in self.sites:
            n = int(np.prod(shape))
            out[name] = z[o:o + n].reshape(shape)
            o += n
        return out

    def pe_grad64(self, Z):
        """(U [C], dU/dz [C, D]) in float64 by autograd, chain by chain."""
        fn = self.torch_fn(torch.float64)
        Z = np.atleast_2d(np.asarray(Z, np.float64))
        U, G = np.zeros(Z.shape[0]), np.zeros(Z.shape)
        for c, row in enumerate(Z):
            z = torch.tensor(row, dtype=torch.float64, requires_grad=True)
            u = fn(self.unflatten(z))
            (g,) = torch.autograd.grad(u, z)
            U[c], G[c] = float(u.detach()), g.numpy()
        return U, G

    def pe_grad_one(self, z, dtype=torch.float64):
        """One chain, for the NUTS oracle."""
        fn = self.torch_fn(dtype)
        zt = torch.tensor(np.asarray(z), dtype=dtype, requires_grad=True)
        u = fn(self.unflatten(zt))
        (g,) = torch.autograd.grad(u, zt)
        return u.detach().numpy(), g.numpy()

    def init_params(self, num_chains, dtype=torch.float32, device="cpu", seed=0):
        rs = np.random.RandomState(seed)
        return {name: torch.as_tensor(rs.uniform(-1, 1, (num_chains,) + tuple(shape)), dtype=dtype, device=device)
                for name, shape, _ in self.sites}


# ---- robust8: eight schools with mu ~ N(0, 10) and a StudentT(4) likelihood
def robust8_model(J, sigma, y=None):
    mu = numpyro.sample("mu", dist.Normal(0, 10))
    tau = numpyro.sample("tau", dist.HalfCauchy(5))
    with numpyro.plate("J", J):
        theta = numpyro.sample("theta", dist.Normal(mu, tau))
        numpyro.sample("obs", dist.StudentT(4.0, theta, sigma), obs=y)


def _robust8_u(s, d):
    mu, u, theta = s["mu"], s["tau"], s["theta"]
    tau = torch.exp(u)
    lp = _normal(mu, 0.0, 10.0) + _half_cauchy(tau, 5.0) + u
    lp = lp + _normal(theta, mu, tau).sum() + _student_t(d["y"], 4.0, theta, d["sigma"]).sum()
    return -lp


def robust8():
    sigma = np.asarray(datasets.EIGHT_SCHOOLS_SIGMA, np.float64)
    y = np.asarray(datasets.EIGHT_SCHOOLS_Y, np.float64)
    return Case("robust8", robust8_model, (8, sigma, y), [("mu", (), False), ("tau", (), True), ("theta", (8,), False)],
                _robust8_u, {"y": y, "sigma": sigma})


# ---- poisson: varying intercepts, y ~ Poisson(exp(a[group] + X @ b))
def poisson_model(X, group, y, G):
    mu_a = numpyro.sample("mu_a", dist.Normal(0.0, 2.0))
    sigma_a = numpyro.sample("sigma_a", dist.HalfNormal(1.0))
    with numpyro.plate("groups", G):
        a = numpyro.sample("a", dist.Normal(mu_a, sigma_a))
    b = numpyro.sample("b", dist.Normal(np.zeros(X.shape[1]), np.ones(X.shape[1])))
    rate = jnp.exp(a[group] + jnp.matmul(X, b))
    numpyro.sample("y", dist.Poisson(rate), obs=y)


def _poisson_u(s, d):
    a, b, mu_a, u = s["a"], s["b"], s["mu_a"], s["sigma_a"]
    sig = torch.exp(u)
    eta = a[d["group"]] + d["X"] @ b
    lp = _normal(mu_a, 0.0, 2.0) + _half_normal(sig, 1.0) + u + _normal(a, mu_a, sig).sum() + _normal(b, 0.0, 1.0).sum()
    lp = lp + (d["y"] * eta - torch.exp(eta) - torch.lgamma(d["y"] + 1.0)).sum()
    return -lp


def poisson(N=40, G=5, K=3, seed=5):
    """Group id G // 2 is absent from `group` (its intercept gets a zero likelihood adjoint);
    the others repeat."""
    rs = np.random.RandomState(seed)
    X = 0.5 * rs.randn(N, K)
    group = rs.randint(0, G - 1, N)
    group = np.where(group >= G // 2, group + 1, group).astype(np.int64)
    rate = np.exp(0.5 + 0.4 * rs.randn(G)[group] + X @ (0.3 * rs.randn(K)))
    y = rs.poisson(rate).astype(np.float64)
    assert G // 2 not in group
    return Case("poisson", poisson_model, (X, group, y, G),
                [("a", (G,), False), ("b", (K,), False), ("mu_a", (), False), ("sigma_a", (), True)],
                _poisson_u, {"X": X, "group": group, "y": y})


# ---- treg: robust regression with latent degrees of freedom (lgamma / digamma)
def treg_model(X, y):
    b = numpyro.sample("b", dist.Normal(np.zeros(X.shape[1]), np.ones(X.shape[1])))
    nu = numpyro.sample("nu", dist.Gamma(2.0, 0.1))
    sigma = numpyro.sample("sigma", dist.Exponential(1.0))
    numpyro.sample("y", dist.StudentT(nu, jnp.matmul(X, b), sigma), obs=y)


def _treg_u(s, d):
    b, un, us = s["b"], s["nu"], s["sigma"]
    nu, sigma = torch.exp(un), torch.exp(us)
    lp = _normal(b, 0.0, 1.0).sum() + _gamma(nu, 2.0, 0.1) + un + _exponential(sigma, 1.0) + us
    lp = lp + _student_t(d["y"], nu, d["X"] @ b, sigma).sum()
    return -lp


def treg(N=30, K=3, seed=11):
    rs = np.random.RandomState(seed)
    X = rs.randn(N, K)
    y = X @ np.array([0.5, -1.0, 0.25])[:K] + 0.7 * rs.standard_t(5, N)
    return Case("treg", treg_model, (X, y), [("b", (K,), False), ("nu", (), True), ("sigma", (), True)],
                _treg_u, {"X": X, "y": y})


# ---- logit: logistic regression with an intercept
def logit_model(X, y):
    b0 = numpyro.sample("b0", dist.Normal(0.0, 5.0))
    b = numpyro.sample("b", dist.Normal(np.zeros(X.shape[1]), 2.0 * np.ones(X.shape[1])))
    numpyro.sample("y", dist.Bernoulli(logits=b0 + jnp.matmul(X, b)), obs=y)


def _logit_u(s, d):
    b, b0 = s["b"], s["b0"]
    eta = b0 + d["X"] @ b
    lp = _normal(b0, 0.0, 5.0) + _normal(b, 0.0, 2.0).sum() + (d["y"] * eta - torch.nn.functional.softplus(eta)).sum()
    return -lp


def logit(N=25, K=4, seed=3):
    rs = np.random.RandomState(seed)
    X = rs.randn(N, K)
    y = (rs.rand(N) < 0.5).astype(np.float64)
    return Case("logit", logit_model, (X, y), [("b", (K,), False), ("b0", (), False)], _logit_u, {"X": X, "y": y})


# ---- edge: the corner shapes
def edge_model(M1, idx1, y1, y2):
    with numpyro.plate("T", 3):
        tau = numpyro.sample("tau", dist.HalfCauchy(1.0))  # a vector POSITIVE site
    w = numpyro.sample("w", dist.Cauchy(0.0, 2.0))  # used by two sites below
    numpyro.sample("free", dist.LogNormal(0.5, 0.7))  # no likelihood uses it
    with numpyro.plate("one", 1):
        v = numpyro.sample("v", dist.Normal(w, 1.0))
    s = jnp.sum(tau ** 2.0)  # sum and pow
    m = jnp.matmul(M1, v)  # N = 1, K = 1
    numpyro.sample("y1", dist.Normal(m + tau[idx1], jnp.sqrt(s)), obs=y1)  # a length-1 gather
    numpyro.sample("y2", dist.Normal(w * tau, 1.0), obs=y2)


def _edge_u(s, d):
    uf, ut, v, w = s["free"], s["tau"], s["v"], s["w"]
    free, tau = torch.exp(uf), torch.exp(ut)
    lp = _half_cauchy(tau, 1.0).sum() + ut.sum() + _cauchy(w, 0.0, 2.0) + _log_normal(free, 0.5, 0.7) + uf
    lp = lp + _normal(v, w, 1.0).sum()
    sd = torch.sqrt((tau ** 2).sum())
    lp = lp + _normal(d["y1"], d["M1"] @ v + tau[d["idx1"]], sd).sum() + _normal(d["y2"], w * tau, 1.0).sum()
    return -lp


def edge():
    M1, idx1 = np.array([[1.5]]), np.array([2])
    y1, y2 = np.array([0.3]), np.array([0.5, -1.0, 2.0])
    return Case("edge", edge_model, (M1, idx1, y1, y2),
                [("free", (), True), ("tau", (3,), True), ("v", (1,), False), ("w", (), False)],
                _edge_u, {"M1": M1, "idx1": idx1, "y1": y1, "y2": y2})


CASES = {"robust8": robust8, "poisson": poisson, "treg": treg, "logit": logit, "edge": edge}


def poisson_large():
    return poisson(N=2000, G=50, K=8, seed=6)
