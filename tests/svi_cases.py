"""Models and closed forms of the SVI tests (tests/test_svi.py on the host, tests/test_gpu_svi.py
on the device).

* ``zoo(name)``: the tests/program_zoo.py cases, plus ``eight_schools`` -- the fused eight-schools
  model (numpyro_amd.potentials.eight_schools) with its potential written in torch like the zoo's.
* ``pe_grad_fn(case, dtype)``: ``Z [P, D] -> (U [P], dU/dz [P, D])`` in ``dtype`` by torch.func on the
  CPU: float64 is the oracle's potential, float32 the second float32 implementation's.
* ``Conjugate``: J = 5 independent normal means with known noise, whose posterior is exactly the
  mean-field normal N(m_j, s_j^2): prec_j = 1 / s0_j^2 + n_j / sigma_j^2,
  m_j = (m0_j / s0_j^2 + sum_k y_jk / sigma_j^2) / prec_j, s_j = prec_j^-1/2.
"""
import functools

import numpy as np
import torch

import numpyro_amd as numpyro
import program_zoo as Zoo
from numpyro_amd import datasets
from numpyro_amd import distributions as dist
from numpyro_amd import potentials as P


def _eight_schools_u(s, d):
    mu, u, theta = s["mu"], s["tau"], s["theta"]
    tau = torch.exp(u)
    lp = Zoo._normal(mu, 0.0, 5.0) + Zoo._half_cauchy(tau, 5.0) + u
    lp = lp + Zoo._normal(theta, mu, tau).sum() + Zoo._normal(d["y"], theta, d["sigma"]).sum()
    return -lp


def eight_schools():
    sigma = np.asarray(datasets.EIGHT_SCHOOLS_SIGMA, np.float64)
    y = np.asarray(datasets.EIGHT_SCHOOLS_Y, np.float64)
    return Zoo.Case("eight_schools", P.eight_schools, (8, sigma, y),
                    [("mu", (), False), ("tau", (), True), ("theta", (8,), False)], _eight_schools_u,
                    {"y": y, "sigma": sigma})


@functools.lru_cache(maxsize=None)
def zoo(name):
    return eight_schools() if name == "eight_schools" else Zoo.CASES[name]()


def pe_grad_fn(case, dtype=np.float64):
    tdt = {np.float64: torch.float64, np.float32: torch.float32}[dtype]
    fn = case.torch_fn(tdt)

    def unflatten(z):
        out, o = {}, 0
        for name, shape, _ in case.sites:
            n = int(np.prod(shape))
            out[name] = z[o:o + n].reshape(shape)
            o += n
        return out

    batched = torch.func.vmap(torch.func.grad_and_value(lambda z: fn(unflatten(z))))

    def pe_grad(Z):
        g, u = batched(torch.as_tensor(np.ascontiguousarray(Z), dtype=tdt))
        return u.numpy(), g.numpy()

    return pe_grad


def mixed_model(y, c):
    """A real, a positive and a simplex site: D = 1 + 1 + 2 coordinates, sorted (rate, w, x)."""
    w = numpyro.sample("w", dist.Dirichlet(np.ones(3)))
    rate = numpyro.sample("rate", dist.HalfNormal(2.0))
    x = numpyro.sample("x", dist.Normal(0.0, 1.0))
    numpyro.sample("c", dist.Categorical(probs=w), obs=c)
    numpyro.sample("y", dist.Normal(x, rate), obs=y)


MIXED_ARGS = (np.array([0.3, -0.2, 1.1, 0.4]), np.array([0, 1, 2, 2, 1, 2]))
MIXED_SHAPES = {"rate": (), "w": (2,), "x": ()}  # unconstrained
MIXED_CONSTRAINED = {"rate": (), "w": (3,), "x": ()}


class Conjugate:
    J = 5

    def __init__(self, seed=3):
        rs = np.random.RandomState(seed)
        J = self.J
        self.m0 = np.array([-1.0, 0.0, 0.5, 2.0, -3.0])
        self.s0 = np.array([1.0, 2.0, 0.5, 3.0, 1.5])
        self.sigma_j = np.array([0.5, 1.0, 2.0, 0.7, 1.3])
        self.n = np.array([3, 1, 6, 4, 2])
        self.group = np.repeat(np.arange(J), self.n).astype(np.int64)
        truth = self.m0 + self.s0 * rs.randn(J)
        self.sigma = self.sigma_j[self.group]
        self.y = truth[self.group] + self.sigma * rs.randn(self.group.size)
        sum_y = np.bincount(self.group, weights=self.y / self.sigma ** 2, minlength=J)
        self.prec = 1.0 / self.s0 ** 2 + self.n / self.sigma_j ** 2
        self.m = (self.m0 / self.s0 ** 2 + sum_y) / self.prec
        self.s = self.prec ** -0.5
        self.args = (self.y, self.group, self.sigma, self.m0, self.s0)
        self.dim = J

    @staticmethod
    def model(y, group, sigma, m0, s0):
        mu = numpyro.sample("mu", dist.Normal(m0, s0))
        numpyro.sample("y", dist.Normal(mu[group], sigma), obs=y)

    def pe_grad(self, Z):
        """U up to its constant (which no parameter of the guide sees) and dU/dz, exactly."""
        d = np.asarray(Z) - self.m
        return 0.5 * (self.prec * d * d).sum(-1), self.prec * d

    # the settings of the conjugate tests, chosen on the host (tests/test_svi.py
    # test_conjugate_posterior_is_recovered records the margin they leave)
    SEED, NUM_STEPS, STEP_SIZE, NUM_PARTICLES = 7, 400, 0.05, 1024
    LOC_BOUND, LOG_SCALE_BOUND = 0.1, 0.1  # |loc - m| <= 0.1 s, |log(scale / s)| <= 0.1
