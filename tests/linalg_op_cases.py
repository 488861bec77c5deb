"""Cases for the dense ops of the program kernel (cholesky, trisolve; csrc/nmx_program.h) and the
MultivariateNormal models built on them: tests/test_linalg_ops.py runs them on the host
interpreter, tests/test_gpu_linalg_ops.py on the device.

A one-op case is a ``Program`` written row by row ([opcode, dst, a, b, n, sa, sb, aux], a constant
as ~offset), wrapped as ``ProgramPotential(prog, [("z", (D,), 0)])``, with 16 rows of z and the
same function written as a torch expression ``fn(Z, consts)`` of any float dtype: float64 with
autograd is the reference (``Program.run_host`` never is), float32 on the CPU the restatement that
calibrates the device's tolerance.  Constants are float32 numbers and z is rounded to float32, so
host and device see the same inputs.  Matrices are A = B B^T / n + I with B standard normal from a
fixed seed: condition numbers stay below about 10.

``cholesky``   z = A (n x n, flat); U = sum(w * chol(A)), w = linspace(0.5, 1.5, n * n): every
               element of Lbar differs.
``tri.*``      U = sum(w * L^-1 b), w = linspace(0.5, 1.5, n), with L and b slots (z = L then b), L a
               constant, or b a constant.
``mvn``        z = A; L = chol(A), x = L^-1 y (y constant), U = 0.5 sum(x^2) + sum(log diag L): the
               chain the compiler emits for a MultivariateNormal with a latent covariance.
A model case (``gp``, ``latent_f``) is a model on numpyro_amd's primitives with its potential
restated in torch over the unconstrained coordinates."""
import functools
import math
import zlib

import numpy as np
import torch

import numpyro_amd as numpyro
from numpyro_amd import distributions as dist
from numpyro_amd import jnp
from numpyro_amd.native import OPCODE
from numpyro_amd.program import Program, ProgramPotential, compile_model

ROWS = 16
SIZES = (1, 2, 3, 30, 63, 64, 65, 128)
KINDS = ("cholesky", "tri.Ls_bs", "tri.Lc_bs", "tri.Ls_bc", "mvn")
_HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def spd(rs, n, rows=ROWS):
    B = rs.randn(rows, n, n)
    return _f32(B @ B.transpose(0, 2, 1) / n + np.eye(n))


def _tri_solve(L, b):
    """L^-1 b over a batch, lower triangle of L."""
    return torch.linalg.solve_triangular(torch.tril(L), b.unsqueeze(-1), upper=False).squeeze(-1)


class OpCase:
    """``fn(Z, consts) -> U [C]`` in the dtype of Z; consts: the program's pool as a tensor."""

    def __init__(self, name, program, fn, Z):
        self.name, self.program, self.fn, self.Z = name, program, fn, Z
        self.dim = program.dim
        self.pot = ProgramPotential(program, [("z", (self.dim,), 0)])

    def evaluate(self, Z, dtype):
        """(U [C], dU/dz [C, D]) from the torch expression in ``dtype``, gradient by autograd."""
        Zt = torch.tensor(np.asarray(Z, np.float64), dtype=dtype, requires_grad=True)
        U = self.fn(Zt, torch.tensor(self.program.consts64, dtype=dtype))
        (G,) = torch.autograd.grad(U.sum(), Zt)
        return U.detach().numpy().astype(np.float64), G.numpy().astype(np.float64)

    @functools.cached_property
    def reference(self):
        return self.evaluate(self.Z, torch.float64)

    @functools.cached_property
    def float32(self):
        return self.evaluate(self.Z, torch.float32)


def _cholesky_case(n):
    rs = np.random.RandomState(zlib.crc32(f"cholesky.{n}".encode()))
    D = n * n
    w = _f32(np.linspace(0.5, 1.5, D))
    rows = [[OPCODE["cholesky"], D, 0, 0, D, 1, 0, n],
            [OPCODE["mul"], 2 * D, D, ~0, D, 1, 1, 0],
            [OPCODE["reduce_sum"], 3 * D, 2 * D, 0, D, 1, 0, 0]]

    def fn(Z, c):
        L = torch.linalg.cholesky(Z.reshape(-1, n, n))
        return (L.reshape(-1, D) * c[:D]).sum(1)

    return OpCase(f"cholesky.n{n}", Program(rows, w, [], 3 * D + 1, D), fn, spd(rs, n).reshape(ROWS, D))


def _trisolve_case(n, layout):
    rs = np.random.RandomState(zlib.crc32(f"tri.{layout}.{n}".encode()))
    N2 = n * n
    const_L, const_b = layout == "Lc_bs", layout == "Ls_bc"
    L = _f32(np.linalg.cholesky(spd(rs, n, 1 if const_L else ROWS))).reshape(-1, N2)
    b = _f32(rs.randn(1 if const_b else ROWS, n))
    w = _f32(np.linspace(0.5, 1.5, n))
    consts, zcols = [w], []  # w at pool offset 0
    if const_L:
        ref_L, ref_b = ~n, 0
        consts.append(L[0])
        zcols.append(b)
    elif const_b:
        ref_L, ref_b = 0, ~n
        consts.append(b[0])
        zcols.append(L)
    else:
        ref_L, ref_b = 0, N2
        zcols += [L, b]
    Z = np.concatenate(zcols, 1)
    D = Z.shape[1]
    rows = [[OPCODE["trisolve"], D, ref_L, ref_b, n, 1, 1, 0],
            [OPCODE["mul"], D + n, D, ~0, n, 1, 1, 0],
            [OPCODE["reduce_sum"], D + 2 * n, D + n, 0, n, 1, 0, 0]]

    def fn(Z, c):
        Lt = (c[n:n + N2].expand(Z.shape[0], N2) if const_L else Z[:, :N2]).reshape(-1, n, n)
        bt = c[n:2 * n].expand(Z.shape[0], n) if const_b else Z[:, D - n:]
        return (_tri_solve(Lt, bt) * c[:n]).sum(1)

    return OpCase(f"tri.{layout}.n{n}", Program(rows, np.concatenate(consts), [], D + 2 * n + 1, D), fn, Z)


def _mvn_case(n):
    rs = np.random.RandomState(zlib.crc32(f"mvn.{n}".encode()))
    D = n * n
    y = _f32(rs.randn(n))
    diag = np.arange(n) * (n + 1)
    # the index pool of a gather: the indices, then the transposed (CSR) form (_Builder.gather)
    start = np.concatenate([[0], np.cumsum(np.bincount(diag, minlength=D))])
    index = diag.tolist() + start.tolist() + np.argsort(diag, kind="stable").tolist()
    s = 2 * D  # first slot after L
    rows = [[OPCODE["cholesky"], D, 0, 0, D, 1, 0, n],
            [OPCODE["trisolve"], s, D, ~0, n, 1, 1, 0],
            [OPCODE["square"], s + n, s, 0, n, 1, 0, 0],
            [OPCODE["reduce_sum"], s + 2 * n, s + n, 0, n, 1, 0, 0],
            [OPCODE["gather"], s + 2 * n + 1, D, D, n, 1, 0, 0],
            [OPCODE["log"], s + 3 * n + 1, s + 2 * n + 1, 0, n, 1, 0, 0],
            [OPCODE["reduce_sum"], s + 4 * n + 1, s + 3 * n + 1, 0, n, 1, 0, 0],
            [OPCODE["mul"], s + 4 * n + 2, s + 2 * n, ~n, 1, 1, 1, 0],
            [OPCODE["add"], s + 4 * n + 3, s + 4 * n + 2, s + 4 * n + 1, 1, 1, 1, 0]]

    def fn(Z, c):
        L = torch.linalg.cholesky(Z.reshape(-1, n, n))
        x = _tri_solve(L, c[:n].expand(Z.shape[0], n))
        return 0.5 * (x * x).sum(1) + torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(1)

    prog = Program(rows, np.concatenate([y, [0.5]]), index, s + 4 * n + 4, D)
    return OpCase(f"mvn.n{n}", prog, fn, spd(rs, n).reshape(ROWS, D))


@functools.lru_cache(maxsize=None)
def op_case(kind, n):
    if kind == "cholesky":
        return _cholesky_case(n)
    if kind == "mvn":
        return _mvn_case(n)
    return _trisolve_case(n, kind.split(".")[1])


# ------------------------------------------------------------------------------------------ models
def _mvn_logp(y, loc, K):
    """MultivariateNormal(loc, K).log_prob(y), written out."""
    L = torch.linalg.cholesky(K)
    x = torch.linalg.solve_triangular(L, (y - loc).unsqueeze(-1), upper=False).squeeze(-1)
    n = y.shape[-1]
    return -0.5 * (x * x).sum(-1) - torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1) - n * _HALF_LOG_2PI


def _normal_logp(x, loc, scale):
    return -0.5 * ((x - loc) / scale) ** 2 - torch.log(scale) - _HALF_LOG_2PI


class ModelCase:
    """A model and its potential restated in torch: ``potential(z [D], dtype) -> U`` over the
    unconstrained coordinates (sites in sorted order); ``sites``: [(name, shape, positive)]."""

    def __init__(self, name, model, args, sites, potential, seed):
        self.name, self.model, self.args, self.sites, self.potential = name, model, args, sites, potential
        self.dim = int(sum(int(np.prod(s)) for _, s, _ in sites))
        self.Z = _f32(np.random.RandomState(seed).uniform(-1.0, 1.0, (ROWS, self.dim)))

    @functools.cached_property
    def pot(self):
        return compile_model(self.model, self.args)

    def unflatten(self, z):
        out, o = {}, 0
        for name, shape, _ in self.sites:
            n = int(np.prod(shape))
            out[name] = z[o:o + n].reshape(shape)
            o += n
        return out

    def evaluate(self, Z, dtype):
        Z = np.atleast_2d(np.asarray(Z, np.float64))
        U, G = np.zeros(Z.shape[0]), np.zeros(Z.shape)
        for c, row in enumerate(Z):
            z = torch.tensor(row, dtype=dtype, requires_grad=True)
            u = self.potential(z, dtype)
            (g,) = torch.autograd.grad(u, z)
            U[c], G[c] = float(u.detach()), g.numpy()
        return U, G

    def pe_grad_one(self, z):
        U, G = self.evaluate(z, torch.float64)
        return U[0], G[0]

    @functools.cached_property
    def reference(self):
        return self.evaluate(self.Z, torch.float64)

    @functools.cached_property
    def float32(self):
        return self.evaluate(self.Z, torch.float32)


# squared exponential kernel with diagonal noise term, and the model over it: the smallest Gaussian
# process, three LogNormal hyperparameters and Y ~ MultivariateNormal(0, k)
def kernel(X, Z, var, length, noise, jitter=1.0e-6):
    scaled = (X[:, None] - Z) / length  # (n, 1) against (n,): rank 2
    k = var * jnp.exp(-0.5 * jnp.power(scaled, 2.0))
    k += (noise + jitter) * jnp.eye(X.shape[0])
    return k


def gp_model(X, Y):
    hyper = {name: numpyro.sample(f"kernel_{name}", dist.LogNormal(0.0, 10.0)) for name in ("var", "noise", "length")}
    k = kernel(X, X, hyper["var"], hyper["length"], hyper["noise"])
    numpyro.sample("Y", dist.MultivariateNormal(loc=jnp.zeros(X.shape[0]), covariance_matrix=k), obs=Y)


def _gp_data(N=30):
    rs = np.random.RandomState(0)
    X = np.linspace(-1.0, 1.0, N)
    Y = X + 0.2 * X ** 3 + 0.5 * (0.5 + X) ** 2 * np.sin(4.0 * X) + 0.15 * rs.randn(N)
    Y = (Y - Y.mean()) / Y.std()
    return _f32(X), _f32(Y)


def _sq_exp(X, var, length, noise, dtype):
    d = (X[:, None] - X[None, :]) / length
    return var * torch.exp(-0.5 * d * d) + (noise + 1.0e-6) * torch.eye(X.shape[0], dtype=dtype)


@functools.lru_cache(maxsize=None)
def gp_case():
    X, Y = _gp_data()

    def potential(z, dtype):  # z = log of (kernel_length, kernel_noise, kernel_var)
        Xt, Yt = torch.tensor(X, dtype=dtype), torch.tensor(Y, dtype=dtype)
        length, noise, var = torch.exp(z[0]), torch.exp(z[1]), torch.exp(z[2])
        # LogNormal(0, 10) at exp(u) with the Jacobian u: Normal(0, 10) at u
        prior = _normal_logp(z, torch.zeros((), dtype=dtype), torch.tensor(10.0, dtype=dtype)).sum()
        K = _sq_exp(Xt, var, length, noise, dtype)
        return -(prior + _mvn_logp(Yt, torch.zeros_like(Yt), K))

    sites = [("kernel_length", (), True), ("kernel_noise", (), True), ("kernel_var", (), True)]
    return ModelCase("gp", gp_model, (X, Y), sites, potential, seed=11)


def latent_f_model(X, y):
    """A latent GP vector: f ~ MVN(0, K(theta)), y ~ Normal(f, s)."""
    length = numpyro.sample("length", dist.LogNormal(0.0, 1.0))
    s = numpyro.sample("s", dist.HalfNormal(1.0))
    k = kernel(X, X, 1.0, length, 0.1)
    f = numpyro.sample("f", dist.MultivariateNormal(0.0, covariance_matrix=k))
    numpyro.sample("y", dist.Normal(f, s), obs=y)


@functools.lru_cache(maxsize=None)
def latent_f_case(N=8):
    X = _f32(np.linspace(-1.0, 1.0, N))
    y = _f32(np.sin(3.0 * X) + 0.1 * np.random.RandomState(3).randn(N))

    def potential(z, dtype):  # z = (f [N], log length, log s)
        Xt, yt = torch.tensor(X, dtype=dtype), torch.tensor(y, dtype=dtype)
        f, ul, us = z[:N], z[N], z[N + 1]
        one = torch.ones((), dtype=dtype)
        lp = _normal_logp(ul, 0.0 * one, one)  # LogNormal(0, 1) with its Jacobian
        lp = lp + (-0.5 * torch.exp(us) ** 2 + 0.5 * math.log(2.0 / math.pi) + us)  # HalfNormal(1) and Jacobian
        K = _sq_exp(Xt, one, torch.exp(ul), 0.1 * one, dtype)
        lp = lp + _mvn_logp(f, torch.zeros_like(f), K) + _normal_logp(yt, f, torch.exp(us)).sum()
        return -lp

    sites = [("f", (N,), False), ("length", (), True), ("s", (), True)]
    return ModelCase("latent_f", latent_f_model, (X, y), sites, potential, seed=12)
