"""The dense ops (cholesky, trisolve) on the host: Program.run_host against torch float64
autograd, nmx_program_check's refusals, rank-2 values in the lowering, and MultivariateNormal on
the program path (tests/linalg_op_cases.py holds the cases)."""
import ctypes

import numpy as np
import pytest
import torch

import linalg_op_cases as LC
import numpyro_amd as numpyro
from numpyro_amd import distributions as dist
from numpyro_amd import jnp, native
from numpyro_amd.infer import NUTS
from numpyro_amd.loglik_program import compile_log_likelihood
from numpyro_amd.potentials import MultivariateNormal as FusedMVN
from numpyro_amd.predictive_program import compile_predictive
from numpyro_amd.program import Program, ProgramPotential, compile_model

RTOL = 1e-9  # float64 against float64


def _close(x, ref):
    np.testing.assert_allclose(x, ref, rtol=RTOL, atol=0.0)


# ------------------------------------------------------------------ 1: op semantics
@pytest.mark.parametrize("n", LC.SIZES)
@pytest.mark.parametrize("kind", LC.KINDS)
def test_run_host_matches_float64_torch(kind, n):
    c = LC.op_case(kind, n)
    assert c.program.native_check() == (0, "")
    U64, G64 = c.reference
    assert np.all(np.isfinite(U64)) and np.all(np.isfinite(G64))
    U, G = c.program.run_host(c.Z)
    _close(U, U64)
    _close(G, G64)


def test_cholesky_writes_an_exact_lower_triangle_and_nan_from_a_bad_pivot():
    from numpyro_amd.program import _host_cholesky

    A = np.array([[[4.0, 99.0], [2.0, 5.0]], [[1.0, 2.0], [2.0, 1.0]]])  # the upper triangle is not read
    L = _host_cholesky(A)
    np.testing.assert_array_equal(L[0], [[2.0, 0.0], [1.0, 2.0]])
    assert L[1, 0, 0] == 1.0 and L[1, 1, 0] == 2.0 and L[1, 0, 1] == 0.0 and np.isnan(L[1, 1, 1])
    c = LC.op_case("mvn", 2)
    Z = c.Z.copy()
    Z[5] = [1.0, 2.0, 2.0, 1.0]
    U, G = c.program.run_host(Z)
    assert np.isnan(U[5]) and np.all(np.isfinite(np.delete(U, 5)))
    np.testing.assert_array_equal(np.delete(U, 5), np.delete(c.program.run_host(c.Z)[0], 5))


def test_cost_model_and_names_know_the_ops():
    c = LC.op_case("mvn", 30)
    text = "\n".join(c.program.describe())
    assert "cholesky" in text and "trisolve" in text
    assert c.program.flops_per_eval(1) > 30 ** 3 and c.program.bytes_per_eval() > 4 * 4 * 900
    assert native.OPCODE["cholesky"] > native.OPCODE["concat"] and native.OPCODE["trisolve"] < native.DRAW_BASE


# ------------------------------------------------------------------ 2: nmx_program_check
def _check(rows, consts, num_slots, dim):
    prog = Program(rows, consts, [], num_slots, dim)
    return prog.native_check()


@pytest.mark.parametrize("which", ["chol_n0", "chol_n129", "chol_past_slots", "chol_not_square", "tri_n0", "tri_n129",
                                   "tri_past_slots", "tri_two_constants", "tri_overlap"])
def test_program_check_refuses_naming_the_op(which):
    C, T, R = native.OPCODE["cholesky"], native.OPCODE["trisolve"], native.OPCODE["reduce_sum"]
    big = 129 * 129
    consts = np.ones(big + 129)
    rows, slots, dim, name = {
        "chol_n0": ([[C, 4, 0, 0, 0, 1, 0, 0]], 5, 4, "cholesky"),
        "chol_n129": ([[C, big, 0, 0, big, 1, 0, 129], [R, 2 * big, big, 0, big, 1, 0, 0]], 2 * big + 1, big, "cholesky"),
        # a 3 x 3 matrix read from slot 2 of a z of 9: runs past the value
        "chol_past_slots": ([[C, 9, 2, 0, 9, 1, 0, 3], [R, 18, 9, 0, 9, 1, 0, 0]], 19, 9, "cholesky"),
        "chol_not_square": ([[C, 9, 0, 0, 8, 1, 0, 3], [R, 17, 9, 0, 8, 1, 0, 0]], 18, 9, "cholesky"),
        "tri_n0": ([[T, 4, 0, ~0, 0, 1, 1, 0]], 5, 4, "trisolve"),
        "tri_n129": ([[T, big, 0, ~0, 129, 1, 1, 0], [R, big + 129, big, 0, 129, 1, 0, 0]], big + 130, big, "trisolve"),
        "tri_past_slots": ([[T, 9, 4, ~0, 3, 1, 1, 0], [R, 12, 9, 0, 3, 1, 0, 0]], 13, 9, "trisolve"),
        "tri_two_constants": ([[T, 4, ~0, ~9, 3, 1, 1, 0], [R, 7, 4, 0, 3, 1, 0, 0]], 8, 4, "trisolve"),
        "tri_overlap": ([[T, 9, 0, 6, 3, 1, 1, 0], [R, 12, 9, 0, 3, 1, 0, 0]], 13, 9, "trisolve"),
    }[which]
    st, msg = _check(rows, consts, slots, dim)
    assert st == 1 and msg.startswith(f"op 0 ({name})"), msg
    # the predictive and log-likelihood checks share the rules
    prog = Program(rows, consts, [], slots, dim)
    out = np.array([[slots - 1, 1, 0]], np.int32)
    lib = native.lib()
    if which != "tri_overlap":  # adjoints alone care about overlapping z operands
        assert lib.nmx_loglik_program_check(ctypes.byref(prog.native_struct()), int(out.ctypes.data), 1, 1) == 1
        assert lib.nmx_last_error().decode().startswith(f"op 0 ({name})")
        pair = np.array([[slots - 1, 1]], np.int32)
        assert lib.nmx_predict_program_check(ctypes.byref(prog.native_struct()), int(pair.ctypes.data), 1) == 1
        assert lib.nmx_last_error().decode().startswith(f"op 0 ({name})")


def test_every_program_kind_accepts_the_ops():
    prog = LC.op_case("mvn", 3).program
    lib = native.lib()
    out = np.array([[prog.num_slots - 1, 1, 0]], np.int32)
    assert lib.nmx_loglik_program_check(ctypes.byref(prog.native_struct()), int(out.ctypes.data), 1, 1) == 0
    assert lib.nmx_predict_program_check(ctypes.byref(prog.native_struct()), int(out.ctypes.data), 1) == 0


# ------------------------------------------------------------------ 3: rank 2 in the lowering
def test_rank_two_values_broadcast_by_numpy_rules():
    """(n,) against (n, n), (n, 1) against (1, n), a scalar against (n, n), on symbolic values."""
    n = 4
    M = np.arange(16.0).reshape(n, n) / 7.0
    y = np.linspace(-1.0, 1.0, n)

    def model():
        a = numpyro.sample("a", dist.Normal(np.zeros(n), np.ones(n)))
        s = numpyro.sample("s", dist.Normal(0.0, 1.0))
        k = jnp.exp(0.1 * (a + M)) * s  # (n,) + (n, n): a runs along the rows
        k = k + jnp.power(y[:, None] - a, 2.0)  # a constant (n, 1) against a symbolic (n,): (1, n)
        k = k + (2.0 + jnp.square(s)) * jnp.eye(n)
        numpyro.sample("y", dist.MultivariateNormal(y, scale_tril=k), obs=np.zeros(n))

    pot = compile_model(model)
    names = [native.op_name(o) for o in pot.program.ops[:, 0]]
    assert "trisolve" in names and "cholesky" not in names and "gather" in names
    Z = np.random.RandomState(0).uniform(-1, 1, (LC.ROWS, n + 1))
    U, G = pot.program.run_host(Z)
    Zt = torch.tensor(Z, requires_grad=True)
    a, s = Zt[:, :n], Zt[:, n]
    k = torch.exp(0.1 * (a[:, None, :] + torch.tensor(M))) * s[:, None, None]
    k = k + (torch.tensor(y)[None, :, None] - a[:, None, :]) ** 2
    k = k + (2.0 + s[:, None, None] ** 2) * torch.eye(n, dtype=torch.float64)
    ref = -(torch.distributions.MultivariateNormal(torch.tensor(y), scale_tril=torch.tril(k)).log_prob(torch.zeros(n))
            + torch.distributions.Normal(0.0, 1.0).log_prob(Zt).sum(1))
    (g,) = torch.autograd.grad(ref.sum(), Zt)
    _close(U, ref.detach().numpy())
    _close(G, g.numpy())


def _rank2_refused():
    y = np.zeros(3)

    def with_k(f):
        def model():
            a = numpyro.sample("a", dist.Normal(np.zeros(3), np.ones(3)))
            k = np.ones((3, 1)) * a + np.eye(3)
            numpyro.sample("y", dist.Normal(f(a, k), 1.0), obs=y)
        return model

    def rank3():
        a = numpyro.sample("a", dist.Normal(np.zeros(3), np.ones(3)))
        numpyro.sample("y", dist.Normal(jnp.sum(a) + np.zeros((2, 3, 3)), 1.0), obs=0.0)

    def latent2():
        numpyro.sample("w", dist.Normal(np.zeros((2, 2)), np.ones((2, 2))))

    return {"getitem": ("y", with_k(lambda a, k: k[0]), "rank > 1"),
            "matmul_symbolic": ("y", with_k(lambda a, k: jnp.matmul(k, a)), "two symbolic"),
            "matmul_const": ("y", with_k(lambda a, k: jnp.matmul(np.ones((3, 3)), k)), "rank > 1"),
            "rank3": ("y", rank3, "rank > 1"), "latent2": ("w", latent2, "latents of rank > 1")}


@pytest.mark.parametrize("case", sorted(_rank2_refused()))
def test_rank_two_operations_outside_the_class_stay_refused(case):
    site, model, why = _rank2_refused()[case]
    with pytest.raises(NotImplementedError, match=f"(?s)site '{site}'.*{why}"):
        compile_model(model)


def test_reductions_of_a_rank_two_symbolic_value_stay_refused():
    a = jnp.Sym("latent", ("a",), (3, 3))
    for f in (jnp.sum, jnp.cumsum, jnp.logsumexp, lambda x: jnp.concatenate([x, x])):
        with pytest.raises(NotImplementedError):
            f(a)


def test_jnp_additions_on_constants():
    np.testing.assert_array_equal(jnp.power(np.array([2.0, 3.0]), 2.0), [4.0, 9.0])
    np.testing.assert_array_equal(jnp.eye(3), np.eye(3))
    A = np.array([[4.0, 2.0], [2.0, 5.0]])
    np.testing.assert_allclose(jnp.linalg.cholesky(A), np.linalg.cholesky(A))
    s = jnp.linalg.cholesky(jnp.Sym("latent", ("k",), (3, 3)))
    assert s.op == "cholesky" and s.shape == (3, 3)
    with pytest.raises(NotImplementedError):
        jnp.linalg.cholesky(jnp.Sym("latent", ("k",), (3,)))


# ------------------------------------------------------------------ 4: MultivariateNormal
_N = 5
_RS = np.random.RandomState(5)
_B = _RS.randn(_N, _N)
_COV = _B @ _B.T / _N + np.eye(_N)
_Y = _RS.randn(_N)
_LOC = _RS.randn(_N)


def _mvn_model(param, symbolic):
    """y ~ MVN(loc + m, matrix) observed, m a latent vector; symbolic: the matrix scaled by a latent s."""
    L = np.linalg.cholesky(_COV)

    def model():
        m = numpyro.sample("m", dist.Normal(np.zeros(_N), np.ones(_N)))
        s = numpyro.sample("s", dist.LogNormal(0.0, 1.0)) if symbolic else 1.0
        kw = {"covariance": dict(covariance_matrix=s * _COV), "scale_tril": dict(scale_tril=s * L),
              "precision": dict(precision_matrix=np.linalg.inv(_COV))}[param]
        numpyro.sample("y", dist.MultivariateNormal(_LOC + m, **kw), obs=_Y)

    return model


def _mvn_reference(param, symbolic, Z):
    Zt = torch.tensor(Z, requires_grad=True)
    m = Zt[:, :_N]
    s = torch.exp(Zt[:, _N]) if symbolic else torch.ones(Z.shape[0], dtype=torch.float64)
    cov, L = torch.tensor(_COV), torch.tensor(np.linalg.cholesky(_COV))
    kw = {"covariance": dict(covariance_matrix=s[:, None, None] * cov),
          "scale_tril": dict(scale_tril=s[:, None, None] * L),
          "precision": dict(precision_matrix=torch.linalg.inv(cov).expand(Z.shape[0], _N, _N))}[param]
    lp = torch.distributions.MultivariateNormal(torch.tensor(_LOC) + m, **kw).log_prob(torch.tensor(_Y))
    lp = lp + torch.distributions.Normal(0.0, 1.0).log_prob(m).sum(1)
    if symbolic:  # LogNormal(0, 1) at exp(u) with the Jacobian: Normal(0, 1) at u
        lp = lp + torch.distributions.Normal(0.0, 1.0).log_prob(Zt[:, _N])
    (g,) = torch.autograd.grad(-lp.sum(), Zt)
    return -lp.detach().numpy(), g.numpy()


@pytest.mark.parametrize("param,symbolic", [("covariance", True), ("scale_tril", True), ("covariance", False),
                                            ("scale_tril", False), ("precision", False)])
def test_compiled_density_matches_torch_log_prob(param, symbolic):
    pot = compile_model(_mvn_model(param, symbolic))
    assert isinstance(pot, ProgramPotential) and pot.program.native_check() == (0, "")
    names = [native.op_name(o) for o in pot.program.ops[:, 0]]
    if symbolic:
        assert "trisolve" in names and ("cholesky" in names) == (param == "covariance")
    else:  # folded: the factor on the host, L^-1 through matvec, the log-determinant in the pool
        assert "cholesky" not in names and "trisolve" not in names and "matvec" in names
    Z = np.random.RandomState(6).uniform(-1, 1, (LC.ROWS, pot.dim))
    U, G = pot.program.run_host(Z)
    U64, G64 = _mvn_reference(param, symbolic, Z)
    _close(U, U64)
    _close(G, G64)


def test_diagonal_covariance_equals_the_normal_model():
    y = np.linspace(-1.0, 2.0, 4)

    def mvn():
        sigma = numpyro.sample("sigma", dist.HalfNormal(np.ones(4)))
        mu = numpyro.sample("mu", dist.Normal(0.0, 3.0))
        numpyro.sample("y", dist.MultivariateNormal(mu, covariance_matrix=jnp.square(sigma) * jnp.eye(4)), obs=y)

    def normal():
        sigma = numpyro.sample("sigma", dist.HalfNormal(np.ones(4)))
        mu = numpyro.sample("mu", dist.Normal(0.0, 3.0))
        numpyro.sample("y", dist.Normal(mu, sigma), obs=y)

    a, b = compile_model(mvn), compile_model(normal)
    assert a.sites == b.sites
    Z = np.random.RandomState(7).uniform(-1, 1, (LC.ROWS, 5))
    Ua, Ga = a.program.run_host(Z)
    Ub, Gb = b.program.run_host(Z)
    _close(Ua, Ub)
    _close(Ga, Gb)


def test_latent_vector_with_a_latent_covariance():
    c = LC.latent_f_case()
    assert c.pot.sites == [("f", (8,), 0), ("length", (), 1), ("s", (), 1)]
    U, G = c.pot.program.run_host(c.Z)
    _close(U, c.reference[0])
    _close(G, c.reference[1])


def test_constant_mvn_target_keeps_its_fused_kernel():
    def model():
        numpyro.sample("x", dist.MultivariateNormal(np.zeros(_N), covariance_matrix=_COV))

    assert isinstance(NUTS(model).potential(), FusedMVN)
    L = np.linalg.cholesky(_COV)
    d = dist.MultivariateNormal(_LOC, scale_tril=L)
    assert d.scale_tril is None and d.event_shape == (_N,) and d.batch_shape == ()
    np.testing.assert_allclose(d.covariance_matrix, _COV)


def _mvn_refused():
    k3 = np.stack([_COV, _COV, _COV])

    def precision():
        s = numpyro.sample("s", dist.LogNormal(0.0, 1.0))
        numpyro.sample("y", dist.MultivariateNormal(0.0, precision_matrix=s * _COV), obs=_Y)

    def batched_matrix():
        s = numpyro.sample("s", dist.LogNormal(0.0, 1.0))
        numpyro.sample("y", dist.MultivariateNormal(0.0, covariance_matrix=s * k3), obs=_Y)

    def batched_loc():
        s = numpyro.sample("s", dist.LogNormal(0.0, 1.0))
        numpyro.sample("y", dist.MultivariateNormal(np.zeros((3, _N)), covariance_matrix=s * _COV), obs=_Y)

    def plated():
        s = numpyro.sample("s", dist.LogNormal(0.0, 1.0))
        with numpyro.plate("p", 3):
            numpyro.sample("y", dist.MultivariateNormal(0.0, covariance_matrix=s * _COV), obs=_Y)

    def n129():
        s = numpyro.sample("s", dist.LogNormal(0.0, 1.0))
        numpyro.sample("y", dist.MultivariateNormal(0.0, covariance_matrix=s * np.eye(129)), obs=np.zeros(129))

    def indefinite():
        s = numpyro.sample("s", dist.Normal(0.0, 1.0))
        numpyro.sample("y", dist.MultivariateNormal(s, covariance_matrix=np.array([[1.0, 2.0], [2.0, 1.0]])),
                       obs=np.zeros(2))

    return {"precision": (precision, "precision_matrix"), "batched_matrix": (batched_matrix, "batch dimensions"),
            "batched_loc": (batched_loc, "batch dimensions"), "plated": (plated, "plate"), "n129": (n129, "129"),
            "indefinite": (indefinite, "positive definite")}


@pytest.mark.parametrize("case", sorted(_mvn_refused()))
def test_mvn_outside_the_class_is_refused_naming_the_site(case):
    model, why = _mvn_refused()[case]
    with pytest.raises(NotImplementedError, match=f"(?s)site 'y'.*{why}"):
        compile_model(model)


# ------------------------------------------------------------------ 5: the Gaussian process
def test_gp_model_compiles_and_matches_float64():
    """Three LogNormal hyperparameters, a squared-exponential kernel matrix built from them and
    Y ~ MultivariateNormal(0, k), 30 points: U and its gradient at 16 unconstrained points."""
    c = LC.gp_case()
    pot = c.pot
    assert isinstance(pot, ProgramPotential) and pot.dim == 3
    assert [s[0] for s in pot.sites] == ["kernel_length", "kernel_noise", "kernel_var"]
    names = [native.op_name(o) for o in pot.program.ops[:, 0]]
    assert names.count("cholesky") == 1 and names.count("trisolve") == 1
    assert pot.program.native_check() == (0, "")
    U64, G64 = c.reference
    assert np.all(np.isfinite(U64)) and np.all(np.isfinite(G64))
    U, G = pot.program.run_host(c.Z)
    _close(U, U64)
    _close(G, G64)
    assert isinstance(NUTS(c.model).potential(c.args), ProgramPotential)


def test_log_likelihood_of_the_gp_is_one_observation_per_sample():
    c = LC.gp_case()
    prog = compile_log_likelihood(c.model, c.args, {}, [n for n, _, _ in c.sites])
    assert prog.native_check() == (0, "") and prog.num_columns == 1
    assert [(o.name, o.n, o.shape) for o in prog.outputs] == [("Y", 1, ())]
    Z = c.Z[:5]
    out = prog.run_host(np.exp(Z))  # the inputs are constrained values
    assert out["Y"].shape == (5,)
    X, Y = (torch.tensor(a) for a in c.args)
    for r in range(5):
        length, noise, var = (torch.tensor(v) for v in np.exp(Z[r]))
        K = LC._sq_exp(X, var, length, noise, torch.float64)
        ref = torch.distributions.MultivariateNormal(torch.zeros(30, dtype=torch.float64), K).log_prob(Y)
        np.testing.assert_allclose(out["Y"][r], float(ref), rtol=RTOL)


def test_predictive_keeps_an_observed_mvn_and_refuses_to_draw_one():
    c = LC.gp_case()
    prog = compile_predictive(c.model, c.args, {}, {"kernel_length", "kernel_noise", "kernel_var"})
    assert "Y" in prog.observed and not prog.outputs
    with pytest.raises(NotImplementedError, match="(?s)site 'Y'.*drawing a MultivariateNormal"):
        compile_predictive(c.model, (c.args[0], None), {}, {"kernel_length", "kernel_noise", "kernel_var"})
