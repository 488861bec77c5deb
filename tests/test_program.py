"""The program compiler and its float64 interpreter (numpyro_amd/program.py), the host-side
program check of the C ABI, and the front end's wiring -- no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import numpyro_amd as numpyro
import program_zoo as Zoo
from numpyro_amd import datasets, native
from numpyro_amd import distributions as dist
from numpyro_amd import jnp
from numpyro_amd import potentials as P
from numpyro_amd.frontend import LocScaleReparam, potential_from_model, reparam
from numpyro_amd.infer import HMC, NUTS
from numpyro_amd.jnp import Sym
from numpyro_amd.program import ProgramPotential, compile_model


# ------------------------------------------------------------------ 1: compiler + interpreter
@pytest.mark.parametrize("name", sorted(Zoo.CASES))
def test_program_matches_hand_written_float64(name):
    """Both sides are float64; only the order of operations differs."""
    case = Zoo.CASES[name]()
    pot = compile_model(case.model, case.args)
    assert pot.program.native_check() == (0, "")
    Z = np.random.RandomState(0).uniform(-2, 2, (200, case.dim))
    U, G = pot.program.run_host(Z)
    Ur, Gr = case.pe_grad64(Z)
    np.testing.assert_allclose(U, Ur, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(G, Gr, rtol=1e-9, atol=1e-9)


# ------------------------------------------------------------------ 2: structure of the program
@pytest.mark.parametrize("name", sorted(Zoo.CASES))
def test_sites_are_sorted_with_shapes_and_transforms(name):
    case = Zoo.CASES[name]()
    pot = compile_model(case.model, case.args)
    assert pot.sites == [(n, tuple(s), P.POSITIVE if pos else P.REAL) for n, s, pos in case.sites]
    assert [n for n, _, _ in pot.sites] == sorted(n for n, _, _ in pot.sites)
    assert pot.dim == case.dim == pot.program.dim
    pot.device, pot._codes = torch.device("cpu"), None  # as bind() sets them; the codes come from the sites
    codes = pot.transform_codes().numpy()
    expect = np.concatenate([np.full(int(np.prod(s)), int(pos)) for _, s, pos in case.sites])
    np.testing.assert_array_equal(codes, expect)


@pytest.mark.parametrize("name", sorted(Zoo.CASES))
def test_constants_are_folded(name):
    """No op reads only constants: whatever does not depend on a latent is in the pool."""
    prog = compile_model(*(lambda c: (c.model, c.args))(Zoo.CASES[name]())).program
    unary = native.OPCODE["add"]
    for op, dst, a, b, n, sa, sb, aux in prog.ops.tolist():
        if op < unary or op >= native.OPCODE["reduce_sum"]:
            assert a >= 0
        else:
            assert a >= 0 or b >= 0
    assert np.all(np.isfinite(prog.consts))
    # the last op defines U in the last slot
    assert prog.ops[-1, 1] == prog.num_slots - 1


def test_shared_expressions_are_one_slot():
    """A Sym used by two sites, and the same expression written twice on one Sym, is computed once."""
    def model(y1, y2):
        x = numpyro.sample("x", dist.Normal(np.zeros(3), np.ones(3)))
        e = jnp.exp(x)
        numpyro.sample("y1", dist.Normal(e, 1.0), obs=y1)
        numpyro.sample("y2", dist.Normal(e, 2.0), obs=y2)

    prog = compile_model(model, (np.arange(3.0), np.ones(3))).program
    ops = prog.ops.tolist()
    exps = [o for o in ops if o[0] == native.OPCODE["exp"]]
    assert len(exps) == 1
    users = [o for o in ops if o[2] == exps[0][1] or (o[0] >= native.OPCODE["add"] and o[3] == exps[0][1])]
    assert len(users) == 2  # fan-out 2


def test_cost_model_counts_the_ops():
    small = compile_model(*(lambda c: (c.model, c.args))(Zoo.CASES["poisson"]()))
    large = compile_model(*(lambda c: (c.model, c.args))(Zoo.poisson_large()))
    assert large.bytes_per_eval() > 20 * small.bytes_per_eval() > 0
    assert large.flops_per_eval(2) == 2 * large.flops_per_eval(1) > small.flops_per_eval(1) > 0


# ------------------------------------------------------------------ 3: refusals and wiring
class _Beta(dist.Distribution):
    support = "unit_interval"

    def __init__(self, a, b):
        super().__init__(())
        self.a, self.b = a, b


def _refused_models():
    y = np.zeros(4)

    def rank2():
        w = numpyro.sample("w", dist.Normal(np.zeros((2, 2)), np.ones((2, 2))))
        numpyro.sample("y", dist.Normal(jnp.matmul(np.ones((4, 2)), w), 1.0), obs=np.zeros((4, 2)))

    def grw():
        s = numpyro.sample("s", dist.Exponential(1.0))
        numpyro.sample("walk", dist.GaussianRandomWalk(s, 4))
        numpyro.sample("extra", dist.Normal(0.0, 1.0))

    def mvn():
        m = numpyro.sample("m", dist.Normal(np.zeros(2), np.ones(2)))
        numpyro.sample("v", dist.MultivariateNormal(m, covariance_matrix=np.eye(2)))

    def bounded():
        p = numpyro.sample("p", _Beta(2.0, 2.0))
        numpyro.sample("y", dist.Bernoulli(probs=p), obs=y)

    def discrete_latent():
        lam = numpyro.sample("lam", dist.Gamma(2.0, 1.0))
        numpyro.sample("k", dist.Poisson(lam))

    def bad_op():
        x = numpyro.sample("x", dist.Normal(np.zeros(4), np.ones(4)))
        numpyro.sample("y", dist.Normal(Sym("erf", (x,), (4,)), 1.0), obs=y)

    def two_symbolic():
        x = numpyro.sample("x", dist.Normal(np.zeros(4), np.ones(4)))
        numpyro.sample("y", dist.Normal(jnp.matmul(x, x), 1.0), obs=0.5)

    def rp():
        t = numpyro.sample("t", dist.HalfCauchy(1.0))
        numpyro.sample("x", dist.Normal(np.zeros(3), t))

    return {"rank2": ("w", rank2), "random_walk": ("walk", grw), "mvn": ("v", mvn), "bounded": ("p", bounded),
            "discrete_latent": ("k", discrete_latent), "bad_op": ("y", bad_op), "two_symbolic": ("y", two_symbolic),
            "reparam": ("x", reparam(rp, config={"x": LocScaleReparam(0)}))}


@pytest.mark.parametrize("case", sorted(_refused_models()))
def test_out_of_class_models_are_refused_naming_the_site(case):
    site, model = _refused_models()[case]
    with pytest.raises(NotImplementedError, match=f"site '{site}'"):
        compile_model(model)
    # NUTS reports both: no fused kernel, and why the program compiler refused
    with pytest.raises(NotImplementedError, match="(?s)^no fused kernel.*program compiler: site"):
        NUTS(model).potential()


def test_model_without_sites_is_still_refused():
    with pytest.raises(NotImplementedError, match="^no fused kernel"):
        NUTS(lambda: None).potential()


@pytest.mark.parametrize("change", ["prior", "likelihood", "structure"])
def test_structures_without_a_fused_kernel_compile(change):
    """The three models tests/test_frontend.py shows refused by the fused matchers."""
    def m(J, sigma, y):
        mu = numpyro.sample("mu", dist.Normal(0, 5 if change != "prior" else 10))
        tau = numpyro.sample("tau", dist.HalfCauchy(5))
        with numpyro.plate("J", J):
            theta = numpyro.sample("theta", dist.Normal(mu, tau))
            if change == "likelihood":
                numpyro.sample("obs", dist.StudentT(4.0, theta, sigma), obs=y)
            else:
                numpyro.sample("obs", dist.Normal(theta, sigma), obs=y)
        if change == "structure":
            numpyro.sample("extra", dist.Exponential(1.0))

    args = (8, datasets.EIGHT_SCHOOLS_SIGMA, datasets.EIGHT_SCHOOLS_Y)
    with pytest.raises(NotImplementedError, match="no fused kernel"):
        potential_from_model(m, args)
    for kernel in (NUTS, HMC):
        pot = kernel(m).potential(args)
        assert isinstance(pot, ProgramPotential)
        assert [n for n, _, _ in pot.sites] == sorted(["mu", "tau", "theta"] + (["extra"] if change == "structure" else []))
    assert isinstance(compile_model(m, args), ProgramPotential)


def test_fused_structures_keep_their_kernels():
    args = (8, datasets.EIGHT_SCHOOLS_SIGMA, datasets.EIGHT_SCHOOLS_Y)

    def m(J, sigma, y):
        mu = numpyro.sample("mu", dist.Normal(0, 5))
        tau = numpyro.sample("tau", dist.HalfCauchy(5))
        with numpyro.plate("J", J):
            theta = numpyro.sample("theta", dist.Normal(mu, tau))
            numpyro.sample("obs", dist.Normal(theta, sigma), obs=y)

    assert isinstance(NUTS(m).potential(args), P.EightSchools)
    # ... and the compiler agrees with the fused kernel's float64 oracle on the same model
    from oracle import potentials as OP

    ref = OP.EightSchools(datasets.EIGHT_SCHOOLS_Y, datasets.EIGHT_SCHOOLS_SIGMA)
    Z = np.random.RandomState(3).uniform(-2, 2, (20, 10))
    U, G = compile_model(m, args).program.run_host(Z)
    for c in range(20):
        pr, gr = ref.pe_grad(Z[c])
        np.testing.assert_allclose(U[c], pr, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(G[c], gr, rtol=1e-9, atol=1e-9)


def test_workspace_cap_is_reported():
    case = Zoo.CASES["poisson"]()
    pot = compile_model(case.model, case.args, max_workspace_bytes=1 << 16)
    with pytest.raises(NotImplementedError, match=r"(?s)4096 chains.*workspace of \d+ bytes"):
        pot.bind(4096, 4096, "cpu")


# ------------------------------------------------------------------ 4: nmx_program_check
def _tampered(which):
    prog = compile_model(*(lambda c: (c.model, c.args))(Zoo.CASES["poisson"]())).program
    ops, index = prog.ops.copy(), prog.index.copy()
    names = [native.OPCODES[o] for o in ops[:, 0]]
    k = {"opcode": 3, "slot": names.index("square"), "constant": names.index("mul"), "index": names.index("gather"),
         "count": names.index("exp")}[which]
    if which == "opcode":
        ops[k, 0] = len(native.OPCODES)
    elif which == "slot":
        ops[k, 2] = prog.num_slots + 5
    elif which == "constant":
        col = 2 if ops[k, 2] < 0 else 3
        assert ops[k, col] < 0
        ops[k, col] = ~(prog.consts.size + 3)
    elif which == "index":
        index[ops[k, 7] + 1] = ops[k, 3]  # == its source length
    else:
        ops[k, 4] = 0
    return prog, prog.native_struct(ops=ops, index=index), k, (ops, index)


@pytest.mark.parametrize("which", ["opcode", "slot", "constant", "index", "count"])
def test_program_check_names_the_bad_op(which):
    prog, bad, k, keep = _tampered(which)
    lib = native.lib()
    assert lib.nmx_program_check(ctypes.byref(prog.native_struct())) == 0
    assert lib.nmx_program_check(ctypes.byref(bad)) == 1  # NMX_ERR_INVALID
    msg = lib.nmx_last_error().decode()
    assert msg.startswith(f"op {k}"), msg
    word = {"opcode": "opcode", "slot": "slot", "constant": "constant", "index": "index", "count": "count"}[which]
    assert word in msg, msg


def test_bind_refuses_a_malformed_program():
    prog, bad, k, (ops, index) = _tampered("index")
    prog.index = index
    pot = ProgramPotential(prog, [("a", (5,), 0), ("b", (3,), 0), ("mu_a", (), 0), ("sigma_a", (), 1)])
    with pytest.raises(native.NativeError, match=f"op {k}"):
        pot.bind(4, 64, "cpu")


# ------------------------------------------------------------------ 5: deterministic sites
def test_new_operations_in_deterministic_sites():
    group = np.array([2, 0, 0, 1])

    def model(y):
        a = numpyro.sample("a", dist.Normal(np.zeros(3), np.ones(3)))
        s = numpyro.sample("s", dist.HalfNormal(1.0))
        numpyro.deterministic("picked", a[group])
        numpyro.deterministic("first", a[0])
        numpyro.deterministic("tail", a[1:])
        numpyro.deterministic("l1p", jnp.log1p(jnp.square(a)))
        numpyro.deterministic("total", jnp.sum(a * s))
        numpyro.sample("y", dist.Normal(a[group], s), obs=y)

    pot = compile_model(model, (np.zeros(4),))
    rs = np.random.RandomState(0)
    a, s = rs.randn(5, 2, 3), rs.rand(5, 2) + 0.5
    out = pot.deterministic({"a": torch.tensor(a, dtype=torch.float32), "s": torch.tensor(s, dtype=torch.float32)})
    assert out["picked"].shape == (5, 2, 4) and out["first"].shape == (5, 2) and out["tail"].shape == (5, 2, 2)
    assert out["l1p"].shape == (5, 2, 3) and out["total"].shape == (5, 2)
    np.testing.assert_allclose(out["picked"].numpy(), a[..., group], rtol=1e-6)
    np.testing.assert_allclose(out["first"].numpy(), a[..., 0], rtol=1e-6)
    np.testing.assert_allclose(out["tail"].numpy(), a[..., 1:], rtol=1e-6)
    np.testing.assert_allclose(out["l1p"].numpy(), np.log1p(a ** 2), rtol=1e-5)
    np.testing.assert_allclose(out["total"].numpy(), (a * s[..., None]).sum(-1), rtol=1e-5, atol=1e-6)
