"""The cumsum / logsumexp / concat ops and the models built on them, without a GPU: the host
interpreter against independent float64 torch, nmx_program_check's refusals, the compiled
simplex / Categorical / mixture models against torch.distributions, the host plumbing of a site
whose constrained and unconstrained sizes differ, and the compiler's refusals."""
import os

import numpy as np
import pytest
import torch
import torch.distributions as td

import numpyro_amd as numpyro
import program_zoo as Zoo
import simplex_cases as SC
from numpyro_amd import distributions as dist
from numpyro_amd import jnp, native
from numpyro_amd.potentials import SIMPLEX, stick_breaking
from numpyro_amd.predictive_program import compile_predictive
from numpyro_amd.program import ProgramPotential, compile_model

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "program_zoo_ops.npz")


# ------------------------------------------------------------------ 1: op semantics
def test_the_three_opcodes_follow_matvec():
    assert native.OPCODES[native.OPCODE["matvec"] + 1:] == ["cumsum", "logsumexp", "concat"]


@pytest.mark.parametrize("family", SC.FAMILIES)
def test_run_host_matches_float64_torch(family):
    """Program.run_host on every hand-assembled case against torch.cumsum / torch.logsumexp /
    torch.cat with autograd, in float64: 1e-12 relative to max(1, |reference|)."""
    for c in SC.cases(family):
        U64, G64 = c.reference()
        U, G = c.program.run_host(c.Z)
        assert np.all(np.isfinite(U64)) and np.all(np.isfinite(G64)), c.name
        eU, eG = SC.OC.scaled_errors(U, G, U64, G64)
        assert eU.max() <= 1e-12 and eG.max() <= 1e-12, (c.name, eU.max(), eG.max())
        # and the float32 restatement of this file runs the same program at float32 level
        U32, G32 = SC.run_host_f32(c.program, c.Z)
        eU, eG = SC.OC.scaled_errors(U32, G32, U64, G64)
        assert eU.max() <= 1e-4 and eG.max() <= 1e-4, (c.name, eU.max(), eG.max())


def test_a_row_of_minus_inf_has_a_zero_adjoint():
    pot, Z, (rows, cols), dead, G64 = SC.all_inf_row()
    for U, G in (pot.program.run_host(Z), SC.run_host_f32(pot.program, Z)):
        assert np.all(U == np.inf)
        assert not np.isnan(G).any()
        assert np.all(G[:, dead * cols:(dead + 1) * cols] == 0.0)
        np.testing.assert_allclose(G, G64, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------ 2: nmx_program_check
@pytest.mark.parametrize("family", SC.FAMILIES)
def test_check_accepts_the_cases(family):
    for c in SC.cases(family):
        st, msg = c.program.native_check()
        assert st == 0, (c.name, msg)
    st, msg = SC.all_inf_row()[0].program.native_check()
    assert st == 0, msg


@pytest.mark.parametrize("name,program,op", SC.refused_programs(), ids=[r[0] for r in SC.refused_programs()])
def test_check_refuses_naming_the_op(name, program, op):
    st, msg = program.native_check()
    assert st != 0 and f"({op})" in msg, (name, st, msg)


def test_check_refusals_say_what_is_wrong():
    by = {name: program.native_check()[1] for name, program, _ in SC.refused_programs()}
    assert "overlap at different offsets" in by["concat z overlap"]
    assert "both operands constant" in by["concat both constant"]
    assert "aux" in by["concat aux 0"] and "aux" in by["concat aux n"] and "aux" in by["logsumexp aux 0"]
    assert "out of range" in by["cumsum past its value"] and "out of range" in by["logsumexp past its value"]
    assert "4294967296" in by["logsumexp n * aux wraps int32"]


def test_predictive_check_admits_the_ops():
    """The predictive check shares the impl: a deterministic site through all three ops."""
    def model():
        g = numpyro.sample("g", dist.Normal(np.zeros(5), np.ones(5)))
        numpyro.deterministic("d", jnp.concatenate([jnp.cumsum(g), np.ones(2)]) - jnp.logsumexp(g))

    prog = compile_predictive(model)
    names = prog.op_names()
    assert {"cumsum", "logsumexp", "concat"} <= set(names), names
    st, msg = prog.native_check()
    assert st == 0, msg


# ------------------------------------------------------------------ 3: compiled models
def _compiled(name):
    m = SC.MODELS[name]()
    pot = compile_model(m.model, m.args)
    assert isinstance(pot, ProgramPotential) and pot.dim == m.dim
    st, msg = pot.program.native_check()
    assert st == 0, msg
    return m, pot


@pytest.mark.parametrize("R", [2, 8])
@pytest.mark.parametrize("name", sorted(SC.MODELS))
def test_compiled_models_match_torch_distributions(name, R):
    """run_host against torch.distributions (Dirichlet, StickBreakingTransform, Categorical,
    MixtureSameFamily; autograd) in float64 at Z ~ U(-R, R), 200 rows: 1e-9 relative, and the
    log-space statement of simplex_cases to the same bound.  At R = 8 the models with more than 4
    components, where torch.distributions clamps the weights (simplex_cases.TORCH_AT_8), are held
    to the log-space statement instead."""
    m, pot = _compiled(name)
    Z = SC.wide_rows(m.dim, R)
    U, G = pot.program.run_host(Z)
    Ul, Gl = m.logspace_reference(Z)
    assert np.all(np.isfinite(Ul)) and np.all(np.isfinite(Gl))
    eU, eG = SC.OC.scaled_errors(U, G, Ul, Gl)
    print(f"{name} R={R} run_host against the log-space statement: U {eU.max():.3e}, gradient {eG.max():.3e}")
    assert eU.max() <= 1e-9 and eG.max() <= 1e-9, (eU.max(), eG.max())
    if R == 8 and name not in SC.TORCH_AT_8:
        return
    assert m.min_weight(Z) >= SC.TORCH_VALID_WEIGHT, m.min_weight(Z)
    Ut, Gt = m.torch_reference(Z)
    assert np.all(np.isfinite(Ut)) and np.all(np.isfinite(Gt))
    for what, (Ux, Gx) in (("run_host", (U, G)), ("log-space statement", (Ul, Gl))):
        eU, eG = SC.OC.scaled_errors(Ux, Gx, Ut, Gt)
        print(f"{name} R={R} {what} against torch.distributions: U {eU.max():.3e}, gradient {eG.max():.3e}")
        assert eU.max() <= 1e-9 and eG.max() <= 1e-9, (what, eU.max(), eG.max())


@pytest.mark.parametrize("name", sorted(SC.MODELS))
def test_compiled_models_far_from_the_mode(name):
    """Z ~ U(-16, 16): against the float64 log-space statement of simplex_cases (whose agreement
    with torch.distributions at R = 2 and 8 is the test above).  torch.distributions is not the
    reference here: StickBreakingTransform clips its sigmoid and Categorical clamps its
    probabilities at the float64 epsilon, and stick-breaking weights far from the mode are far
    below that, so its log densities deviate (up to 9e-3 relative on these models)."""
    m, pot = _compiled(name)
    Z = SC.wide_rows(m.dim, 16)
    U64, G64 = m.logspace_reference(Z)
    assert np.all(np.isfinite(U64)) and np.all(np.isfinite(G64))
    U, G = pot.program.run_host(Z)
    eU, eG = SC.OC.scaled_errors(U, G, U64, G64)
    print(f"{name} R=16: scaled error of U {eU.max():.3e}, of the gradient {eG.max():.3e}")
    assert eU.max() <= 1e-9 and eG.max() <= 1e-9, (eU.max(), eG.max())
    # float32 survives: the restatement is finite on every row
    U32, G32 = SC.run_host_f32(pot.program, Z)
    assert np.all(np.isfinite(U32)) and np.all(np.isfinite(G32))


def test_every_log_of_a_simplex_value_reads_log_x():
    """No log op in the Dirichlet-Categorical program: log x of the density and of the
    likelihood is the transform's own log x (log(exp(v)) folds to v)."""
    _, pot = _compiled("dirichlet_categorical.K3")
    names = [native.OPCODES[o] for o in pot.program.ops[:, 0]]
    assert "log" not in names and "exp" not in names, names
    assert {"cumsum", "concat"} <= set(names)


def test_existing_models_compile_to_the_same_program():
    """Programs without the new ops are unchanged: the op arrays, constants and index pools of two
    program_zoo models equal those pinned from the commit before the ops were added."""
    gold = np.load(GOLDEN)
    for name in ("poisson", "treg"):
        case = Zoo.CASES[name]()
        p = compile_model(case.model, case.args).program
        np.testing.assert_array_equal(p.ops, gold[name + "_ops"])
        np.testing.assert_array_equal(p.consts64, gold[name + "_consts"])
        np.testing.assert_array_equal(p.index, gold[name + "_index"])
        assert [p.num_slots, p.dim] == gold[name + "_shape"].tolist()


# ------------------------------------------------------------------ 4: host plumbing
def test_sites_carry_the_unconstrained_shape():
    m, pot = _compiled("normal_mixture.N5K3")
    assert pot.sites == [("mu", (3,), 0), ("sigma", (3,), 1), ("w", (2,), SIMPLEX)]
    assert pot.constrained_shapes() == {"mu": (3,), "sigma": (3,), "w": (3,)}
    flat = torch.zeros(6, 8)
    parts = pot.unflatten(flat)
    assert parts["w"].shape == (6, 2)
    assert pot.flatten({k: v for k, v in parts.items()}).shape == (6, 8)


@pytest.mark.parametrize("K", [2, 3, 65, 130])
def test_constrain_maps_to_the_simplex_and_round_trips(K):
    """Rows sum to 1 within 1e-6 (float32 and float64), u = 0 is the uniform point, and the
    reference's inverse (StickBreakingTransform.inv, as torch.distributions states it) recovers u."""
    pot = ProgramPotential.__new__(ProgramPotential)
    pot.sites, pot.affine = [("w", (K - 1,), SIMPLEX)], {}
    u64 = torch.from_numpy(np.random.RandomState(K).uniform(-4, 4, (50, K - 1)))
    for u, tol in ((u64, 1e-12), (u64.float(), 1e-6)):
        x = pot.constrain({"w": u})["w"]
        assert x.shape == (50, K) and x.dtype == u.dtype and bool((x > 0).all())
        assert float((x.sum(-1) - 1.0).abs().max()) <= max(tol, 1e-6 if u.dtype == torch.float32 else 0.0)
    x = stick_breaking(u64)
    np.testing.assert_allclose(x.numpy(), td.StickBreakingTransform()(u64).numpy(), rtol=1e-9, atol=1e-15)
    # the inverse divides by the remaining stick 1 - cumsum(x), so its error is the rounding of x over
    # that mass: rows near the uniform point, where the last sticks keep a mass of about 1 / K
    near = torch.from_numpy(np.random.RandomState(K).uniform(-1, 1, (50, K - 1)))
    np.testing.assert_allclose(td.StickBreakingTransform().inv(stick_breaking(near)).numpy(), near.numpy(),
                               rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(stick_breaking(torch.zeros(1, K - 1, dtype=torch.float64)).numpy(), 1.0 / K, rtol=1e-12)


def test_deterministic_sites_see_the_constrained_simplex():
    y = np.array([0, 1, 2, 2])

    def model(y):
        w = numpyro.sample("w", dist.Dirichlet(np.ones(3)))
        numpyro.deterministic("top", jnp.logsumexp(jnp.log(w)) + jnp.sum(jnp.cumsum(w)))
        numpyro.deterministic("both", jnp.concatenate([w, np.zeros(2)]))
        numpyro.sample("y", dist.Categorical(probs=w), obs=y)

    pot = compile_model(model, (y,))
    u = torch.from_numpy(np.random.RandomState(0).uniform(-2, 2, (4, 5, 2))).float()
    x = pot.constrain({"w": u})
    assert x["w"].shape == (4, 5, 3)
    d = pot.deterministic(x)
    assert d["both"].shape == (4, 5, 5) and d["top"].shape == (4, 5)
    np.testing.assert_allclose(d["both"][..., :3].numpy(), x["w"].numpy())
    w = x["w"].double()
    np.testing.assert_allclose(d["top"].numpy(), (torch.logsumexp(w.log(), -1) + w.cumsum(-1).sum(-1)).numpy(), rtol=1e-5)


def test_jnp_functions_on_arrays():
    a = np.array([0.5, -1.0, 2.0])
    np.testing.assert_allclose(jnp.cumsum(a), np.cumsum(a))
    np.testing.assert_allclose(jnp.logsumexp(a), torch.logsumexp(torch.from_numpy(a), 0).item())
    assert jnp.logsumexp(np.array([-np.inf, -np.inf])) == -np.inf
    np.testing.assert_array_equal(jnp.concatenate([a, [1.0]]), np.concatenate([a, [1.0]]))


# ------------------------------------------------------------------ 5: refusals
_Y = np.array([0, 1, 2])


def _refused(model, args=()):
    with pytest.raises(NotImplementedError) as e:
        compile_model(model, args)
    return str(e.value)


def test_refusals_name_the_site():
    def rank2_logits(y):
        b = numpyro.sample("b", dist.Normal(0.0, 1.0))
        numpyro.sample("obs", dist.Categorical(logits=b * np.ones((3, 4))), obs=y)

    def latent_categorical():
        w = numpyro.sample("w", dist.Dirichlet(np.ones(3)))
        numpyro.sample("k", dist.Categorical(probs=w))

    def multivariate_components(y):
        w = numpyro.sample("w", dist.Dirichlet(np.ones(2)))
        comp = dist.Dirichlet(np.ones((2, 3)))
        numpyro.sample("obs", dist.MixtureSameFamily(dist.Categorical(probs=w), comp), obs=y)

    def one_category(y):
        b = numpyro.sample("b", dist.Normal(np.zeros(1), np.ones(1)))
        numpyro.sample("obs", dist.Categorical(logits=b), obs=y)

    def one_component_dirichlet():
        numpyro.sample("w", dist.Dirichlet(np.ones(1)))

    def batched_dirichlet():
        numpyro.sample("w", dist.Dirichlet(np.ones((2, 3))))

    def out_of_range(y):
        w = numpyro.sample("w", dist.Dirichlet(np.ones(3)))
        numpyro.sample("obs", dist.Categorical(probs=w), obs=y)

    def non_categorical_mixing(y):
        mu = numpyro.sample("mu", dist.Normal(np.zeros(2), np.ones(2)))
        numpyro.sample("obs", dist.MixtureSameFamily(dist.Normal(np.zeros(2), 1.0), dist.Normal(mu, 1.0)), obs=y)

    assert "'obs'" in _refused(rank2_logits, (_Y,))
    msg = _refused(latent_categorical)
    assert "'k'" in msg and "latent" in msg
    assert "'obs'" in _refused(multivariate_components, (np.array([0.2, 0.3, 0.5]),))
    assert "'obs'" in _refused(one_category, (np.array([0, 0]),))
    assert "'w'" in _refused(one_component_dirichlet)
    assert "'w'" in _refused(batched_dirichlet)
    msg = _refused(out_of_range, (np.array([0, 3]),))
    assert "'obs'" in msg and "[0, 3)" in msg
    assert "'obs'" in _refused(non_categorical_mixing, (np.array([0.5, 1.0]),))


def test_predictive_refuses_to_draw_a_categorical_or_a_mixture():
    def categorical(y=None):
        w = numpyro.sample("w", dist.Dirichlet(np.ones(3)))
        numpyro.sample("obs", dist.Categorical(probs=w), obs=y)

    def mixture(y=None):
        w = numpyro.sample("w", dist.Dirichlet(np.ones(2)))
        numpyro.sample("obs", dist.MixtureSameFamily(dist.Categorical(probs=w), dist.Normal(np.zeros(2), 1.0)), obs=y)

    for model in (categorical, mixture):
        with pytest.raises(NotImplementedError, match="'obs'.*data-dependent index"):
            compile_predictive(model, (None,))
        prog = compile_predictive(model, (np.array([0, 1]),))  # with its data the site is kept, w is drawn
        assert [o.name for o in prog.outputs] == ["w"] and "obs" in prog.observed
        assert {"draw_gamma", "reduce_sum", "div"} <= set(prog.op_names())
