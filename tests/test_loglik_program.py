"""Log-likelihood programs on the host (numpyro_amd/loglik_program.py): the lowering against
torch.distributions, its consistency with the program potential, the refusals of the compiler and
of nmx_loglik_program_check, and compile_model's programs unchanged.  No GPU."""
import json
import os

import numpy as np
import pytest

import loglik_cases as LC
import numpyro_amd as numpyro
from numpyro_amd import distributions as dist
from numpyro_amd import native
from numpyro_amd.frontend import LocScaleReparam, reparam
from numpyro_amd.loglik_program import LogLikProgram, compile_log_likelihood
from numpyro_amd.native import OPCODE
from numpyro_amd.program import compile_model

HERE = os.path.dirname(os.path.abspath(__file__))
S = 5


def _compile(case, samples):
    return compile_log_likelihood(case.model, case.args, {}, given=samples)


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_host_interpreter_against_torch_distributions(name):
    """run_host in float64 against torch.distributions in float64, every element of every observed
    site at S = 5 points strictly inside the supports: |d| <= 1e-10 (1 + |ref|), the project's
    relative measure.  (|d| / |ref| is printed too: it is below 2e-14 everywhere but at one element
    of `logit`, where the *reference* is 7e-16 off: binary_cross_entropy_with_logits forms
    12.3 - 12.3 + 4.5e-6, while the program's -x softplus(-eta) - (1 - x) softplus(eta) agrees with
    an extended-precision evaluation to 1e-21.)"""
    case = LC.CASES[name]()
    samples = case.constrain(case.points(S))
    prog = _compile(case, samples)
    assert [n for n, _, _, _ in prog.inputs] == [n for n, _, _ in case.sites]
    assert prog.native_check() == (0, "")
    ref = LC.reference64(case, samples)
    got = prog.run_host(samples)
    assert sorted(got) == sorted(ref)
    for site, r in ref.items():
        assert np.all(np.isfinite(r)), (name, site)
        assert got[site].shape == r.shape and got[site].dtype == np.float64, (name, site, got[site].shape, r.shape)
        rel, err = float((np.abs(got[site] - r) / np.abs(r)).max()), LC.scaled_error(got[site], r)
        print(f"{name}.{site}: largest |d| / (1 + |ref|) = {err:.2e}, |d| / |ref| = {rel:.2e} over {r.size} elements")
        assert err <= 1e-10, (name, site, err)
    # the float32 run is the same arithmetic in float32 (the calibration of the device tests)
    r32 = prog.run_host(samples, dtype=np.float32)
    for site, r in ref.items():
        assert r32[site].dtype == np.float32 and LC.scaled_error(r32[site], r) < 1e-4, (name, site)


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_consistent_with_the_program_potential(name):
    """sum of the log likelihood over sites and elements + log prior + log|J| = -U of compile_model's
    program at the matching unconstrained point, to 1e-9.  log prior + log|J| is float64 and
    independent of both compilers: the zoo's hand-written potential minus the torch.distributions
    log likelihood."""
    case = LC.CASES[name]()
    Z = case.points(S)
    samples = case.constrain(Z)
    loglik = sum(v.reshape(S, -1).sum(1) for v in _compile(case, samples).run_host(samples).values())
    ref_loglik = sum(v.reshape(S, -1).sum(1) for v in LC.reference64(case, samples).values())
    prior_and_jacobian = -case.potential64(Z) - ref_loglik
    U = compile_model(case.model, case.args).program.run_host(Z)[0]
    err = float((np.abs(loglik + prior_and_jacobian + U) / (1.0 + np.abs(U))).max())
    print(f"{name}: |loglik + log prior + log|J| + U| / (1 + |U|) = {err:.2e}")
    assert err <= 1e-9, (name, err)


# ---------------------------------------------------------------------------------- refusals
def test_a_latent_site_missing_from_the_samples_is_named():
    case = LC.CASES["robust8"]()
    samples = case.constrain(case.points(S))
    del samples["theta"]
    with pytest.raises(ValueError, match="'theta'"):
        _compile(case, samples)


def test_a_reparam_config_is_refused():
    def rp(y):
        t = numpyro.sample("t", dist.HalfCauchy(1.0))
        x = numpyro.sample("x", dist.Normal(np.zeros(3), t))
        numpyro.sample("y", dist.Normal(x, 1.0), obs=y)

    model = reparam(rp, config={"x": LocScaleReparam(0)})
    with pytest.raises(NotImplementedError, match="reparam"):
        compile_log_likelihood(model, (np.zeros(3),), {}, given=("t", "x", "x_decentered"))


def _hand_program(rows, num_slots, outputs):
    """dim = 4, eight zero constants; outputs: (slot, n, column)."""
    outs = []
    for j, (slot, n, column) in enumerate(outputs):
        from numpyro_amd.loglik_program import LogLikOutput
        outs.append(LogLikOutput(f"o{j}", slot, n, (n,), column))
    return LogLikProgram(rows, [0.0] * 8, [], num_slots, 4, [("z", 0, 4, (4,))], outs, {})


_TANH4 = [OPCODE["tanh"], 4, 0, 0, 4, 1, 0, 0]
_EXP4 = [OPCODE["exp"], 8, 4, 0, 4, 1, 0, 0]


def test_check_accepts_a_hand_program_and_runs_it_on_the_host():
    prog = _hand_program([_TANH4, _EXP4], 12, [(4, 4, 4), (8, 4, 0)])
    assert prog.native_check() == (0, "")
    z = np.linspace(-1, 1, 8).reshape(2, 4)
    out = prog.run_host({"z": z})
    np.testing.assert_allclose(out["o1"], np.exp(np.tanh(z)), rtol=1e-15)


def test_check_refuses_a_draw_op():
    draw = [native.DRAW_OPCODE["draw_normal"], 8, 0, 0, 4, 0, 0, 0]
    prog = _hand_program([_TANH4, draw], 12, [(8, 4, 0)])
    st, msg = prog.native_check()
    assert st != 0 and "draw" in msg and "op 1" in msg, (st, msg)


def test_check_refuses_overlapping_outputs():
    prog = _hand_program([_TANH4, _EXP4], 12, [(4, 4, 0), (8, 4, 3)])
    st, msg = prog.native_check(ldo=8)
    assert st != 0 and "overlap" in msg, (st, msg)


def test_check_refuses_a_column_past_ldo():
    prog = _hand_program([_TANH4, _EXP4], 12, [(4, 4, 0), (8, 4, 4)])
    assert prog.native_check(ldo=8) == (0, "")
    st, msg = prog.native_check(ldo=7)
    assert st != 0 and "output 1" in msg and "outside" in msg, (st, msg)
    st, msg = prog.native_check(outputs=[[4, 4, -1]], ldo=8)
    assert st != 0 and "output 0" in msg, (st, msg)


def test_check_refuses_an_output_outside_a_value():
    prog = _hand_program([_TANH4, _EXP4], 12, [(6, 4, 0)])  # straddles two values
    st, msg = prog.native_check()
    assert st != 0 and "output 0" in msg, (st, msg)


def test_compile_model_programs_are_unchanged():
    """The ops of compile_model for every zoo model, against the arrays recorded from the commit
    before the elementwise expansions were split off (tests/golden/compile_model_ops.json)."""
    import bounded_zoo as BZ
    import program_zoo as PZ
    import simplex_cases as SC

    gold = json.load(open(os.path.join(HERE, "golden", "compile_model_ops.json")))
    models = {}
    for zoo in (PZ.CASES, BZ.CASES):
        for n, make in zoo.items():
            c = make()
            models[n] = (c.model, c.args)
    for n, make in SC.MODELS.items():
        m = make()
        models[n] = (m.model, m.args)
    assert sorted(models) == sorted(gold)
    for n, (model, args) in models.items():
        ops = compile_model(model, args).program.ops
        assert ops.tolist() == gold[n], n


# ---------------------------------------------------------------------------------- lowering details
def test_constant_sites_scalar_values_and_constant_terms():
    """A site without a latent is a host constant; a scalar value under a site of 7 elements
    keeps one column; constant terms are part of the answer."""
    import torch
    import torch.distributions as td

    y7 = np.linspace(0.1, 0.9, 7)
    yc = np.array([0.5, -1.0, 2.0])

    def model(y7, yc, ys):
        hi = numpyro.sample("hi", dist.Exponential(1.0))
        numpyro.sample("y7", dist.Uniform(0.0, 1.0 + hi), obs=y7)
        numpyro.sample("yc", dist.Normal(0.5, 2.0), obs=yc)
        numpyro.sample("ys", dist.Normal(hi, 1.0), obs=ys)

    hi = np.array([0.3, 1.7, 4.0])
    prog = compile_log_likelihood(model, (y7, yc, 0.25), {}, given={"hi": hi})
    assert list(prog.constant_outputs) == ["yc"]
    by = {o.name: o for o in prog.outputs}
    assert (by["y7"].n, by["y7"].shape) == (1, (7,)) and (by["ys"].n, by["ys"].shape) == (1, ())
    assert prog.num_columns == 2 and prog.native_check() == (0, "")
    out = prog.run_host({"hi": hi})
    h = torch.as_tensor(hi)
    np.testing.assert_allclose(out["y7"], td.Uniform(0.0, 1.0 + h[:, None]).log_prob(torch.as_tensor(y7)).numpy(),
                               rtol=1e-12)
    half = torch.tensor(0.5, dtype=torch.float64)
    np.testing.assert_allclose(out["yc"], np.broadcast_to(td.Normal(half, 2.0).log_prob(torch.as_tensor(yc)).numpy(),
                                                          (3, 3)), rtol=1e-12)
    np.testing.assert_allclose(out["ys"], td.Normal(h, 1.0).log_prob(torch.as_tensor(0.25)).numpy(), rtol=1e-12)
    assert out["ys"].shape == (3,)


def test_observed_dirichlet_is_one_value():
    import torch
    import torch.distributions as td

    x = np.array([0.2, 0.5, 0.3])

    def model(x):
        s = numpyro.sample("s", dist.HalfNormal(2.0))
        numpyro.sample("x", dist.Dirichlet(0.5 + s * np.array([1.0, 2.0, 3.0])), obs=x)

    s = np.array([0.4, 1.1])
    prog = compile_log_likelihood(model, (x,), {}, given={"s": s})
    (o,) = prog.outputs
    assert (o.n, o.shape) == (1, ())
    ref = td.Dirichlet(0.5 + torch.as_tensor(s)[:, None] * torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64))
    np.testing.assert_allclose(prog.run_host({"s": s})["x"], ref.log_prob(torch.as_tensor(x)).numpy(), rtol=1e-12)


# ---------------------------------------------------------------------------------- public interface
def test_public_names():
    from numpyro_amd.diagnostics import lppd, waic  # noqa: F401
    from numpyro_amd.infer import log_likelihood, pointwise_predictive  # noqa: F401

    import numpyro_amd.infer as infer
    assert "log_likelihood" in infer.__all__ and "pointwise_predictive" in infer.__all__


def test_interface_errors_need_no_gpu():
    from numpyro_amd.infer import log_likelihood

    case = LC.CASES["robust8"]()
    samples = case.samples(4)
    with pytest.raises(ValueError, match="Batch shapes at site"):
        log_likelihood(case.model, {**samples, "mu": samples["mu"][:3]}, *case.args)
    with pytest.raises(ValueError, match="batch_ndims"):
        log_likelihood(case.model, samples, *case.args, batch_ndims=3)
    with pytest.raises(ValueError, match="No sample sites"):
        log_likelihood(case.model, {}, *case.args)


def test_fused_model_objects_are_refused():
    import numpyro_amd.potentials as P
    from numpyro_amd.infer import log_likelihood, pointwise_predictive

    for fn in (log_likelihood, pointwise_predictive):
        with pytest.raises(NotImplementedError, match="FusedModel"):
            fn(P.eight_schools, {"theta": np.zeros((3, 8))}, 8, np.ones(8), np.zeros(8))


def test_all_constant_model_runs_without_a_gpu():
    """Every output a host constant: no program, no device."""
    import torch
    import torch.distributions as td

    from numpyro_amd.infer import log_likelihood, pointwise_predictive

    y = np.array([0.5, -1.0, 2.0])

    def model(y):
        numpyro.sample("free", dist.Normal(0.0, 1.0))
        numpyro.sample("y", dist.Normal(0.5, 2.0), obs=y)

    samples = {"free": np.zeros((2, 3))}
    ref = td.Normal(torch.tensor(0.5, dtype=torch.float64), 2.0).log_prob(torch.as_tensor(y)).float()
    ll = log_likelihood(model, samples, y, batch_ndims=2)["y"]
    assert tuple(ll.shape) == (2, 3, 3) and ll.dtype == torch.float32
    assert torch.equal(ll.cpu(), ref.expand(2, 3, 3))
    pw = pointwise_predictive(model, samples, y, batch_ndims=2)["y"]
    assert torch.equal(pw["lppd"].cpu(), ref) and torch.equal(pw["p_waic"].cpu(), torch.zeros(3))
