"""Predictive programs without a GPU (numpyro_amd/predictive_program.py): what compile_predictive
emits, the host checks of both program kinds, the refusals, and the float64 host interpreter --
which defines every draw op -- against the oracle's predictive draws and the distributions'
analytic moments."""
import ctypes

import numpy as np
import pytest
import torch

import numpyro_amd as numpyro
import predictive_cases as PC
import program_zoo as Zoo
from numpyro_amd import distributions as dist
from numpyro_amd import jnp, native
from numpyro_amd.frontend import LocScaleReparam, reparam
from numpyro_amd.infer import Predictive
from numpyro_amd.jnp import Sym
from numpyro_amd.predictive_program import compile_predictive
from numpyro_amd.program import compile_model
from oracle import predictive as OPred

DRAWS = {"robust8": ["draw_normal", "draw_gamma"], "poisson": ["draw_poisson"], "treg": ["draw_normal", "draw_gamma"],
         "logit": ["draw_bernoulli"], "edge": ["draw_normal", "draw_normal"]}
OUT_SHAPES = {"robust8": {"obs": (8,)}, "poisson": {"y": (40,)}, "treg": {"y": (30,)}, "logit": {"y": (25,)},
              "edge": {"y1": (1,), "y2": (3,)}}


def _compiled(name, given=None):
    case = Zoo.CASES[name]()
    given = [n for n, _, _ in case.sites] if given is None else given
    return case, compile_predictive(case.model, PC.unobserved_args(case), {}, given)


# ------------------------------------------------------------------ 1: what the compiler emits
@pytest.mark.parametrize("name", sorted(Zoo.CASES))
def test_zoo_models_compile_to_draws_of_their_observed_sites(name):
    case, prog = _compiled(name)
    # inputs: the given sites in sorted order, packed, with their shapes
    assert [(n, s) for n, _, _, s in prog.inputs] == [(n, tuple(s)) for n, s, _ in case.sites]
    offs = np.cumsum([0] + [k for _, _, k, _ in prog.inputs])
    assert [o for _, o, _, _ in prog.inputs] == offs[:-1].tolist() and prog.dim == offs[-1] == case.dim
    assert [n for n in prog.op_names() if n.startswith("draw_")] == DRAWS[name]
    assert {o.name: o.shape for o in prog.outputs} == OUT_SHAPES[name]
    assert {o.name: o.integer for o in prog.outputs} == {n: name in ("poisson", "logit") for n in OUT_SHAPES[name]}
    for name_, slot, n, shape, integer in prog.outputs:  # (name, slot, n, shape, integer?)
        assert prog.dim <= slot and slot + n <= prog.num_slots and n == int(np.prod(shape))
    # stream ids are the draws' ordinals
    assert [o[7] for o in prog.ops.tolist() if o[0] >= native.DRAW_BASE] == list(range(prog.num_draws))
    assert prog.native_check() == (0, "")
    assert not prog.observed and not prog.host_deterministics


def test_data_passed_leaves_no_draw_for_that_site():
    case = Zoo.CASES["edge"]()
    M1, idx1, y1, y2 = case.args
    prog = compile_predictive(case.model, (M1, idx1, y1, None), {}, [n for n, _, _ in case.sites])
    assert [o.name for o in prog.outputs] == ["y2"] and prog.num_draws == 1
    assert set(prog.observed) == {"y1"} and np.array_equal(prog.observed["y1"][0], y1)
    prog = compile_predictive(case.model, case.args, {}, [n for n, _, _ in case.sites])
    assert prog.num_ops == 0 and not prog.outputs and set(prog.observed) == {"y1", "y2"}


def test_sites_not_given_are_drawn_in_dependency_order():
    case, prog = _compiled("robust8", given=[])
    assert prog.dim == 0 and not prog.inputs
    assert [o.name for o in prog.outputs] == ["mu", "tau", "theta", "obs"]
    assert [n for n in prog.op_names() if n.startswith("draw_")] == \
        ["draw_normal", "draw_cauchy", "draw_normal", "draw_normal", "draw_gamma"]
    assert [o.streams for o in prog.outputs] == [(0,), (1,), (2,), (3, 4)]
    assert prog.native_check() == (0, "")
    # a subset: tau given, the rest drawn; keys that are no sample sites are not inputs
    prog = compile_predictive(case.model, PC.unobserved_args(case), {}, ["tau", "not_a_site"])
    assert [n for n, _, _, _ in prog.inputs] == ["tau"] and [o.name for o in prog.outputs] == ["mu", "theta", "obs"]


def test_deterministic_sites_follow_what_they_depend_on():
    def model(X):
        b = numpyro.sample("b", dist.Normal(np.zeros(3), np.ones(3)))
        eta = numpyro.deterministic("eta", jnp.matmul(X, b))
        y = numpyro.sample("y", dist.Normal(eta, 0.5))
        numpyro.deterministic("total", jnp.sum(y))

    X = np.random.RandomState(0).randn(6, 3)
    prog = compile_predictive(model, (X,), {}, ["b", "eta"])  # a deterministic site's key is no input
    assert [n for n, _, _, _ in prog.inputs] == ["b"]
    assert [(o.name, o.shape, o.streams) for o in prog.outputs] == [("y", (6,), (0,)), ("total", (), ())]
    assert set(prog.host_deterministics) == {"eta"}
    b = np.random.RandomState(1).randn(4, 3)
    out = prog.run_host({"b": b}, 5, PC.words)
    np.testing.assert_allclose(out["total"], out["y"].sum(1), rtol=1e-12)
    prior = compile_predictive(model, (X,), {}, [])
    assert [o.name for o in prior.outputs] == ["b", "y", "eta", "total"] and not prior.host_deterministics


# ------------------------------------------------------------------ 2: the host checks
def test_potential_program_check_refuses_a_draw_opcode():
    case = Zoo.CASES["poisson"]()
    prog = compile_model(case.model, case.args).program
    ops = prog.ops.copy()
    k = [native.OPCODES[o] for o in ops[:, 0]].index("exp")
    ops[k, 0] = native.DRAW_OPCODE["draw_exponential"]
    lib = native.lib()
    assert lib.nmx_program_check(ctypes.byref(prog.native_struct(ops=ops))) == 1
    assert lib.nmx_last_error().decode().startswith(f"op {k}: bad opcode")
    # ... and a predictive program (no U, draw ops) is no potential program
    _, pred = _compiled("poisson")
    assert lib.nmx_program_check(ctypes.byref(pred.native_struct())) == 1


def _tampered(which):
    _, prog = _compiled("treg")
    ops, outputs = prog.ops.copy(), prog.output_table()
    names = prog.op_names()
    k = {"opcode": 4, "draw_opcode": names.index("draw_gamma"), "slot": names.index("sqrt"),
         "parameter": names.index("draw_gamma"), "constant": names.index("draw_gamma") + 1, "count": names.index("div"),
         "draw_count": names.index("draw_normal"), "stream": names.index("draw_gamma"), "stride": names.index("draw_gamma"),
         "output": None, "output_straddles": None}[which]
    if which == "opcode":
        ops[k, 0] = len(native.OPCODES)
    elif which == "draw_opcode":
        ops[k, 0] = native.DRAW_BASE + len(native.DRAW_OPCODES)
    elif which in ("slot", "parameter"):
        ops[k, 2] = prog.num_slots + 5
    elif which == "constant":
        assert names[k] == "mul" and ops[k, 2] < 0
        ops[k, 2] = ~(prog.consts.size + 3)
    elif which == "count":
        ops[k, 4] = 0
    elif which == "draw_count":
        ops[k, 4] = -3
    elif which == "stream":
        ops[k, 7] = 5
    elif which == "stride":
        ops[k, 5] = 2
    elif which == "output":
        outputs[0, 0] = prog.num_slots - 1  # n slots from the last one: past the tape
    else:
        outputs[0, 0] -= 1  # ends inside y, starts in the value before it
    return prog, prog.native_struct(ops=ops), outputs, k, ops


@pytest.mark.parametrize("which", ["opcode", "draw_opcode", "slot", "parameter", "constant", "count", "draw_count",
                                   "stream", "stride", "output", "output_straddles"])
def test_predict_program_check_names_the_bad_op(which):
    prog, bad, outputs, k, keep = _tampered(which)
    assert prog.native_check() == (0, "")
    lib = native.lib()
    st = lib.nmx_predict_program_check(ctypes.byref(bad), int(outputs.ctypes.data), outputs.shape[0])
    assert st == 1  # NMX_ERR_INVALID
    msg = lib.nmx_last_error().decode()
    if which.startswith("output"):
        assert msg.startswith("output 0") and "defined" in msg, msg
    else:
        assert msg.startswith(f"op {k}"), msg
        word = {"draw_opcode": "opcode", "parameter": "parameter", "draw_count": "count"}.get(which, which)
        assert word.replace("slot", "slot") in msg, msg


def test_predict_program_check_accepts_given_sites_as_outputs_and_no_inputs():
    _, prog = _compiled("logit")
    assert prog.native_check(outputs=[[0, 4], [4, 1], [prog.outputs[0].slot + 3, 2]]) == (0, "")
    st, msg = prog.native_check(outputs=[[3, 2]])  # across two given sites is inside z: allowed; past z is not
    assert st == 0
    st, msg = prog.native_check(outputs=[[4, 2]])
    assert st == 1 and msg.startswith("output 0")
    _, prior = _compiled("robust8", given=[])
    assert prior.dim == 0 and prior.native_check() == (0, "")
    assert native.lib().nmx_predict_program_workspace_bytes(prior.num_slots, 5) == 5 * prior.num_slots * 4


# ------------------------------------------------------------------ 3: refusals
def _refused_models():
    def rank2():
        numpyro.sample("w", dist.Normal(np.zeros((2, 2)), np.ones((2, 2))))

    def rank2_observed():
        w = numpyro.sample("w", dist.Normal(np.zeros(2), np.ones(2)))
        numpyro.sample("y", dist.Normal(jnp.sum(w), 1.0), obs=np.zeros((4, 2)))

    def grw():
        s = numpyro.sample("s", dist.Exponential(1.0))
        numpyro.sample("walk", dist.GaussianRandomWalk(s, 4))

    def mvn():
        m = numpyro.sample("m", dist.Normal(np.zeros(2), np.ones(2)))
        numpyro.sample("v", dist.MultivariateNormal(m, covariance_matrix=np.eye(2)))

    class Beta(dist.Distribution):
        support = "unit_interval"

        def __init__(self, a, b):
            super().__init__(())
            self.a, self.b = a, b

    def outside_table():
        p = numpyro.sample("p", Beta(2.0, 2.0))
        numpyro.sample("y", dist.Bernoulli(probs=p))

    def bad_op():
        x = numpyro.sample("x", dist.Normal(np.zeros(4), np.ones(4)))
        numpyro.sample("y", dist.Normal(Sym("erf", (x,), (4,)), 1.0))

    def mismatched():
        x = numpyro.sample("x", dist.Normal(np.zeros(4), np.ones(4)))
        with numpyro.plate("n", 4):
            numpyro.sample("y", dist.Normal(x[:2], 1.0))

    def rp():
        t = numpyro.sample("t", dist.HalfCauchy(1.0))
        numpyro.sample("x", dist.Normal(np.zeros(3), t))

    return {"rank2": ("w", rank2), "rank2_observed": ("y", rank2_observed), "random_walk": ("walk", grw),
            "mvn": ("v", mvn), "outside_table": ("p", outside_table), "bad_op": ("y", bad_op),
            "reparam": ("x", reparam(rp, config={"x": LocScaleReparam(0)}))}


@pytest.mark.parametrize("case", sorted(_refused_models()))
def test_out_of_class_models_are_refused_naming_the_site(case):
    site, model = _refused_models()[case]
    with pytest.raises(NotImplementedError, match=f"site '{site}'"):
        compile_predictive(model)
    # Predictive surfaces the refusal when it is called (before it needs a device)
    with pytest.raises(NotImplementedError, match=f"site '{site}'"):
        Predictive(model, num_samples=3)(0)


def test_a_drawn_site_above_the_counter_field_is_refused():
    def big():
        with numpyro.plate("n", (1 << 24) + 1):
            numpyro.sample("y", dist.Normal(0.0, 1.0))

    with pytest.raises(NotImplementedError, match="site 'y'.*2\\^24"):
        compile_predictive(big)


def test_predictive_argument_errors_of_the_program_path():
    model = Zoo.robust8_model
    with pytest.raises(ValueError):
        Predictive(model)  # neither posterior samples nor num_samples
    with pytest.raises(ValueError):
        Predictive(model, {"mu": torch.zeros(3)}, guide=lambda: None)
    with pytest.raises(NotImplementedError):
        Predictive(model, {"mu": torch.zeros(3)}, infer_discrete=True)
    with pytest.raises(ValueError, match="Batch shapes"):
        Predictive(model, {"mu": torch.zeros(3), "theta": torch.zeros(4, 8)})
    with pytest.raises(ValueError):
        Predictive(model, {})  # nothing to infer num_samples from
    with pytest.raises(ValueError):
        Predictive(model, num_samples=0)
    with pytest.raises(NotImplementedError):
        Predictive("not a model", {"mu": torch.zeros(3)})
    with pytest.warns(UserWarning):
        p = Predictive(model, {"mu": torch.zeros(5)}, num_samples=7)
    assert p.num_samples == 5
    p = Predictive(model, {"theta": torch.zeros(2, 5, 8)}, batch_ndims=2)
    assert p.num_samples == 10 and p._batch_shape == (2, 5)
    p = Predictive(model, num_samples=6)
    assert p.num_samples == 6 and p._batch_shape == (6,)
    # a given site of the wrong shape is reported by name at the call
    with pytest.raises(ValueError, match="theta"):
        Predictive(model, {"theta": torch.zeros(4, 7)})(0, 8, np.ones(8))
    # everything given or observed: nothing is drawn, no device is needed
    case = Zoo.CASES["logit"]()
    given = {k: torch.from_numpy(v) for k, v in PC.posterior_like(case, 3).items()}
    out = Predictive(case.model, given)(0, *case.args)
    assert set(out) == {"y"} and out["y"].dtype == torch.int32
    assert np.array_equal(out["y"].cpu().numpy(), np.broadcast_to(case.args[1].astype(np.int32), (3, 25)))


# ------------------------------------------------------------------ 4: the host interpreter
def test_run_host_normal_site_is_the_oracles_predict_normal():
    sigma = np.asarray(numpyro.datasets.EIGHT_SCHOOLS_SIGMA, np.float64)
    rs = np.random.RandomState(4)
    samples = {"mu": rs.randn(40), "tau": np.abs(rs.randn(40)) + 0.1, "theta": 3 * rs.randn(40, 8)}
    prog = compile_predictive(PC.eight_schools_model, (8, sigma), {}, samples)
    out = prog.run_host(samples, 11, PC.words)
    assert set(out) == {"obs"}
    # the oracle rounds its float64 Box-Muller normal to float32: a relative 2^-24 of sigma z
    ref = OPred.predict_normal(samples["theta"], sigma, 11)
    np.testing.assert_allclose(out["obs"], ref, rtol=0, atol=6 * sigma.max() * 2.0 ** -24)
    # observed passthrough: with data there is nothing to run
    with_y = compile_predictive(PC.eight_schools_model, (8, sigma, np.arange(8.0)), {}, samples)
    assert with_y.num_ops == 0 and np.array_equal(with_y.observed["obs"][0], np.arange(8.0))


@pytest.mark.parametrize("N", [25, 65])
def test_run_host_logit_is_the_oracles_predict_logreg(N):
    case = Zoo.logit(N=N)
    samples = PC.posterior_like(case, 40, seed=N)
    prog = compile_predictive(case.model, PC.unobserved_args(case), {}, samples)
    X1 = np.concatenate([np.ones((N, 1)), case.args[0]], 1)
    coefs = np.concatenate([samples["b0"][:, None], samples["b"]], 1).astype(np.float64)
    ref, p, u = OPred.predict_logreg(X1, coefs, 9)
    out = prog.run_host(samples, 9, PC.words)["y"]
    assert np.array_equal(out, ref)
    # the float32 run stays within the device test's rule for this seed: mismatches only where u ~ p
    out32 = prog.run_host(samples, 9, PC.words, dtype=np.float32)["y"]
    mismatch = out32 != ref
    assert mismatch.mean() <= 1e-3 and np.all(np.abs(u[mismatch] - p[mismatch]) < 1e-5)


def test_run_host_depends_on_the_global_sample_index_only():
    case, prog = _compiled("poisson")
    samples = PC.posterior_like(case, 6)
    whole = prog.run_host(samples, 2, PC.words)["y"]
    tail = prog.run_host({k: v[4:] for k, v in samples.items()}, 2, PC.words, sample_offset=4)["y"]
    assert np.array_equal(whole[4:], tail)
    # batch_ndims = 2 is the flattened call: [2, 3] draws are samples 0..5
    assert np.array_equal(prog.run_host(prog.flatten_inputs(samples).reshape(6, -1), 2, PC.words)["y"], whole)


def test_run_host_prior_predictive_feeds_drawn_sites_forward():
    case, prog = _compiled("robust8", given=[])
    info = {}
    out = prog.run_host(5, 3, PC.words, info=info)
    assert [k for k in out] == ["mu", "tau", "theta", "obs"]
    assert out["mu"].shape == (5,) and out["tau"].shape == (5,) and out["theta"].shape == (5, 8)
    assert np.all(out["tau"] > 0) and sorted(info) == [0, 1, 2, 3, 4]
    # theta = mu + tau z with z the normals of stream 2: the drawn mu and tau parameterise theta
    w = PC.words(3, np.arange(5)[:, None], 2, np.arange(8)[None, :], 0)
    from oracle import philox
    z = np.sqrt(-2 * np.log(philox.u01_open0(w[..., 0]).astype(np.float64))) * \
        np.cos(6.283185307179586 * philox.u01(w[..., 1]).astype(np.float64))
    np.testing.assert_allclose(out["theta"], out["mu"][:, None] + out["tau"][:, None] * z, rtol=1e-12)
    # given tau instead: the same mu (its stream and sample are unchanged), another theta
    sub = compile_predictive(case.model, PC.unobserved_args(case), {}, ["tau"])
    o2 = sub.run_host({"tau": np.full(5, 2.0)}, 3, PC.words)
    assert np.array_equal(o2["mu"], out["mu"])


def test_out_of_support_parameters_give_nan_without_looping():
    def model():
        c = numpyro.sample("c", dist.HalfNormal(1.0))
        with numpyro.plate("n", 3):
            numpyro.sample("g", dist.Gamma(c, 2.0))
            numpyro.sample("k", dist.Poisson(c * 20.0))
            numpyro.sample("k_small", dist.Poisson(c))
            numpyro.sample("b", dist.Bernoulli(probs=c))

    prog = compile_predictive(model, (), {}, ["c"])
    info = {}
    out = prog.run_host({"c": np.array([0.5, -1.0, np.nan, np.inf, 0.0, 2.0 ** 24, 2.0 ** 24 - 1])}, 1, PC.words,
                        info=info)
    for name in ("g", "k", "k_small", "b"):
        assert np.all(np.isfinite(out[name][0])), name
        assert np.all(np.isnan(out[name][1:4])), name  # negative, NaN, infinite
    assert np.all(np.isnan(out["g"][4])) and np.all(out["k"][4] == 0) and np.all(out["b"][4] == 0)
    # NMX_POISSON_MAX_RATE: a rate of 2^24 or more is refused before any loop, the rate below it is drawn
    (stream,) = [o for o in prog.outputs if o.name == "k_small"][0].streams
    assert np.all(np.isnan(out["k"][5:])) and np.all(np.isnan(out["k_small"][5])) and np.all(info[stream][5] == -1)
    assert np.all(np.isfinite(out["k_small"][6])) and np.all(np.abs(out["k_small"][6] - 2.0 ** 24) < 6 * 2.0 ** 12)
    with pytest.raises(NotImplementedError, match="site 'k'.*rate"):
        compile_predictive(lambda: numpyro.sample("k", dist.Poisson(2.0 ** 24)), (), {}, [])


@pytest.fixture(scope="module")
def moment_draws():
    prog = compile_predictive(PC.moments_model)
    assert prog.dim == 0 and prog.native_check() == (0, "")
    return prog.run_host(PC.MOMENT_SAMPLES, 17, PC.words)


def test_host_interpreter_draws_have_the_distributions_moments(moment_draws):
    PC.check_moments(moment_draws)
    for name in ("poisson_inversion", "poisson_ptrs", "bernoulli", "bernoulli_logits"):
        assert np.array_equal(moment_draws[name], np.round(moment_draws[name])) and moment_draws[name].min() >= 0
