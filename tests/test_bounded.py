"""Bounded-support latents and Binomial likelihoods without a GPU: the program compiler on the
cases of tests/bounded_zoo.py against their hand-written float64 potentials, the stable forms of
the sigmoid sites, the refusals, Potential.constrain, the new draw programs on the float64 host
interpreter (moments, a chi-square against the Binomial pmf, guards, loop bounds) and the host
check of a two-operand draw op."""
import ctypes
import functools
import math

import numpy as np
import pytest
import scipy.stats
import torch

import bounded_zoo as BZ
import numpyro_amd as numpyro
import predictive_cases as PC
from numpyro_amd import distributions as dist
from numpyro_amd import jnp, native
from numpyro_amd.potentials import LOWER, POSITIVE, REAL, UNIT, Potential
from numpyro_amd.predictive_program import compile_predictive
from numpyro_amd.program import ProgramPotential, compile_model

# the kernel tests' tolerances (tests/test_gpu_program.py)
U_TOL = dict(rtol=1e-5, atol=1e-4)
G_TOL = dict(rtol=1e-4, atol=1e-4)


@functools.lru_cache(maxsize=None)
def _compiled(name):
    case = BZ.CASES[name]()
    return case, compile_model(case.model, case.args)


# ------------------------------------------------------------------ 1: the compiler against float64
@pytest.mark.parametrize("name", sorted(BZ.CASES))
def test_zoo_case_compiles_and_matches_the_hand_written_potential(name):
    case, pot = _compiled(name)
    assert isinstance(pot, ProgramPotential) and pot.sites == [(n, tuple(s), c) for n, s, c in case.sites]
    assert set(pot.affine) == set(BZ.AFFINE[name])
    for site, (lo, width) in BZ.AFFINE[name].items():
        assert float(pot.affine[site][0]) == lo and float(pot.affine[site][1]) == width
    assert pot.program.native_check() == (0, "")
    Z = np.random.RandomState(1).uniform(-2, 2, (64, case.dim))
    U, G = pot.program.run_host(Z)
    U64, G64 = case.pe_grad64(Z)
    np.testing.assert_allclose(U, U64, rtol=1e-9)
    np.testing.assert_allclose(G, G64, rtol=1e-9, atol=1e-9)
    # central differences of the interpreter's own U
    h = 1e-5
    for d in range(case.dim):
        e = np.zeros(case.dim)
        e[d] = h
        num = (pot.program.run_host(Z[:8] + e)[0] - pot.program.run_host(Z[:8] - e)[0]) / (2 * h)
        np.testing.assert_allclose(G[:8, d], num, rtol=1e-6, atol=1e-6)


# ------------------------------------------------------------------ 2: the stable forms
@pytest.mark.parametrize("name", [n for n in sorted(BZ.CASES) if any(c == UNIT for _, _, c in BZ.CASES[n]().sites)])
def test_unit_sites_stay_finite_and_accurate_far_out(name):
    """u = -30 ... 30 on every unit site: with the constants the device holds (float32) the
    program is finite and within the kernel tests' tolerances of the float64 one."""
    case, pot = _compiled(name)
    Z = BZ.edge_rows(case)
    assert Z.shape[0] == len(BZ.EDGE_U) * sum(c == UNIT for _, _, c in case.sites)
    U32, G32 = pot.program.run_host(Z, f32_consts=True)
    U64, G64 = pot.program.run_host(Z)
    assert np.all(np.isfinite(U32)) and np.all(np.isfinite(G32))
    print(name, "max |dU|", np.abs(U32 - U64).max(), "max |dG|", np.abs(G32 - G64).max())
    np.testing.assert_allclose(U32, U64, **U_TOL)
    np.testing.assert_allclose(G32, G64, **G_TOL)
    # and the float64 one is the hand-written potential there too (its logsigmoid forms are stable)
    Uh, Gh = case.pe_grad64(Z)
    np.testing.assert_allclose(U64, Uh, rtol=1e-9)
    np.testing.assert_allclose(G64, Gh, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("name", ["fully_pooled", "not_pooled", "partially_pooled"])
def test_binomial_probs_of_a_unit_site_forms_no_log1p_of_its_exp(name):
    """log(p) is the site's log x and log1p(-p) its log(1 - x): no log, and no log1p of the
    negated value, is taken of the exp that makes the site's value."""
    _, pot = _compiled(name)
    ops = pot.program.ops.tolist()
    names = [native.OPCODES[o[0]] for o in ops]
    made = {o[1]: k for k, o in enumerate(ops)}

    def producer(slot):
        return names[made[slot]] if slot in made else None

    for k, o in enumerate(ops):
        if names[k] == "log1p":
            assert not (producer(o[2]) == "neg" and producer(ops[made[o[2]]][2]) == "exp"), pot.program.describe()
        if names[k] == "log":
            assert producer(o[2]) != "exp", pot.program.describe()
    if name != "partially_pooled":
        assert "log1p" not in names and "log" not in names


# ------------------------------------------------------------------ 3: refusals
class _MyUnit(dist.Distribution):
    support = "unit_interval"


def _refused(model, args, match):
    with pytest.raises(NotImplementedError, match=match):
        compile_model(model, args)


def test_refusals_name_the_site():
    def user_class():
        numpyro.sample("w", _MyUnit())

    _refused(user_class, (), "site 'w'.*_MyUnit is not supported")

    def latent_bound():
        hi = numpyro.sample("hi", dist.Exponential(1.0))
        numpyro.sample("x", dist.Uniform(0.0, hi + 1.0))

    _refused(latent_bound, (), "site 'x'.*bound.*latent")

    def latent_scale_bound():
        lo = numpyro.sample("lo", dist.Exponential(1.0))
        numpyro.sample("k", dist.Pareto(lo, 2.0))

    _refused(latent_scale_bound, (), "site 'k'.*bound.*latent")

    def latent_count(y):
        n = numpyro.sample("n", dist.Exponential(0.1))
        numpyro.sample("y", dist.Binomial(n, probs=0.5), obs=y)

    _refused(latent_count, (np.array([1.0, 2.0]),), "site 'y'.*total_count")

    def latent_binomial():
        numpyro.sample("k", dist.Binomial(10, probs=0.5))

    _refused(latent_binomial, (), "site 'k'.*BinomialProbs is not supported as a latent site")
    with pytest.raises(ValueError):
        dist.Binomial(10)
    assert isinstance(dist.Binomial(10, logits=0.0), dist.BinomialLogits)
    # a constant total_count that float32 cannot count is refused where it would be drawn
    with pytest.raises(NotImplementedError, match="site 'k'.*total_count"):
        compile_predictive(lambda: numpyro.sample("k", dist.Binomial(2.0 ** 24, probs=0.5)), (), {}, [])


# ------------------------------------------------------------------ 4: the constrain helper
class _FourCodes(Potential):
    sites = [("a", (3,), REAL), ("b", (), POSITIVE), ("c", (2,), UNIT), ("d", (2,), UNIT), ("e", (), LOWER),
             ("f", (2,), LOWER)]
    dim = 11
    affine = {"d": (np.array([0.5, -1.0]), np.array([5.5, 2.0])), "f": (np.float64(2.0), np.float64(1.0))}


def test_constrain_matches_the_closed_forms_for_every_code():
    pot = _FourCodes()
    z = torch.from_numpy(np.random.RandomState(0).uniform(-3, 3, (4, 5, 11)))
    z[0, 0, 4:8] = torch.tensor([-40.0, 40.0, -800.0, 800.0], dtype=z.dtype)  # c and d: the stable sigmoid
    sites = pot.unflatten(z)
    assert {k: tuple(v.shape) for k, v in sites.items()} == {"a": (4, 5, 3), "b": (4, 5), "c": (4, 5, 2),
                                                             "d": (4, 5, 2), "e": (4, 5), "f": (4, 5, 2)}
    sig = lambda u: np.where(u >= 0, 1 / (1 + np.exp(-np.abs(u))), np.exp(-np.abs(u)) / (1 + np.exp(-np.abs(u))))  # noqa: E731
    n = {k: v.numpy() for k, v in sites.items()}
    want = {"a": n["a"], "b": np.exp(n["b"]), "c": sig(n["c"]),
            "d": np.array([0.5, -1.0]) + np.array([5.5, 2.0]) * sig(n["d"]), "e": np.exp(n["e"]),
            "f": 2.0 + np.exp(n["f"])}
    # from all-unconstrained values (MCMC's host-side branch, HMC.postprocess_fn)
    out = pot.constrain(sites)
    assert list(out) == [s[0] for s in pot.sites]
    for k in want:
        np.testing.assert_allclose(out[k].numpy(), want[k], rtol=1e-13, atol=0, err_msg=k)
    assert np.all(np.isfinite(out["d"].numpy())) and out["d"][0, 0, 0] == 0.5 and out["d"][0, 0, 1] == 1.0
    # after the device collection, which has mapped the POSITIVE coordinates through exp already
    dev = dict(sites, b=torch.exp(sites["b"]))
    out = pot.constrain(dev, device_exp=True)
    for k in want:
        np.testing.assert_allclose(out[k].numpy(), want[k], rtol=1e-13, atol=0, err_msg=k)
    # flatten / unflatten stay maps of unconstrained values
    flat = pot.flatten({k: v.reshape(20, *v.shape[2:]) for k, v in sites.items()})
    assert flat.shape == (20, 11) and torch.equal(flat, z.reshape(20, 11).to(torch.float32))
    back = pot.unflatten(flat)
    assert all(torch.equal(back[k], sites[k].reshape(20, *sites[k].shape[2:]).to(torch.float32)) for k in sites)


def test_existing_potentials_carry_no_affine_part():
    from numpyro_amd.potentials import EightSchools

    pot = EightSchools(8, np.ones(8), np.zeros(8))
    assert pot.affine == {}
    out = pot.constrain(pot.unflatten(torch.zeros(2, 10)))
    assert float(out["tau"][0]) == 1.0 and float(out["mu"][0]) == 0.0


def test_expit_symbol_host_form_and_lowering():
    x = np.array([-800.0, -2.0, 0.0, 3.0, 800.0])
    np.testing.assert_allclose(jnp.expit(x), [0.0, 1 / (1 + math.exp(2.0)), 0.5, 1 / (1 + math.exp(-3.0)), 1.0], rtol=1e-15)

    def model(y):
        a = numpyro.sample("a", dist.Normal(0.0, 1.5))
        p = numpyro.deterministic("p", jnp.expit(a))
        numpyro.sample("y", dist.Binomial(12, probs=p), obs=y)

    pot = compile_model(model, (np.array([3.0, 5.0]),))
    names = [native.OPCODES[o] for o in pot.program.ops[:, 0]]
    assert "log" not in names and names.count("softplus") >= 1  # log(expit(a)) folds to -softplus(-a)
    a = torch.tensor([[-1.0], [0.5]], dtype=torch.float64)
    Z = a.numpy()
    lp = (scipy.stats.binom.logpmf([3.0, 5.0], 12, 1 / (1 + np.exp(-Z))).sum(1) + scipy.stats.norm.logpdf(Z[:, 0], 0, 1.5))
    np.testing.assert_allclose(pot.program.run_host(Z)[0], -lp, rtol=1e-12)
    det = pot.deterministic({"a": a[:, 0].to(torch.float32)})
    np.testing.assert_allclose(det["p"].numpy(), 1 / (1 + np.exp(-Z[:, 0])), rtol=1e-6)


# ------------------------------------------------------------------ 5: draw programs on the host
def test_draw_programs_streams_and_integer_sites():
    prog = compile_predictive(BZ.partially_pooled, (BZ.AT_BATS,), {}, [])
    assert [o.name for o in prog.outputs] == ["m", "kappa", "phi", "obs"]
    assert [n for n in prog.op_names() if n.startswith("draw_")] == \
        ["draw_uniform", "draw_exponential", "draw_gamma", "draw_gamma", "draw_binomial"]
    assert [o.streams for o in prog.outputs] == [(0,), (1,), (2, 3), (4,)]  # Beta takes two streams
    assert [o[7] for o in prog.ops.tolist() if o[0] >= native.DRAW_BASE] == list(range(5))
    assert [o.integer for o in prog.outputs] == [False, False, False, True]
    assert prog.native_check() == (0, "")
    # bounded sites given are inputs as constrained values
    post = compile_predictive(BZ.partially_pooled, (BZ.AT_BATS,), {}, ["m", "kappa", "phi"])
    assert [n for n, _, _, _ in post.inputs] == ["kappa", "m", "phi"] and post.op_names() == ["draw_binomial"]
    logit = compile_predictive(BZ.partially_pooled_with_logit, (BZ.AT_BATS,), {}, ["alpha", "loc", "scale"])
    assert logit.op_names()[-1] == "draw_binomial" and logit.outputs[0].integer and logit.native_check() == (0, "")


BINOMIAL_CASES = [(1, 0.3), (20, 0.2), (20, 0.8), (40, 0.24), (40, 0.26), (1000, 0.5), (100000, 0.001)]
_COUNTER_SAMPLES = 196  # x 512 elements: 1e5 draws per case; the first 64 rows are the moment rule's draws


def _moments_model():
    with numpyro.plate("n", PC.MOMENT_ELEMENTS):
        numpyro.sample("uniform", dist.Uniform(-1.0, 3.0))
        numpyro.sample("pareto", dist.Pareto(2.0, 10.0))
        numpyro.sample("beta", dist.Beta(2.0, 3.0))
        numpyro.sample("beta_below1", dist.Beta(0.5, 0.7))
        for k, (n, p) in enumerate(BINOMIAL_CASES):
            numpyro.sample(f"binomial{k}", dist.Binomial(n, probs=p))
        numpyro.sample("binomial_logits", dist.Binomial(20, logits=math.log(0.2 / 0.8)))


@functools.lru_cache(maxsize=None)
def _moment_draws():
    prog = compile_predictive(_moments_model, (), {}, [])
    info = {}
    out = prog.run_host(_COUNTER_SAMPLES, 23, PC.words, info=info)
    return prog, out, info


def _beta_raw(a, b, k):
    return math.prod((a + r) / (a + b + r) for r in range(k))


def _analytic():
    """site -> (mean, variance, fourth central moment)."""
    out = {"uniform": (1.0, 16.0 / 12, 256.0 / 80)}
    s, al = 2.0, 10.0
    raw = [al * s ** k / (al - k) for k in range(1, 5)]
    out["pareto"] = (raw[0], raw[1] - raw[0] ** 2, PC._central4(*raw))
    for name, a, b in (("beta", 2.0, 3.0), ("beta_below1", 0.5, 0.7)):
        raw = [_beta_raw(a, b, k) for k in range(1, 5)]
        out[name] = (raw[0], raw[1] - raw[0] ** 2, PC._central4(*raw))
    for k, (n, p) in list(enumerate(BINOMIAL_CASES)) + [("_logits", (20, 0.2))]:
        v = n * p * (1 - p)
        out[f"binomial{k}"] = (n * p, v, v * (1 + 3 * (n - 2) * p * (1 - p)))
    return out


def test_host_draws_have_the_distributions_moments():
    """The existing moment rule (predictive_cases.check_moments): mean and variance within 5
    standard errors, the variance's from the fourth central moment, over 64 x 512 draws."""
    _, out, _ = _moment_draws()
    N = PC.MOMENT_SAMPLES * PC.MOMENT_ELEMENTS
    for name, (mean, var, mu4) in _analytic().items():
        x = out[name][:PC.MOMENT_SAMPLES]
        assert x.shape == (PC.MOMENT_SAMPLES, PC.MOMENT_ELEMENTS) and np.all(np.isfinite(x)), name
        zm = (x.mean() - mean) / math.sqrt(var / N)
        zv = (x.var() - var) / math.sqrt((mu4 - var ** 2) / N)
        print(f"{name}: mean {x.mean():.5f} ({zm:+.2f} se), variance {x.var():.5f} ({zv:+.2f} se)")
        assert abs(zm) <= 5.0 and abs(zv) <= 5.0, (name, zm, zv)
    assert out["uniform"].min() >= -1.0 and out["uniform"].max() < 3.0 and out["pareto"].min() >= 2.0
    assert out["beta"].min() > 0.0 and out["beta"].max() < 1.0
    for k, (n, p) in enumerate(BINOMIAL_CASES):
        x = out[f"binomial{k}"]
        assert np.array_equal(x, np.round(x)) and x.min() >= 0 and x.max() <= n


@pytest.mark.parametrize("k", [0, 1, 2])
def test_binomial_draws_pass_a_chi_square_against_the_pmf(k):
    """Pearson's chi-square of 64 x 512 draws against scipy's pmf, cells with an expected count
    below 5 pooled into one; the level 1e-3 is fixed, and so is the seed."""
    n, p = BINOMIAL_CASES[k]
    x = _moment_draws()[1][f"binomial{k}"][:PC.MOMENT_SAMPLES].astype(np.int64).reshape(-1)
    expected = scipy.stats.binom.pmf(np.arange(n + 1), n, p) * x.size
    observed = np.bincount(x, minlength=n + 1).astype(np.float64)
    big = expected >= 5.0
    obs_cells = np.append(observed[big], observed[~big].sum())
    exp_cells = np.append(expected[big], expected[~big].sum())
    if exp_cells[-1] == 0.0:
        assert obs_cells[-1] == 0.0
        obs_cells, exp_cells = obs_cells[:-1], exp_cells[:-1]
    stat = ((obs_cells - exp_cells) ** 2 / exp_cells).sum()
    pvalue = scipy.stats.chi2.sf(stat, len(exp_cells) - 1)
    print(f"Binomial({n}, {p}): chi2 {stat:.2f} on {len(exp_cells) - 1} df, p = {pvalue:.3f}")
    assert pvalue > 1e-3


def test_binomial_loops_stay_inside_their_bounds():
    """1e5 draws per case: every draw is made (no NaN), no BTRS draw needs NMX_DRAW_MAX_ATTEMPTS
    attempts and no inversion walks NMX_BINOMIAL_MAX_STEPS steps."""
    prog, out, info = _moment_draws()
    assert _COUNTER_SAMPLES * PC.MOMENT_ELEMENTS >= 100000
    by_name = {o.name: o for o in prog.outputs}
    for k, (n, p) in enumerate(BINOMIAL_CASES):
        (stream,) = by_name[f"binomial{k}"].streams
        att, steps = info[stream], info[("steps", stream)]
        assert np.all(np.isfinite(out[f"binomial{k}"])) and att.min() >= 0
        btrs = n * min(p, 1 - p) >= native.BINOMIAL_BTRS_MEAN
        print(f"Binomial({n}, {p}): {'BTRS' if btrs else 'inversion'}, most attempts {att.max() + 1}, "
              f"most steps {steps.max()}")
        assert att.max() < native.DRAW_MAX_ATTEMPTS - 1 and steps.max() < native.BINOMIAL_MAX_STEPS
        assert (steps.max() == 0) == btrs and (btrs or att.max() == 0)


def test_binomial_guards_give_nan_or_the_fixed_value_before_any_loop():
    def model():
        n = numpyro.sample("n", dist.Normal(np.zeros(11), np.ones(11)))
        p = numpyro.sample("p", dist.Normal(np.zeros(11), np.ones(11)))
        numpyro.sample("k", dist.Binomial(n, probs=p))

    prog = compile_predictive(model, (), {}, ["n", "p"])
    nan = np.nan
    n = np.array([20.0, 20.0, 20.0, -1.0, 2.5, 20.0, 20.0, 0.0, nan, 2.0 ** 24, 2.0 ** 24 - 1])
    p = np.array([nan, -0.1, 1.1, 0.5, 0.5, 0.0, 1.0, 0.5, 0.5, 0.5, 1.0])
    want = np.array([nan, nan, nan, nan, nan, 0.0, 20.0, 0.0, nan, nan, 2.0 ** 24 - 1])
    for dtype in (np.float64, np.float32):
        info = {}
        out = prog.run_host({"n": np.tile(n, (5, 1)), "p": np.tile(p, (5, 1))}, 1, PC.words, dtype=dtype, info=info)["k"]
        np.testing.assert_array_equal(out, np.tile(want, (5, 1)))
        assert np.all(info[("steps", 0)] == 0) and np.all(info[0] == np.where(np.isnan(want), -1, 0))


@pytest.mark.parametrize("kind", BZ.OPERAND_KINDS)
@pytest.mark.parametrize("n", BZ.PLATE_SIZES)
def test_device_test_seeds_show_no_float32_mismatch_on_the_host(n, kind):
    """The configurations tests/test_gpu_bounded.py runs on the device: at their seed the float32
    NumPy interpreter draws the float64 one's integers and makes the same accept decisions."""
    samples, args = BZ.binomial_plate_inputs(n)
    model = BZ.binomial_plate_model(n, kind)
    prog = compile_predictive(model, args, {}, samples)
    assert prog.native_check() == (0, "")
    r64, r32, flipped = PC.host_runs(prog, samples, BZ.PLATE_SEED)
    assert set(r64) == set(BZ.PLATE_RULES)
    for site in ("probs", "count"):
        assert np.all(np.isfinite(r64[site])) and np.array_equal(r64[site], r32[site]), site
    assert np.array_equal(r64["uniform"].astype(np.float32), r32["uniform"])
    assert not any(f.any() for f in flipped.values())
    # both samplers ran, mirrored and not (plates of more than one element)
    if n > 1 and kind == "constant":
        counts, probs = args
        mean = counts * np.minimum(probs, 1 - probs)
        assert (mean < 10).any() and (mean >= 10).any() and (probs > 0.5).any()


# ------------------------------------------------------------------ 6: the host check of two operands
def _binomial_program():
    def model(n_obs):
        p = numpyro.sample("p", dist.Beta(np.full(5, 2.0), np.full(5, 2.0)))
        numpyro.sample("k", dist.Binomial(n_obs, probs=p))

    return compile_predictive(model, (np.arange(1.0, 6.0),), {}, ["p"])


def test_predict_program_check_validates_both_operands():
    prog = _binomial_program()
    assert prog.op_names() == ["draw_binomial"]
    op = prog.ops[0].tolist()
    assert op[2] < 0 and op[3] == 0 and op[5] == 1 and op[6] == 1  # a: the constant counts, b: the slots of p
    assert prog.native_check() == (0, "")
    lib = native.lib()

    def status(ops):
        st = lib.nmx_predict_program_check(ctypes.byref(prog.native_struct(ops=ops)), int(prog.output_table().ctypes.data), 1)
        return st, lib.nmx_last_error().decode()

    for word, value, what in ((3, prog.num_slots + 3, "second parameter slot"), (3, 3, "second parameter slot"),
                              (3, ~prog.consts.size, "second parameter constant"), (6, 2, "second stride"),
                              (6, -1, "second stride"), (2, ~(prog.consts.size - 2), "parameter constant")):
        ops = prog.ops.copy()
        ops[0, word] = value
        st, msg = status(ops)
        assert st == 1 and msg.startswith("op 0 (draw_binomial)") and what in msg, (word, value, msg)
    # stride 0 reads one element: a broadcast second operand is accepted
    ops = prog.ops.copy()
    ops[0, 6] = 0
    assert status(ops)[0] == 0
    # a draw op is no op of a potential program
    assert lib.nmx_program_check(ctypes.byref(prog.native_struct())) == 1
    assert lib.nmx_last_error().decode().startswith("op 0: bad opcode")
    pot = _compiled("fully_pooled")[1].program
    ops = pot.ops.copy()
    k = [native.OPCODES[o] for o in ops[:, 0]].index("mul")
    ops[k, 0] = native.DRAW_OPCODE["draw_binomial"]
    assert lib.nmx_program_check(ctypes.byref(pot.native_struct(ops=ops))) == 1
    assert lib.nmx_last_error().decode().startswith(f"op {k}: bad opcode")
