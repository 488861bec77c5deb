"""The count likelihoods on the host: the exact log masses against scipy.stats, the reverse mode
against central differences, the two special ops alone (lrising, logaddexp) on hand-assembled
programs, what float32 can meet at the corners the device test uses, the composed samplers against
their exact pmfs, and the refusals.  No GPU: the float64 interpreter (Program.run_host,
LogLikProgram.run_host, PredictiveProgram.run_host) and its float32 restatement."""
import numpy as np
import pytest

import numpyro_amd as numpyro
import count_cases as CC
from numpyro_amd import distributions as dist
from numpyro_amd import jnp, native
from numpyro_amd.loglik_program import compile_log_likelihood
from numpyro_amd.predictive_program import compile_predictive
from numpyro_amd.program import Program, _Builder, compile_model
from test_gpu_program import G_TOL, U_TOL


# ------------------------------------------------------------------------------ 1: exact log mass
@pytest.mark.parametrize("name", sorted(CC.MASS))
def test_log_mass_equals_scipy(name):
    """One value per observation (the log-likelihood program) at the full parameter grid, and the
    potential's sum of them at the same rows: the float64 interpreter against scipy.stats, rtol 1e-9
    plus the rounding of scipy's own gammaln sums (count_cases.mass_reference_rounding: below 4e-10,
    and below 2e-12 except at concentrations of 1e4)."""
    case = CC.MASS[name]
    model, samples = CC.mass_model(case), CC.mass_grid(case)
    ref = CC.mass_reference(case, samples)
    assert np.all(np.isfinite(ref)), name
    prog = compile_log_likelihood(model, (CC.Y,), {}, given=samples)
    assert prog.native_check() == (0, ""), prog.native_check()
    got = prog.run_host(samples)["y"]
    assert got.shape == ref.shape
    print(name, "rows", ref.shape[0], "max relative error", np.max(np.abs(got - ref) / np.abs(ref)))
    err = CC.mass_reference_rounding(case, samples)
    assert np.all(np.abs(got - ref) <= 1e-9 * np.abs(ref) + err), np.max(np.abs(got - ref) - 1e-9 * np.abs(ref) - err)
    # the potential: U + log prior + log|J| is minus the site's total (the priors by scipy, in the test's hands)
    pot = compile_model(model, (CC.Y,))
    assert pot.program.native_check() == (0, "")
    Z = CC.unconstrain(case, samples)
    U, _ = pot.program.run_host(Z)
    base = compile_model(_prior_only(case), ())
    U0, _ = base.program.run_host(Z)
    np.testing.assert_allclose(U - U0, -ref.sum(1), rtol=1e-9, atol=1e-9 * np.abs(U0).max() + len(CC.Y) * err.max())


def _prior_only(case):
    def model():
        for k, kind in sorted(case.kinds.items()):
            numpyro.sample(k, CC._PRIOR[kind]())
    return model


# ------------------------------------------------------------------------------ 2: gradient
@pytest.mark.parametrize("name", sorted(CC.MASS))
def test_reverse_mode_is_the_central_difference_of_the_forward_pass(name):
    """dU/dz of the float64 interpreter against central differences of its own U, every parameter
    latent (the concentrations and total_counts among them).  As tests/test_svi.py's loss-gradient
    test: h = 1e-5 in the unconstrained coordinates, where the truncation error h^2 U''' / 6 and the
    rounding error 1e-16 |U| / h (|U| below 1e4 here: 1e-7) are both below 1e-6 of the gradient's
    scale; the value and the derivative of lrising are series cut at the same order, which agree to
    1e-10."""
    case = CC.MASS[name]
    pot = compile_model(CC.mass_model(case), (CC.Y,))
    Z = CC.unconstrain(case, CC.moderate(case))
    U, G = pot.program.run_host(Z)
    assert np.all(np.isfinite(U)) and np.all(np.isfinite(G))
    h = 1e-5
    fd = np.zeros_like(G)
    for d in range(Z.shape[1]):
        hi, lo = Z.copy(), Z.copy()
        hi[:, d] += h
        lo[:, d] -= h
        fd[:, d] = (pot.program.run_host(hi)[0] - pot.program.run_host(lo)[0]) / (2 * h)
    print(name, "max |g - fd|", np.abs(G - fd).max(), "max |g|", np.abs(G).max())
    np.testing.assert_allclose(G, fd, rtol=1e-6, atol=1e-6 * np.abs(G).max())


# ------------------------------------------------------------------------------ 3: the ops alone
def test_special_opcodes_are_numbered_apart():
    assert native.SPECIAL_BASE == 40 and native.SPECIAL_OPCODES == ["lrising", "logaddexp"]
    assert native.OPCODE["lrising"] == 40 and native.OPCODE["logaddexp"] == 41
    assert native.op_name(40) == "lrising" and native.op_name(41) == "logaddexp"
    assert "lrising" not in native.OPCODES and native.LINALG_BASE + len(native.LINALG_OPCODES) <= native.SPECIAL_BASE
    assert native.SPECIAL_BASE + len(native.SPECIAL_OPCODES) <= native.DRAW_BASE


def test_op_programs_pass_the_check_and_match_scipy():
    """Every layout and size: nmx_program_check accepts the program, and the float64 interpreter's
    U is the weighted sum of scipy.special.gammaln differences (np.logaddexp) within the
    reference's own rounding (count_cases.rising_reference) plus 1e-9 of the sum's terms, the cut of
    the op's Stirling and log1p series."""
    seen = set()
    for c in CC.op_cases():
        assert c.program.native_check() == (0, ""), (c.name, c.program.native_check())
        assert {"lrising", "logaddexp"} & set(c.program.op_names()), c.name
        U, G = c.program.run_host(c.Z)
        want, err = c.expect
        assert np.all(np.isfinite(U)) and np.all(np.isfinite(G)), c.name
        np.testing.assert_allclose(U, want, rtol=1e-9, atol=np.max(err) + 1e-12, err_msg=c.name)
        seen.add(c.name.split(".")[0])
    assert seen == {"lrising", "logaddexp"}


def test_rising_grid_against_gammaln():
    """The grid a x k, pair by pair: the op's float64 value against gammaln differences, within
    their rounding and rtol 1e-9; its float32 value within 4e-7 of it (three float32 roundings of
    terms no larger than the result's own size)."""
    from numpyro_amd.program import _host_lrising

    a, k = np.meshgrid(CC.f32(CC.RISING_A), CC.f32(CC.RISING_K), indexing="ij")
    ref, err = CC.rising_reference(a, k)
    got = _host_lrising(a, k)
    assert np.all(np.abs(got - ref) <= err + 1e-9 * np.abs(ref)), np.max(np.abs(got - ref) - err)
    got32 = _host_lrising(a.astype(np.float32), k.astype(np.float32))
    assert got32.dtype == np.float32
    rel = np.abs(got32 - got) / np.maximum(np.abs(got), 1e-30)
    print("float32 lrising: largest relative deviation", rel.max())
    assert rel.max() <= 4e-7
    assert np.all(got[:, 0] == 0.0) and np.all(got[:, 1] == 0.0)  # k = 0 and k = 1: nothing rises


def test_logaddexp_grid():
    from numpyro_amd.program import _host_logaddexp, _host_rev

    x = np.array([-3.0, 0.0, 2.5])[:, None] + np.zeros(len(CC.LAE_GAPS))
    y = x - np.asarray(CC.LAE_GAPS)[None, :]
    for a, b in ((x, y), (y, x)):
        np.testing.assert_allclose(_host_logaddexp(a, b), np.logaddexp(a, b), rtol=1e-15)
        out = _host_logaddexp(a, b)
        da, db = _host_rev("logaddexp", np.ones_like(out), a, b, out)
        np.testing.assert_allclose(da + db, 1.0, rtol=1e-12)  # the two softmax weights
        np.testing.assert_allclose(da, 1.0 / (1.0 + np.exp(b - a)), rtol=1e-12)
    ninf = np.array([-np.inf])
    out = _host_logaddexp(ninf, ninf)
    assert out[0] == -np.inf
    da, db = _host_rev("logaddexp", np.ones(1), ninf, ninf, out)
    assert da[0] == 0.0 and db[0] == 0.0
    assert jnp.logaddexp(1.0, 2.0) == np.logaddexp(1.0, 2.0)


def test_check_refuses_a_slot_as_the_step_count():
    c = CC.rising_slot_k()
    st, msg = c.program.native_check()
    assert st != 0 and "lrising" in msg and "constant" in msg, (st, msg)
    # ... and in a predictive and a log-likelihood program's check, which share it
    ops = c.program.ops.copy()
    fwd = Program(ops[:-2], c.program.consts64, [], int(ops[-3, 1] + ops[-3, 4]), c.program.dim)
    table = np.asarray([[ops[-3, 1], ops[-3, 4]]], np.int32)
    lib = native.lib()
    import ctypes
    assert lib.nmx_predict_program_check(ctypes.byref(fwd.native_struct()), int(table.ctypes.data), 1) != 0
    assert b"lrising" in lib.nmx_last_error()
    table3 = np.asarray([[ops[-3, 1], ops[-3, 4], 0]], np.int32)
    assert lib.nmx_loglik_program_check(ctypes.byref(fwd.native_struct()), int(table3.ctypes.data), 1, int(ops[-3, 4])) != 0
    assert b"lrising" in lib.nmx_last_error()


# ------------------------------------------------------------------------------ 4: float32 can meet the device bound
def _share(x, ref, rtol, atol):
    return float(np.max(np.abs(x - ref) / (atol + rtol * np.abs(ref))))


@pytest.mark.parametrize("N", [8, 1, 65])
@pytest.mark.parametrize("corner", CC.corners(), ids=lambda c: c.name)
def test_float32_restatement_is_inside_the_device_tolerances(corner, N):
    """On the corner rows and on 64 random rows the float32 restatement of the interpreter is
    within U_TOL / G_TOL of the float64 interpreter: the device test's bound can be met, with the 8
    observations as they are and cycled to the device test's 1 and 65."""
    pot = compile_model(corner.model, CC.observed_at(corner, N))
    names = set(pot.program.op_names())
    assert "lrising" in names or "logaddexp" in names
    for what, Z in (("corner rows", corner.Z), ("random rows", CC.random_rows(corner))):
        U, G = pot.program.run_host(Z)
        U32, G32 = pot.program.run_host(Z, dtype=np.float32)
        assert np.all(np.isfinite(U)) and np.all(np.isfinite(G)) and np.all(np.isfinite(U32)) and np.all(np.isfinite(G32))
        print(f"{corner.name} N={N} {what}: share of U_TOL {_share(U32, U, **U_TOL):.3f}, of G_TOL {_share(G32, G, **G_TOL):.3f}")
        np.testing.assert_allclose(U32, U, **U_TOL)
        np.testing.assert_allclose(G32, G, **G_TOL)


def test_plain_lgamma_expansion_misses_the_tolerance_at_the_top_concentration(monkeypatch):
    """What the lrising op is for: the same regression with R(a, k) spelt as lgamma(a + k) - lgamma(a)
    - k log(a) over the plain lgamma op is outside U_TOL or G_TOL, in float32, at phi = 1e5."""
    corner = CC.corners()[0]
    Z = corner.Z[np.isclose(corner.Z[:, 1], np.log(max(CC.PHIS)), rtol=1e-6)]
    assert len(Z) == len(CC.INTERCEPTS)
    good = compile_model(corner.model, corner.args).program

    def plain(self, a, k):
        a, k = self.const(a), self.const(k)
        return self.ew("lgamma", a + k) - self.ew("lgamma", a) - k * self.ew("log", a)

    monkeypatch.setattr(_Builder, "lrising", plain)
    bad = compile_model(corner.model, corner.args).program
    assert "lrising" not in bad.op_names() and "lgamma" in bad.op_names()
    U, G = good.run_host(Z)
    Ub, Gb = bad.run_host(Z)
    np.testing.assert_allclose(Ub, U, rtol=1e-9)  # the same function in float64 ...
    U32, G32 = bad.run_host(Z, dtype=np.float32)
    su, sg = _share(U32, U, **U_TOL), _share(G32, G, **G_TOL)
    print(f"plain lgamma at phi = {max(CC.PHIS):g}: share of U_TOL {su:.2f}, of G_TOL {sg:.2f}")
    assert su > 1.0 or sg > 1.0  # ... and outside the tolerance in float32


# ------------------------------------------------------------------------------ 5: draws follow their laws
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_draws_follow_their_laws(dtype):
    """Pearson's chi-square against the exact pmfs under draw_cases' decision rule and seeds."""
    CC.check_draws(lambda seed: CC.host_draws(seed, dtype))


def test_draws_are_composed_from_the_existing_draw_ops():
    prog = compile_predictive(CC.draw_model, (), {}, [])
    assert {n for n in prog.op_names() if n.startswith("draw_")} <= set(native.DRAW_OPCODES)
    assert len(native.DRAW_OPCODES) == 8


# ------------------------------------------------------------------------------ 6: refusals
def test_refusals_name_the_site():
    y = CC.Y30

    def latent_count():
        numpyro.sample("k", dist.NegativeBinomial2(3.0, 2.0))
        numpyro.sample("y", dist.Normal(0.0, 1.0), obs=y)

    with pytest.raises(NotImplementedError, match=r"site 'k'.*NegativeBinomial2 is not supported as a latent site"):
        compile_model(latent_count)

    def latent_zi():
        numpyro.sample("k", dist.ZeroInflatedPoisson(0.3, 2.0))
        numpyro.sample("y", dist.Normal(0.0, 1.0), obs=y)

    with pytest.raises(NotImplementedError, match=r"site 'k'.*ZeroInflatedPoisson is not supported as a latent site"):
        compile_model(latent_zi)

    def bad_base():
        g = numpyro.sample("g", dist.Beta(1.0, 1.0))
        numpyro.sample("y", dist.ZeroInflatedDistribution(dist.Bernoulli(probs=0.5), gate=g), obs=np.zeros(4))

    with pytest.raises(NotImplementedError, match=r"site 'y'.*zero-inflated BernoulliProbs"):
        compile_model(bad_base)
    with pytest.raises(NotImplementedError, match=r"site 'y'.*zero-inflated BernoulliProbs"):
        compile_log_likelihood(bad_base, (), {}, given={"g"})
    with pytest.raises(NotImplementedError, match=r"site 'y'.*zero-inflated Normal"):
        compile_predictive(lambda: numpyro.sample("y", dist.ZeroInflatedDistribution(dist.Normal(0.0, 1.0), gate=0.5)))

    def latent_total():
        n = numpyro.sample("n", dist.Gamma(20.0, 1.0))
        numpyro.sample("y", dist.BetaBinomial(2.0, 3.0, n), obs=np.array([1.0, 2.0]))

    with pytest.raises(NotImplementedError, match=r"site 'y'.*total_count that depends on a latent site"):
        compile_model(latent_total)
    with pytest.raises(NotImplementedError, match=r"site 'y'.*total_count that depends on a latent site"):
        compile_log_likelihood(latent_total, (), {}, given={"n"})
    with pytest.raises(ValueError, match="gate"):
        dist.ZeroInflatedDistribution(dist.Poisson(1.0))
    with pytest.raises(ValueError, match="probs"):
        dist.NegativeBinomial(3.0)
