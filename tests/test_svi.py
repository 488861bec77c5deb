"""SVI on the host: the NumPy restatement of the step (numpyro_amd/svi_host.py), the guides'
naming, initial parameters, median / quantiles, and the refusals.  No GPU."""
import numpy as np
import pytest
import torch
from scipy.special import ndtri

import program_zoo as Zoo
import svi_cases as C
from numpyro_amd import optim, svi_host
from numpyro_amd.infer import NUTS, SVI, Trace_ELBO, autoguide
from numpyro_amd.infer.autoguide import AutoDiagonalNormal, AutoNormal
from oracle import philox


def _host(case, P, seed, opt, dtype=np.float64):
    return svi_host.HostSVI(C.pe_grad_fn(case, dtype), case.dim, P, seed, philox.rng, opt, dtype)


# ------------------------------------------------------------------------------ the restatement
def test_noise_is_the_momentum_ordering_of_the_block():
    """Normal number d % 4 of block d // 4, ordered as philox.normals orders a momentum block."""
    for D in (1, 4, 7):
        eps = svi_host.normals(philox.rng, 5, np.arange(3), 2, philox.EV_MOMENTUM, D)
        for p in range(3):
            np.testing.assert_allclose(eps[p], philox.normals(5, p, 2, D), rtol=0, atol=1e-6)
    a = svi_host.normals(philox.rng, 5, [0, 1], 2, svi_host.EV_SVI, 5)
    b = svi_host.normals(philox.rng, 5, [0, 1], 2, svi_host.EV_GUIDE, 5)
    c = svi_host.normals(philox.rng, 5, [0, 1], 3, svi_host.EV_SVI, 5)
    assert np.abs(a - b).min() > 0 and np.abs(a - c).min() > 0
    assert (svi_host.EV_SVI, svi_host.EV_GUIDE) == (9, 10)


@pytest.mark.parametrize("name", sorted(Zoo.CASES))
def test_gradient_is_the_finite_difference_of_the_loss(name):
    """g_loc and g_rho of the float64 restatement against a central difference of its own loss with
    the noise of the step held fixed (eps is a function of seed, particle and step).  h = 1e-5: the
    truncation error h^2 f''' / 6 and the rounding error 1e-16 |loss| / h are both below 1e-7 of the
    gradients' scale here."""
    case = C.zoo(name)
    h = _host(case, 3, 11, optim.SGD(1.0))
    st = h.init(philox.init_uniform(11, 0, 0, case.dim), init_scale=0.3)
    st["t"] = 2
    loss, g_loc, g_rho = h.grads(st)
    assert loss == h.loss_at(st["loc"], st["rho"], 2)
    step = 1e-5
    for which, g in (("loc", g_loc), ("rho", g_rho)):
        fd = np.zeros(case.dim)
        for d in range(case.dim):
            hi, lo = {"loc": st["loc"].copy(), "rho": st["rho"].copy()}, {"loc": st["loc"].copy(), "rho": st["rho"].copy()}
            hi[which][d] += step
            lo[which][d] -= step
            fd[d] = (h.loss_at(hi["loc"], hi["rho"], 2) - h.loss_at(lo["loc"], lo["rho"], 2)) / (2 * step)
        print(name, which, "max |g - fd|", np.abs(g - fd).max(), "max |g|", np.abs(g).max())
        np.testing.assert_allclose(g, fd, rtol=1e-6, atol=1e-6 * np.abs(g).max())


def test_loss_is_the_closed_form_entropy_elbo():
    """loss = mean U - sum log scale - D / 2 (1 + log 2 pi); for the conjugate case with the guide at
    the posterior the expectation of mean U is D / 2, so the loss is -sum log s - D / 2 log(2 pi)
    up to the Monte-Carlo error of 4096 particles."""
    cj = C.Conjugate()
    h = svi_host.HostSVI(cj.pe_grad, cj.dim, 4096, 1, philox.rng, optim.SGD(1.0))
    st = h.init(cj.m, scale=cj.s)
    loss, g_loc, g_rho = h.grads(st)
    expect = -np.log(cj.s).sum() - 0.5 * cj.dim * np.log(2 * np.pi)
    # Var(0.5 chi2_D) = D / 2 per particle
    assert abs(loss - expect) < 5 * np.sqrt(cj.dim / 2 / 4096)
    # the gradient vanishes at the posterior, to Monte-Carlo error: g_loc ~ N(0, prec / P)
    assert np.all(np.abs(g_loc) < 5 * np.sqrt(cj.prec / 4096))


def test_adam_and_sgd_updates():
    """One coordinate, a quadratic potential U = z^2 / 2, one particle: the update formulas by hand."""
    pe_grad = lambda Z: (0.5 * (Z ** 2).sum(-1), Z)  # noqa: E731
    for opt in (optim.SGD(0.5), optim.Adam(0.1, b1=0.8, b2=0.9, eps=1e-3)):
        h = svi_host.HostSVI(pe_grad, 1, 1, 3, philox.rng, opt)
        st = h.init([1.5], scale=[0.7])
        eps = h.noise(0)[0, 0]
        z = 1.5 + 0.7 * eps
        g_loc, g_rho = z, (z * eps - 1 / 0.7) * svi_host.sigmoid(st["rho"][0])
        new, loss = h.update(st)
        assert loss == pytest.approx(0.5 * z * z - np.log(0.7) - svi_host.HALF_LOG_2PI_E, rel=1e-14)
        if isinstance(opt, optim.SGD):
            want = (1.5 - 0.5 * g_loc, st["rho"][0] - 0.5 * g_rho)
        else:
            want = []
            for x, g in ((1.5, g_loc), (st["rho"][0], g_rho)):
                m, v = 0.2 * g, 0.1 * g * g
                want.append(x - 0.1 * (m / (1 - 0.8)) / (np.sqrt(v / (1 - 0.9)) + 1e-3))
        np.testing.assert_allclose([new["loc"][0], new["rho"][0]], want, rtol=1e-13)
        assert new["t"] == 1 and new["scale"][0] == svi_host.softplus(new["rho"][0])


def test_float32_restatement_stays_float32():
    case = C.zoo("poisson")
    h = _host(case, 5, 2, optim.Adam(0.05), np.float32)
    st, losses = h.run(h.init(philox.init_uniform(2, 0, 0, case.dim)), 3)
    assert all(st[k].dtype == np.float32 for k in st if k != "t") and losses.dtype == np.float32
    h64 = _host(case, 5, 2, optim.Adam(0.05))
    st64, losses64 = h64.run(h64.init(philox.init_uniform(2, 0, 0, case.dim)), 3)
    np.testing.assert_allclose(st["loc"], st64["loc"], atol=1e-4)
    np.testing.assert_allclose(losses, losses64, rtol=1e-5)


def test_conjugate_posterior_is_recovered():
    """J = 5 normal means with known noise: the posterior is the mean-field normal N(m, s^2).  Bound:
    |loc - m| <= 0.1 s and |log(scale / s)| <= 0.1.  Settings chosen here on the host so that the
    float64 restatement ends within half of it: Adam(step_size = 0.05), 400 steps, P = 1024
    particles, seed 7.  Observed: max |loc - m| / s = 0.011, max |log(scale / s)| = 0.014 (600 steps
    at P = 256 gave 0.031 and 0.025, 1000 steps of 0.02 at P = 64 gave 0.038 and 0.037)."""
    cj = C.Conjugate()
    h = svi_host.HostSVI(cj.pe_grad, cj.dim, cj.NUM_PARTICLES, cj.SEED, philox.rng, optim.Adam(cj.STEP_SIZE))
    st, losses = h.run(h.init(philox.init_uniform(cj.SEED, 0, 0, cj.dim)), cj.NUM_STEPS)
    d_loc, d_scale = np.abs(st["loc"] - cj.m) / cj.s, np.abs(np.log(st["scale"] / cj.s))
    print("max |loc - m| / s", d_loc.max(), "max |log(scale / s)|", d_scale.max())
    assert d_loc.max() <= 0.5 * cj.LOC_BOUND and d_scale.max() <= 0.5 * cj.LOG_SCALE_BOUND
    assert losses[-50:].mean() < losses[:50].mean()


# ------------------------------------------------------------------------------ the guides
def _guide(cls, **kw):
    g = cls(C.mixed_model, **kw)
    pot = NUTS(C.mixed_model).potential(C.MIXED_ARGS)
    g._setup(pot)
    return g, pot


def test_parameter_names_and_shapes():
    loc, scale = torch.arange(4.0), torch.arange(1.0, 5.0)
    g, pot = _guide(AutoNormal)
    assert [(n, tuple(s)) for n, s, _ in pot.sites] == sorted(C.MIXED_SHAPES.items())
    p = g._params(loc, scale)
    assert set(p) == {f"{s}_auto_{k}" for s in C.MIXED_SHAPES for k in ("loc", "scale")}
    for s, shape in C.MIXED_SHAPES.items():
        assert tuple(p[f"{s}_auto_loc"].shape) == shape and tuple(p[f"{s}_auto_scale"].shape) == shape
    np.testing.assert_array_equal(p["w_auto_loc"].numpy(), [1.0, 2.0])  # sorted: rate, w[2], x
    np.testing.assert_array_equal(p["x_auto_scale"].numpy(), 4.0)
    d, _ = _guide(AutoDiagonalNormal)
    q = d._params(loc, scale)
    assert set(q) == {"auto_loc", "auto_scale"} and tuple(q["auto_loc"].shape) == (4,)
    # either naming reads back as the same flat vectors, in either guide
    for guide in (g, d):
        for params in (p, q):
            l2, s2 = guide._flat(params)
            np.testing.assert_array_equal(l2.numpy(), loc.numpy())
            np.testing.assert_array_equal(s2.numpy(), scale.numpy())
    g2, _ = _guide(AutoNormal, prefix="q")
    assert "w_q_loc" in g2._params(loc, scale)
    with pytest.raises(ValueError, match="unknown parameter"):
        g._flat({"v_auto_loc": 1.0})
    with pytest.raises(ValueError, match="shape"):
        g._flat({**p, "w_auto_loc": torch.zeros(3)})
    with pytest.raises(ValueError, match="positive"):
        g._flat({**p, "x_auto_scale": torch.tensor(0.0)})
    with pytest.raises(RuntimeError, match="SVI.init"):
        AutoNormal(C.mixed_model).median(p)


def test_init_params_round_trip():
    """initial_params: the defaults (the drawn loc, rho = softplus^-1(init_scale)), and init_params in
    either naming overriding both, or part of them."""
    g, pot = _guide(AutoNormal, init_scale=0.25)
    svi = SVI(C.mixed_model, g, optim.Adam(0.01), Trace_ELBO())
    drawn = philox.init_uniform(4, 0, 0, 4)
    loc, rho, scale = svi.initial_params(drawn)
    np.testing.assert_array_equal(loc, drawn)
    np.testing.assert_allclose(scale, 0.25, rtol=1e-7)
    np.testing.assert_allclose(svi_host.softplus(rho.astype(np.float64)), 0.25, rtol=1e-6)
    assert loc.dtype == rho.dtype == scale.dtype == np.float32
    want_loc, want_scale = np.array([0.5, -1.0, 2.0, 0.25], np.float32), np.array([0.1, 0.2, 0.3, 2.0], np.float32)
    for guide in (g, _guide(AutoDiagonalNormal)[0]):
        params = guide._params(torch.from_numpy(want_loc), torch.from_numpy(want_scale))
        loc, rho, scale = svi.initial_params(drawn, params)
        np.testing.assert_array_equal(loc, want_loc)
        np.testing.assert_array_equal(scale, want_scale)
        np.testing.assert_allclose(svi_host.softplus(rho.astype(np.float64)), want_scale, rtol=1e-6)
        back = g._params(torch.from_numpy(loc), torch.from_numpy(scale))
        for k, v in g._params(torch.from_numpy(want_loc), torch.from_numpy(want_scale)).items():
            np.testing.assert_array_equal(back[k].numpy(), v.numpy())
    # a part: w's loc only
    loc, rho, scale = svi.initial_params(drawn, {"w_auto_loc": np.array([7.0, 8.0])})
    np.testing.assert_array_equal(loc, [drawn[0], 7.0, 8.0, drawn[3]])
    np.testing.assert_allclose(scale, 0.25, rtol=1e-7)


def test_median_and_quantiles():
    """loc + scale * ndtri(q) pushed through constrain: exp for the positive site, stick breaking for
    the simplex (K = 3 weights from 2 coordinates)."""
    g, pot = _guide(AutoNormal)
    loc, scale = torch.tensor([0.3, -0.5, 0.8, 1.5]), torch.tensor([0.2, 0.4, 0.1, 0.5])
    params = g._params(loc, scale)
    med = g.median(params)
    assert {k: tuple(v.shape) for k, v in med.items()} == C.MIXED_CONSTRAINED
    want = pot.constrain(pot.unflatten(loc))
    for k in med:
        np.testing.assert_array_equal(med[k].numpy(), want[k].numpy())
    np.testing.assert_allclose(med["rate"].item(), np.exp(0.3), rtol=1e-6)
    np.testing.assert_allclose(med["w"].sum().item(), 1.0, rtol=1e-6)
    qs = [0.05, 0.5, 0.95]
    out = g.quantiles(params, qs)
    assert {k: tuple(v.shape) for k, v in out.items()} == {k: (3,) + s for k, s in C.MIXED_CONSTRAINED.items()}
    z = loc.double().numpy()[None, :] + scale.double().numpy()[None, :] * ndtri(np.array(qs))[:, None]
    want = pot.constrain(pot.unflatten(torch.from_numpy(z)))
    for k in out:
        np.testing.assert_allclose(out[k].numpy(), want[k].numpy(), rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(out["rate"].numpy(), np.exp(0.3 + 0.2 * ndtri(np.array(qs))), rtol=2e-6)
    for k in out:
        np.testing.assert_allclose(out[k][1].numpy(), med[k].numpy(), rtol=1e-6)
    np.testing.assert_allclose(out["w"].sum(-1).numpy(), 1.0, rtol=1e-6)


# ------------------------------------------------------------------------------ refusals
def test_refusals_name_what_is_refused():
    model = C.mixed_model
    guide = AutoNormal(model)

    class Lion:
        pass

    with pytest.raises(NotImplementedError, match="unknown optimiser 'Lion'"):
        SVI(model, guide, Lion(), Trace_ELBO())
    with pytest.raises(NotImplementedError, match="Adagrad"):
        optim.Adagrad(0.1)
    with pytest.raises(NotImplementedError, match="schedule"):
        optim.Adam(lambda i: 0.1)

    def my_guide(y, c):
        pass

    with pytest.raises(NotImplementedError, match="'my_guide'.*hand-written"):
        SVI(model, my_guide, optim.Adam(0.1), Trace_ELBO())
    with pytest.raises(NotImplementedError, match="AutoDelta.*without the Jacobian"):
        autoguide.AutoDelta(model)
    for name in ("AutoLaplaceApproximation", "AutoMultivariateNormal", "AutoLowRankMultivariateNormal"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(autoguide, name)(model)
    from numpyro_amd import infer

    with pytest.raises(NotImplementedError, match="TraceMeanField_ELBO"):
        infer.TraceMeanField_ELBO()
    with pytest.raises(NotImplementedError, match="loss"):
        SVI(model, guide, optim.Adam(0.1), object())
    with pytest.raises(ValueError, match="another model"):
        SVI(lambda: None, guide, optim.Adam(0.1), Trace_ELBO())
    from numpyro_amd import primitives

    with pytest.raises(NotImplementedError, match="param.*'w'.*not supported"):
        primitives.param("w", 1.0)
    with pytest.raises(NotImplementedError, match="subsampl"):
        SVI(model, guide, optim.Adam(0.1), Trace_ELBO())._potential(C.MIXED_ARGS, {"subsample_size": 10})


def test_native_entry_points_check_their_arguments():
    """nmx_svi_* refuse bad sizes before any launch (no GPU needed)."""
    from numpyro_amd import native

    L = native.lib()
    ok = dict(dim=5, num_particles=3, ldc=64, optimizer=native.SVI_ADAM, step_size=0.1, b1=0.9, b2=0.999, eps=1e-8)

    def cfg(**kw):
        return native.SviConfig(**{**ok, **kw})

    cases = [(cfg(dim=0), "dim"), (cfg(num_particles=0), "num_particles"), (cfg(ldc=2), "ldc"),
             (cfg(ldc=96), "ldc")]
    for c, word in cases:
        assert L.nmx_svi_draw(c, 8, 8, native.SVI_EVENT_STEP, 0, 0, 8, None, None) == 1
        assert word in L.nmx_last_error().decode()
        assert L.nmx_svi_step(c, 0, 8, 1 << 20, 8, 8, 8, 8, 8, None) == 1
        assert L.nmx_svi_loss(c, 8, 8, 8, None) == 1
    assert L.nmx_svi_draw(cfg(), None, 8, native.SVI_EVENT_STEP, 0, 0, 8, None, None) == 1
    assert L.nmx_svi_draw(cfg(), 8, 8, 1, 0, 0, 8, None, None) == 1 and b"event" in L.nmx_last_error()
    assert L.nmx_svi_draw(cfg(), 8, 8, native.SVI_EVENT_GUIDE, 0, -1, 8, None, None) == 1
    assert L.nmx_svi_step(cfg(), 0, 1024, 1024 + 4 * 5, 8, 8, 8, 8, 8, None) == 1 and b"overlap" in L.nmx_last_error()
    assert L.nmx_svi_step(cfg(), -1, 8, 1 << 20, 8, 8, 8, 8, 8, None) == 1 and b"step" in L.nmx_last_error()
    assert L.nmx_svi_step(cfg(optimizer=7), 0, 8, 1 << 20, 8, 8, 8, 8, 8, None) == 1
    assert L.nmx_svi_step(cfg(b1=1.0), 0, 8, 1 << 20, 8, 8, 8, 8, 8, None) == 1 and b"b1" in L.nmx_last_error()
    assert L.nmx_svi_step(cfg(), 0, 8, 1 << 20, None, 8, 8, 8, 8, None) == 1
    assert L.nmx_svi_loss(cfg(), 8, None, 8, None) == 1
