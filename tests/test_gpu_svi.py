"""SVI on the device (csrc/svi.hip through numpyro_amd.infer.SVI) against the float64 restatement
numpyro_amd/svi_host.py.

Tolerances.  The draw: atol = 1e-5 max(scale) -- the float32 Box-Muller's angle rounding of at most
2.4e-7 rad times a radius of at most 5.8 bounds the error of eps below 3e-6.  The loss: U_TOL of
tests/test_gpu_program.py (a mean of U's plus a host-exact term).  The reduced gradient (one SGD
step of step_size 1) and the twenty Adam steps have no fixed tolerance: each takes the deviation of
the float32 restatement from the float64 one on the same inputs, times 4 (the factor allows for the
different order of the sum over particles).  Every test recomputes its tolerance from the two
restatements; the numbers of one MI355X run, for the record (max over coordinates of |x - float64|:
"f32" the float32 restatement, whose 4-fold is the tolerance, "dev" the device; the steps themselves
are as large as 530 for loc and 60 for rho, the start being an init_to_uniform draw):

  one SGD step            loc_0 - loc_1: f32 / dev      rho_0 - rho_1: f32 / dev
    poisson       P = 1     8.8e-06 / 8.8e-06             4.2e-06 / 1.7e-06
                  P = 65    4.8e-05 / 1.3e-05             1.7e-06 / 2.7e-07
                  P = 300   4.6e-05 / 1.5e-05             1.5e-06 / 8.1e-07
    robust8       P = 1     2.5e-05 / 5.5e-05             1.6e-06 / 6.0e-06
                  P = 65    6.8e-06 / 6.0e-06             9.7e-07 / 3.7e-07
                  P = 300   9.2e-05 / 1.1e-05             2.9e-07 / 2.2e-07
    eight_schools P = 1     2.5e-05 / 5.8e-06             1.6e-06 / 1.6e-06
                  P = 65    2.2e-05 / 6.4e-06             9.7e-07 / 4.9e-07
                  P = 300   9.2e-05 / 3.5e-06             7.0e-07 / 7.5e-07
  twenty Adam steps, poisson, P = 64:  loc 2.1e-07 / 1.9e-07, scale 6.9e-08 / 6.9e-08,
                                       losses 5.7e-05 / 2.6e-05
  conjugate case on the device: max |loc - m| / s = 0.0109, max |log(scale / s)| = 0.0141
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import svi_cases as C
from numpyro_amd import native, optim, svi_host
from numpyro_amd.infer import SVI, Trace_ELBO
from numpyro_amd.infer.autoguide import AutoDiagonalNormal, AutoNormal
from oracle import philox
from test_gpu_program import U_TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------ 1: the draw
def _draw(device, D, P, loc, scale, seed, event=native.SVI_EVENT_STEP, it=0, offset=0, pad=0):
    """z and eps [4 ceil(D / 4)][ldc] of a NaN-filled arena after the draw-only launch."""
    ldc = (P + 63) // 64 * 64 + pad
    rows = (D + 3) // 4 * 4
    z = torch.full((rows, ldc), float("nan"), device=device)
    eps = torch.full((rows, ldc), float("nan"), device=device)
    d_loc, d_scale = torch.from_numpy(loc).to(device), torch.from_numpy(scale).to(device)
    cfg = native.SviConfig(dim=D, num_particles=P, ldc=ldc, seed=seed)
    native.check(native.lib().nmx_svi_draw(cfg, native.ptr(d_loc), native.ptr(d_scale), event, it, offset,
                                           native.ptr(z), native.ptr(eps), native.stream_ptr()), "nmx_svi_draw")
    torch.cuda.synchronize()
    return z.cpu().numpy(), eps.cpu().numpy()


@pytest.mark.parametrize("D", [1, 3, 4, 5, 9])
def test_draw_matches_the_oracle_at_every_shape(device, D):
    rs = np.random.RandomState(D)
    loc = rs.uniform(-2, 2, D).astype(np.float32)
    scale = rs.uniform(0.05, 3.0, D).astype(np.float32)
    seed, it = 0x1234567890ABCDEF, 7
    assert native.SVI_EVENT_STEP == svi_host.EV_SVI
    want_eps = svi_host.normals(philox.rng, seed, np.arange(300), it, svi_host.EV_SVI, D)  # [300, D] float64
    z300, _ = _draw(device, D, 300, loc, scale, seed, it=it)
    for P in (1, 63, 64, 65, 300):
        for pad in (0, 128):
            z, eps = _draw(device, D, P, loc, scale, seed, it=it, pad=pad)
            want = loc[None, :].astype(np.float64) + scale[None, :].astype(np.float64) * want_eps[:P]
            err = np.abs(z[:D, :P].T - want).max()
            print(f"D={D} P={P} pad={pad}: max |z - oracle| = {err:.3g}, max |eps - oracle| = "
                  f"{np.abs(eps[:D, :P].T - want_eps[:P]).max():.3g}")
            np.testing.assert_allclose(z[:D, :P].T, want, rtol=0, atol=1e-5 * scale.max())
            np.testing.assert_allclose(eps[:D, :P].T, want_eps[:P], rtol=0, atol=3e-6)
            # z = loc + scale * eps in float32 with both roundings
            np.testing.assert_array_equal(z[:D, :P], loc[:, None] + scale[:, None] * eps[:D, :P])
            # row p is the same whatever P and the padding
            np.testing.assert_array_equal(z[:D, :P], z300[:D, :P])
            # pad particles and the tail coordinates of the last block stay NaN
            assert np.all(np.isnan(z[:, P:])) and np.all(np.isnan(eps[:, P:]))
            assert np.all(np.isnan(z[D:])) and np.all(np.isnan(eps[D:]))


def test_draw_words_of_the_counter(device):
    """The particle offset goes in the chain word, the iteration and the event in theirs."""
    D, seed = 6, 99
    loc, scale = np.zeros(D, np.float32), np.ones(D, np.float32)
    base, _ = _draw(device, D, 70, loc, scale, seed, it=3)
    off, _ = _draw(device, D, 65, loc, scale, seed, it=3, offset=5)
    np.testing.assert_array_equal(off[:D, :65], base[:D, 5:70])
    guide, _ = _draw(device, D, 70, loc, scale, seed, event=native.SVI_EVENT_GUIDE, it=0)
    want = svi_host.normals(philox.rng, seed, np.arange(70), 0, svi_host.EV_GUIDE, D)
    np.testing.assert_allclose(guide[:D, :70].T, want, rtol=0, atol=1e-5)
    other, _ = _draw(device, D, 70, loc, scale, seed, it=4)
    assert np.abs(other[:D, :70] - base[:D, :70]).min() > 0


# ------------------------------------------------------------------------------ 2, 3: one SGD step
def _np(t):
    return t.detach().cpu().numpy().copy()


@functools.lru_cache(maxsize=None)
def _sgd_step(device, name, P):
    """One SGD step of step_size 1 on the device, and the two restatements fed the device's own
    parameters, z and eps."""
    case = C.zoo(name)
    svi = SVI(case.model, AutoDiagonalNormal(case.model), optim.SGD(1.0), Trace_ELBO(P))
    state = svi.init(21, *case.args, device=device)
    before = {k: _np(state.row(k)) for k in ("loc", "rho", "scale")}
    Z, eps = _np(state.z)[:, :P].T, _np(state.eps)[:, :P].T
    state, loss = svi.update(state)
    torch.cuda.synchronize()
    after = {k: _np(state.row(k)) for k in ("loc", "rho", "scale")}
    out = {"dev": (before["loc"].astype(np.float64) - after["loc"], before["rho"].astype(np.float64) - after["rho"],
                   float(loss)), "after": after, "before": before}
    for dtype in (np.float64, np.float32):
        h = svi_host.HostSVI(C.pe_grad_fn(case, dtype), case.dim, P, 21, philox.rng, optim.SGD(1.0), dtype)
        st = {k: v.astype(dtype) for k, v in before.items()}
        st.update(t=0, **{k: np.zeros(case.dim, dtype) for k in ("m_loc", "v_loc", "m_rho", "v_rho")})
        new, hl = h.update(st, Z=Z, eps=eps)
        out[dtype] = (st["loc"].astype(np.float64) - new["loc"], st["rho"].astype(np.float64) - new["rho"], float(hl))
    return out


@pytest.mark.parametrize("P", [1, 65, 300])
@pytest.mark.parametrize("name", ["poisson", "robust8", "eight_schools"])
def test_one_sgd_step_is_the_reduced_gradient(device, name, P):
    r = _sgd_step(device, name, P)
    for i, what in enumerate(("loc_0 - loc_1", "rho_0 - rho_1")):
        dev, f64, f32 = r["dev"][i], r[np.float64][i], r[np.float32][i]
        spread = np.abs(f32 - f64).max()
        err = np.abs(dev - f64).max()
        print(f"{name} P={P} {what}: float32 restatement vs float64 {spread:.3g}, device vs float64 {err:.3g}, "
              f"max |step| {np.abs(f64).max():.3g}")
        assert err <= 4 * spread
    # the kept scale is softplus of the new rho
    np.testing.assert_allclose(r["after"]["scale"], svi_host.softplus(r["after"]["rho"].astype(np.float64)), rtol=3e-7)


@pytest.mark.parametrize("P", [1, 65, 300])
@pytest.mark.parametrize("name", ["poisson", "robust8", "eight_schools"])
def test_loss_of_that_step(device, name, P):
    r = _sgd_step(device, name, P)
    print(f"{name} P={P}: loss device {r['dev'][2]!r}, float64 {r[np.float64][2]!r}")
    np.testing.assert_allclose(r["dev"][2], r[np.float64][2], **U_TOL)


# ------------------------------------------------------------------------------ 4: twenty Adam steps
ADAM_SEED, ADAM_P, ADAM_STEPS = 5, 64, 20


def _adam_svi(guide=AutoDiagonalNormal):
    case = C.zoo("poisson")
    return case, SVI(case.model, guide(case.model), optim.Adam(0.05), Trace_ELBO(ADAM_P))


@functools.lru_cache(maxsize=None)
def _adam_run(device):
    case, svi = _adam_svi()
    res = svi.run(ADAM_SEED, ADAM_STEPS, *case.args, device=device)
    torch.cuda.synchronize()
    return {"loc": _np(res.state.loc), "rho": _np(res.state.rho), "scale": _np(res.state.scale),
            "losses": _np(res.losses), "par": _np(res.state.par[res.state.cur]), "z": _np(res.state.z),
            "params": {k: _np(v) for k, v in res.params.items()}}


def test_twenty_adam_steps_match_the_restatement(device):
    case, _ = _adam_svi()
    dev = _adam_run(device)
    runs = {}
    for dtype in (np.float64, np.float32):
        h = svi_host.HostSVI(C.pe_grad_fn(case, dtype), case.dim, ADAM_P, ADAM_SEED, philox.rng, optim.Adam(0.05), dtype)
        st, losses = h.run(h.init(philox.init_uniform(ADAM_SEED, 0, 0, case.dim)), ADAM_STEPS)
        runs[dtype] = {"loc": st["loc"].astype(np.float64), "scale": st["scale"].astype(np.float64),
                       "losses": losses.astype(np.float64)}
    for k in ("loc", "scale", "losses"):
        spread = np.abs(runs[np.float32][k] - runs[np.float64][k]).max()
        err = np.abs(dev[k] - runs[np.float64][k]).max()
        print(f"poisson P={ADAM_P}, {ADAM_STEPS} Adam steps, {k}: float32 restatement vs float64 {spread:.3g}, "
              f"device vs float64 {err:.3g}")
        assert err <= 4 * spread
    assert dev["losses"][-1] < dev["losses"][0]
    np.testing.assert_array_equal(dev["params"]["auto_loc"], dev["loc"])
    np.testing.assert_array_equal(dev["params"]["auto_scale"], dev["scale"])


def test_runs_are_bitwise_reproducible_and_run_is_twenty_updates(device):
    case, svi = _adam_svi()
    first = _adam_run(device)
    again = svi.run(ADAM_SEED, ADAM_STEPS, *case.args, device=device)
    np.testing.assert_array_equal(_np(again.state.par[again.state.cur]), first["par"])
    np.testing.assert_array_equal(_np(again.losses), first["losses"])
    np.testing.assert_array_equal(_np(again.state.z), first["z"])
    state = svi.init(ADAM_SEED, *case.args, device=device)
    losses = []
    for _ in range(ADAM_STEPS):
        state, loss = svi.update(state, *case.args)
        losses.append(loss)
    np.testing.assert_array_equal(_np(torch.stack(losses)), first["losses"])
    np.testing.assert_array_equal(_np(state.par[state.cur]), first["par"])
    assert state.t == ADAM_STEPS
    # the per-site naming reports the same numbers, site by site
    _, by_site = _adam_svi(AutoNormal)
    res = by_site.run(ADAM_SEED, ADAM_STEPS, *case.args, device=device)
    flat = np.concatenate([_np(res.params[f"{s}_auto_loc"]).reshape(-1) for s, _, _ in case.sites])
    np.testing.assert_array_equal(flat, first["loc"])
    for s, shape, _ in case.sites:
        assert tuple(res.params[f"{s}_auto_scale"].shape) == tuple(shape)


def test_evaluate_changes_no_state(device):
    case, svi = _adam_svi()
    state = svi.init(ADAM_SEED, *case.args, device=device)
    for _ in range(3):
        state, _ = svi.update(state)
    snap = (_np(state.par), _np(state.z), _np(state.eps), state.cur, state.t)
    value = float(svi.evaluate(state, *case.args))
    assert float(svi.evaluate(state)) == value
    for a, b in zip(snap, (_np(state.par), _np(state.z), _np(state.eps), state.cur, state.t)):
        np.testing.assert_array_equal(a, b)
    state, loss = svi.update(state)
    assert float(loss) == value  # the loss the next update reports
    assert float(loss) == _adam_run(device)["losses"][3]


def test_init_params_are_uploaded(device):
    case, svi = _adam_svi(AutoNormal)
    loc = np.linspace(-1, 1, case.dim).astype(np.float32)
    scale = np.linspace(0.1, 0.5, case.dim).astype(np.float32)
    state = svi.init(1, *case.args, init_params={"auto_loc": loc, "auto_scale": scale}, device=device)
    np.testing.assert_array_equal(_np(state.loc), loc)
    np.testing.assert_array_equal(_np(state.scale), scale)
    np.testing.assert_array_equal(_np(state.z)[:, :ADAM_P], loc[:, None] + scale[:, None] * _np(state.eps)[:, :ADAM_P])
    back = svi.get_params(state)
    state2 = svi.init(1, *case.args, init_params=back, device=device)
    np.testing.assert_array_equal(_np(state2.par[0, :3]), _np(state.par[0, :3]))
    # the default start: the engine's init_to_uniform draw of chain 0, attempt 0
    np.testing.assert_array_equal(_np(svi.init(1, *case.args, device=device).loc), philox.init_uniform(1, 0, 0, case.dim))


# ------------------------------------------------------------------------------ 5: the conjugate case
def test_conjugate_posterior_on_the_device(device):
    """The bound and the settings of tests/test_svi.py test_conjugate_posterior_is_recovered."""
    cj = C.Conjugate()
    svi = SVI(cj.model, AutoNormal(cj.model), optim.Adam(cj.STEP_SIZE), Trace_ELBO(cj.NUM_PARTICLES))
    res = svi.run(cj.SEED, cj.NUM_STEPS, *cj.args, device=device)
    loc, scale = _np(res.params["mu_auto_loc"]).astype(np.float64), _np(res.params["mu_auto_scale"]).astype(np.float64)
    d_loc, d_scale = np.abs(loc - cj.m) / cj.s, np.abs(np.log(scale / cj.s))
    print("device: max |loc - m| / s", d_loc.max(), "max |log(scale / s)|", d_scale.max())
    assert d_loc.max() <= cj.LOC_BOUND and d_scale.max() <= cj.LOG_SCALE_BOUND
    assert res.losses.shape == (cj.NUM_STEPS,) and bool(torch.isfinite(res.losses).all())


# ------------------------------------------------------------------------------ 6: sample_posterior
def test_sample_posterior(device):
    model = C.mixed_model
    guide = AutoNormal(model)
    svi = SVI(model, guide, optim.Adam(0.05), Trace_ELBO(8))
    res = svi.run(3, 30, *C.MIXED_ARGS, device=device)
    params = res.params
    loc, scale = (_np(t).astype(np.float64) for t in guide._flat(params))
    S = 4096
    z = _np(guide._draw(17, *guide._flat(params), S)).astype(np.float64)  # unconstrained [S, D]
    assert z.shape == (S, 4)
    print("mean err / se", np.abs(z.mean(0) - loc) / (scale / np.sqrt(S)), "sd err / se",
          np.abs(z.std(0, ddof=1) - scale) / (scale / np.sqrt(2 * S)))
    assert np.all(np.abs(z.mean(0) - loc) <= 5 * scale / np.sqrt(S))
    assert np.all(np.abs(z.std(0, ddof=1) - scale) <= 5 * scale / np.sqrt(2 * S))
    want = loc[None, :] + scale[None, :] * svi_host.normals(philox.rng, 17, np.arange(S), 0, svi_host.EV_GUIDE, 4)
    np.testing.assert_allclose(z, want, rtol=0, atol=1e-5 * scale.max())
    draws = guide.sample_posterior(17, params, sample_shape=(S,))
    assert {k: tuple(v.shape) for k, v in draws.items()} == {k: (S,) + s for k, s in C.MIXED_CONSTRAINED.items()}
    assert bool((draws["rate"] > 0).all()) and bool((draws["w"] > 0).all())
    np.testing.assert_allclose(_np(draws["w"].sum(-1)), 1.0, rtol=1e-5)
    np.testing.assert_allclose(_np(draws["rate"]), np.exp(z[:, 0]), rtol=1e-5)
    np.testing.assert_array_equal(_np(draws["x"]), z[:, 3].astype(np.float32))
    block = guide.sample_posterior(17, params, sample_shape=(2, 3))
    assert tuple(block["w"].shape) == (2, 3, 3) and tuple(block["x"].shape) == (2, 3)
    np.testing.assert_array_equal(_np(block["x"]).reshape(-1), _np(draws["x"])[:6])
    one = guide.sample_posterior(17, params)
    assert tuple(one["w"].shape) == (3,) and tuple(one["rate"].shape) == ()
    med = guide.median(params)
    np.testing.assert_allclose(_np(med["rate"]), np.exp(loc[0]), rtol=1e-5)


# ------------------------------------------------------------------------------ the debug build
DEBUG_SCRIPT = r"""
import sys
sys.path.insert(0, "tests")
import numpy as np, torch
import svi_cases as C
from numpyro_amd import native, optim
from numpyro_amd.infer import SVI, Trace_ELBO
from numpyro_amd.infer.autoguide import AutoNormal
assert native.LIB_PATH.endswith("libnumpyro_amd_debug.so"), native.LIB_PATH
cj = C.Conjugate()
for P in (1, 65, 300):
    for opt in (optim.Adam(0.05), optim.SGD(0.001)):
        guide = AutoNormal(cj.model)
        svi = SVI(cj.model, guide, opt, Trace_ELBO(P))
        res = svi.run(1, 5, *cj.args)
        svi.evaluate(res.state)
        guide.sample_posterior(2, res.params, sample_shape=(70,))
        assert bool(torch.isfinite(res.losses).all())
torch.cuda.synchronize()
print("svi debug build ok")
"""


def test_debug_build_runs_the_svi_kernels_without_a_failed_check():
    """D = 5 (a last block with one coordinate) at P = 1, 65 and 300 under the NMX_DCHECK build."""
    lib = os.path.join(ROOT, "numpyro_amd", "_lib", "libnumpyro_amd_debug.so")
    if not os.path.exists(lib):
        pytest.fail("debug library missing: run numpyro_amd.build(debug=True) (done by __graft_entry__.build())")
    env = dict(os.environ, NUMPYRO_AMD_DEBUG="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", DEBUG_SCRIPT], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=110)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "NMX_DCHECK failed" not in out, out[-3000:]
    assert "svi debug build ok" in out
