"""Device NUTS/HMC engine vs the NumPy oracle (oracle/hmc_ref.py) on identical Philox
streams, plus schedule-invariance and statistical checks.

Parity bar: the oracle restates numpyro's sample kernel in float32 with the same event
keys, so per-chain trajectories coincide until an fp32 rounding difference (transcendental
ulps, dot-product order) flips a discrete decision; tests require the large majority of
chains to reproduce the oracle's num_steps sequence exactly and their draws to 1e-3.
"""
import numpy as np
import pytest
import torch

from numpyro_amd import datasets, native
from numpyro_amd import potentials as P
from numpyro_amd.infer import HMC, MCMC, NUTS
import parity_cases as PC
from oracle import hmc_ref as H
from oracle import parity as PR
from oracle import philox
from oracle import potentials as OP

pytestmark = pytest.mark.gpu


def _oracle_chain(pe_grad, dim, seed, chain, num_warmup, num_iters, algo="NUTS", z0=None, **kw):
    """Oracle states of one chain."""
    o = H.NUTSOracle(lambda z: tuple(np.asarray(v, np.float32) if np.ndim(v) else np.float32(v)
                                     for v in pe_grad(z)),
                     dim, num_warmup, algo=algo, **kw)
    if z0 is None:
        z0 = philox.init_uniform(seed, chain, 0, dim)
    s = o.init(z0, seed, chain)
    out = []
    for _ in range(num_iters):
        s = o.sample(s)
        out.append(s)
    return out


def _run_engine(model_args, model, num_chains, num_warmup, num_samples, seed, kernel_cls=NUTS,
                sync=False, chain_offset=None, init_params=None, **kw):
    kernel = kernel_cls(model, **kw)
    mcmc = MCMC(kernel, num_warmup=num_warmup, num_samples=num_samples, num_chains=num_chains,
                chain_method="vectorized", progress_bar=False, sync_chains=sync,
                chain_offset=chain_offset)
    if num_warmup > 0:
        mcmc.warmup(seed, *model_args, collect_warmup=True,
                    extra_fields=("num_steps", "accept_prob", "potential_energy", "adapt_state.step_size"))
        warm = mcmc.get_samples(group_by_chain=True), mcmc.get_extra_fields(group_by_chain=True)
    else:
        warm = ({}, {"num_steps": torch.zeros(num_chains, 0, dtype=torch.int32)})
    mcmc.run(seed, *model_args, init_params=init_params,
             extra_fields=("num_steps", "accept_prob", "potential_energy", "adapt_state.step_size"))
    return mcmc, warm


def _dev_paths(mcmc, warm):
    ws, wf = warm
    ef = mcmc.get_extra_fields(True)
    sm = mcmc.get_samples(True)
    ns = np.concatenate([wf["num_steps"].cpu().numpy(), ef["num_steps"].cpu().numpy()], axis=1)
    flat = {k: np.concatenate([ws[k].cpu().numpy(), sm[k].cpu().numpy()], axis=1) if k in ws
            else sm[k].cpu().numpy() for k in sm}
    return ns, flat


@pytest.mark.parametrize("algo", ["NUTS", "HMC"])
def test_engine_matches_oracle_eight_schools(device, algo):
    """Adaptive run: the centred 8-schools posterior is a funnel, where fp32 rounding
    differences grow along trajectories (chaotic dynamics), so exact agreement is required
    over the first transitions only; later agreement is statistical (other tests)."""
    seed, C, W, S, T0 = 1234, 32, 30, 10, 4
    args = (8, datasets.EIGHT_SCHOOLS_SIGMA, datasets.EIGHT_SCHOOLS_Y)
    kcls = NUTS if algo == "NUTS" else HMC
    kw = {} if algo == "NUTS" else {"trajectory_length": 1.0}
    mcmc, warm = _run_engine(args, P.eight_schools, C, W, S, seed, kernel_cls=kcls, **kw)
    ns_dev, site = _dev_paths(mcmc, warm)
    ref = OP.EightSchools(datasets.EIGHT_SCHOOLS_Y, datasets.EIGHT_SCHOOLS_SIGMA)
    match = 0
    for c in range(C):
        states = _oracle_chain(ref.pe_grad, 10, seed, c, W, T0, algo=algo, **kw)
        ns = np.array([s.num_steps for s in states])
        assert ns[0] == ns_dev[c, 0], (c, ns, ns_dev[c, :T0])
        if np.array_equal(ns, ns_dev[c, :T0]):
            match += 1
            mu = np.array([s.z[0] for s in states])
            th = np.stack([s.z[2:] for s in states])
            np.testing.assert_allclose(site["mu"][c, :T0], mu, rtol=2e-3, atol=2e-3)
            np.testing.assert_allclose(site["theta"][c, :T0], th, rtol=2e-3, atol=2e-3)
    assert match >= int(0.9 * C), f"only {match}/{C} chains reproduced the oracle path"


_fixed_step_case = PC.fixed_step_case


@pytest.mark.parametrize("algo", ["NUTS", "HMC"])
@pytest.mark.parametrize("model,dim", [("logreg", 4), ("logreg", 24), ("logreg", 40), ("logreg", 60),
                                       ("diag_normal", 300), ("diag_normal", 1500), ("funnel", 600),
                                       ("sv", 302), ("bnn", 46), ("bnn", 321), ("bnn", 5038)])
def test_engine_matches_oracle_fixed_step(device, algo, model, dim):
    """No adaptation, fixed step size: every transition is a deterministic function of the
    Philox stream, so device and oracle take the same discrete path up to rounding.  D < 257
    runs the fused step kernel (dim 4, 24, 40, 46, 60: logreg's KB = 1, 2, 3 kernels and, at 64
    chains of D = 60, its H = 0 role-split form), SV / funnel / diagonal normal the persistent wide
    kernel, the BNN the launched D-slice schedule.  Leaf-located (oracle/parity.py, the device's
    decision trace): the reference is the oracle with the potential in rounded float64; a chain
    that parts must do so at a leaf whose decision is a rounding flip of that leaf (HMC: the
    Metropolis decision), and a draw that differs with every decision equal must lie within
    DRAW_MULT x the drift of the rounding calibration (a second float32 potential against the
    same reference) -- tests/parity_cases.py."""
    seed, C, T = 77, 64, 3
    if model == "bnn":
        T = 2  # BNN trees run 255-511 leapfrogs of a tanh network
    extra = {"trajectory_length": 15 * PC.fixed_step_case(model, dim, np.random.RandomState(dim))[5]} \
        if algo == "HMC" else {}
    eng, ref, step, frac, z0, ns, z, _, _ = PC.engine_fixed(model, dim, C, T, seed, C, algo=algo, **extra)
    tr = eng.trace_records()
    kw = dict(algo=algo, **extra)
    hist = PC.oracle_runs(PC.reference_f64(model, ref), dim, C, T, seed, step, z0, **kw)
    constrain = PC.constrain_fn(eng)
    tol = dict(atol=1e-3, rtol=1e-3) if frac < 0.95 else dict(atol=1e-4, rtol=1e-3)
    par = PR.compare_traced(hist, tr, ns, z, to_model=constrain, **tol)
    ctr, cns, cz = PC.as_trace(PC.oracle_runs(PC.second_f32(model, dim, ref), dim, C, T, seed, step, z0, **kw))
    cal = PR.compare_traced(hist, ctr, cns, np.stack([[constrain(w) for w in cc] for cc in cz]), to_model=constrain,
                            through_draws=True, **tol)
    PC.report(par, f"fixed-step {algo} {model} D={dim}", cal=cal, frac=frac)
    # the trace's layout: a NUTS transition records every leaf of its tree, the last one ends it;
    # an HMC transition records its Metropolis decision as leaf 0
    for c in range(C):
        for t in range(T):
            n = int(ns[c, t]) if algo == "NUTS" else 1
            assert np.all(np.isfinite(tr[t, c, :n, PR.T_FLAGS])) and np.all(np.isnan(tr[t, c, n:, PR.T_FLAGS]))
            assert int(tr[t, c, n - 1, PR.T_FLAGS]) & PR.TF_ITER_DONE


def test_covtype_full_size_nuts_matches_oracle(device):
    """BASELINE config 1 at its full data size (581012 x 55, synthetic covtype): after a device
    warmup, 8 chains run 2 traced sampling transitions on the GPU; the oracle's NUTS resumes the
    same chains from the device's post-warmup state on the same Philox stream.  Reference: the
    potential in rounded float64 over the full data (oracle/potentials.py pe_grad_batch);
    calibration: the float32 C restatement (oracle/c/logreg_batch.c) against it.  Tree sizes
    must agree and draws to 1e-4 (posterior sd ~3e-3 at this N) for >= 7 of 8 chains; a chain
    that parts must do so at a leaf whose decision is a rounding flip of that leaf, a draw with
    every decision equal within DRAW_MULT x the calibration's drift (hmc_util.py:1088-1180
    build_tree, examples/covtype.py:66-71)."""
    from numpyro_amd.random import key_to_seed
    from oracle import cpu_batched as CB

    X, y = datasets.covtype_synthetic(seed=0)
    assert X.shape == (581012, 55)
    C, W, T, seed = 8, 100, 2, 5
    Xd, yd = torch.from_numpy(X).to(device), torch.from_numpy(y).to(device)
    mcmc = MCMC(NUTS(P.logistic_regression), num_warmup=W, num_samples=T, num_chains=C)
    mcmc.warmup(seed, Xd, yd)
    st = mcmc.post_warmup_state
    mcmc._engine.set_trace(C, W, T)
    mcmc.run(seed + 1, Xd, yd, extra_fields=("num_steps",))
    tr = mcmc._engine.trace_records()
    mcmc._engine.set_trace(0, 0, 0)
    ns = mcmc.get_extra_fields(group_by_chain=True)["num_steps"].cpu().numpy()
    z = mcmc.get_samples(group_by_chain=True)["coefs"].to(torch.float64).cpu().numpy()
    cols = lambda t: t.detach().cpu().numpy()  # noqa: E731

    def resume():
        return CB.chains_from_state(
            cols(st.z["coefs"]), cols(st.z_grad), cols(st.potential_energy), cols(st.adapt_state.step_size),
            cols(st.adapt_state.inverse_mass_matrix), cols(st.adapt_state.mass_matrix_sqrt), W, key_to_seed(seed + 1),
            W)

    r64 = OP.LogisticRegression(X.astype(np.float64), y.astype(np.float64), dtype=np.float64)
    f64 = lambda Z: tuple(np.asarray(v, np.float32) for v in r64.pe_grad_batch(Z))  # noqa: E731
    _, hist, evals, _ = CB.run_chains(f64, *resume(), T, record=True)
    _, hist32, _, _ = CB.run_chains(CB.LogRegBatch(X, y), *resume(), T, record=True)
    par = PR.compare_traced(hist, tr, ns, z, atol=1e-4)
    ctr, cns, cz = PC.as_trace(hist32)
    cal = PR.compare_traced(hist, ctr, cns, cz, atol=1e-4, through_draws=True)
    print(f"[covtype 581012x55] {evals} oracle leapfrogs per side")
    PC.report(par, "covtype full size", cal=cal)
    assert par["matched"] >= C - 1


def _device_adapt_run(model, dim, C, seed, W):
    """Device warmup of W transitions in segments split at the window ends; returns per-transition
    fields [C, W] (step size, accept prob, tree size), draws [C, W, D] and, at every window
    end e, the device state after transition e - 1 (what the oracle restarts from)."""
    rs = np.random.RandomState(dim)
    args, fm, ref, *_ = _fixed_step_case(model, dim, rs)
    eng = NUTS(fm).make_engine(C, args)
    eng.initialize(seed, W)
    ends = [e + 1 for _, e in H.build_adaptation_schedule(W)]
    cols = {k: native.COLLECT.index(k) for k in ("step_size", "accept_prob", "num_steps")}
    fl, zs, snaps, traces = {k: [] for k in cols}, [], {}, {}
    for e in ends:
        it0 = eng.iteration
        if it0 in ends:  # the oracle restarts from this window end: trace its next 3 transitions
            eng.set_trace(C, it0, 3)
        samples, fields, _ = eng.run(e - eng.iteration, seed)
        if it0 in ends:
            traces[it0] = eng.trace_records()
            eng.set_trace(0, 0, 0)
        for k, i in cols.items():
            fl[k].append(fields[:, i, :C].cpu().numpy())
        zs.append(samples[:, :, :C].cpu().numpy())
        snaps[e] = {n: eng.chain_state(n).cpu().numpy().copy() for n in (
            "z", "zgrad", "pe", "step_size", "inv_mass", "mass_sqrt", "wf_mean", "wf_m2", "wf_n",
            "da_xt", "da_xavg", "da_gavg", "da_t", "da_prox", "window_idx", "mean_acc", "iter")}
    out = {k: np.concatenate(v).T for k, v in fl.items()}
    out["num_steps"] = out["num_steps"].round().astype(int)
    return ref, out, np.concatenate(zs).transpose(2, 0, 1), snaps, ends, traces


@pytest.mark.parametrize("model,dim,C", [("diag_normal", 300, 64), ("logreg", 55, 64)])
def test_adaptation_matches_oracle(device, model, dim, C):
    """warmup_adapter parity (hmc_util.py:518-707) over W = 300, windows [0-74], [75-99],
    [100-149], [150-249], [250-299] (build_adaptation_schedule :387-436).  D = 300 runs the
    wide (D-split) step, D = 55 the fused one.

    1. Teacher-forced adapter: the oracle's warmup_adapter.update_fn fed the device's own accept
       probability and draw of every transition must reproduce the device's step size after
       every transition (dual averaging :637-672, the final x_avg at t = W - 1, the restart at
       window ends :596-635) and its inverse mass diagonal at every window end (diagonal Welford
       :172-196 over the middle windows, the n/(n+5) regularised finalize :198-237).  Same
       inputs, same f32 formulas: rtol 1e-5.
    2. Restarts: from the device's full state at each window end (z, U, grad, step size, mass,
       dual-averaging and Welford state, window index), the oracle's next three transitions must
       take the device's tree sizes, step sizes and draws (the new mass and step size are the
       ones used).  End to end over all 300 transitions the two cannot stay equal: dual averaging
       multiplies accept-probability rounding by sqrt(t)/gamma = 20 sqrt(t), so f32 ΔE rounding
       (~1e-5) grows to 2e-4 step-size differences within 10 transitions even when every tree
       size agrees (measured; DESIGN.md "Adaptation parity")."""
    seed, W = 2024, 300
    ref, dev, draws, snaps, ends, traces = _device_adapt_run(model, dim, C, seed, W)
    assert ends == [75, 100, 150, 250, 300]
    # 1. teacher-forced adapter
    wa_init, wa_update = H.warmup_adapter(W)
    worst_ss, worst_imm = 0.0, 0.0
    for c in range(C):
        st = wa_init((np.zeros(dim, np.float32),), None, np.float32(1.0), mass_matrix_size=dim)
        for t in range(W):
            st = wa_update(t, np.float32(dev["accept_prob"][c, t]), draws[c, t].astype(np.float32), st)
            np.testing.assert_allclose(dev["step_size"][c, t], st.step_size, rtol=1e-5,
                                       err_msg=f"chain {c} step size after transition {t}")
            worst_ss = max(worst_ss, abs(float(dev["step_size"][c, t]) / float(st.step_size) - 1))
            if t + 1 in snaps:
                np.testing.assert_allclose(snaps[t + 1]["inv_mass"][c], st.inverse_mass_matrix, rtol=1e-5,
                                           err_msg=f"chain {c} inverse mass after transition {t}")
                worst_imm = max(worst_imm, float(np.max(np.abs(snaps[t + 1]["inv_mass"][c] /
                                                              st.inverse_mass_matrix - 1))))
                assert int(snaps[t + 1]["window_idx"][c]) == st.window_idx
    print(f"[adapt {model} D={dim}] teacher-forced: max rel diff step size {worst_ss:.2e}, inverse mass {worst_imm:.2e}")
    # 2. oracle restarts from the device state at each window end, leaf-located against the
    # device's decision trace of those transitions
    K = 3
    match, total, drift = 0, 0, 0.0
    for e in ends[:-1]:
        sn = snaps[e]
        hist = []
        for c in range(C):
            o = H.NUTSOracle(PC.f32(ref.pe_grad), dim, W)
            imm = sn["inv_mass"][c].astype(np.float32)
            wa = H.HMCAdaptState(
                np.float32(sn["step_size"][c]), imm, sn["mass_sqrt"][c].astype(np.float32), np.sqrt(imm),
                (np.float32(sn["da_xt"][c]), np.float32(sn["da_xavg"][c]), np.float32(sn["da_gavg"][c]),
                 int(sn["da_t"][c]), np.float32(sn["da_prox"][c])),
                (sn["wf_mean"][c].astype(np.float32), sn["wf_m2"][c].astype(np.float32), int(sn["wf_n"][c])),
                int(sn["window_idx"][c]), None)
            assert int(sn["iter"][c]) == e
            st = H.HMCState(e, sn["z"][c].astype(np.float32), sn["zgrad"][c].astype(np.float32),
                            np.float32(sn["pe"][c]), None, None, None, 0, np.float32(0),
                            np.float32(sn["mean_acc"][c]), False, wa, (seed, c))
            h = []
            for k in range(K):
                if k > 0:
                    # the step size the device adapted to (teacher-forced): dual averaging
                    # restarted at t = 0 multiplies accept-probability rounding by 20 sqrt(t)
                    # (2.6e-4 relative drift measured), which moves later trajectories by more
                    # than rounding; the restart checks the transitions, the teacher-forced
                    # check above the adapter
                    st = st._replace(adapt_state=st.adapt_state._replace(
                        step_size=np.float32(dev["step_size"][c, e + k - 1])))
                h += PC.traced(o, st, 1)
                st = h[-1][0]
                drift = max(drift, abs(float(dev["step_size"][c, e + k]) / float(st.adapt_state.step_size) - 1))
            hist.append(h)
        par = PR.compare_traced(hist, traces[e], dev["num_steps"][:, e:e + K], draws[:, e:e + K], atol=1e-3,
                                rtol=1e-3)
        PC.report(par, f"adapt {model} D={dim} restart at {e}")
        match += par["matched"]
        total += C
    print(f"[adapt {model} D={dim}] restarts at window ends: {match}/{total} chain-windows reproduce "
          f"the next {K} transitions (max step-size rel drift {drift:.1e}: dual averaging restarts at "
          f"t = 0 after a window end, where its gain on accept-probability rounding is largest)")
    assert drift < 1e-2
    assert match >= int(0.95 * total)


@pytest.mark.parametrize("model", ["logreg", "wide"])
def test_num_steps_equals_potential_evaluations(device, model):
    """Every leaf consumes exactly one potential evaluation (the compacted list length),
    summed over the run -- guards the multi-wave / D-split step kernels' state handling."""
    rs = np.random.RandomState(3)
    if model == "logreg":
        X = rs.randn(2000, 55).astype(np.float32)
        y = (rs.rand(2000) < 0.5).astype(np.float32)
        fm = P.logistic_regression
    else:
        X = rs.randn(900).astype(np.float32)
        y = (0.3 + rs.rand(900)).astype(np.float32)
        fm = P.diag_normal
    mcmc = MCMC(NUTS(fm), num_warmup=20, num_samples=10, num_chains=200)
    mcmc.warmup(0, X, y)
    eng = mcmc._engine
    cnt = eng.view("counters")
    logged = torch.zeros(100000, dtype=torch.int32, device=eng.device)
    n = [0]
    orig = eng.potential.evaluate

    def counting(ev, s):
        p = 0 if ev is eng.eval_lists[0] else 1
        logged[n[0]] = cnt[2 + p]
        n[0] += 1
        orig(ev, s)

    eng.potential.evaluate = counting
    mcmc.run(1, X, y, extra_fields=("num_steps",))
    eng.potential.evaluate = orig
    evals = int(logged[:n[0]].sum().item())
    assert evals == int(mcmc.get_extra_fields()["num_steps"].sum().item())


@pytest.mark.parametrize("model", ["eight_schools", "diag_normal"])
def test_persistent_schedule_is_bitwise_the_launched_one(device, model, monkeypatch):
    """nmx_nuts_run_small (one launch for the whole run, potential inline, SURVEY.md §8f row
    1) draws bitwise the samples and extra fields of the launched step/potential loop."""
    if model == "eight_schools":
        fm, args = P.eight_schools, (8, datasets.EIGHT_SCHOOLS_SIGMA, datasets.EIGHT_SCHOOLS_Y)
    else:
        fm, args = P.diag_normal, (np.array([1.0, -2.0, 0.5], np.float32), np.array([1.0, 0.3, 2.0], np.float32))
    out = {}
    from numpyro_amd.engine import Engine

    for mode in ("0", "1"):
        monkeypatch.setattr(Engine, "persistent", mode == "1")
        mcmc = MCMC(NUTS(fm), num_warmup=150, num_samples=100, num_chains=70)
        mcmc.run(5, *args, extra_fields=("num_steps", "diverging", "potential_energy", "accept_prob"))
        out[mode] = (mcmc.get_samples(True), mcmc.get_extra_fields(True), mcmc.last_run_stats["launches"])
    assert out["1"][2] <= 2 and out["0"][2] > 100
    for k, v in out["0"][0].items():
        np.testing.assert_array_equal(out["1"][0][k].cpu().numpy(), v.cpu().numpy(), err_msg=k)
    for k, v in out["0"][1].items():
        np.testing.assert_array_equal(out["1"][1][k].cpu().numpy(), v.cpu().numpy(), err_msg=k)


def test_sync_and_async_schedules_are_bitwise_identical(device):
    args = (8, datasets.EIGHT_SCHOOLS_SIGMA, datasets.EIGHT_SCHOOLS_Y)
    a, _ = _run_engine(args, P.eight_schools, 64, 50, 30, 99, sync=False)
    b, _ = _run_engine(args, P.eight_schools, 64, 50, 30, 99, sync=True)
    for k in ("mu", "tau", "theta"):
        np.testing.assert_array_equal(a.get_samples()[k].cpu().numpy(), b.get_samples()[k].cpu().numpy())
    np.testing.assert_array_equal(a.get_extra_fields()["num_steps"].cpu().numpy(),
                                  b.get_extra_fields()["num_steps"].cpu().numpy())
    # the sync schedule wastes leapfrogs waiting for the slowest chain
    assert b.last_run_stats["launches"] >= a.last_run_stats["launches"]


def test_wide_schedule_invariances(device):
    """D-split step (dim >= 257): sync == async and sharded == unsharded, bitwise; and
    every leaf consumes exactly one evaluation."""
    assert native.lib().nmx_nuts_num_slices(700) > 0 and native.lib().nmx_nuts_num_slices(200) == 0
    rs = np.random.RandomState(0)
    mu = rs.randn(700).astype(np.float32)
    sd = (0.5 + rs.rand(700)).astype(np.float32)
    args = (mu, sd)
    a, _ = _run_engine(args, P.diag_normal, 96, 40, 15, 3, sync=False)
    b, _ = _run_engine(args, P.diag_normal, 96, 40, 15, 3, sync=True)
    lo, _ = _run_engine(args, P.diag_normal, 30, 40, 15, 3, chain_offset=0)
    hi, _ = _run_engine(args, P.diag_normal, 66, 40, 15, 3, chain_offset=30)
    xa = a.get_samples(True)["x"].cpu().numpy()
    np.testing.assert_array_equal(xa, b.get_samples(True)["x"].cpu().numpy())
    np.testing.assert_array_equal(xa[:30], lo.get_samples(True)["x"].cpu().numpy())
    np.testing.assert_array_equal(xa[30:], hi.get_samples(True)["x"].cpu().numpy())
    x = xa.reshape(-1, 700)
    assert np.abs(x.mean(0) - mu).mean() < 0.2 and np.abs(x.std(0) / sd - 1).mean() < 0.2


def _wide_model_case(which):
    if which == "sv":
        return (datasets.sp500_synthetic(T=700),), P.stochastic_volatility, "s"
    if which == "funnel":
        return (900,), P.funnel, "x"
    return (900,), P.funnel_reparam, "x_decentered"


@pytest.mark.parametrize("which", ["sv", "funnel", "funnel_reparam", "funnel_reparam_hmc"])
def test_wide_model_step_matches_launched_loop(device, which, monkeypatch):
    """The two fused schedules of a D-split model against the launched potential +
    nmx_nuts_step loop (six launches per leaf): nmx_nuts_step_wide_model (the model's row
    gradients fused with the leapfrog end, the potential finished in the reduction's last
    block: three launches per leaf) and the persistent per-chain nmx_nuts_run_wide (one launch
    per run, chain-row arena).  Same arithmetic per coordinate; U, the scalar-site gradients
    and the dot products are summed in other fixed orders, so they agree to rounding: fixed
    step size, the discrete paths of >= 90% of chains and their draws to 1e-3 (fp32 rounding
    grows along SV's long trajectories as in the oracle comparisons)."""
    from numpyro_amd.engine import Engine

    hmc = which.endswith("_hmc")
    which = which.replace("_hmc", "")
    args, fm, site = _wide_model_case(which)
    kw = dict(step_size={"sv": 0.005, "funnel": 0.05, "funnel_reparam": 0.3}[which], adapt_step_size=False,
              adapt_mass_matrix=False)
    if which == "sv":
        kw["max_tree_depth"] = 7  # fp32 rounding differences grow along SV's 1023-leaf trees
    if hmc:
        kw.update(kernel_cls=HMC, num_steps=7)
    out, launches = {}, {}
    for mode, (fused, pers) in {"launched": (False, False), "fused": (True, False), "persistent": (True, True)}.items():
        monkeypatch.setattr(Engine, "fused_wide", fused)
        monkeypatch.setattr(Engine, "wide_persistent", pers)
        mcmc, _ = _run_engine(args, fm, 96, 0, 3, 21, **kw)
        out[mode] = (mcmc.get_samples(True)[site].cpu().numpy(),
                     mcmc.get_extra_fields(True)["num_steps"].cpu().numpy(),
                     mcmc.get_extra_fields(True)["potential_energy"].cpu().numpy())
        launches[mode] = mcmc.last_run_stats["launches"]
    assert launches["persistent"] <= 2 < launches["fused"]  # one launch runs the whole segment
    x0, n0, u0 = out["launched"]
    for mode in ("fused", "persistent"):
        x1, n1, u1 = out[mode]
        same = np.all(n0 == n1, axis=1) & np.all(np.isclose(x0, x1, rtol=1e-3, atol=1e-3).reshape(96, -1), axis=1)
        print(f"[wide model {which}{' hmc' if hmc else ''} {mode}] {int(same.sum())}/96 chains: same tree sizes "
              "and draws as the launched loop")
        assert same.sum() >= 86  # the oracle tests' bar (>= 90%) for these stiff targets
        # U agrees where the draws agree closely (at 1e-3-close draws U itself can move by ~1e-2
        # relative: |grad U| ~ 1e2-1e3 along SV's random walk)
        close = same & np.all(np.isclose(x0, x1, rtol=1e-5, atol=1e-5).reshape(96, -1), axis=1)
        # (U ~ 1e2 is the cancellation of sums of ~700 terms whose magnitudes add to ~1e4, summed in
        # another order, at draws equal to 1e-5 with |grad U| ~ 1e3: ~1e-1 absolute)
        np.testing.assert_allclose(u1[close], u0[close], rtol=3e-4, atol=0.2)


@pytest.mark.parametrize("persistent", [True, False])
def test_wide_model_step_invariances(device, persistent, monkeypatch):
    """Both fused wide-model schedules keep the engine's invariances bitwise: sync == async
    (the persistent kernel's lockstep schedule is one launch per transition), and two chain
    shards reproduce the unsharded run (sums in an order fixed by D only)."""
    from numpyro_amd.engine import Engine

    monkeypatch.setattr(Engine, "wide_persistent", persistent)
    args, fm, site = _wide_model_case("sv")
    a, _ = _run_engine(args, fm, 96, 30, 10, 4, sync=False)
    b, _ = _run_engine(args, fm, 96, 30, 10, 4, sync=True)
    lo, _ = _run_engine(args, fm, 40, 30, 10, 4, chain_offset=0)
    hi, _ = _run_engine(args, fm, 56, 30, 10, 4, chain_offset=40)
    xa = a.get_samples(True)[site].cpu().numpy()
    np.testing.assert_array_equal(xa, b.get_samples(True)[site].cpu().numpy())
    np.testing.assert_array_equal(xa[:40], lo.get_samples(True)[site].cpu().numpy())
    np.testing.assert_array_equal(xa[40:], hi.get_samples(True)[site].cpu().numpy())
    assert a.last_run_stats["launches"] > 0


def test_chain_sharding_is_bitwise_invariant(device):
    """Chains keyed by global id: two shards reproduce the full run exactly."""
    args = (8, datasets.EIGHT_SCHOOLS_SIGMA, datasets.EIGHT_SCHOOLS_Y)
    full, _ = _run_engine(args, P.eight_schools, 96, 40, 20, 5)
    lo, _ = _run_engine(args, P.eight_schools, 40, 40, 20, 5, chain_offset=0)
    hi, _ = _run_engine(args, P.eight_schools, 56, 40, 20, 5, chain_offset=40)
    f = full.get_samples(True)["theta"].cpu().numpy()
    np.testing.assert_array_equal(f[:40], lo.get_samples(True)["theta"].cpu().numpy())
    np.testing.assert_array_equal(f[40:], hi.get_samples(True)["theta"].cpu().numpy())


@pytest.mark.parametrize("kernel_cls,dense", [(NUTS, False), (HMC, False)])
def test_unnormalized_normal(device, kernel_cls, dense):
    """test/infer/test_mcmc.py:28-72: mean/std of a Gaussian target, rtol 0.07."""
    true_mean, true_std = 1.0, 2.0
    pot = P.DiagNormal([true_mean], [true_std])
    kw = {"trajectory_length": 8.0} if kernel_cls is HMC else {}
    kernel = kernel_cls(potential_fn=pot, **kw)
    mcmc = MCMC(kernel, num_warmup=500, num_samples=2000, num_chains=32, progress_bar=False)
    mcmc.run(0, init_params=torch.zeros(32, 1))
    x = mcmc.get_samples()["x"].cpu().numpy().ravel()
    np.testing.assert_allclose(x.mean(), true_mean, rtol=0.07)
    np.testing.assert_allclose(x.std(), true_std, rtol=0.07)


def test_eight_schools_posterior(device):
    """README.md:75-91 table (statistical): mu ~ 4.1 +- 3.2 and tau ~ 4 (wide tolerance)."""
    kernel = NUTS(P.eight_schools)
    mcmc = MCMC(kernel, num_warmup=500, num_samples=1000, num_chains=256, chain_method="vectorized")
    mcmc.run(0, 8, datasets.EIGHT_SCHOOLS_SIGMA, y=datasets.EIGHT_SCHOOLS_Y,
             extra_fields=("potential_energy",))
    s = mcmc.get_samples()
    mu = s["mu"].cpu().numpy()
    assert abs(mu.mean() - 4.4) < 0.6
    assert 2.8 < mu.std() < 3.8
    assert 2.5 < s["tau"].cpu().numpy().mean() < 4.5
    pe = mcmc.get_extra_fields()["potential_energy"].cpu().numpy()
    assert -58 < np.mean(-pe) < -50  # "Expected log joint density: -54.55"


def test_logistic_regression_recovers_coefs(device):
    """test/infer/test_mcmc.py:104-168 analogue: N=3000, dim 3, coefs atol 0.4."""
    rs = np.random.RandomState(0)
    true = np.array([1.0, 2.0, 3.0], np.float32)
    X = rs.randn(3000, 3).astype(np.float32)
    y = (rs.rand(3000) < 1 / (1 + np.exp(-X @ true))).astype(np.float32)
    mcmc = MCMC(NUTS(P.logistic_regression), num_warmup=300, num_samples=300, num_chains=64)
    mcmc.run(2, X, y)
    m = mcmc.get_samples()["coefs"].cpu().numpy().mean(0)
    np.testing.assert_allclose(m, true, atol=0.4)


def test_resume_from_post_warmup_state(device):
    args = (8, datasets.EIGHT_SCHOOLS_SIGMA, datasets.EIGHT_SCHOOLS_Y)
    mcmc = MCMC(NUTS(P.eight_schools), num_warmup=100, num_samples=50, num_chains=32)
    mcmc.warmup(3, *args)
    st = mcmc.post_warmup_state
    assert int(st.i[0]) == 100
    mcmc.run(4, *args)
    first = mcmc.get_samples()["mu"].cpu().numpy()
    assert first.shape == (32 * 50,)
    mcmc.run(4, *args)  # post_warmup_state still set -> same samples again
    np.testing.assert_array_equal(first, mcmc.get_samples()["mu"].cpu().numpy())
    assert int(mcmc.last_state.i[0]) == 150


def test_stochastic_volatility_runs_and_is_sane(device):
    """Config C4 shape (T=2517) at small chain count: finite draws, sigma and nu in range."""
    r = datasets.sp500_synthetic()
    mcmc = MCMC(NUTS(P.stochastic_volatility), num_warmup=100, num_samples=50, num_chains=64)
    mcmc.run(0, r, extra_fields=("num_steps", "diverging"))
    s = mcmc.get_samples()
    assert s["s"].shape == (64 * 50, r.size)
    assert torch.isfinite(s["s"]).all()
    sig = s["sigma"].cpu().numpy()
    assert 0.0 < np.median(sig) < 0.2
    assert np.median(s["nu"].cpu().numpy()) > 1.0


def test_funnel_diag_runs(device):
    mcmc = MCMC(NUTS(P.funnel), num_warmup=200, num_samples=200, num_chains=128)
    mcmc.run(0, 10, extra_fields=("diverging",))
    y = mcmc.get_samples()["y"].cpu().numpy()
    assert abs(y.mean()) < 1.5 and 1.5 < y.std() < 4.0  # y ~ N(0, 3) (centred funnel is hard)


def test_funnel_reparam_non_centered(device, capsys):
    """examples/funnel.py non-centred run: y ~ N(0, 3) and x_decentered ~ N(0, 1) are recovered
    without divergences; the deterministic site x = exp(y/2) x_decentered comes back with the
    samples and print_summary leaves it out unless exclude_deterministic=False."""
    mcmc = MCMC(NUTS(P.funnel_reparam), num_warmup=300, num_samples=300, num_chains=128)
    mcmc.run(0, 10, extra_fields=("diverging",))
    s = {k: v.cpu().numpy() for k, v in mcmc.get_samples().items()}
    assert set(s) == {"x", "x_decentered", "y"}
    assert s["x"].shape == s["x_decentered"].shape == (128 * 300, 9)
    np.testing.assert_allclose(s["x"], np.exp(s["y"] / 2)[:, None] * s["x_decentered"], rtol=1e-6)
    assert abs(s["y"].mean()) < 0.3 and abs(s["y"].std() - 3.0) < 0.3
    assert abs(s["x_decentered"].mean()) < 0.05 and abs(s["x_decentered"].std() - 1.0) < 0.05
    assert int(mcmc.get_extra_fields()["diverging"].sum()) == 0
    def row_names():
        return {ln.split()[0] for ln in capsys.readouterr().out.splitlines() if ln.strip()}

    mcmc.print_summary()
    names = row_names()
    assert "x_decentered[0]" in names and "y" in names and "x[0]" not in names
    mcmc.print_summary(exclude_deterministic=False)
    assert "x[0]" in row_names()


@pytest.mark.parametrize("dense", [False, True])
def test_bnn_fits_data(device, dense):
    """examples/bnn.py (small H): the posterior-mean network fits the training data and
    prec_obs is of the order of the noise level (Y is standardized, sigma_obs 0.05 before).
    dense=True: per-chain dense matrices (D = 61)."""
    X, Y = datasets.bnn_data(N=60, D_X=3)
    H = 6
    mcmc = MCMC(NUTS(P.bnn, dense_mass=dense), num_warmup=300, num_samples=100, num_chains=64)
    mcmc.run(0, X, Y, H)
    s = {k: v.cpu().numpy().astype(np.float64) for k, v in mcmc.get_samples().items()}
    assert all(np.isfinite(v).all() for v in s.values())
    h1 = np.tanh(np.einsum("nd,sdh->snh", X.astype(np.float64), s["w1"]))
    h2 = np.tanh(np.einsum("snh,shk->snk", h1, s["w2"]))
    yhat = np.einsum("snk,sko->sno", h2, s["w3"])[..., 0].mean(0)
    r2 = 1 - ((Y[:, 0] - yhat) ** 2).mean() / Y[:, 0].var()
    assert r2 > 0.8, r2
    assert np.median(s["prec_obs"]) > 5.0


@pytest.mark.parametrize("model,dense", [("logreg", False), ("diag_normal", False), ("mvn", True)])
def test_kernel_init_sample_loop_matches_mcmc_run(device, model, dense):
    """MCMCKernel plug-in surface (mcmc.py:90-120, hmc.py:740-822): a caller that drives the
    kernel itself -- init, then one sample() per transition, as _single_chain_mcmc's
    fori_collect loop does (mcmc.py:461-513) -- gets bitwise the draws, tree sizes and step
    sizes of MCMC.run with the same key (fused, wide and dense pooled-adaptation paths; the
    dense window's pool persists across sample() calls)."""
    rs = np.random.RandomState(11)
    if model == "mvn":
        D = 6
        a = rs.randn(D, D)
        args, fm, site = (np.zeros(D), a @ a.T + 0.5 * np.eye(D)), P.multivariate_normal, "x"
    else:
        dim = 40 if model == "logreg" else 300
        args, fm, _, site, *_ = _fixed_step_case(model, dim, rs)
    C, W, S, seed = 40, 30, 12, 7
    kern = NUTS(fm, dense_mass=dense)
    st = kern.init(seed, W, model_args=args, num_chains=C)
    zs, ns, ss = [], [], []
    for i in range(W + S):
        st = kern.sample(st, args, {})
        if i >= W:
            zs.append(st.z[site].clone())
            ns.append(st.num_steps.clone())
            ss.append(st.adapt_state.step_size.clone())
    post = kern.postprocess_fn(args, {})(st.z)
    assert set(post) >= {site}
    mcmc = MCMC(NUTS(fm, dense_mass=dense), num_warmup=W, num_samples=S, num_chains=C)
    mcmc.run(seed, *args, extra_fields=("num_steps", "adapt_state.step_size"))
    ref = mcmc.get_samples(group_by_chain=True)[site]
    ef = mcmc.get_extra_fields(group_by_chain=True)
    torch.testing.assert_close(torch.stack(zs, 1), ref, rtol=0, atol=0)
    torch.testing.assert_close(torch.stack(ns, 1), ef["num_steps"], rtol=0, atol=0)
    torch.testing.assert_close(torch.stack(ss, 1), ef["adapt_state.step_size"], rtol=0, atol=0)
    # a state the engine has moved past holds no device copy: resuming from it is refused
    kern.sample(st, args, {})
    with pytest.raises(ValueError):
        kern.sample(st, args, {})


@pytest.mark.parametrize("model,dim", [("diag_normal", 40), ("logreg", 55), ("diag_normal", 300)])
def test_find_heuristic_step_size_matches_oracle(device, model, dim):
    """find_heuristic_step_size=True (hmc.py:320-331): find_reasonable_step_size
    (hmc_util.py:314-384) at init and at the middle window end of W = 150 ([75-99]).  The
    oracle's adapter with the same search (same Philox momentum per attempt), fed the device's
    accept probabilities and draws, must reproduce the device's step size after every
    transition: the initial search from each chain's initial point, and the window-end search
    from its draw at t = 99 (rtol 1e-5; the search's result is a power-of-two multiple of its
    start, so a mismatch would be a whole factor 2)."""
    seed, C, W = 31, 64, 150
    rs = np.random.RandomState(dim)
    args, fm, ref, *_ = _fixed_step_case(model, dim, rs)
    eng = NUTS(fm, find_heuristic_step_size=True).make_engine(C, args)
    eng.initialize(seed, W)
    ss0 = eng.chain_state("step_size").cpu().numpy().copy()
    z0 = eng.chain_state("z").cpu().numpy().copy()
    samples, fields, _ = eng.run(W, seed)
    acc = fields[:, native.COLLECT.index("accept_prob"), :C].cpu().numpy().T
    ss = fields[:, native.COLLECT.index("step_size"), :C].cpu().numpy().T
    draws = samples[:, :, :C].cpu().numpy().transpose(2, 0, 1)
    pe_grad = lambda z: tuple(np.asarray(v, np.float32) if np.ndim(v) else np.float32(v)  # noqa: E731
                              for v in ref.pe_grad(z))
    moved = 0
    for c in range(C):
        o = H.NUTSOracle(pe_grad, dim, W, find_heuristic_step_size=True)
        st = o.init(z0[c], seed, c)
        np.testing.assert_allclose(ss0[c], st.adapt_state.step_size, rtol=1e-6, err_msg=f"chain {c} initial search")
        wa = st.adapt_state
        for t in range(W):
            z = draws[c, t].astype(np.float32)
            pe, g = pe_grad(z)
            wa = o.wa_update(t, np.float32(acc[c, t]), H.IntegratorState(z, None, pe, g), wa)
            np.testing.assert_allclose(ss[c, t], wa.step_size, rtol=1e-5, err_msg=f"chain {c} after transition {t}")
        moved += int(ss0[c] != 1.0)
    assert moved > 0  # the search changed the initial step size of at least some chains


# a step-size search attempt decided within this fraction of its energies' magnitude (|E_current| +
# |E_new|) of the threshold is a rounding tie: two float32 implementations (the device's whitened
# products, the oracle's mass_matrix_sqrt @ eps) may decide it either way
SEARCH_TIE = 1e-5


@pytest.mark.parametrize("mass", ["adapted", "given"])
@pytest.mark.parametrize("model,dim", [("diag_normal", 40), ("logreg", 55)])
def test_find_heuristic_step_size_dense_matches_oracle(device, model, dim, mass):
    """find_heuristic_step_size with dense_mass=True: the search runs in the engine's whitened
    coordinates with momentum p = T^T M^-1 eps (the reference's r = M^-1 eps,
    hmc_util.py:359) at init and after the window-end re-expression.  "adapted": per-chain
    matrices from the window [75, 99] (searched at the new matrix, hmc_util.py:609-626);
    "given": a fixed non-diagonal inverse_mass_matrix, adapt_mass_matrix=False (one shared
    whitening; the window end still searches).  Oracle: the reference adapter with dense_mass,
    fed the device's accept probabilities and draws, reproduces every transition's step size
    (rtol 1e-5: a search mismatch would be a whole factor 2), except where a search attempt's
    decision margin (-dE - log 0.8) is within rounding of zero (SEARCH_TIE x the energies'
    magnitude): there the device's result is teacher-forced and the count of such ties printed."""
    seed, C, W = 31, 64, 150
    rs = np.random.RandomState(dim)
    args, fm, ref, *_ = _fixed_step_case(model, dim, rs)
    kw = {}
    if mass == "given":
        q = rs.randn(dim, dim) / np.sqrt(dim)
        kw = dict(inverse_mass_matrix=(q @ q.T + 0.5 * np.eye(dim)).astype(np.float32), adapt_mass_matrix=False)
    eng = NUTS(fm, find_heuristic_step_size=True, dense_mass=True, **kw).make_engine(C, args)
    assert eng.chain_dense == (mass == "adapted")
    eng.initialize(seed, W)
    ss0 = eng.chain_state("step_size").cpu().numpy().copy()
    z0 = eng.model_state()[0].cpu().numpy()
    samples, fields, _ = eng.run(W, seed)
    acc = fields[:, native.COLLECT.index("accept_prob"), :C].cpu().numpy().T
    ss = fields[:, native.COLLECT.index("step_size"), :C].cpu().numpy().T
    draws = samples[:, :, :C].cpu().numpy().transpose(2, 0, 1)
    pe_grad = lambda z: tuple(np.asarray(v, np.float32) if np.ndim(v) else np.float32(v)  # noqa: E731
                              for v in ref.pe_grad(z))
    changed, ties = 0, []

    def at_tie(o):
        return any(abs(m) <= SEARCH_TIE * sc for m, sc in o.search_margins)

    for c in range(C):
        o = H.NUTSOracle(pe_grad, dim, W, find_heuristic_step_size=True, dense_mass=True, **kw)
        st = o.init(z0[c], seed, c)
        if not np.isclose(ss0[c], st.adapt_state.step_size, rtol=1e-5):
            assert at_tie(o), (c, ss0[c], st.adapt_state.step_size, o.search_margins)
            ties.append((c, "init"))
            o.force_search = ss0[c]
            st = o.init(z0[c], seed, c)
        wa = st.adapt_state
        for t in range(W):
            z = draws[c, t].astype(np.float32)
            pe, g = pe_grad(z)
            zi = H.IntegratorState(z, None, pe, g)
            wa_new = o.wa_update(t, np.float32(acc[c, t]), zi, wa)
            if not np.isclose(ss[c, t], wa_new.step_size, rtol=1e-5) and o.search_margins and at_tie(o):
                ties.append((c, t))
                o.force_search = ss[c, t]
                wa_new = o.wa_update(t, np.float32(acc[c, t]), zi, wa)
            o.search_margins = []
            wa = wa_new
            np.testing.assert_allclose(ss[c, t], wa.step_size, rtol=1e-5, err_msg=f"chain {c} after transition {t}")
        changed += int(ss[c, 99] != ss[c, 98])
    print(f"[heuristic dense {model} {mass}] {len(ties)} searches decided at a rounding tie (teacher-forced): {ties}")
    assert len(ties) <= C // 8
    assert np.any(ss0 != 1.0) and changed > 0


@pytest.mark.parametrize("model,dim", [("diag_normal", 40), ("logreg", 55)])
def test_find_heuristic_step_size_without_warmup(device, model, dim):
    """num_warmup = 0: wa_init still runs find_reasonable_step_size whenever adapt_step_size is
    set (hmc.py:319-339 -> hmc_util.py:572-576), and with no warmup the chains sample at the
    searched step size.  Oracle: the same search on the same Philox stream from each chain's
    initial point."""
    seed, C, S = 31, 64, 3
    rs = np.random.RandomState(dim)
    args, fm, ref, *_ = _fixed_step_case(model, dim, rs)
    eng = NUTS(fm, find_heuristic_step_size=True).make_engine(C, args)
    eng.initialize(seed, 0)
    ss0 = eng.chain_state("step_size").cpu().numpy().copy()
    z0 = eng.chain_state("z").cpu().numpy().copy()
    _, fields, _ = eng.run(S, seed)
    ss = fields[:, native.COLLECT.index("step_size"), :C].cpu().numpy().T
    np.testing.assert_array_equal(ss, np.repeat(ss0[:, None], S, axis=1))
    pe_grad = lambda z: tuple(np.asarray(v, np.float32) if np.ndim(v) else np.float32(v)  # noqa: E731
                              for v in ref.pe_grad(z))
    for c in range(C):
        st = H.NUTSOracle(pe_grad, dim, 0, find_heuristic_step_size=True).init(z0[c], seed, c)
        np.testing.assert_allclose(ss0[c], st.adapt_state.step_size, rtol=1e-6, err_msg=f"chain {c}")
    assert np.any(ss0 != 1.0)


@pytest.mark.parametrize("which", ["covtype", "eight_schools", "funnel_reparam", "sv", "bnn"])
def test_frontend_models_run_like_fused_models(device, which):
    """NUTS(model) with a model written against numpyro's API (tests/model_zoo.py) runs on the
    fused kernel its structure maps to: draws, tree sizes and deterministic sites are bitwise
    those of the registered fused model."""
    import model_zoo as Z

    if which == "covtype":
        X, y = datasets.covtype_synthetic(n_rows=2000, seed=0)
        args, m, fm = (X, y), Z.covtype_model, P.logistic_regression
    elif which == "eight_schools":
        args, m, fm = (8, datasets.EIGHT_SCHOOLS_SIGMA, datasets.EIGHT_SCHOOLS_Y), Z.eight_schools, P.eight_schools
    elif which == "funnel_reparam":
        args, m, fm = (10,), Z.funnel_reparam, P.funnel_reparam
    elif which == "sv":
        args, m, fm = (datasets.sp500_synthetic(T=300),), Z.stochastic_volatility, P.stochastic_volatility
    else:
        X, Y = datasets.bnn_data(N=40, D_X=3)
        args, m, fm = (X, Y, 5), Z.bnn, P.bnn
    out = []
    for model in (m, fm):
        mcmc = MCMC(NUTS(model), num_warmup=40, num_samples=20, num_chains=48)
        mcmc.run(3, *args, extra_fields=("num_steps",))
        out.append((mcmc.get_samples(True), mcmc.get_extra_fields(True)["num_steps"]))
    (sa, na), (sb, nb) = out
    assert set(sa) == set(sb)
    for k in sa:
        np.testing.assert_array_equal(sa[k].cpu().numpy(), sb[k].cpu().numpy(), err_msg=k)
    np.testing.assert_array_equal(na.cpu().numpy(), nb.cpu().numpy())


@pytest.mark.parametrize("groups,C,sync", [(2, 256, False), (4, 512, False), (2, 256, True), (4, 512, True)])
def test_chain_groups_are_bitwise_the_one_stream_loop(device, groups, C, sync, monkeypatch):
    """Chain groups (nmx_nuts_config.num_groups): the launched fused step and the covtype
    potential per group on its own stream, each group with its own compacted lists and DONE
    count.  A chain's computation does not depend on its group or on how the streams
    interleave: draws, tree sizes and energies equal the one-stream loop bitwise -- also under
    the lockstep schedule (sync), where a waiting chain's release is read while other groups'
    streams are still adding to the transition counts (decided once per chain: nuts.hip
    wait_released; round 5 caught a 16-chain block whose waves disagreed)."""
    from numpyro_amd.engine import Engine

    X, y = datasets.covtype_synthetic(n_rows=4000, seed=1)
    out = {}
    for G in (1, groups):
        monkeypatch.setattr(Engine, "chain_groups", G)
        mcmc, _ = _run_engine((X, y), P.logistic_regression, C, 30, 12, 3, sync=sync)
        assert mcmc._engine._groups() == G
        ef = mcmc.get_extra_fields(True)
        out[G] = (mcmc.get_samples(True)["coefs"].cpu().numpy(), ef["num_steps"].cpu().numpy(),
                  ef["potential_energy"].cpu().numpy())
    for a, b in zip(out[1], out[groups]):
        np.testing.assert_array_equal(a, b)


def test_covtype_full_size_recovers_ref_params(device):
    """BASELINE config 1's data at full size: the synthetic covtype labels are drawn from
    Bernoulli(sigmoid(X . ref_params)) with the reference's coefficient vector
    (examples/covtype.py:79-139, datasets.COVTYPE_REF_COEFS), so at N = 581012 the posterior
    concentrates around ref_params (sd ~ 3e-3): each posterior mean lies within 5 posterior sd of
    its generating value, and the standardized errors are of unit size (mean square <= 3)."""
    X, y = datasets.covtype_synthetic(seed=0)
    Xd, yd = torch.from_numpy(X).to(device), torch.from_numpy(y).to(device)
    mcmc = MCMC(NUTS(P.logistic_regression), num_warmup=150, num_samples=40, num_chains=32, progress_bar=False)
    mcmc.run(11, Xd, yd)
    c = mcmc.get_samples()["coefs"].to(torch.float64).cpu().numpy()  # [C * S, 55]
    m, sd = c.mean(0), c.std(0)
    zerr = (m - datasets.COVTYPE_REF_COEFS) / sd
    print(f"[covtype ref_params] posterior sd {sd.min():.2e}..{sd.max():.2e}, max |z| {np.abs(zerr).max():.2f}, "
          f"mean z^2 {np.mean(zerr ** 2):.2f}")
    assert np.all(np.abs(zerr) <= 5.0), np.argsort(-np.abs(zerr))[:5]
    assert np.mean(zerr ** 2) <= 3.0


def test_derived_extra_fields(device):
    """HMCState fields the device does not collect per transition (hmc.py:31-48): z_grad is the
    model's potential evaluated again at the unconstrained draws -- the same per-chain kernel, so
    the last draw's gradient equals last_state.z_grad bitwise and every draw's matches the float64
    oracle's gradient to f32 rounding; r is None (fresh momentum every transition), NUTS has no
    trajectory_length (None), HMC's is its configured value; the sampling draws' inverse mass
    matrix is the post-warmup one.  Samples are unchanged by asking for z_grad (positive sites
    constrained on the host instead of the device: to the ulp)."""
    args = (8, datasets.EIGHT_SCHOOLS_SIGMA, datasets.EIGHT_SCHOOLS_Y)
    C, W, S = 16, 60, 12
    plain = MCMC(NUTS(P.eight_schools), num_warmup=W, num_samples=S, num_chains=C, progress_bar=False)
    plain.run(3, *args)
    mcmc = MCMC(NUTS(P.eight_schools), num_warmup=W, num_samples=S, num_chains=C, progress_bar=False)
    mcmc.run(3, *args, extra_fields=("z_grad", "trajectory_length", "r", "adapt_state.inverse_mass_matrix"))
    ef = mcmc.get_extra_fields(group_by_chain=True)
    assert ef["r"] is None and ef["trajectory_length"] is None
    zg = ef["z_grad"]
    assert set(zg) == {"mu", "tau", "theta"} and zg["theta"].shape == (C, S, 8)
    pot = mcmc._engine.model_potential
    flat = torch.cat([zg[n].reshape(C, S, -1) for n, _, _ in pot.sites], dim=2)  # [C, S, D]
    assert torch.equal(flat[:, -1].cpu(), mcmc.last_state.z_grad.cpu())
    imm = ef["adapt_state.inverse_mass_matrix"]
    assert imm.shape == (C, S, 10) and torch.equal(imm[:, 0].cpu(), mcmc.last_state.adapt_state.inverse_mass_matrix.cpu())
    for k, v in plain.get_samples(True).items():
        torch.testing.assert_close(mcmc.get_samples(True)[k].cpu(), v.cpu(), rtol=1e-6, atol=0)
    ref = OP.EightSchools(datasets.EIGHT_SCHOOLS_Y, datasets.EIGHT_SCHOOLS_SIGMA)
    s = mcmc.get_samples(True)
    for c in range(C):
        for t in range(S):
            zu = np.concatenate([[float(s["mu"][c, t])], [np.log(float(s["tau"][c, t]))],
                                 s["theta"][c, t].cpu().numpy()])
            g64 = ref.pe_grad(zu.astype(np.float64))[1]
            np.testing.assert_allclose(flat[c, t].cpu().numpy(), g64, rtol=1e-4, atol=1e-4)
    h = MCMC(HMC(P.eight_schools, trajectory_length=1.5), num_warmup=20, num_samples=4, num_chains=4,
             progress_bar=False)
    h.run(1, *args, extra_fields=("trajectory_length",))
    tl = h.get_extra_fields()["trajectory_length"]
    assert tl.shape == (16,) and torch.all(tl == 1.5)
    with pytest.raises(ValueError):
        MCMC(NUTS(P.eight_schools), num_warmup=10, num_samples=2, num_chains=4, progress_bar=False).warmup(
            0, *args, collect_warmup=True, extra_fields=("adapt_state.inverse_mass_matrix",))
