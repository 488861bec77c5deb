"""How a device transition ends, and what it writes when it does, against the oracle on every
step schedule (tests/ending_cases.py: the schedule table, the oracle cases and their legs).

tree_phase (csrc/nuts.hip) decides the end of a transition -- a divergent leaf, a U-turn inside
the subtree or of the whole tree, the depth cap -- writes the per-transition fields and picks the
collection slot, once per kernel family.  The leaf-by-leaf parity tests (test_gpu_nuts.py,
test_gpu_parity_trace.py, test_gpu_dense.py) run at settings where every transition ends by a
U-turn; here each schedule runs

* a mixed leg whose step and divergence threshold make the reference end transitions by a
  divergence (at the transition's first leaf and at the first, a middle and the last leaf of a later
  subtree) as well as by both kinds of U-turn -- counted on the reference's leaf records and
  asserted before the device is looked at;
* a cap leg, max_tree_depth = (2, 4) over the switch from warmup to sampling depth, and depth 1;
  on the one-lane schedules the library's deepest tree (depth 12, 4095 leaves);
* an HMC leg whose divergences must follow the energy threshold whatever the Metropolis decision;

with the decision trace compared leaf by leaf (oracle/parity.py compare_traced, the tolerances of
test_engine_matches_oracle_fixed_step) and the fields of every transition checked: exactly against
the device's own trace on every chain, and against the reference on the chains that follow it.

Measured on an MI355X (device / calibration matched chains of 70, largest energy and
potential-energy discrepancy on matched chains relative to max(1, |value|)): docs/DESIGN_LOG.md."""
import numpy as np
import pytest

import ending_cases as EC
import parity_cases as PC
from numpyro_amd import native
from oracle import parity as PR

pytestmark = pytest.mark.gpu

C, T, SEED = EC.C, EC.T, EC.SEED
SLACK = max(2, C // 20)  # matched chains: the device may trail the calibration by this many


def _fields(fields, n):
    """{collected field: [n, T]} of an engine run's field buffer [T, NC, ldc]."""
    f = fields[:, :, :n].permute(2, 0, 1).cpu().numpy()
    return {name: f[:, :, i] for i, name in enumerate(native.COLLECT)}


def _run(row, leg, monkeypatch, **over):
    """The row's device run of a leg: (case, key, engine, trace, num_steps, draws, fields, step,
    threshold, oracle keywords)."""
    EC.patch_engine(monkeypatch, row)
    key = EC.ROWS[row][0]
    cs = EC.row_case(row, leg)
    kw = dict(case=cs.case, dense_matrix=cs.dense)
    chains, iters, k = C, T, C
    if leg == "mixed":
        step, mde = cs.mixed
    elif leg == "cap":
        step, mde = EC.CAP_STEP, 1000.0
        kw.update(max_tree_depth=EC.CAP_DEPTHS, num_warmup=EC.CAP_WARMUP)
    elif leg == "cap1":
        step, mde = EC.CAP_STEP, 1000.0
        kw.update(max_tree_depth=1)
    elif leg == "hmc":
        step, mde = cs.hmc
        kw.update(algo="HMC", num_steps=EC.HMC_STEPS, trajectory_length=None)
    elif leg == "deep":
        step, mde, iters, k = EC.DEEP_STEP, 1000.0, EC.DEEP_T, EC.DEEP_CHAINS
        kw.update(max_tree_depth=native.MAX_TREE_DEPTH)
    kw.update(over)
    eng, _, _, _, _, ns, z, _, fields = PC.engine_fixed(cs.model, cs.dim, chains, iters, SEED, k, step=step,
                                                        max_delta_energy=mde, **kw)
    EC.assert_schedule(eng, row)
    assert eng.cfg.max_delta_energy == np.float32(mde)
    return cs, key, eng, eng.trace_records(), ns, z, _fields(fields, chains), step, mde


def _parity(label, key, leg, cs, tr, ns, z, mde):
    """compare_traced of the device against the leg's reference, with the calibration's record:
    every parting a rounding flip at its leaf, draws within the calibration's drift, and the
    matched chains within SLACK of the calibration's."""
    hist = EC.history(key, leg, "ref")
    n = len(hist)
    par = PR.compare_traced(hist, tr, ns[:n], z[:n], max_delta_energy=mde, **cs.tol)
    cal = EC.calibration(key, leg, L=max(1024, tr.shape[2]))
    PC.report(par, label, cal=cal)
    print(f"[{label}] matched chains: device {par['matched']}, calibration {cal['matched']} of {n}")
    assert par["matched"] >= cal["matched"] - SLACK, (par["matched"], cal["matched"])
    return hist, par, cal


def _check_fields(label, key, leg, hist, par, tr, F, step, hmc=False, first_iter=0):
    """The fields a transition writes at its end (tree_phase: it_accept, it_nsteps, it_div, the
    slot's row).  On every traced chain, exactly, against the device's own trace; on the chains that
    follow the reference through a transition, against the reference's fields."""
    k, iters = tr.shape[1], tr.shape[0]
    flags = tr[..., PR.T_FLAGS]
    rows = np.isfinite(flags).sum(axis=2).T  # [k, iters]
    ns = np.rint(F["num_steps"]).astype(np.int64)
    # --- every chain, exact
    np.testing.assert_array_equal(F["i"], np.tile(np.arange(first_iter + 1, first_iter + iters + 1), (len(ns), 1)),
                                  err_msg=f"{label}: iter")
    bits = np.ascontiguousarray(F["step_size"]).view(np.uint32)
    assert np.all(bits == np.float32(step).view(np.uint32)), f"{label}: step_size"
    if hmc:
        assert np.all(rows == 1) and np.all(ns == EC.HMC_STEPS), f"{label}: HMC rows / num_steps"
    else:
        np.testing.assert_array_equal(ns[:k], rows, err_msg=f"{label}: num_steps vs finite trace rows")
    worst = 0.0
    for c in range(k):
        for t in range(iters):
            n = int(rows[c, t])
            last = int(tr[t, c, n - 1, PR.T_FLAGS])
            assert last & PR.TF_ITER_DONE, (label, c, t)
            assert bool(F["diverging"][c, t] > 0.5) == bool(last & PR.TF_DIVERGE), \
                f"{label}: chain {c} transition {t}: diverging {F['diverging'][c, t]} vs the last leaf's flag {last}"
            de = tr[t, c, :n, PR.T_DE].astype(np.float64)
            de = np.where(np.isnan(de), np.inf, de)
            want = float(np.mean(np.minimum(1.0, np.exp(-de))))
            err, bound = abs(float(F["accept_prob"][c, t]) - want), (n + 4) * 2.0 ** -24
            worst = max(worst, err / bound)
            assert err <= bound, (f"{label}: chain {c} transition {t}: accept_prob {F['accept_prob'][c, t]} vs the "
                                  f"mean over its {n} leaves {want} (bound {bound:.3g})")
    print(f"[{label}] accept_prob vs the mean over the trace's leaves: worst error / bound {worst:.3g}")
    # --- chains on the reference's path
    R = EC.state_fields(hist)
    ok = EC.matched_through(par, len(hist), iters)
    np.testing.assert_array_equal(ns[:len(hist)][ok], R["num_steps"][ok], err_msg=f"{label}: num_steps")
    np.testing.assert_array_equal(F["diverging"][:len(hist)][ok] > 0.5, R["diverging"][ok],
                                  err_msg=f"{label}: diverging")
    for c, h in enumerate(hist):
        for t in range(iters):
            if not ok[c, t]:
                continue
            leaves = h[t][2]
            d = tr[t, c, :len(leaves), PR.T_DE].astype(np.float64)
            o = np.array([r["dE"] for r in leaves], np.float64)
            with np.errstate(invalid="ignore"):
                diff = np.where((d == o) | (np.isnan(d) & np.isnan(o)), 0.0, np.abs(d - o))
            bound = float(np.max(diff)) + PR.P_FLOOR
            err = abs(float(F["accept_prob"][c, t]) - R["accept_prob"][c, t])
            assert err <= bound, (f"{label}: chain {c} transition {t}: accept_prob {F['accept_prob'][c, t]} vs "
                                  f"reference {R['accept_prob'][c, t]} (leaf energies differ by <= {bound:.3g})")
    # energy / potential energy: within DE_REL_MULT x the calibration's own discrepancy
    Q = EC.state_fields(EC.history(key, leg, "cal"))
    cal_ok = EC.matched_through(EC.calibration(key, leg, L=max(1024, tr.shape[2])), len(hist), iters)
    dcal = EC.field_discrepancy(Q, R, cal_ok)
    ddev = EC.field_discrepancy({n_: F[n_][:len(hist)].astype(np.float64) for n_ in ("energy", "potential_energy")},
                                R, ok)
    print(f"[{label}] on matched chains, relative to max(1, |value|): energy device {ddev['energy']:.3g} / "
          f"calibration {dcal['energy']:.3g}, potential_energy device {ddev['potential_energy']:.3g} / "
          f"calibration {dcal['potential_energy']:.3g}")
    for n_ in ("energy", "potential_energy"):
        assert ddev[n_] <= PR.DE_REL_MULT * dcal[n_], f"{label}: {n_} {ddev[n_]:.3g} vs calibration {dcal[n_]:.3g}"
    return R, ok


@pytest.mark.parametrize("row", list(EC.ROWS))
def test_mixed_endings_match_oracle(device, row, monkeypatch):
    """Divergent endings (first leaf of the transition; first, middle, last leaf of a subtree),
    in-subtree and whole-tree U-turns in one run per schedule: the reference reaches them (asserted
    first), the device takes them at the same leaves, and the transition's fields say so."""
    key = EC.ROWS[row][0]
    kinds, pos = EC.assert_mixed_conditions(key)
    if EC.ROWS[row][2]:
        EC.assert_wide_conditions()
    print(f"[mixed {row}] reference: {EC.fmt_counts(kinds, pos)}")
    cs, key, eng, tr, ns, z, F, step, mde = _run(row, "mixed", monkeypatch)
    hist, par, _ = _parity(f"mixed {row}", key, "mixed", cs, tr, ns, z, mde)
    R, ok = _check_fields(f"mixed {row}", key, "mixed", hist, par, tr, F, step)
    # the device reaches the endings too (not only the chains that parted early do)
    assert int((F["diverging"][ok] > 0.5).sum()) >= 10 and int((F["diverging"][ok] < 0.5).sum()) >= 10


@pytest.mark.parametrize("leg", ["cap", "cap1"])
@pytest.mark.parametrize("row", list(EC.ROWS))
def test_depth_cap_ends_the_transition(device, row, leg, monkeypatch):
    """cap: max_tree_depth = (2, 4) with num_warmup = 2 -- 3, 3, 15, 15 leaves on every chain, the
    depth switching at the first sampling transition; cap1: depth 1, where the single leaf is its
    own subtree and the whole tree."""
    cs, key, eng, tr, ns, z, F, step, mde = _run(row, leg, monkeypatch)
    want = EC.CAP_SIZES if leg == "cap" else (1,) * T
    np.testing.assert_array_equal(ns, np.tile(want, (C, 1)))
    assert not (F["diverging"] > 0.5).any()
    hist, par, _ = _parity(f"{leg} {row}", key, leg, cs, tr, ns, z, mde)
    _check_fields(f"{leg} {row}", key, leg, hist, par, tr, F, step)


@pytest.mark.parametrize("row", EC.SMALL_ROWS)
def test_deepest_tree(device, row, monkeypatch):
    """native.MAX_TREE_DEPTH = 12: 4095 leaves on every transition of 70 chains (the checkpoint
    rows up to max_depth_alloc - 1 are only touched at full depth), 4 traced chains x 2
    transitions against the oracle."""
    cs, key, eng, tr, ns, z, F, step, mde = _run(row, "deep", monkeypatch)
    assert eng.md == native.MAX_TREE_DEPTH == 12 and tr.shape[1:3] == (EC.DEEP_CHAINS, 4096)
    np.testing.assert_array_equal(ns, np.full((C, EC.DEEP_T), 4095))
    assert not (F["diverging"] > 0.5).any() and np.all(np.isfinite(F["accept_prob"]))
    hist, par, _ = _parity(f"depth 12 {row}", key, "deep", cs, tr, ns, z, mde)
    _check_fields(f"depth 12 {row}", key, "deep", hist, par, tr, F, step)


@pytest.mark.parametrize("row", EC.HMC_ROWS)
def test_hmc_divergence_follows_the_energy_threshold(device, row, monkeypatch):
    """HMC, 5 leapfrogs, a lowered threshold: `diverging` is dE > max_delta_energy at the end point,
    whether the Metropolis step accepts it or not (hmc.py:401-414)."""
    key = EC.ROWS[row][0]
    div, div_acc = EC.hmc_counts(EC.history(key, "hmc", "ref"))
    print(f"[hmc {row}] reference: {div} divergent transitions, {div_acc} of them accepted")
    assert div >= 5 and div_acc >= 1
    cs, key, eng, tr, ns, z, F, step, mde = _run(row, "hmc", monkeypatch)
    hist, par, _ = _parity(f"hmc {row}", key, "hmc", cs, tr, ns, z, mde)
    _check_fields(f"hmc {row}", key, "hmc", hist, par, tr, F, step, hmc=True)
    de, fl = tr[:, :, 0, PR.T_DE].T, tr[:, :, 0, PR.T_FLAGS].T.astype(np.int64)
    np.testing.assert_array_equal(F["diverging"] > 0.5, de > np.float32(mde))
    accepted = (fl & PR.TF_TAKE_LEAF) != 0
    n_acc, n_rej = int(((F["diverging"] > 0.5) & accepted).sum()), int(((F["diverging"] > 0.5) & ~accepted).sum())
    print(f"[hmc {row}] device: {n_acc} divergent and accepted, {n_rej} divergent and rejected")
    assert n_acc >= 1 and n_rej >= 1


@pytest.mark.parametrize("row", list(EC.ROWS))
def test_mean_accept_prob_restarts_after_warmup(device, row, monkeypatch):
    """mean_accept_prob is the float32 running mean m + (a - m) / n of the transition's accept_prob
    with n restarting at 1 at the first sampling transition (hmc.py:509-513): 5 warmup and 5
    sampling transitions, nothing adapted, all collected; the recurrence fed the device's own
    accept_prob gives the device's field."""
    EC.patch_engine(monkeypatch, row)
    cs = EC.row_case(row)
    W, n_it = 5, 10
    eng, _, _, _, _, ns, _, _, fields = PC.engine_fixed(cs.model, cs.dim, C, n_it, SEED, 0, trace=False,
                                                        case=cs.case, dense_matrix=cs.dense, step=EC.CAP_STEP,
                                                        num_warmup=W)
    EC.assert_schedule(eng, row)
    F = _fields(fields, C)
    a = F["accept_prob"].astype(np.float32)
    assert np.ptp(a) > 1e-3 and np.all(a > 0.25)  # the mean is not trivially constant, and no term is tiny
    m, want = np.zeros(C, np.float32), np.zeros((C, n_it), np.float32)
    for t in range(n_it):
        n = np.float32(t + 1 if t < W else t + 1 - W)
        m = (m + (a[:, t] - m) / n).astype(np.float32)
        want[:, t] = m
    np.testing.assert_allclose(F["mean_accept_prob"], want, rtol=1e-6)
    np.testing.assert_allclose(F["mean_accept_prob"][:, W], a[:, W], rtol=1e-6)
    np.testing.assert_array_equal(F["i"], np.tile(np.arange(1, n_it + 1), (C, 1)))
