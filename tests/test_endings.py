"""The inputs of tests/test_gpu_endings.py on the CPU: the reference oracle and the calibration
(a second float32 statement of the potential) alone end transitions in every way the GPU legs are
meant to test -- so a badly chosen step or threshold fails here, and cannot pass quietly there --
and the calibration's own record against the reference is clean (every parting a rounding flip at
its leaf).  Prints the ending counts of every case (tests/ending_cases.py holds the table)."""
import numpy as np
import pytest

import ending_cases as EC
from numpyro_amd import native
from oracle import parity as PR

KEYS = ("dn3", "dn40", "dn300", "fnc300", "fnc300d")


def test_ending_classification():
    """ending(): kind and divergent position from hand-written leaf records."""
    def leaf(depth, **kw):
        r = dict(depth=depth, diverge=False, turn_sub=False, turn_tree=False, iter_done=False)
        r.update(kw)
        return r
    assert EC.ending([leaf(0, diverge=True, iter_done=True)]) == ("divergent", "d0")
    assert EC.ending([leaf(0), leaf(1, diverge=True, iter_done=True)]) == ("divergent", "first")
    assert EC.ending([leaf(0), leaf(1), leaf(1, diverge=True, iter_done=True)]) == ("divergent", "last")
    three = [leaf(0), leaf(1), leaf(1), leaf(2), leaf(2)]
    assert EC.ending(three + [leaf(2, diverge=True, iter_done=True)]) == ("divergent", "mid")
    assert EC.ending(three + [leaf(2), leaf(2, diverge=True, iter_done=True)]) == ("divergent", "last")
    # an in-subtree U-turn sets the combined tree's turning flag too: it is the in-subtree kind
    assert EC.ending(three + [leaf(2, turn_sub=True, turn_tree=True, iter_done=True)]) == ("turn_sub", None)
    assert EC.ending([leaf(0), leaf(1), leaf(1, turn_tree=True, iter_done=True)]) == ("turn_tree", None)
    assert EC.ending([leaf(0), leaf(1), leaf(1, iter_done=True)]) == ("cap", None)


@pytest.mark.parametrize("side", ["ref", "cal"])
@pytest.mark.parametrize("key", KEYS)
def test_mixed_leg_reaches_every_ending(key, side):
    """Per case: >= 10 divergent endings and >= 10 others; a divergence at the transition's first
    leaf and at the first leaf of a later subtree at least twice each; no transition capped."""
    kinds, pos = EC.assert_mixed_conditions(key, side)
    cs = EC.cases()[key]
    rows = ", ".join(r for r in EC.ROWS if EC.ROWS[r][0] == key)
    print(f"[mixed {key} {side}; rows {rows}] step {cs.mixed[0]}, max_delta_energy {cs.mixed[1]}: "
          f"{EC.fmt_counts(kinds, pos)}")
    assert kinds["cap"] == 0 and kinds["turn_tree"] + kinds["turn_sub"] >= 10


@pytest.mark.parametrize("side", ["ref", "cal"])
def test_wide_rows_diverge_inside_and_at_the_end_of_a_subtree(side):
    tot = EC.assert_wide_conditions(side)
    print(f"[mixed wide rows {side}] divergent at d0 / first / mid / last: {[tot[p] for p in EC.POSITIONS]}")


@pytest.mark.parametrize("leg", ["mixed", "cap", "cap1"])
@pytest.mark.parametrize("key", KEYS)
def test_calibration_record_is_clean(key, leg):
    """The calibration against the reference: every located parting is a rounding flip at its
    leaf (also those after a draw mismatch), so what it measures is rounding alone."""
    cal = EC.calibration(key, leg)
    bad = [PR.describe(m) for m in cal["mismatches"] if m["leaf"] is not None and not m["explained"]]
    bad += [str(m) for m in cal["partings_after_draw"] if not m["explained"]]
    print(f"[{leg} {key}] calibration {PR.counts(cal)}, leaf-energy discrepancy {cal['max_dE_err']:.3g} "
          f"(relative {cal['max_dE_rel']:.3g})")
    assert not bad, bad
    assert cal["matched"] >= EC.C - EC.C // 5  # a calibration that mostly left the path measures nothing


@pytest.mark.parametrize("side", ["ref", "cal"])
@pytest.mark.parametrize("key", KEYS)
def test_cap_leg_caps_every_transition(key, side):
    """max_tree_depth = (2, 4) with two warmup transitions: 3, 3, 15, 15 leaves on every chain,
    none by a U-turn or a divergence; max_tree_depth = 1: single-leaf trees."""
    ns = EC.state_fields(EC.history(key, "cap", side))["num_steps"]
    np.testing.assert_array_equal(ns, np.tile(EC.CAP_SIZES, (EC.C, 1)))
    kinds, _ = EC.ending_counts(EC.history(key, "cap", side))
    assert kinds["cap"] == EC.C * EC.T, kinds
    ns1 = EC.state_fields(EC.history(key, "cap1", side))["num_steps"]
    np.testing.assert_array_equal(ns1, np.ones((EC.C, EC.T), int))
    kinds1, _ = EC.ending_counts(EC.history(key, "cap1", side))
    print(f"[cap {key} {side}] depth (2, 4): sizes {ns[0].tolist()} on every chain; depth 1: endings {kinds1}")


@pytest.mark.parametrize("side", ["ref", "cal"])
@pytest.mark.parametrize("key", [EC.ROWS[r][0] for r in EC.HMC_ROWS])
def test_hmc_leg_diverges_whatever_the_metropolis_decision(key, side):
    """>= 5 divergent HMC transitions, >= 1 of them accepted."""
    div, div_acc = EC.hmc_counts(EC.history(key, "hmc", side))
    cs = EC.cases()[key]
    print(f"[hmc {key} {side}] step {cs.hmc[0]}, max_delta_energy {cs.hmc[1]}: {div} divergent of {EC.C * EC.T}, "
          f"{div_acc} of them accepted")
    assert div >= 5 and div_acc >= 1 and div - div_acc >= 1


def test_deepest_tree_runs_to_the_cap():
    """max_tree_depth = 12 (native.MAX_TREE_DEPTH): 4095 leaves on every transition, no divergence."""
    hist = EC.history("dn3", "deep", "ref")
    f = EC.state_fields(hist)
    assert native.MAX_TREE_DEPTH == 12
    np.testing.assert_array_equal(f["num_steps"], np.full((EC.DEEP_CHAINS, EC.DEEP_T), 4095))
    assert not f["diverging"].any() and np.all(np.isfinite(f["accept_prob"]))
