"""The covtype kernel's hand-placed, rotated tile loop (potential_logreg.hip, x3_item SCHED 1) at
the smallest shapes where a software pipeline that carries part of a tile's epilogue across the
tile boundary can go wrong.

D = 55 is the instance k_logreg_x3<4, 2, 1> that has the schedule.  For N in {1, 33, 257, 768,
1061} x3_num_splits gives 8 row splits, which then hold 0 / 1 tiles (N = 1, 33: only the bare
prologue and the last-tile code), 2 / 1 / 0 (257: one pipelined step, then the drain), 3 each
(768: both copies of the step, the accumulators ending on the other one) and 5 / ... / 4 / 0
(1061: odd and even counts side by side, a ragged last tile).  300 chains are three chain groups,
the last with 44 chains -- one full wave, one partial, two inactive waves in a live workgroup --
and 257 chains leave a single chain in the last group.  A compacted list of 300 scattered chains
inside ldc = 512 runs the same kernel through the index list.

Checks, for O(1) and saturated logits (potential_cases.logreg_case): potential_cases.check_logreg
against the float64 oracle, and U and the gradient of chains 0:70 and 0:20 evaluated again as tail
launches (the role-split and the narrow form, which the schedule does not touch) bitwise equal to
the same chains of the main-form launch.
"""
import numpy as np
import pytest

import potential_cases as K
from test_gpu_potentials import _eval, _eval_list

pytestmark = pytest.mark.gpu

NS = (1, 33, 257, 768, 1061)
TAILS = (70, 20)  # the role-split form (33..256 chains), the narrow form (<= 32)


def _check_main_and_tails(pot, X, y, Z, ref, device, label):
    """Main-form launches over 300 and 257 chains against the oracle; chains 0:70 and 0:20 of the
    300-chain launch bitwise equal to their tail launches."""
    pe_r, g_r = ref
    pe_a, g_a = _eval(pot, Z, device)
    ra = K.logreg_errors(pe_a, g_a, X, y, Z, ref)
    print(f"[logreg schedule] {label} C={len(Z)}: error / tolerance U {ra[0]:.3f} grad {ra[1]:.3f}")
    K.check_logreg(pe_a, g_a, X, y, Z, ref, label=f"{label} C={len(Z)}")
    n = 257
    pe_b, g_b = _eval(pot, Z[:n], device)
    K.check_logreg(pe_b, g_b, X, y, Z[:n], (pe_r[:n], g_r[:n]), label=f"{label} C={n}")
    np.testing.assert_array_equal(pe_b, pe_a[:n], err_msg=f"{label}: 257 vs 300 chains")
    np.testing.assert_array_equal(g_b, g_a[:n], err_msg=f"{label}: 257 vs 300 chains")
    for n in TAILS:
        pe_t, g_t = _eval(pot, Z[:n], device)
        np.testing.assert_array_equal(pe_t, pe_a[:n], err_msg=f"{label}: tail launch of chains 0:{n}")
        np.testing.assert_array_equal(g_t, g_a[:n], err_msg=f"{label}: tail launch of chains 0:{n}")


@pytest.mark.parametrize("regime", K.REGIMES)
@pytest.mark.parametrize("N", NS)
def test_logreg_schedule_tile_counts_and_chain_groups(device, N, regime):
    """D = 55 at every tile count per split named above, 300 and 257 chains."""
    from numpyro_amd.potentials import LogisticRegression

    with np.errstate(over="ignore"):
        X, y, Z, ref = K.logreg_reference(N, 55, K.LOGREG_C, regime)
    _check_main_and_tails(LogisticRegression(X, y), X, y, Z, ref, device, f"D=55 N={N} {regime}")


@pytest.mark.parametrize("regime", K.REGIMES)
@pytest.mark.parametrize("N", NS)
def test_logreg_schedule_compacted_list(device, N, regime):
    """300 scattered chains of a 512-chain batch as a compacted list (the main form: more than
    256 listed chains): against the oracle, and the first 70 and 20 listed chains bitwise equal to
    their own dense tail launches."""
    from numpyro_amd.potentials import LogisticRegression

    with np.errstate(over="ignore"):
        X, y, Z, (pe_r, g_r) = K.logreg_reference(N, 55, 512, regime)
    pot = LogisticRegression(X, y)
    idx = np.random.RandomState(N).permutation(512)[:300]
    pe_l, g_l = _eval_list(pot, Z, idx, device)
    label = f"D=55 N={N} {regime} 300 listed of 512"
    K.check_logreg(pe_l, g_l, X, y, Z[idx], (pe_r[idx], g_r[idx]), label=label)
    for n in TAILS:
        pe_t, g_t = _eval(pot, Z[idx[:n]], device)
        np.testing.assert_array_equal(pe_t, pe_l[:n], err_msg=f"{label}: tail launch of the first {n}")
        np.testing.assert_array_equal(g_t, g_l[:n], err_msg=f"{label}: tail launch of the first {n}")


@pytest.mark.parametrize("regime", K.REGIMES)
def test_logreg_schedule_other_instance(device, regime):
    """D = 60 (KB = 4, H = 0) at N = 257 with the same two checks.  Only k_logreg_x3<4, 2, 1> has
    the hand-placed schedule; this instance keeps SCHED 0 and must be untouched by it."""
    from numpyro_amd.potentials import LogisticRegression

    with np.errstate(over="ignore"):
        X, y, Z, ref = K.logreg_reference(257, 60, K.LOGREG_C, regime)
    _check_main_and_tails(LogisticRegression(X, y), X, y, Z, ref, device, f"D=60 N=257 {regime}")
