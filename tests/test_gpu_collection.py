"""Thinned collection on every step schedule.

A chain's computation does not depend on what is collected, so a run with thinning k equals the
unthinned run of the same seed bitwise on the rows fori_collect keeps: for n transitions the rows
start + k - 1 :: k with start = n % k (numpyro/util.py:330-346).  The device reads
collect_thinning in tree_phase (csrc/nuts.hip: the slot off / thin, written when off % thin ==
thin - 1) once per kernel family -- one row of tests/ending_cases.py's schedule table each -- and the
dense path has a host twin (Engine._run_window copies the slots of a middle window,
_convert_slots maps the others to model space, _search_at_window_end rewrites a slot's step
size).  The expected rows are indexed out of the unthinned arrays here, not by Engine._slot_of
(the code under test).  Every site and every collected field is compared with assert_array_equal."""
import numpy as np
import pytest

import ending_cases as EC
from numpyro_amd import datasets
from numpyro_amd import potentials as P
from numpyro_amd.infer import MCMC, NUTS
from oracle import hmc_ref as H

pytestmark = pytest.mark.gpu

C, SEED = EC.C, 5
FIELDS = ("num_steps", "accept_prob", "mean_accept_prob", "potential_energy", "energy", "diverging",
          "adapt_state.step_size")


def kept(n, k):
    """Rows of n transitions that fori_collect keeps at thinning k (util.py:330-346)."""
    start = n % k
    return np.arange(start + k - 1, n, k)


def test_kept_rows():
    assert kept(20, 3).tolist() == [4, 7, 10, 13, 16, 19] and kept(7, 3).tolist() == [3, 6]
    assert kept(7, 7).tolist() == [6] and kept(7, 8).tolist() == [] and kept(20, 8).tolist() == [11, 19]
    assert kept(7, 1).tolist() == list(range(7))


def _arrays(mcmc):
    out = {f"site {k}": v.cpu().numpy() for k, v in mcmc.get_samples(group_by_chain=True).items()}
    out.update({k: v.cpu().numpy() for k, v in mcmc.get_extra_fields(group_by_chain=True).items()})
    assert set(FIELDS) <= set(out)
    return out


def _both_phases(fm, args, W, S, thinning, **kw):
    """warmup(collect_warmup=True) and run of one MCMC: ({name: [C, rows, ...]} of each, engine)."""
    mcmc = MCMC(NUTS(fm, **kw), num_warmup=W, num_samples=S, num_chains=C, thinning=thinning, progress_bar=False)
    mcmc.warmup(SEED, *args, collect_warmup=True, extra_fields=FIELDS)
    warm = _arrays(mcmc)
    mcmc.run(SEED, *args, extra_fields=FIELDS)
    return warm, _arrays(mcmc), mcmc._engine


def _assert_thinned(label, full, thin, n, k):
    rows = kept(n, k)
    assert set(full) == set(thin)
    for name, v in full.items():
        assert v.shape[:2] == (C, n), (label, name, v.shape)
        assert thin[name].shape == (C, len(rows)) + v.shape[2:], (label, name, thin[name].shape)
        np.testing.assert_array_equal(thin[name], v[:, rows], err_msg=f"{label}: {name}")


def _row_kernel(row):
    cs = EC.row_case(row)
    kw = {} if cs.dense is None else dict(dense_mass=True, inverse_mass_matrix=cs.dense, adapt_mass_matrix=False)
    return cs.case[1], cs.case[0], kw


_unthinned = {}


def _full(key, fm, args, W, S, **kw):
    """The unthinned run of a configuration, once per module (never mutated)."""
    if key not in _unthinned:
        _unthinned[key] = _both_phases(fm, args, W, S, 1, **kw)[:2]
    return _unthinned[key]


@pytest.mark.parametrize("thinning", [3, 7, 8])
@pytest.mark.parametrize("row", list(EC.ROWS))
def test_thinned_run_keeps_the_unthinned_rows(device, row, thinning, monkeypatch):
    """Default adaptation (chain-rows: a given dense matrix, the step adapted), 20 warmup
    transitions collected and 7 samples.  thinning 3: both phases start at a non-zero row (20 % 3 =
    2, 7 % 3 = 1); 7: the run keeps its last transition only; 8: the run keeps nothing ([C, 0, ...]
    arrays, no slot written) while the warmup keeps rows 11 and 19."""
    W, S = 20, 7
    EC.patch_engine(monkeypatch, row)
    fm, args, kw = _row_kernel(row)
    full_w, full_s = _full(row, fm, args, W, S, **kw)
    warm, samp, eng = _both_phases(fm, args, W, S, thinning, **kw)
    EC.assert_schedule(eng, row)
    _assert_thinned(f"{row} thinning {thinning} warmup", full_w, warm, W, thinning)
    _assert_thinned(f"{row} thinning {thinning} run", full_s, samp, S, thinning)
    if thinning == 8:
        assert all(v.shape[1] == 0 for v in samp.values())
    # the runs being compared did something: trees of more than one leaf, an adapted step
    assert full_w["num_steps"].max() > 1 and np.ptp(full_w["adapt_state.step_size"]) > 0


@pytest.mark.parametrize("dense_mass, k, search", [
    pytest.param(True, 3, False, id="True"), pytest.param("pooled", 3, False, id="pooled"),
    pytest.param(True, 4, True, id="True-search-thinning4")])
def test_thinned_dense_adaptation_keeps_the_unthinned_rows(device, dense_mass, k, search):
    """Eight schools with an adapted dense mass (per chain, pooled): 40 warmup transitions have one
    middle window (6 to 35), inside which Engine._run_window runs unthinned and copies the kept
    slots on the host; outside it _convert_slots maps the kept slots to model space.  With
    find_heuristic_step_size at thinning 4 the kept rows 3, 7, ..., 39 hold row 35, the window's
    last transition: its slot, copied on the host, is then rewritten by the step-size search
    (Engine._search_at_window_end)."""
    W, S = 40, 7
    sched = H.build_adaptation_schedule(W)
    assert [tuple(w) for w in sched[1:-1]] == [(6, 35)]
    rows = kept(W, k)
    assert np.sum((rows >= 6) & (rows <= 35)) >= 3 and np.sum(rows < 6) >= 1 and np.sum(rows > 35) >= 1
    kw = dict(dense_mass=dense_mass, find_heuristic_step_size=True) if search else dict(dense_mass=dense_mass)
    args = (8, datasets.EIGHT_SCHOOLS_SIGMA, datasets.EIGHT_SCHOOLS_Y)
    full_w, full_s = _full(("eight", dense_mass, search), P.eight_schools, args, W, S, **kw)
    warm, samp, eng = _both_phases(P.eight_schools, args, W, S, k, **kw)
    assert eng.dense and eng.chain_dense == (dense_mass is True)
    _assert_thinned(f"eight schools dense_mass={dense_mass} warmup", full_w, warm, W, k)
    _assert_thinned(f"eight schools dense_mass={dense_mass} run", full_s, samp, S, k)
    if search:
        assert rows.tolist() == list(range(3, 40, 4)) and 35 in rows
        # the searched step is what the window's last transition reports
        step = full_w["adapt_state.step_size"]
        assert np.any(step[:, 35] != step[:, 34])


def test_thinned_step_size_search_rewrites_the_kept_slot(device, monkeypatch):
    """find_heuristic_step_size on the fused-8 row: the search at the end of the middle window
    rewrites the step size of the slot of the window's last transition
    (Engine._search_at_window_end).  30 warmup transitions end their middle window at transition
    26, a row that thinning 3 keeps (rows = 2 mod 3)."""
    W, S, k = 30, 7, 3
    row = "fused-8"
    sched = H.build_adaptation_schedule(W)
    assert len(sched) == 3
    end = sched[1][1]
    assert end in kept(W, k)
    EC.patch_engine(monkeypatch, row)
    fm, args, kw = _row_kernel(row)
    kw["find_heuristic_step_size"] = True
    full_w, full_s = _full((row, "search"), fm, args, W, S, **kw)
    warm, samp, eng = _both_phases(fm, args, W, S, k, **kw)
    EC.assert_schedule(eng, row)
    _assert_thinned(f"{row} search warmup", full_w, warm, W, k)
    _assert_thinned(f"{row} search run", full_s, samp, S, k)
    # the searched step is what the window's last transition reports: it starts the next window
    step = full_w["adapt_state.step_size"]
    assert np.any(step[:, end] != step[:, end - 1])
