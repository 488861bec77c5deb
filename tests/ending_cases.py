"""How a transition ends, on every step schedule: the table of schedules and oracle cases shared
by tests/test_endings.py (CPU: the inputs reach the endings they are meant to) and
tests/test_gpu_endings.py / tests/test_gpu_collection.py (the device against them).  No tests here.

tree_phase (csrc/nuts.hip) ends a transition, writes its fields and picks its collection slot; it
is instantiated by five kernel families, each with its own reduction of the U-turn dots and its
own way of writing the collected draw.  One row per schedule, at the smallest shape that takes it,
70 chains (no multiple of 16 or 64: the last wave and the last block are ragged):

    small-persistent  k_nuts_persistent      diag_normal D = 3
    small-launched    k_nuts_step<1,16>      the same, Engine.persistent off
    fused-8           k_nuts_step<8,16>      diag_normal D = 40
    wide-launched     k_wide_v1/r/s/v2       diag_normal D = 300
    wide-fused        k_wide_leaf/rs/v2      funnel_reparam D = 300, Engine.wide_persistent off
    wide-persistent   k_wide_persistent<256> funnel_reparam D = 300
    chain-rows        k_chain_step<256>      funnel_reparam D = 300 behind a given dense mass matrix

The reference is the oracle (oracle/hmc_ref.py) with the potential in rounded float64, the
calibration the same chains under a second float32 statement of the potential (tests/parity_cases.py).

Legs (fixed step, nothing adapts, T = 4 transitions):

* mixed: a step and a divergence threshold (`Case.mixed`) at which the reference alone ends
  transitions by a divergence (at the transition's first leaf, at the first, a middle and the
  last leaf of a later subtree), by an in-subtree U-turn and by a whole-tree U-turn;
* cap: max_tree_depth = (2, 4) with 2 warmup transitions at step 0.05 -- every tree runs to its
  cap, 3, 3, 15, 15 leaves -- and max_tree_depth = 1 (the small rows on the depth-12 leg's
  potential: leg_case);
* depth 12 (the small rows): the library's deepest tree, 4095 leaves;
* HMC (fused-8, wide-persistent): 5 leapfrogs, a threshold that some end points pass.

Reference ending counts of the mixed leg, 70 chains x 4 transitions (divergent / whole-tree
U-turn / in-subtree U-turn / cap; divergent position d0 / first / mid / last), as
test_endings.py prints them:

    dn3        step 0.3,  threshold 0.3     23 / 146 / 111 / 0    13 /  9 /  1 /  0
    dn40       step 0.8,  threshold 5.0     28 / 238 /  14 / 0    17 /  9 /  2 /  0
    dn300      step 0.8,  threshold 5.0    108 / 172 /   0 / 0    64 / 17 / 11 / 16
    fnc300     step 0.4,  threshold 0.5     90 / 188 /   2 / 0    10 / 31 / 16 / 33
    fnc300d    step 0.4,  threshold 0.5    109 / 135 /  36 / 0    14 / 38 / 24 / 33

(dn300 and fnc300d were tuned on the CPU oracle: at D = 300 a diagonal normal with sd in [0.5, 1.5]
needs step 0.8 before leaf energies pass a threshold of 5; thresholds of 10 and more leave fewer
than 10 divergences past the first leaf.)
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import parity_cases as PC
from numpyro_amd import native
from oracle import parity as PR

C, T, SEED = 70, 4, 77
CAP_DEPTHS, CAP_WARMUP, CAP_STEP, CAP_SIZES = (2, 4), 2, 0.05, (3, 3, 15, 15)
DEEP_STEP, DEEP_CHAINS, DEEP_T = 1e-3, 4, 2  # depth 12: diag_normal D = 3, mu = 0, sd = 4
HMC_STEPS = 5


def funnel_nc_f32(dim):
    """The non-centred funnel's potential (oracle/potentials.py FunnelNonCentered) stated a second
    time in plain float32: the calibration side, as parity_cases.second_f32 is for diag_normal."""
    f = np.float32
    k, half_log_2pi, log_norm_y = f(dim - 1), f(0.9189385332046727), f(2.0175508218727822)

    def pe_grad(z):
        z = np.asarray(z, f)
        x, y = z[:-1], z[-1]
        g = z.copy()
        g[-1] = y / f(9.0)
        return f(y * y / f(18.0) + log_norm_y + f(0.5) * np.dot(x, x) + k * half_log_2pi), g
    return pe_grad


@dataclass
class Case:
    """One oracle case: `case` is a parity_cases.fixed_step_case tuple; mixed / hmc = (step,
    max_delta_energy); dense = the given inverse mass matrix or None; tol = the draw tolerance of
    compare_traced (test_engine_matches_oracle_fixed_step's)."""
    key: str
    model: str
    dim: int
    case: tuple
    mixed: tuple
    hmc: tuple | None = None
    dense: np.ndarray | None = None
    tol: dict = field(default_factory=lambda: dict(atol=1e-4, rtol=1e-3))

    @property
    def ref(self):
        return PC.reference_f64(self.model, self.case[2])

    @property
    def cal(self):
        if self.model == "funnel_reparam":
            return funnel_nc_f32(self.dim)
        return PC.second_f32(self.model, self.dim, self.case[2])

    def oracle_kw(self):
        return {} if self.dense is None else dict(dense_mass=True, inverse_mass_matrix=self.dense)


def _dn3(mu, sd):
    from numpyro_amd import potentials as P
    from oracle import potentials as OP

    mu, sd = np.asarray(mu, np.float32), np.asarray(sd, np.float32)
    return (mu, sd), P.diag_normal, OP.IsoNormal(mu, sd, dtype=np.float32), "x", (lambda z: z), 0.05, 0.95, None


@functools.lru_cache(maxsize=None)
def cases():
    fs = lambda model, dim: PC.fixed_step_case(model, dim, np.random.RandomState(dim))  # noqa: E731
    D = 300
    a = np.random.RandomState(1).randn(D, D) / np.sqrt(12.0 * D)
    M = (a @ a.T + np.eye(D)).astype(np.float32)
    out = [
        # mu, sd of test_persistent_schedule_is_bitwise_the_launched_one
        Case("dn3", "diag_normal", 3, _dn3([1.0, -2.0, 0.5], [1.0, 0.3, 2.0]), mixed=(0.3, 0.3)),
        Case("dn40", "diag_normal", 40, fs("diag_normal", 40), mixed=(0.8, 5.0), hmc=(0.5, 1.0)),
        Case("dn300", "diag_normal", 300, fs("diag_normal", 300), mixed=(0.8, 5.0)),
        Case("fnc300", "funnel_reparam", 300, fs("funnel_reparam", 300), mixed=(0.4, 0.5), hmc=(0.4, 0.5)),
        # the whitening's GEMMs round the draws too: the looser of the fixed-step test's tolerances
        Case("fnc300d", "funnel_reparam", 300, fs("funnel_reparam", 300), mixed=(0.4, 0.5), dense=M,
             tol=dict(atol=1e-3, rtol=1e-3)),
    ]
    return {c.key: c for c in out}


def deep_case():
    """Depth 12: diag_normal D = 3 with mu = 0, sd = 4 at step 1e-3 -- no U-turn within 4095 leaves."""
    return Case("dn3deep", "diag_normal", 3, _dn3([0.0, 0.0, 0.0], [4.0, 4.0, 4.0]), mixed=(DEEP_STEP, 1000.0))


# row -> (oracle case, Engine class attributes to set, wide)
ROWS = {
    "small-persistent": ("dn3", {}, False),
    "small-launched": ("dn3", {"persistent": False}, False),
    "fused-8": ("dn40", {}, False),
    "wide-launched": ("dn300", {}, True),
    "wide-fused": ("fnc300", {"wide_persistent": False}, True),
    "wide-persistent": ("fnc300", {}, True),
    "chain-rows": ("fnc300d", {}, True),
}
SMALL_ROWS = ("small-persistent", "small-launched")
HMC_ROWS = ("fused-8", "wide-persistent")


def leg_case(key, leg):
    """The oracle case of a leg.  The D = 3 case's sd = 0.3 coordinate starts up to 13 sd from its
    mean (init_to_uniform), where the force turns the momentum round within a few leaves at any
    step: its cap legs run on the depth-12 leg's potential (mu = 0, sd = 4) instead."""
    if leg == "deep" or (key == "dn3" and leg in ("cap", "cap1")):
        return deep_case()
    return cases()[key]


def row_case(row, leg="mixed"):
    return leg_case(ROWS[row][0], leg)


def patch_engine(monkeypatch, row):
    from numpyro_amd.engine import Engine

    for k, v in ROWS[row][1].items():
        monkeypatch.setattr(Engine, k, v)


def assert_schedule(eng, row):
    """The engine took the row's schedule, by its own attributes (Engine._run_segment's choices)."""
    slices = native.lib().nmx_nuts_num_slices(eng.D)
    small, wide = eng._persistent_model(), eng._wide_model()
    got = dict(slices=slices, small=small is not None, wide=wide is not None, persist_wide=eng.persist_wide,
               crow=eng.crow, dense=eng.dense, chain_dense=eng.chain_dense, D=eng.D)
    want = {
        "small-persistent": small is not None and slices == 0 and not eng.crow and not eng.dense,
        "small-launched": small is None and eng.D < 16 and slices == 0 and not eng.crow and not eng.dense,
        "fused-8": small is None and 16 <= eng.D and slices == 0 and not eng.crow and not eng.dense,
        "wide-launched": slices > 0 and wide is None and not eng.persist_wide and not eng.crow and not eng.dense,
        "wide-fused": slices > 0 and wide is not None and not eng.persist_wide and not eng.crow and not eng.dense,
        "wide-persistent": slices > 0 and eng.persist_wide and eng.crow and not eng.dense,
        "chain-rows": slices > 0 and eng.dense and eng.crow and not eng.chain_dense and not eng.persist_wide,
    }[row]
    assert want, f"{row}: the engine runs another schedule: {got}"


# ------------------------------------------------------------------ oracle histories (cached)
@functools.lru_cache(maxsize=None)
def history(key, leg, side):
    """Oracle histories of a case's leg ('mixed', 'cap', 'cap1', 'hmc', 'deep'), side 'ref' or
    'cal': hist[c][t] = (state, decisions, leaves).  Cached: never mutate."""
    cs = leg_case(key, leg)
    pe = cs.ref if side == "ref" else cs.cal
    kw = cs.oracle_kw()
    if leg == "mixed":
        step, mde = cs.mixed
        return PC.oracle_runs(pe, cs.dim, C, T, SEED, step, None, max_delta_energy=mde, **kw)
    if leg == "cap":
        return PC.oracle_runs(pe, cs.dim, C, T, SEED, CAP_STEP, None, num_warmup=CAP_WARMUP,
                              max_tree_depth=CAP_DEPTHS, **kw)
    if leg == "cap1":
        return PC.oracle_runs(pe, cs.dim, C, T, SEED, CAP_STEP, None, max_tree_depth=1, **kw)
    if leg == "hmc":
        step, mde = cs.hmc
        return PC.oracle_runs(pe, cs.dim, C, T, SEED, step, None, algo="HMC", num_steps=HMC_STEPS,
                              trajectory_length=None, max_delta_energy=mde, **kw)
    if leg == "deep":
        return PC.oracle_runs(pe, cs.dim, DEEP_CHAINS, DEEP_T, SEED, DEEP_STEP, None,
                              max_tree_depth=native.MAX_TREE_DEPTH, **kw)
    raise ValueError(leg)


def leg_mde(key, leg):
    cs = leg_case(key, leg)
    return {"mixed": cs.mixed[1], "hmc": None if cs.hmc is None else cs.hmc[1]}.get(leg, 1000.0)


# ------------------------------------------------------------------ endings of a history
KINDS = ("divergent", "turn_tree", "turn_sub", "cap")
POSITIONS = ("d0", "first", "mid", "last")


def ending(leaves):
    """(kind, position) of one NUTS transition from its leaf records: how it ended, and for a
    divergent ending where in its subtree the divergent leaf lies (d0: the transition's first
    leaf; first / mid / last: of a subtree of depth >= 1)."""
    last = leaves[-1]
    assert last["iter_done"] and not any(r["iter_done"] for r in leaves[:-1])
    if last["diverge"]:
        j = last["depth"]
        k = sum(1 for r in leaves if r["depth"] == j) - 1
        pos = "d0" if j == 0 else "first" if k == 0 else "last" if k == (1 << j) - 1 else "mid"
        return "divergent", pos
    if last["turn_sub"]:
        return "turn_sub", None
    if last["turn_tree"]:
        return "turn_tree", None
    return "cap", None


def ending_counts(hist):
    """({kind: n}, {position: n}) over every transition of a NUTS history."""
    kinds, pos = dict.fromkeys(KINDS, 0), dict.fromkeys(POSITIONS, 0)
    for h in hist:
        for _, _, leaves in h:
            k, p = ending(leaves)
            kinds[k] += 1
            if p is not None:
                pos[p] += 1
    return kinds, pos


def hmc_counts(hist):
    """(divergent, divergent and accepted) transitions of an HMC history."""
    recs = [leaves[0] for h in hist for _, _, leaves in h]
    return sum(r["diverge"] for r in recs), sum(r["diverge"] and r["take_leaf"] for r in recs)


def fmt_counts(kinds, pos):
    return (" / ".join(str(kinds[k]) for k in KINDS) + " (divergent / whole-tree U-turn / in-subtree U-turn / cap), "
            + " / ".join(str(pos[p]) for p in POSITIONS) + " (divergent at d0 / first / mid / last)")


def assert_mixed_conditions(key, side="ref"):
    """The mixed leg's input reaches what it is meant to, on the oracle alone: per case >= 10
    divergent endings and >= 10 others, a divergence at the transition's first leaf and at a later
    subtree's first leaf at least twice each."""
    kinds, pos = ending_counts(history(key, "mixed", side))
    msg = f"{key} {side}: {fmt_counts(kinds, pos)}"
    assert kinds["divergent"] >= 10 and sum(kinds.values()) - kinds["divergent"] >= 10, msg
    assert pos["d0"] >= 2 and pos["first"] >= 2, msg
    return kinds, pos


def assert_wide_conditions(side="ref"):
    """Over the wide rows' cases: a divergence at a middle and at the last leaf of a subtree at
    least five times each."""
    tot = dict.fromkeys(POSITIONS, 0)
    for key in sorted({ROWS[r][0] for r in ROWS if ROWS[r][2]}):
        _, pos = ending_counts(history(key, "mixed", side))
        for p in POSITIONS:
            tot[p] += pos[p]
    assert tot["mid"] >= 5 and tot["last"] >= 5, f"wide rows {side}: {tot}"
    return tot


# ------------------------------------------------------------------ comparisons
def calibration(key, leg, L=1024):
    """compare_traced of the leg's calibration history against its reference (through draws)."""
    cs = leg_case(key, leg)
    ctr, cns, cz = PC.as_trace(history(key, leg, "cal"), L=L)
    return PR.compare_traced(history(key, leg, "ref"), ctr, cns, cz, through_draws=True,
                             max_delta_energy=leg_mde(key, leg), **cs.tol)


def matched_through(par, C_, T_):
    """ok[c, t]: chain c reproduces the reference through transition t (compare_traced record)."""
    ok = np.ones((C_, T_), bool)
    for m in par["mismatches"]:
        ok[m["chain"], m["transition"]:] = False
    return ok


def state_fields(hist):
    """The reference's per-transition fields of a history: {name: [C, T]} (float64 / int)."""
    get = lambda f: np.array([[f(st) for st, _, _ in h] for h in hist])  # noqa: E731
    return {"num_steps": get(lambda s: int(s.num_steps)), "accept_prob": get(lambda s: float(s.accept_prob)),
            "mean_accept_prob": get(lambda s: float(s.mean_accept_prob)),
            "energy": get(lambda s: float(s.energy)), "potential_energy": get(lambda s: float(s.potential_energy)),
            "diverging": get(lambda s: bool(s.diverging)), "i": get(lambda s: int(s.i))}


def field_discrepancy(a, b, ok):
    """{energy, potential_energy: max over ok of |a - b| / max(1, |b|)} of two state_fields."""
    out = {}
    for n in ("energy", "potential_energy"):
        d = np.abs(a[n] - b[n]) / np.maximum(1.0, np.abs(b[n]))
        out[n] = float(np.max(d[ok])) if ok.any() else 0.0
    return out
