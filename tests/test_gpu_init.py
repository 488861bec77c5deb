"""Chain start-up on the device: k_nuts_reset / k_nuts_init_draw / k_nuts_init_from /
k_nuts_init_check (csrc/nuts.hip) and Engine.initialize against the Philox oracle and the float64
potentials, on both arena layouts, and the ways init_params reach them (MCMC.run, NUTS.init,
several devices, torch.distributed ranks).  Predictions and bounds come from tests/init_cases.py;
tests/test_init.py shows on the CPU that they hold for the references alone."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import init_cases as IC
from numpyro_amd import datasets, native
from numpyro_amd import potentials as P
from numpyro_amd import random as R
from numpyro_amd.engine import INIT_ATTEMPTS, Engine, SamplerOptions
from numpyro_amd.infer import MCMC, NUTS, init_to_uniform
from numpyro_amd.potentials import TorchPotential
from oracle import potentials as OP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO = ["cuda:0", "cuda:0"]
STEP = 0.37
BIG_SEED = (5 << 32) | 1234567  # both words of the Philox key in use


def _np(t):
    return t.detach().cpu().numpy()


class layout:
    """Engine.wide_persistent for engines made inside the block (decided at construction)."""

    def __init__(self, wide_persistent):
        self.value = wide_persistent

    def __enter__(self):
        self.old = Engine.wide_persistent
        Engine.wide_persistent = self.value

    def __exit__(self, *exc):
        Engine.wide_persistent = self.old


# ---------------------------------------------------------------- the arena after initialize
# (model, C, D, chain_offset, radius, wide_persistent, given inverse mass, seed): every value of
# C in {1, 63, 64, 65, 130}, D in {1, 3, 4, 5, 257, 258}, offset in {0, 37} and radius in {2, 0.3}
# occurs; D = 257 / 258 run with both settings of Engine.wide_persistent.  diag_normal has no wide
# model, so its arena is chain-minor at every D and the setting must not matter; the funnel at the
# same sizes is what runs on the chain-row layout (wide_persistent True) and on the chain-minor one.
ARENA_CASES = [
    ("diag", 1, 1, 0, 2.0, True, False, 3),
    ("diag", 63, 3, 37, 0.3, True, True, BIG_SEED),
    ("diag", 64, 4, 0, 0.3, True, False, 3),
    ("diag", 65, 5, 37, 2.0, True, True, 3),
    ("diag", 130, 4, 37, 2.0, True, False, BIG_SEED),
    ("diag", 130, 257, 0, 2.0, True, True, 3),
    ("diag", 130, 257, 0, 2.0, False, True, 3),
    ("diag", 65, 258, 37, 0.3, True, False, BIG_SEED),
    ("diag", 65, 258, 37, 0.3, False, False, BIG_SEED),
    ("funnel", 130, 257, 37, 2.0, True, True, BIG_SEED),
    ("funnel", 130, 257, 37, 2.0, False, True, BIG_SEED),
    ("funnel", 65, 258, 0, 0.3, True, False, 3),
    ("funnel", 65, 258, 0, 0.3, False, False, 3),
    ("funnel", 1, 257, 37, 0.3, True, True, 3),
    ("funnel", 1, 257, 37, 0.3, False, True, 3),
]
_arena_cache = {}


def _arena(case):
    """Engine.initialize for the case; every arena field the tests read, as NumPy arrays (read-only)."""
    if case in _arena_cache:
        return _arena_cache[case]
    model, C, D, off, radius, wp, with_imm, seed = case
    imm = IC.imm_diag(D) if with_imm else None
    kw = dict(step_size=STEP, inverse_mass_matrix=imm, adapt_mass_matrix=not with_imm)
    if model == "diag":
        kernel, args = NUTS(P.diag_normal, **kw), IC.diag_params(D)
    else:
        kernel, args = NUTS(P.funnel, **kw), (D,)
    with layout(wp):
        eng = kernel.make_engine(C, args, chain_offset=off)
    eng.initialize(seed, 30, radius=radius)
    torch.cuda.synchronize()
    out = {"crow": eng.crow, "ldc": eng.ldc, "imm": imm}
    for name in ("z", "zgrad", "inv_mass", "mass_sqrt", "wf_mean", "wf_m2"):
        out[name] = _np(eng.chain_state(name)).copy()
    for name in ("pe", "energy", "step_size", "step_eff", "da_prox", "da_xt", "da_xavg", "da_gavg", "da_t", "wf_n",
                 "phase", "iter", "window_idx", "counters", "finished"):
        out[name] = _np(eng.view(name)).copy()
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _arena_cache[case] = out
    return out


def _oracle_at(model, D, z):
    ref = OP.IsoNormal(*IC.diag_params(D)) if model == "diag" else OP.Funnel(D)
    return [ref.pe_grad(zc.astype(np.float64)) for zc in z]


@pytest.mark.parametrize("case", ARENA_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_arena_after_initialize(device, case):
    """Every field Engine.initialize leaves behind, against the oracle: the start is BITWISE
    attempt 0 of chain chain_offset + c at the case's radius; U and grad U there meet the standing
    tolerances; energy == U; phases; step sizes; da_prox, inverse mass and its root against float64
    at rtol 1e-6 (one or two float32 operations of <= 2 ulp each); adaptation state zero."""
    model, C, D, off, radius, wp, with_imm, seed = case
    a = _arena(case)
    ldc = (C + 63) // 64 * 64
    assert a["ldc"] == ldc
    assert a["crow"] == (model == "funnel" and wp)
    want = IC.draws(seed, off, C, 0, D, radius)
    assert a["z"].shape == (C, D)
    assert np.array_equal(IC.bits(a["z"]), IC.bits(want))
    for c in (0, C - 1):
        assert IC.attempt_of(a["z"][c], seed, off + c, D, radius, 2) == 0
    chk = IC.check_diag if model == "diag" else IC.check_funnel
    for c, ref in enumerate(_oracle_at(model, D, a["z"])):
        chk(np.float64(a["pe"][c]), a["zgrad"][c].astype(np.float64), ref)
    assert np.array_equal(IC.bits(a["energy"][:C]), IC.bits(a["pe"][:C]))
    assert np.all(a["phase"][:C] == native.PH_START) and np.all(a["phase"][C:] == native.PH_DONE)
    assert a["phase"].shape == (ldc,)
    step = np.float32(STEP)
    assert np.all(a["step_size"] == step) and np.all(a["step_eff"] == step)
    np.testing.assert_allclose(a["da_prox"], np.log(10.0 * float(step)), rtol=1e-6)
    imm = np.ones(D) if a["imm"] is None else a["imm"].astype(np.float64)
    np.testing.assert_allclose(a["inv_mass"], np.broadcast_to(imm, (C, D)), rtol=1e-6)
    np.testing.assert_allclose(a["mass_sqrt"], np.broadcast_to(1.0 / np.sqrt(imm), (C, D)), rtol=1e-6)
    for name in ("wf_mean", "wf_m2", "wf_n", "da_xt", "da_xavg", "da_gavg", "da_t", "counters", "finished", "iter",
                 "window_idx"):
        assert not a[name].any(), name


@pytest.mark.parametrize("pair", [(i, i + 1) for i in (5, 7, 9, 11, 13)], ids=lambda p: str(p[0]))
def test_both_layouts_start_bitwise_equal(device, pair):
    """D = 257 / 258: the chain-row arena (vidx's other branch, _evaluate_all through transposed
    copies) and the chain-minor one hold bitwise the same z, U and grad U per chain."""
    rows, minor = _arena(ARENA_CASES[pair[0]]), _arena(ARENA_CASES[pair[1]])
    assert ARENA_CASES[pair[0]][:5] == ARENA_CASES[pair[1]][:5]
    if ARENA_CASES[pair[0]][0] == "funnel":
        assert rows["crow"] and not minor["crow"]
    C = ARENA_CASES[pair[0]][1]
    for name in ("z", "zgrad", "pe", "energy", "inv_mass", "mass_sqrt"):
        assert np.array_equal(IC.bits(rows[name][:C]), IC.bits(minor[name][:C])), name


def test_wrong_oracles_fail_the_bitwise_start_check(device):
    """The check has teeth: attempt a + 1 in place of a, the other chain_offset, the other radius
    and a neighbouring chain are all different bits."""
    case = ARENA_CASES[3]
    _, C, D, off, radius, _, _, seed = case
    z = _arena(case)["z"]
    right = IC.bits(IC.draws(seed, off, C, 0, D, radius))
    assert np.array_equal(IC.bits(z), right)
    for wrong in (IC.draws(seed, off, C, 1, D, radius), IC.draws(seed, 0, C, 0, D, radius),
                  IC.draws(seed, off, C, 0, D, 0.3), IC.draws(seed, off + 1, C, 0, D, radius),
                  IC.draws(seed + 1, off, C, 0, D, radius)):
        assert not (IC.bits(wrong) == IC.bits(z)).all(axis=1).any()
    assert IC.attempt_of(z[2], seed, off + 2, D, radius, 4) == 0
    assert IC.attempt_of(z[2], seed, 0 + 2, D, radius, 4) is None
    assert IC.attempt_of(IC.draws(seed, off, C, 1, D, radius)[2], seed, off + 2, D, radius, 4) == 1


# ---------------------------------------------------------------- retries, exactly predicted
def gated(kind, t):
    """0.5 |z|^2 where z[0] <= t; elsewhere +inf, NaN, or a finite value with a NaN gradient."""
    def fn(z):
        base = 0.5 * (z * z).sum()
        bad = z[0] > t
        if kind == "inf":
            return torch.where(bad, torch.full_like(base, float("inf")), base)
        if kind == "nan":
            return torch.where(bad, torch.full_like(base, float("nan")), base)
        # sqrt at 0 has an infinite slope and d(z0 - z0) = 1 - 1: the product is NaN, the value 0;
        # valid chains take the constant branch, whose gradient is 0
        arg = torch.where(bad, z[0] - z[0], torch.ones_like(z[0]))
        return base + (torch.sqrt(arg) - torch.where(bad, torch.zeros_like(z[0]), torch.ones_like(z[0])))
    return fn


@pytest.mark.parametrize("kind", ["inf", "nan", "nangrad"])
def test_retries_are_exactly_predicted(device, kind):
    """A torch potential_fn valid exactly where z[0] <= radius / 2: each chain's first valid attempt
    is an exact function of the known draws (tests/test_init.py: at this seed 38 of 130 chains
    retry, up to 4 redraws, chains 0 / 63 / 64 / 129 accept at attempts 1, 1, 0, 0).  Every chain
    must hold BITWISE the draw of that attempt -- so a chain accepted early is neither redrawn nor
    overwritten while its neighbours retry -- with U and grad U of that point, and the tally of
    chains still searching (counters[1]) must have reached zero."""
    k = IC.GATE_CASE
    C, D, radius, seed = k["C"], k["D"], k["radius"], k["seed"]
    first = IC.gate_first_valid(seed, C, D, radius)
    assert first.max() >= 3 and len(set(first[list(IC.GATE_EDGE_CHAINS)].tolist())) > 1
    eng = Engine(TorchPotential(gated(kind, float(IC.gate_threshold(radius))), torch.zeros(D)), C,
                 SamplerOptions(step_size=STEP))
    eng.initialize(seed, 0, radius=radius)
    z, pe, g = _np(eng.chain_state("z")), _np(eng.chain_state("pe")), _np(eng.chain_state("zgrad"))
    got = np.array([-1 if (a := IC.attempt_of(z[c], seed, c, D, radius, INIT_ATTEMPTS)) is None else a
                    for c in range(C)])
    assert np.array_equal(got, first), np.nonzero(got != first)
    z64 = z.astype(np.float64)
    np.testing.assert_allclose(pe, 0.5 * (z64 * z64).sum(1), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(g, z64, rtol=1e-5, atol=1e-6)
    assert np.array_equal(IC.bits(_np(eng.chain_state("energy"))), IC.bits(pe))
    ph = _np(eng.view("phase"))
    assert np.all(ph[:C] == native.PH_START) and np.all(ph[C:] == native.PH_DONE)
    assert not _np(eng.view("counters")).any()


# ---------------------------------------------------------------- retries on the fused paths
def _check_fused_retries(model, z, pe, g, case, D, oracle64, chk, predicted):
    acc, evaluated, ambiguous, refs = IC.check_accepted(z, case["seed"], case["chain_offset"], D, case["radius"],
                                                        oracle64, INIT_ATTEMPTS)
    print(f"[init {model}] device: {int((acc > 0).sum())} of {len(acc)} chains retried, most redraws {int(acc.max())}, "
          f"{evaluated} draws evaluated, {ambiguous} ambiguous (band {IC.BAND}); differs from the float32 oracle's "
          f"attempt at chains {np.nonzero(acc != predicted.accepted)[0].tolist()}")
    assert ambiguous <= IC.AMBIGUOUS_CAP * evaluated
    for c, (pe_r, g_r, v) in enumerate(refs):
        if v == IC.VALID:  # ambiguous evaluations are left out
            chk(np.float64(pe[c]), g[c].astype(np.float64), (pe_r, g_r))
    # where no draw up to the predicted attempt is ambiguous, the two properties above pin the attempt
    clear = np.array([IC.AMBIGUOUS not in predicted.verdicts[c] for c in range(len(acc))])
    assert np.array_equal(acc[clear], predicted.accepted[clear])
    return acc


def test_retries_eight_schools_one_wave(device):
    """Eight schools at init_to_uniform(radius=100), 130 chains, seed 1 (the one-wave persistent
    schedule's model, chain-minor arena; the launched potential evaluates the starts).  Final z is
    bitwise one attempt's draw; that draw is not invalid and every rejected earlier draw is not
    valid by the float64 oracle; U and grad U meet test_eight_schools_matches_oracle's tolerance.

    Band: valid below FLT_MAX / 4, invalid above 4 FLT_MAX (tests/init_cases.py BAND).  CPU, float32
    oracle and plain float32 restatement alike: 31 chains retry, at most 3 redraws, 169 draws
    evaluated, 1 ambiguous.  Device: the same 31 / 3 / 169 / 1, every chain at the predicted attempt.

    This test found NmxEightSchools rejecting valid draws: tau = e^u went through
    log1p((tau / 5)^2) and 2 q / (1 + q), not finite in float32 at u > 44.4 (28% of U(-100, 100)
    draws) where U ~ 9 u; the kernel now takes those terms from u past u = 40."""
    k = IC.SCHOOLS_CASE
    kernel = NUTS(P.eight_schools, init_strategy=init_to_uniform(radius=k["radius"]))
    eng = kernel.make_engine(k["C"], (8, datasets.EIGHT_SCHOOLS_SIGMA, datasets.EIGHT_SCHOOLS_Y),
                             chain_offset=k["chain_offset"])
    assert eng._persistent_model() is not None and not eng.crow
    eng.initialize(k["seed"], 10, radius=kernel.init_radius())
    z, pe, g = _np(eng.chain_state("z")), _np(eng.chain_state("pe")), _np(eng.chain_state("zgrad"))
    _check_fused_retries("eight schools", z, pe, g, k, 10, IC.schools_oracle(), IC.check_schools, IC.schools_retry())
    assert not _np(eng.view("counters")).any()
    assert np.all(_np(eng.view("phase"))[:k["C"]] == native.PH_START)


def test_retries_funnel_both_layouts(device):
    """Funnel D = 300 at init_to_uniform(radius=100), 130 chains from chain_offset 7, seed 1, on the
    chain-row arena of the persistent wide schedule and on the chain-minor one: the same properties
    as for eight schools (check_funnel_outer's tolerance), and both layouts accept the same attempt
    per chain with bitwise equal z.

    Band: FLT_MAX / 4 .. 4 FLT_MAX.  CPU (float32 oracle and plain float32 restatement): 14 chains
    retry, at most 2 redraws, 147 draws evaluated, 2 ambiguous.  Device, both layouts: the same
    14 / 2 / 147 / 2, every chain at the predicted attempt."""
    k = IC.FUNNEL_CASE
    out = {}
    for wp in (True, False):
        kernel = NUTS(P.funnel, init_strategy=init_to_uniform(radius=k["radius"]))
        with layout(wp):
            eng = kernel.make_engine(k["C"], (k["dim"],), chain_offset=k["chain_offset"])
        assert eng.crow == wp and eng.persist_wide == wp
        eng.initialize(k["seed"], 10, radius=kernel.init_radius())
        z, pe, g = _np(eng.chain_state("z")), _np(eng.chain_state("pe")), _np(eng.chain_state("zgrad"))
        acc = _check_fused_retries(f"funnel 300 {'rows' if wp else 'minor'}", z, pe, g, k, k["dim"],
                                   IC.funnel_oracle(k["dim"]), IC.check_funnel, IC.funnel_retry())
        assert not _np(eng.view("counters")).any()
        out[wp] = (acc, z, pe, g)
    assert np.array_equal(out[True][0], out[False][0])
    assert np.array_equal(IC.bits(out[True][1]), IC.bits(out[False][1]))
    print(f"[init funnel 300] layouts: U bitwise equal {np.array_equal(IC.bits(out[True][2]), IC.bits(out[False][2]))}, "
          f"grad bitwise equal {np.array_equal(IC.bits(out[True][3]), IC.bits(out[False][3]))}")


# ---------------------------------------------------------------- failures
def _logreg(C=130, N=200, D=8):
    rs = np.random.RandomState(4)
    X = rs.randn(N, D).astype(np.float32)
    y = (rs.rand(N) < 0.4).astype(np.float32)
    ip = torch.from_numpy((0.3 * rs.randn(C, D)).astype(np.float32))
    return X, y, ip


def test_no_valid_start_raises_and_the_object_recovers(device):
    """A potential invalid everywhere init_to_uniform can reach (finite only at z[0] > 5, radius 2)
    raises after exactly INIT_ATTEMPTS draws; the same MCMC object then runs from valid init_params."""
    calls = []

    def far(z):
        calls.append(1)  # vmap runs the Python function once per evaluation of the batch
        base = 0.5 * ((z - 7.0) ** 2).sum()
        return torch.where(z[0] > 5.0, base, torch.full_like(base, float("inf")))

    C = 70
    mcmc = MCMC(NUTS(potential_fn=far, step_size=0.1, adapt_step_size=False, adapt_mass_matrix=False),
                num_warmup=0, num_samples=3, num_chains=C, progress_bar=False)
    mcmc.sampler.bind_potential_fn(torch.zeros(C, 3), C)
    with pytest.raises(RuntimeError, match="Cannot find valid initial parameters"):
        mcmc.run(2)
    assert len(calls) == INIT_ATTEMPTS
    mcmc.run(2, init_params=torch.full((C, 3), 7.0))
    x = mcmc.get_samples(group_by_chain=True)
    assert x.shape == (C, 3, 3) and bool(torch.isfinite(x).all()) and bool((x[:, :, 0] > 5.0).all())


def test_nonfinite_init_params_name_the_chains(device):
    """NaN in chains 0, 63, 64 and 129 of 130 (fused logreg): the error counts 4 -- not the padded
    lanes 130 .. 191, and across both waves' atomics."""
    X, y, ip = _logreg()
    ip = ip.clone()
    ip[[0, 63, 64, 129], 3] = float("nan")
    mcmc = MCMC(NUTS(P.logistic_regression), num_warmup=0, num_samples=1, num_chains=130, progress_bar=False)
    with pytest.raises(RuntimeError, match=r"Cannot find valid initial parameters: 4 chains"):
        mcmc.run(0, X, y, init_params=ip)
    ip[64, 3] = float("inf")
    ip[[0, 63], 3] = 0.0
    with pytest.raises(RuntimeError, match=r": 2 chains"):
        mcmc.run(0, X, y, init_params={"coefs": ip})


def test_bad_leading_dimension_and_strategy(device):
    X, y, ip = _logreg()
    mcmc = MCMC(NUTS(P.logistic_regression), num_warmup=0, num_samples=1, num_chains=130, progress_bar=False)
    for bad in (ip[:7], {"coefs": ip[:129]}, torch.zeros(2, 130, 8)):
        with pytest.raises(ValueError, match="same leading dimension"):
            mcmc.run(0, X, y, init_params=bad)
    for strategy in (lambda site=None: None, ("median", 15)):
        mcmc = MCMC(NUTS(P.logistic_regression, init_strategy=strategy), num_warmup=0, num_samples=1, num_chains=4,
                    progress_bar=False)
        with pytest.raises(NotImplementedError, match="init_to_uniform"):
            mcmc.run(0, X, y)


# ---------------------------------------------------------------- nothing left behind
@pytest.mark.parametrize("model", ["logreg", "eight_schools", "funnel"])
def test_rerun_from_the_same_seed_is_bitwise_equal(device, model):
    """Fused step, one-wave persistent and chain-row schedules: an MCMC object that has already
    run -- with warmup, from another seed, and for more iterations than the next run allocates --
    draws from a seed bitwise what a fresh object draws from it, and again on a third run."""
    if model == "logreg":
        X, y, _ = _logreg()
        fm, args, C = P.logistic_regression, (X, y), 130
    elif model == "eight_schools":
        fm, args, C = P.eight_schools, (8, datasets.EIGHT_SCHOOLS_SIGMA, datasets.EIGHT_SCHOOLS_Y), 70
    else:
        fm, args, C = P.funnel, (300,), 70
    fields = ("num_steps", "accept_prob", "potential_energy", "energy", "adapt_state.step_size", "mean_accept_prob")

    def result(m):
        return {**m.get_samples(True), **m.get_extra_fields(True)}

    def new(S):
        return MCMC(NUTS(fm, max_tree_depth=5), num_warmup=12, num_samples=S, num_chains=C, progress_bar=False)

    fresh = new(4)
    fresh.run(9, *args, extra_fields=fields)
    want = result(fresh)
    used = new(9)
    used.run(8, *args, extra_fields=fields)
    eng = used._engine
    assert eng.crow == (model == "funnel") and (eng._persistent_model() is not None) == (model == "eight_schools")
    used.num_samples = 4
    for _ in range(2):
        used.run(9, *args, extra_fields=fields)
        assert used._engine is eng and used.post_warmup_state is None
        got = result(used)
        assert set(got) == set(want)
        for name in want:
            assert want[name].shape == got[name].shape and torch.equal(want[name].cpu(), got[name].cpu()), name


# ---------------------------------------------------------------- init_params through every entry
@pytest.fixture
def starts(monkeypatch):
    """(chain_offset, z [C, D]) of every Engine.initialize, read right after it."""
    log, orig = [], Engine.initialize

    def initialize(self, *a, **kw):
        orig(self, *a, **kw)
        log.append((self.chain_offset, self.chain_state("z").clone().cpu()))

    monkeypatch.setattr(Engine, "initialize", initialize)
    return log


def _all_starts(log):
    z = torch.cat([z for _, z in sorted(log, key=lambda e: e[0])])
    log.clear()
    return z


def test_init_params_reach_the_arena_through_every_entry(device, starts):
    """One [C, D] start, as an array and as a site dict, through MCMC.run, NUTS.init (chain count
    given, inferred from a batch of keys, from the dict's values, from the array) and two engines on
    one device (the ip_all[lo:hi] sharding): z is bitwise the given float32 values; a [D] value is
    every chain's start; the two-engine draws equal the one-engine draws bitwise."""
    C, D = 130, 8
    X, y, ip = _logreg(C)
    forms = {"array": ip, "dict": {"coefs": ip}, "numpy": ip.numpy(), "float64": ip.double()}

    def mcmc_of(devices=None):
        return MCMC(NUTS(P.logistic_regression, max_tree_depth=4), num_warmup=3, num_samples=2, num_chains=C,
                    devices=devices, progress_bar=False)

    draws = {}
    for devices in (None, TWO):
        for name, form in forms.items():
            m = mcmc_of(devices)
            m.run(6, X, y, init_params=form, extra_fields=("num_steps",))
            assert (m._engines is not None) == (devices is not None)
            assert len(starts) == (2 if devices else 1)
            assert torch.equal(_all_starts(starts), ip), (devices, name)
            draws[(devices is None, name)] = (m.get_samples(True)["coefs"].cpu(), m.get_extra_fields(True)["num_steps"].cpu())
        m = mcmc_of(devices)
        m.run(6, X, y, init_params=ip[5])
        assert torch.equal(_all_starts(starts), ip[5][None].expand(C, D))
    ref = draws[(True, "array")]
    for key, (x, ns) in draws.items():
        assert torch.equal(x, ref[0]) and torch.equal(ns, ref[1]), key
    # the kernel API
    row = ip[5][None].expand(C, D)
    keys = R.split(R.PRNGKey(6), C)
    for key, kw, want in ((6, dict(init_params=ip, num_chains=C), ip), (6, dict(init_params={"coefs": ip}, num_chains=C), ip),
                          (6, dict(init_params=ip), ip),               # C from the array
                          (6, dict(init_params={"coefs": ip}), ip),    # C from the dict's values
                          (6, dict(init_params=ip[5], num_chains=C), row),
                          (keys, dict(init_params=ip[5]), row),        # C from the batch of keys
                          (keys, dict(init_params={"coefs": ip}), ip)):
        st = NUTS(P.logistic_regression).init(key, 3, model_args=(X, y), **kw)
        assert torch.equal(_all_starts(starts), want)
        assert st.z["coefs"].shape == (C, D) and torch.equal(st.z["coefs"].cpu(), want)


# ---------------------------------------------------------------- the chain axis of init_params
def banana(z):
    """x1 ~ N(0, 1), x2 | x1 ~ N(x1^2 / 2, 1), written without reductions: a chain's value does not
    depend on how many chains are evaluated with it."""
    x1, x2 = z["x"][0], z["x"][1]
    return 0.5 * x1 * x1 + 0.5 * (x2 - 0.5 * x1 * x1) * (x2 - 0.5 * x1 * x1)


BANANA_START = torch.tensor([[0.3, -0.2], [-1.1, 0.7]])


def banana_run(shard=None):
    """num_chains = 2, fixed step, no warmup, 3 draws from BANANA_START; shard = (lo, hi, local)
    makes the MCMC one rank's (torch.distributed sets the same three fields).  Returns the potential's
    dimension, the draws [local, 3, 2] and the start."""
    mcmc = MCMC(NUTS(potential_fn=banana, step_size=0.25, adapt_step_size=False, adapt_mass_matrix=False),
                num_warmup=0, num_samples=3, num_chains=2, progress_bar=False)
    if shard is not None:
        mcmc.chain_lo, mcmc.chain_hi, mcmc.local_chains = shard
    mcmc.run(4, init_params={"x": BANANA_START})
    return mcmc._engine.D, mcmc.get_samples(group_by_chain=True)["x"].cpu(), mcmc


def test_rank_of_one_chain_builds_the_model_dimension(device, starts):
    """num_chains = 2 with this process holding chain 1 alone: batched init_params still carry a
    chain axis, so D = 2 (not 4), the start is chain 1's values and the draws are chain 1's of the
    one-process run, bitwise."""
    D, full, _ = banana_run()
    assert D == 2 and torch.equal(_all_starts(starts), BANANA_START)
    for r in (0, 1):
        D, x, m = banana_run((r, r + 1, 1))
        assert D == 2 and m._engine.C == 1 and m._engine.chain_offset == r
        assert torch.equal(_all_starts(starts), BANANA_START[r:r + 1])
        assert x.shape == (1, 3, 2) and torch.equal(x[0], full[r])


def test_two_ranks_of_one_chain_equal_one_process(device, tmp_path):
    """The same under torch.distributed: 2 ranks (gloo, both on cuda:0) of num_chains = 2
    (tests/dist_init_worker.py).  Both report dimension 2 and their draws are chains 0 and 1 of the
    one-process run, bitwise."""
    _, full, _ = banana_run()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    out = tmp_path / "dist_init.pt"
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                    "--master-addr", "127.0.0.1", "--master-port", str(port),
                    os.path.join(ROOT, "tests", "dist_init_worker.py"), str(out)], check=True, timeout=300, env=env)
    got = torch.load(out, weights_only=True)
    assert got["dims"] == [2, 2] and got["chains"] == [[0, 1, 1], [1, 2, 1]]
    assert got["x"].shape == (2, 3, 2) and torch.equal(got["x"], full)


def test_device_engines_are_rebuilt_for_another_structure(device):
    """Two runs on two engines with init_params of dimension 2 and then 3: the second re-binds the
    potential_fn and must sample at dimension 3, not keep the engines built for 2."""
    def quad(z):
        return 0.5 * (z * z).sum()

    mcmc = MCMC(NUTS(potential_fn=quad), num_warmup=5, num_samples=4, num_chains=6, devices=TWO, progress_bar=False)
    for D in (2, 3, 2):
        mcmc.run(1, init_params=torch.zeros(6, D))
        assert [e.D for e in mcmc._engines] == [D, D]
        x = mcmc.get_samples(group_by_chain=True)
        assert x.shape == (6, 4, D) and bool(torch.isfinite(x).all())
