"""Chain start-up on the host (no GPU): how init_params become [C, D] rows under the global
chain-count rule, init_radius(), and the predictions tests/test_gpu_init.py holds the device to
(tests/init_cases.py) -- shown here for the references alone, at the seeds the GPU tests use."""
import contextlib

import numpy as np
import pytest
import torch

import init_cases as IC
from numpyro_amd import potentials as P
from numpyro_amd.infer import MCMC, NUTS, init_to_uniform
from numpyro_amd.infer.hmc import _flatten_init
from numpyro_amd.potentials import Potential, TorchPotential


def quad(z):
    x = z["x"] if isinstance(z, dict) else z
    return 0.5 * (x ** 2).sum()


# ---------------------------------------------------------------- _flatten_init / bind_potential_fn
def test_flatten_init_global_count_rule():
    """One chain: the reference's unbatched values gain the chain axis.  More chains: the leading
    axis is the chain axis, and an array-valued z of any shape is reshaped to [C, D]."""
    pd = TorchPotential(quad, {"x": torch.zeros(5)})
    out = _flatten_init(pd, {"x": torch.arange(5.0)}, 1)
    assert out.shape == (1, 5) and torch.equal(out[0], torch.arange(5.0))
    out = _flatten_init(pd, {"x": torch.arange(10.0).reshape(2, 5)}, 2)
    assert out.shape == (2, 5) and torch.equal(out[1], torch.arange(5.0, 10.0))
    pa = TorchPotential(quad, torch.zeros(2, 3))
    assert pa.dim == 6 and pa.array_site
    v = torch.arange(6.0).reshape(2, 3)
    assert torch.equal(torch.as_tensor(_flatten_init(pa, v, 1)), torch.arange(6.0)[None])
    out = torch.as_tensor(_flatten_init(pa, torch.stack([v, v + 10]), 2))
    assert out.shape == (2, 6) and torch.equal(out[1], torch.arange(6.0) + 10)

    class Fixed(Potential):  # a model's potential: dicts are flattened in site order, arrays pass
        sites = [("b", (2,), 0), ("a", (), 0)]
        dim = 3

    out = _flatten_init(Fixed(), {"a": torch.tensor([7.0, 8.0]), "b": torch.arange(4.0).reshape(2, 2)}, 2)
    assert torch.equal(out, torch.tensor([[0.0, 1.0, 7.0], [2.0, 3.0, 8.0]]))
    arr = torch.arange(6.0).reshape(2, 3)
    assert _flatten_init(Fixed(), arr, 2) is arr


def test_bind_potential_fn_reads_the_chain_axis_from_the_given_count():
    k = NUTS(potential_fn=quad)
    with pytest.raises(ValueError, match="init_params"):
        k.bind_potential_fn(None, 2)
    k.bind_potential_fn({"x": torch.zeros(2, 5)}, 2)
    first = k._potential
    assert first.dim == 5 and first.sites == [("x", (5,), 0)]
    k.bind_potential_fn({"x": torch.ones(2, 5)}, 2)  # the same structure keeps the potential
    assert k._potential is first
    k.bind_potential_fn(None, 2)                      # and later runs may omit init_params
    assert k._potential is first
    k.bind_potential_fn({"x": torch.zeros(2, 5)}, 1)  # one chain: the same value is unbatched
    assert k._potential is not first and k._potential.dim == 10
    k.bind_potential_fn(torch.zeros(4, 2, 3), 4)
    assert k._potential.array_site and k._potential.sites == [("z", (2, 3), 0)]


# ---------------------------------------------------------------- MCMC with a recording engine
class Started(Exception):
    pass


class Wrapper:
    """Stands for the whitening wrappers of a dense mass matrix: not a TorchPotential, no flatten."""

    def __init__(self, base):
        self.base, self.dim, self.sites = base, base.dim, base.sites


class RecordingEngine:
    """What MCMC needs of an engine up to initialize(), which records its arguments and stops the run."""

    log = []

    def __init__(self, potential, num_chains, opts=None, device=None, chain_offset=0, sync_chains=False):
        self.model_potential, self.potential = potential, Wrapper(potential)
        self.C, self.D, self.chain_offset = int(num_chains), int(potential.dim), int(chain_offset)
        self.device, self.device_group = torch.device("cpu"), None

    def initialize(self, seed, num_warmup, init_params=None, radius=2.0):
        self.start = None if init_params is None else torch.as_tensor(init_params).clone()
        RecordingEngine.log.append(self)
        raise Started


@pytest.fixture
def recording(monkeypatch):
    import numpyro_amd.engine as E

    RecordingEngine.log = []
    monkeypatch.setattr(E, "Engine", RecordingEngine)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())

    def make_engine(self, num_chains, model_args=(), model_kwargs=None, device=None, chain_offset=0, sync_chains=False):
        return RecordingEngine(self.potential(model_args, model_kwargs), num_chains, None, device, chain_offset)

    monkeypatch.setattr(NUTS, "make_engine", make_engine)
    return RecordingEngine


def _start(mcmc, init_params):
    with pytest.raises(Started):
        mcmc.run(0, init_params=init_params)
    return mcmc._engine


def test_rank_shard_of_one_chain_reads_batched_init_params(recording):
    """num_chains = 2 over two ranks: rank 1 holds one chain.  The batched [2, ...] values still
    carry a chain axis, so the potential has dimension D (not 2 D) and the rank starts from chain
    1's values, whether they come as a dict, an array or an array-valued z."""
    for ip, D in (({"x": torch.arange(10.0).reshape(2, 5)}, 5), (torch.arange(10.0).reshape(2, 5), 5),
                  (torch.arange(12.0).reshape(2, 2, 3), 6)):
        mcmc = MCMC(NUTS(potential_fn=quad), num_warmup=0, num_samples=1, num_chains=2, progress_bar=False)
        mcmc.chain_lo, mcmc.chain_hi, mcmc.local_chains = 1, 2, 1
        eng = _start(mcmc, ip)
        assert eng.D == D and eng.C == 1 and eng.chain_offset == 1
        assert eng.start.shape == (1, D) and torch.equal(eng.start[0], torch.arange(float(D), 2.0 * D))
    # a [D] value is every chain's start
    mcmc = MCMC(NUTS(P.diag_normal), num_warmup=0, num_samples=1, num_chains=4, progress_bar=False)
    mcmc.chain_lo, mcmc.chain_hi, mcmc.local_chains = 2, 4, 2
    with pytest.raises(Started):
        mcmc.run(0, np.zeros(3, np.float32), np.ones(3, np.float32), init_params=torch.tensor([1.0, 2.0, 3.0]))
    assert torch.equal(mcmc._engine.start, torch.tensor([[1.0, 2.0, 3.0]] * 2))


def test_init_params_pass_a_whitening_wrapper(recording):
    """The engine's `potential` is a wrapper under dense_mass; init_params are flattened by the
    model's potential behind it: one chain takes the reference's unbatched values, and an
    array-valued z of shape (2, 3) becomes [C, 6]."""
    mcmc = MCMC(NUTS(potential_fn=quad, dense_mass=True), num_warmup=0, num_samples=1, progress_bar=False)
    eng = _start(mcmc, {"x": torch.arange(5.0)})
    assert eng.start.shape == (1, 5) and torch.equal(eng.start[0], torch.arange(5.0))
    mcmc = MCMC(NUTS(potential_fn=quad, dense_mass=True), num_warmup=0, num_samples=1, progress_bar=False)
    eng = _start(mcmc, torch.arange(6.0).reshape(2, 3))
    assert eng.D == 6 and eng.start.shape == (1, 6) and torch.equal(eng.start[0], torch.arange(6.0))
    mcmc = MCMC(NUTS(potential_fn=quad, dense_mass=True), num_warmup=0, num_samples=1, num_chains=3, progress_bar=False)
    eng = _start(mcmc, torch.arange(18.0).reshape(3, 2, 3))
    assert eng.start.shape == (3, 6) and torch.equal(eng.start[2], torch.arange(12.0, 18.0))


def test_leading_dimension_must_be_the_chain_count(recording):
    mcmc = MCMC(NUTS(potential_fn=quad), num_warmup=0, num_samples=1, num_chains=4, progress_bar=False)
    with pytest.raises(ValueError, match="same leading dimension"):
        mcmc.run(0, init_params={"x": torch.zeros(3, 5)})


def test_device_engines_follow_a_rebound_potential_fn(recording):
    """A second multi-device run whose init_params have another structure re-binds the
    potential_fn; the engines of every device are rebuilt at the new dimension."""
    mcmc = MCMC(NUTS(potential_fn=quad), num_warmup=0, num_samples=1, num_chains=4, progress_bar=False,
                devices=["cuda:0", "cuda:0"])
    devs = mcmc.devices
    mcmc.sampler.bind_potential_fn(torch.zeros(4, 2), 4)
    first = mcmc._get_engines((), {}, devs)
    assert [e.D for e in first] == [2, 2] and [e.C for e in first] == [2, 2]
    assert [e.chain_offset for e in first] == [0, 2]
    assert mcmc._get_engines((), {}, devs) is first  # unchanged binding: the same engines
    mcmc.sampler.bind_potential_fn(torch.zeros(4, 3), 4)
    second = mcmc._get_engines((), {}, devs)
    assert [e.D for e in second] == [3, 3]
    with pytest.raises(Started):  # the whole path: sharded rows of the new dimension
        mcmc.run(0, init_params=torch.arange(8.0).reshape(4, 2))
    assert sorted((e.chain_offset, e.D, e.start.tolist()) for e in recording.log) == \
        [(0, 2, [[0.0, 1.0], [2.0, 3.0]]), (2, 2, [[4.0, 5.0], [6.0, 7.0]])]
    # one run path: the device engines start from the [lo:hi] slices of the rows that a single
    # engine is handed for the same init_params, and HMC.init hands its engine those rows too
    for ip in (torch.arange(8.0).reshape(4, 2), {"x": torch.arange(8.0).reshape(4, 2)}):
        single = MCMC(NUTS(potential_fn=quad), num_warmup=0, num_samples=1, num_chains=4, progress_bar=False)
        one = _start(single, ip).start
        assert one.shape == (4, 2) and one.dtype == torch.float32
        recording.log.clear()
        with pytest.raises(Started):
            mcmc.run(0, init_params=ip)
        shards = {e.chain_offset: e.start for e in recording.log}
        assert sorted(shards) == [0, 2] and all(torch.equal(shards[lo], one[lo:lo + 2]) for lo in shards)
        kernel = NUTS(potential_fn=quad)
        with pytest.raises(Started):
            kernel.init(0, 0, init_params=ip, num_chains=4)
        assert torch.equal(recording.log[-1].start, one)


def test_parallel_chains_without_devices_advise_once(recording, monkeypatch):
    """The default chain_method="parallel" with several local chains, several visible GPUs and no
    devices=: one engine, and the advice to pass devices='all', once per process."""
    import warnings

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 2)
    monkeypatch.setattr(MCMC, "_warned_devices", False, raising=False)
    mcmc = MCMC(NUTS(potential_fn=quad), num_warmup=0, num_samples=1, num_chains=2, progress_bar=False)
    assert mcmc.chain_method == "parallel" and mcmc.devices is None
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        assert mcmc._run_devices() is None
    assert [w.category for w in caught] == [UserWarning] and "devices='all'" in str(caught[0].message)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        assert mcmc._run_devices() is None
    assert caught == []


def test_init_radius():
    assert NUTS(potential_fn=quad).init_radius() == 2.0
    assert NUTS(potential_fn=quad, init_strategy=init_to_uniform(radius=0.3)).init_radius() == pytest.approx(0.3)
    assert NUTS(potential_fn=quad, init_strategy=init_to_uniform(radius=100)).init_radius() == 100.0
    for other in (lambda site=None: None, ("median", 15), "init_to_median"):
        with pytest.raises(NotImplementedError, match="init_to_uniform"):
            NUTS(potential_fn=quad, init_strategy=other).init_radius()


# ---------------------------------------------------------------- attempt_of
@pytest.mark.parametrize("D", [1, 3, 4, 5, 257])
@pytest.mark.parametrize("radius", [2.0, 0.3, 100.0])
def test_attempt_of_identifies_the_draw_bitwise(D, radius):
    seed, chain = 5, 37 + D
    for a in (0, 1, 4):
        z = IC.draw(seed, chain, a, D, radius)
        assert z.dtype == np.float32 and z.shape == (D,) and np.all(np.abs(z) <= np.float32(radius))
        assert IC.attempt_of(z, seed, chain, D, radius, 6) == a
        assert IC.attempt_of(z, seed, chain, D, radius, a) is None          # not within the attempts allowed
        assert IC.attempt_of(z, seed, chain + 1, D, radius, 6) is None      # another chain's stream
        assert IC.attempt_of(z, seed + 1, chain, D, radius, 6) is None
        assert IC.attempt_of(z, seed, chain, D, radius * 2, 6) is None
        off = z.copy()
        off[-1] = np.nextafter(off[-1], np.float32(np.inf))                  # one ulp in the last coordinate
        assert IC.attempt_of(off, seed, chain, D, radius, 6) is None
    assert IC.attempt_of(np.zeros(D + 1, np.float32), seed, chain, D, radius, 6) is None


def test_draws_of_the_block_of_four_edges_share_their_prefix():
    """Coordinate d comes from word d % 4 of Philox block d // 4: a draw at D is the prefix of the
    draw at D + 1 (what makes D = 3, 4, 5 the edges)."""
    for D in (1, 3, 4, 5, 257):
        assert np.array_equal(IC.draw(9, 2, 1, D, 2.0), IC.draw(9, 2, 1, D + 1, 2.0)[:D])


# ---------------------------------------------------------------- verdicts and predicted retries
def test_verdict_bands():
    F = IC.FLT_MAX
    g = np.zeros(3)
    assert IC.verdict(1.0, g) == IC.VALID and IC.verdict(F / 4.1, g) == IC.VALID
    assert IC.verdict(F / 3.9, g) == IC.AMBIGUOUS and IC.verdict(F * 3.9, g) == IC.AMBIGUOUS
    assert IC.verdict(F * 4.1, g) == IC.INVALID and IC.verdict(np.inf, g) == IC.INVALID
    assert IC.verdict(np.nan, g) == IC.INVALID and IC.verdict(0.0, np.array([0.0, np.nan])) == IC.INVALID
    assert IC.verdict(0.0, np.array([0.0, -F * 5])) == IC.INVALID and IC.verdict(-F, g) == IC.AMBIGUOUS
    assert IC.contradicts(IC.VALID, np.inf, g) and IC.contradicts(IC.INVALID, 1.0, g)
    assert not IC.contradicts(IC.AMBIGUOUS, np.inf, g) and not IC.contradicts(IC.AMBIGUOUS, 1.0, g)
    assert IC.contradicts(IC.VALID, 1.0, np.array([np.nan]))


def _evaluated_draws(ret, case, D):
    for c in range(case["C"]):
        for a, v in enumerate(ret.verdicts[c]):
            yield c, a, v, IC.draws(case["seed"], case["chain_offset"], case["C"], a, D, case["radius"])[c]


@pytest.mark.parametrize("model", ["schools", "funnel"])
def test_band_and_retry_counts_at_the_gpu_seeds(model):
    """At the GPU tests' seeds: the float32 oracle contradicts no band of the ladder 2 .. 2^14 (it
    rounds float64 once), the plain float32 restatement of the kernel -- whose intermediates do
    overflow -- contradicts none from BAND up and accepts the same attempts, the retry counts are
    those the GPU test's docstring records, ambiguous draws stay under the cap, and the plain
    float32 evaluation meets the standing tolerance at every accepted point."""
    if model == "schools":
        case, D, retry, plain, chk = IC.SCHOOLS_CASE, 10, IC.schools_retry, IC.schools_plain_f32, IC.check_schools
        o32, want = IC.schools_oracle(np.float32), dict(retrying=31, most=3, evaluated=169, ambiguous=1)
    else:
        case, D, retry, plain, chk = IC.FUNNEL_CASE, 300, IC.funnel_retry, IC.funnel_plain_f32, IC.check_funnel
        o32, want = IC.funnel_oracle(300, np.float32), dict(retrying=14, most=2, evaluated=147, ambiguous=2)
    ret = retry("oracle32")
    o64 = IC.schools_oracle() if model == "schools" else IC.funnel_oracle(300)
    for k in range(1, 15):
        band = 2.0 ** k
        for c, a, _, z in _evaluated_draws(ret, case, D):
            v = IC.verdict(*IC.eval64(o64, z), band)
            assert not IC.contradicts(v, *IC.as_f32(o32, z)), (band, c, a)
            if band >= IC.BAND:
                assert not IC.contradicts(v, *plain(z)), (band, c, a)
    got = dict(retrying=ret.retrying, most=ret.most_redraws, evaluated=ret.evaluated, ambiguous=ret.ambiguous)
    print(f"[init {model}] band {IC.BAND}: {got}")
    assert got == want
    assert ret.ambiguous <= IC.AMBIGUOUS_CAP * ret.evaluated
    assert (ret.accepted >= 0).all()
    rp = retry("plain32")
    assert np.array_equal(rp.accepted, ret.accepted)
    for c in range(case["C"]):
        pe, g = plain(ret.z[c])
        chk(np.float64(pe), g.astype(np.float64), ret.refs[c])


def test_unguarded_eight_schools_formulas_reject_valid_draws():
    """The defect the retry test exposed: with tau = e^u carried through log1p((tau / 5)^2),
    2 q / (1 + q) and log(sqrt(2 pi) tau), a float32 evaluation is not finite at u > 44.4 although
    U ~ 9 u and its gradient are small there -- it contradicts VALID verdicts at every band.  The
    kernel's u > 40 branch (schools_plain_f32's guarded form) does not."""
    case, n_bad = IC.SCHOOLS_CASE, 0
    o64 = IC.schools_oracle()
    for c in range(case["C"]):
        z = IC.draws(case["seed"], 0, case["C"], 0, 10, case["radius"])[c]
        v = IC.verdict(*IC.eval64(o64, z), 2.0 ** 14)
        bad = IC.contradicts(v, *IC.schools_plain_f32(z, guarded=False))
        assert bad == bool(v == IC.VALID and z[1] > np.float32(44.4)), (c, z[1], v)
        assert not IC.contradicts(v, *IC.schools_plain_f32(z))
        n_bad += bad
    assert n_bad >= 20  # more than a quarter of U(-100, 100) draws have u > 44.4


def test_gated_potential_retries_are_predicted_exactly():
    k = IC.GATE_CASE
    assert IC.pick_retry_seed(k["C"], k["D"], k["radius"]) == k["seed"]
    first = IC.gate_first_valid(k["seed"], k["C"], k["D"], k["radius"])
    assert first.min() == 0 and first.max() >= 3
    assert len(set(first[list(IC.GATE_EDGE_CHAINS)].tolist())) > 1
    print(f"[init gate] seed {k['seed']}: {int((first > 0).sum())} of {k['C']} chains retry, most redraws "
          f"{int(first.max())}, chains 0/63/64/129 accept at {first[list(IC.GATE_EDGE_CHAINS)].tolist()}")
    # the prediction is exact: z[0] of the accepted draw is at or under the threshold, every earlier one over it
    t = IC.gate_threshold(k["radius"])
    for c in range(k["C"]):
        col = [IC.draws(k["seed"], 0, k["C"], a, k["D"], k["radius"])[c, 0] for a in range(first[c] + 1)]
        assert col[-1] <= t and all(v > t for v in col[:-1])
