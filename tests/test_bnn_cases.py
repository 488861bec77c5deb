"""What tests/test_gpu_bnn.py asks of the device holds for the references alone, and a reference
with a defect fails it (tests/bnn_cases.py): the two float32 restatements pass
check_float32_level against each other at every shape and regime, the float64 reference and an
independent autograd derivation agree to 1e-12, and each of CORRUPTIONS -- a term lost at a tile
or row edge, or one gradient element 1e-4 off -- is rejected at every shape, while the tolerance
of test_gpu_potentials.py test_bnn_matches_oracle lets some of them through.  A failure of the
same check on the GPU can then only come from the kernel."""
import numpy as np
import pytest

import bnn_cases as B
from oracle.batched import BNNBatch

C = 16
_CASES = [pytest.param(shape, regime, id=f"{shape[0]}-{shape[1]}-{shape[2]}-{regime}")
          for shape in B.SHAPES for regime in B.REGIMES]


def test_case_list_reaches_its_edges():
    """The shapes hold N and H at 1, 15, 16, 17 and around the register-blocked shape, Dx from 1
    to 5, a tile count above the 8 waves, and a D that is no multiple of the transposes' 64."""
    Ns, Dxs, Hs = ({s[i] for s in B.SHAPES} for i in range(3))
    assert {1, 15, 16, 17, 99, 100} <= Ns and {1, 15, 16, 17, 68, 69} <= Hs and {1, 2, 3, 4, 5} <= Dxs
    assert any(-(-n // 16) * -(-h // 16) > 8 for n, _, h in B.SHAPES if (n, h) != (100, 69))
    assert B.dim_of(16, 3, 16) == 321 and B.C3_SHAPE in B.SHAPES and set(B.C3_NEIGHBOURS) <= set(B.SHAPES)
    for shape in B.SHAPES:  # the seed is a function of the shape: no two cases share data
        assert sum(B.shape_seed(*s) == B.shape_seed(*shape) for s in B.SHAPES) == 1


@pytest.mark.parametrize("shape,regime", _CASES)
def test_regimes_are_what_they_claim(shape, regime):
    """Z is float32 with log prec inside the regime's range; `saturated` puts most second-layer
    units of H >= 15 beyond |tanh| = 0.99 and `far_u` spans precisions below 1e-3 and above 50."""
    X, Y, Z, f64, _, _ = B.reference(*shape, C, regime)
    lo, hi = B.REGIMES[regime][1]
    assert Z.dtype == np.float32 and X.dtype == np.float32 and Y.dtype == np.float32
    assert Z.shape == (C, B.dim_of(*shape)) and lo <= Z[:, 0].min() and Z[:, 0].max() <= hi
    assert np.all(np.isfinite(f64[0])) and np.all(np.isfinite(f64[1]))
    if regime == "far_u":
        p = np.exp(Z[:, 0].astype(np.float64))
        assert p.min() < 1e-3 and p.max() > 50.0
    if regime == "saturated" and shape[2] >= 15:
        N, Dx, H = shape
        w1 = Z[:, 1:1 + Dx * H].reshape(C, Dx, H).astype(np.float64)
        w2 = Z[:, 1 + Dx * H:1 + Dx * H + H * H].reshape(C, H, H).astype(np.float64)
        h2 = np.tanh(np.tanh(X.astype(np.float64) @ w1) @ w2)
        assert (np.abs(h2) > 0.99).mean() > 0.5


@pytest.mark.parametrize("shape,regime", _CASES)
def test_restatement_is_bitwise_the_oracle(shape, regime):
    """bnn_cases.restate without a defect is BNNBatch: bit for bit in float32, and in float64 after
    the rounding to float32 that BNNBatch applies to what it returns (so float64_reference is
    BNNBatch(dtype=np.float64) one step earlier)."""
    X, Y, Z, f64, f32, _ = B.reference(*shape, C, regime)
    H = shape[2]
    for dtype, ours in ((np.float32, f32), (np.float64, f64)):
        U, G = BNNBatch(X, Y, H, dtype=dtype)(Z)
        assert U.dtype == np.float32 and G.dtype == np.float32
        np.testing.assert_array_equal(U, ours[0].astype(np.float32))
        np.testing.assert_array_equal(G, ours[1].astype(np.float32))
    if shape == B.SHAPES[0]:  # the batch rows are independent: a row alone gives the same bits
        U1, G1 = B.restate(X, Y, H, Z[3:4], np.float64)
        np.testing.assert_array_equal(U1, f64[0][3:4])
        np.testing.assert_array_equal(G1, f64[1][3:4])


@pytest.mark.parametrize("shape,regime", _CASES)
def test_float64_autograd_agrees_with_the_hand_derived_adjoint(shape, regime):
    """U from the model's log density in torch float64 and its autograd gradient against
    BNNBatch's float64 formulas: 1e-12 of each quantity's scale (the scale of site_errors)."""
    import torch

    X, Y, Z, f64, _, _ = B.reference(*shape, C, regime)
    t64 = B.torch_restatement(X, Y, shape[2], Z, torch.float64)
    for q, e in B.site_errors(t64, f64, shape).items():
        assert e.max() <= 1e-12, (q, e.max())


@pytest.mark.parametrize("shape,regime", _CASES)
def test_float32_restatements_pass_the_check_both_ways(shape, regime):
    """Validity: the torch float32 restatement passes check_float32_level with the NumPy float32
    restatement as the yardstick, and the NumPy one with the torch one as the yardstick, for U and
    each of the four gradient blocks, at all 36 (shape, regime): the margin of 4 leaves a correct
    float32 evaluation in another summation order room, with no quantity needing another scale
    (per-site errors 3e-8 to 8e-6, the largest in `saturated` at (5, 3, 65))."""
    X, Y, Z, f64, f32, t32 = B.reference(*shape, C, regime)
    B.check_float32_level(t32, f32, f64, shape, label=f"torch f32 vs NumPy f32 {regime}")
    B.check_float32_level(f32, t32, f64, shape, label=f"NumPy f32 vs torch f32 {regime}")
    assert max(B.check_float32_level(f32, f32, f64, shape, label="itself", log=lambda s: None).values()) <= 1.0
    for q, e in B.site_errors(f32, f64, shape).items():
        assert e.max() <= 2e-5, (q, e.max())  # float32 level itself: 36 x below the existing 1e-3 at worst


_POWER = [pytest.param(shape, name, id=f"{shape[0]}-{shape[1]}-{shape[2]}-{name}")
          for shape in B.SHAPES for name in B.CORRUPTIONS if B.corruption_applies(name, shape)]


@pytest.mark.parametrize("shape,name", _POWER)
def test_check_rejects_each_corruption(shape, name):
    """Power: the float32 restatement with one defect fails check_float32_level in every regime,
    at every shape where the defect's term exists (a clamped last row needs N >= 2), and the
    failing quantity is one the defect touches."""
    touched = {"gw2_tile_misses_last_k": {"w2"}, "gw2_one_element_1e-4": {"w2"}, "g0_esq_short": {"prec_obs"},
               "ga1_last_row_clamped": {"w1"}, "h2_w2_last_row_zero": {"U", "prec_obs", "w1", "w2", "w3"}}[name]
    for regime in B.REGIMES:
        X, Y, Z, f64, f32, _ = B.reference(*shape, C, regime)
        bad = B.restate(X, Y, shape[2], Z, np.float32, corrupt=name)
        level = B.float32_level(bad, f32, f64, shape)
        failing = {q for q, (e, _, b) in level.items() if not e <= b}
        assert failing and failing <= touched, (regime, failing, level)
        with pytest.raises(AssertionError):
            B.check_float32_level(bad, f32, f64, shape, label=name, log=lambda s: None)


def test_check_rejects_non_finite_and_missing_rows():
    X, Y, Z, f64, f32, _ = B.reference(16, 3, 16, C, "unit")
    for q, col in (("U", None), ("w2", 100)):
        U, G = f32[0].copy(), f32[1].copy()
        if col is None:
            U[5] = np.nan
        else:
            G[5, col] = np.inf
        with pytest.raises(AssertionError):
            B.check_float32_level((U, G), f32, f64, (16, 3, 16), log=lambda s: None)
    with pytest.raises(AssertionError):  # a batch cut short is not a batch with rows excluded
        B.check_float32_level((f32[0][:15], f32[1][:15]), f32, f64, (16, 3, 16), log=lambda s: None)


def test_existing_tolerance_accepts_what_the_check_rejects():
    """Why the per-site check exists.  At test_bnn_matches_oracle's own shape (N, Dx, H) = (100, 3,
    69) and regime (weights 0.5 n, log prec in [-1, 2]), with that test's tolerances (rtol 1e-3,
    atol 1e-3 max |g| over the whole chain, asserted chain by chain):
      * one element of grad W2 off by 1e-4 of itself passes on all 16 chains;
      * grad W2 without its k = N-1 term in a whole 16 x 16 tile passes on several chains, and
      * g[0] from esq over N-1 rows passes on several chains,
    and on exactly those chains, taken as a batch of their own, check_float32_level rejects each."""
    shape = B.C3_SHAPE
    X, Y, Z, f64, f32, _ = B.reference(*shape, C, "unit")
    assert B.existing_tolerance_accepts(f32, f64).all()
    for name, at_least in (("gw2_one_element_1e-4", C), ("gw2_tile_misses_last_k", 3), ("g0_esq_short", 3)):
        bad = B.restate(X, Y, shape[2], Z, np.float32, corrupt=name)
        ok = B.existing_tolerance_accepts(bad, f64)
        print(f"{name}: the existing tolerance accepts {int(ok.sum())} of {C} chains")
        assert ok.sum() >= at_least, (name, int(ok.sum()))
        rows = np.flatnonzero(ok) if name != "gw2_one_element_1e-4" else np.arange(C)
        sub = lambda r: (r[0][rows], r[1][rows])  # noqa: E731
        with pytest.raises(AssertionError):
            B.check_float32_level(sub(bad), sub(f32), sub(f64), shape, label=name, log=lambda s: None)


@pytest.mark.parametrize("N,Dx,H,Dy", B.PREDICT_SHAPES)
def test_predictive_restatement_is_at_float32_level(N, Dx, H, Dy):
    """The float32 restatement of a predictive draw lies within 1e-5 of the oracle (scaled by
    max(1, |ref|)), far inside the existing rtol = atol = 1e-4; the draw minus the oracle's own
    z / sqrt(prec) is the network's mean, whatever the seed; a set of 300 samples begins with
    the set of 16."""
    from oracle import predictive as OPred

    X, smp = B.predict_case(N, Dx, H, Dy)
    ref = OPred.predict_bnn(X, smp["prec_obs"], smp["w1"], smp["w2"], smp["w3"], 5)
    assert ref.shape == (B.PREDICT_S, N, Dy)
    f32 = B.predict_float32(X, smp, N, Dy, 5)
    assert B.check_predict_float32_level(f32, f32, ref, label=f"{(N, Dx, H, Dy)} itself") <= 1.0
    assert (np.abs(f32 - ref) / np.maximum(1.0, np.abs(ref))).max() <= 1e-5
    bad = f32.copy()
    bad[3, N - 1, Dy - 1] += 1e-4 * max(1.0, abs(bad[3, N - 1, Dy - 1]))
    with pytest.raises(AssertionError):
        B.check_predict_float32_level(bad, f32, ref, log=lambda s: None)
    mean5 = ref - B.predict_noise(smp, N, Dy, 5)[1]
    ref9 = OPred.predict_bnn(X, smp["prec_obs"], smp["w1"], smp["w2"], smp["w3"], 9)
    np.testing.assert_allclose(ref9 - B.predict_noise(smp, N, Dy, 9)[1], mean5, rtol=0, atol=1e-12)
    X2, big = B.predict_case(N, Dx, H, Dy, S=40)
    np.testing.assert_array_equal(X2, X)
    for k, v in smp.items():
        np.testing.assert_array_equal(big[k][:B.PREDICT_S], v)
