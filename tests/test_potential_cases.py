"""The conditions tests/test_gpu_potentials.py puts on the device hold for the references alone
(tests/potential_cases.py): the float32 oracle passes every check at every shape the GPU tests
run, the saturated and extreme-q inputs are what they claim to be, and the NumPy restatement of
the packed split-bf16 layout maps back onto X.  A failure of the same check on the GPU can then
only come from the kernel."""
import numpy as np
import pytest

import potential_cases as K
from oracle import potentials as OP


def _f32_logreg(X, y, Z):
    f32 = OP.LogisticRegression(X, y, dtype=np.float32)
    with np.errstate(over="ignore"):  # exp(+|l|) = inf in the saturated sigmoid: 1 / (1 + inf) = 0, exact
        out = [f32.pe_grad(z) for z in Z]
    return np.array([o[0] for o in out], np.float64), np.stack([o[1] for o in out]).astype(np.float64)


@pytest.mark.parametrize("D", K.LOGREG_DS)
def test_float32_oracle_passes_check_logreg(D):
    """Every (N, D, regime) of test_logreg_every_variant_matches_oracle: a plain float32 evaluation
    of the same formulas lies far inside check_logreg's tolerances (worst measured over the whole
    set: 0.011 of the U tolerance, 0.027 of the gradient's), so they leave the kernel room for its
    own rounding and nothing else."""
    for N in K.LOGREG_NS:
        for regime in K.REGIMES:
            with np.errstate(over="ignore"):
                X, y, Z, ref = K.logreg_reference(N, D, K.LOGREG_C, regime)
            pe, g = _f32_logreg(X, y, Z)
            r_pe, r_g = K.check_logreg(pe, g, X, y, Z, ref, label=f"N={N} D={D} {regime}")
            assert r_pe <= 0.1 and r_g <= 0.1, (N, D, regime, r_pe, r_g)


@pytest.mark.parametrize("D", K.LOGREG_DS)
def test_saturated_cases_saturate(D):
    """Saturated cases with N >= 257: at least 25% of the float64 logits beyond |l| = 30, the
    largest beyond 1000, every oracle value finite.  D = 1 cannot reach those figures with this
    generator: its logit is the single product x z with z = 0.3 n e^u, u ~ U(0, 6), so
    P(|l| > 30) = P(|x n| > 100 e^-u) averages to ~0.11 over u and the largest |l| of 300 chains
    is ~0.3 * 3 * 3 * e^6 ~ 1000.  There the bounds are the purpose's own: more than 5% of the
    logits beyond 30 and the largest beyond 104, where float32 exp(-|l|) is 0 even as a
    denormal."""
    for N in (257, 1000):
        with np.errstate(over="ignore"):
            X, y, Z, (pe_r, g_r) = K.logreg_reference(N, D, K.LOGREG_C, "saturated")
        L = np.abs(X.astype(np.float64) @ Z.astype(np.float64).T)
        frac, top = (L > 30).mean(), L.max()
        print(f"D={D} N={N}: {100 * frac:.0f}% of |logit| > 30, largest {top:.0f}")
        assert np.all(np.isfinite(pe_r)) and np.all(np.isfinite(g_r))
        if D == 1:
            assert frac >= 0.05 and top > 104.0
        else:
            assert frac >= 0.25 and top > 1000.0


@pytest.mark.parametrize("T", K.SV_TS)
def test_sv_cases_are_finite_extreme_and_within_f32(T):
    """Every sv_case of test_wide_models_at_slice_and_group_edges: the float64 oracle is finite,
    the float32 oracle passes the existing SV tolerances, and every batch of more than one chain
    holds a row with q < 2^-24 (the u == 1 branch) and a row with q > 1e8 (float64 q)."""
    for C in K.WIDE_CS:
        r, Z, ref64, ref32 = K.wide_reference("sv", T, C)
        assert np.all(np.isfinite(ref64[0])) and np.all(np.isfinite(ref64[1]))
        K.check_sv_outer(*ref32, ref64)
        e = K.wide_errors(*ref32, ref64)
        assert max(e) <= 2.0 ** -24  # the float32 oracle rounds the float64 result once
        if C > 1:
            q = K.sv_q(r, Z)
            assert (q < 2.0 ** -24).any() and (q > 1e8).any(), (q.min(), q.max())
        half_nu = 0.5 * np.exp(Z[:, 0].astype(np.float64))
        assert half_nu.min() >= 0.02 and half_nu.max() <= 60.0  # nmx_lgamma_digamma_half_diff's stated range


@pytest.mark.parametrize("model", ["funnel", "funnel_nc"])
@pytest.mark.parametrize("dim", K.FUNNEL_DIMS)
def test_funnel_cases_are_finite_and_within_f32(model, dim):
    for C in K.WIDE_CS:
        _, Z, ref64, ref32 = K.wide_reference(model, dim, C)
        assert np.all(np.isfinite(ref64[0])) and np.all(np.isfinite(ref64[1]))
        K.check_funnel_outer(*ref32, ref64, centred=model == "funnel")
        assert max(K.wide_errors(*ref32, ref64)) <= 2.0 ** -24
        assert np.abs(Z[:, :-1]).max() <= 2.0 and np.abs(Z[:, -1]).max() <= 6.0


def test_plain_float32_shows_which_quantities_the_rounded_oracle_bound_fits():
    """The float32 oracle evaluates in float64 and rounds once (error <= 2^-24), so 4x its error is
    the floor 4 x 2^-23 everywhere.  A plain float32 evaluation of the kernel's formulas (NumPy:
    libm row math, pairwise float32 row sums) stays inside the existing tolerances at every shape
    and meets that bound on the quantities WIDE_F32_LIMITED leaves unmarked (the centred funnel's
    U), but exceeds it on each marked one (SV's U 17x over, its gradient 1.2x, the centred
    funnel's gradient 9x): those are differences of float32 sums that cancel, so the bound there
    would fail every float32 kernel, right or wrong."""
    worst = {}
    for model, sizes in (("sv", K.SV_TS), ("funnel", K.FUNNEL_DIMS)):
        for size in sizes:
            for C in K.WIDE_CS:
                _, Z, ref64, ref32 = K.wide_reference(model, size, C)
                plain = K.wide_plain_f32(model, size, C)
                if model == "sv":
                    K.check_sv_outer(*plain, ref64)
                else:
                    K.check_funnel_outer(*plain, ref64, centred=True)
                e, r, _ = K.wide_ratios(*plain, ref64, ref32, label=f"plain float32 {model} size={size} C={C}")
                for i in range(2):
                    over = e[i] / max(K.WIDE_MARGIN * r[i], K.WIDE_FLOOR)
                    worst[model, i] = max(worst.get((model, i), 0.0), over)
    for (model, i), over in worst.items():
        print(f"plain float32 {model} {('U', 'grad')[i]}: worst error / bound {over:.2f}")
        assert (over > 1.0) if K.WIDE_F32_LIMITED[model][i] else (over <= 1.0), (model, i, over)


def test_check_wide_vs_f32_rejects_a_wrong_kernel():
    """The check passes the float32 oracle itself (ratio 1) and a result a few float32 ulp off,
    and fails one that is 1e-5 off in U or drops one gradient row."""
    _, Z, ref64, ref32 = K.wide_reference("sv", 65, 65)
    assert K.check_wide_vs_f32(*ref32, ref64, ref32, Z) == (1.0, 1.0)
    K.check_wide_vs_f32(ref32[0] * (1 + 3 * 2.0 ** -23), ref32[1], ref64, ref32, Z)
    with pytest.raises(AssertionError):
        K.check_wide_vs_f32(ref32[0] * (1 + 1e-5), ref32[1], ref64, ref32, Z)
    g = ref32[1].copy()
    g[7, 40] = 0.0
    with pytest.raises(AssertionError):
        K.check_wide_vs_f32(ref32[0], g, ref64, ref32, Z)
    pe = ref32[0].copy()
    pe[3] = np.nan
    with pytest.raises(AssertionError):
        K.check_wide_vs_f32(pe, ref32[1], ref64, ref32, Z)


def test_check_logreg_rejects_a_masked_column():
    """A gradient that misses one feature column's data term (a column mask one short at D = 64)
    or a U that is -inf / NaN fails check_logreg."""
    X, y, Z, ref = K.logreg_reference(257, 64, K.LOGREG_C, "unit")
    K.check_logreg(ref[0], ref[1], X, y, Z, ref)
    g = ref[1].copy()
    g[:, 63] = Z[:, 63]  # the prior term alone
    with pytest.raises(AssertionError):
        K.check_logreg(ref[0], g, X, y, Z, ref)
    for bad in (np.nan, -np.inf):
        pe = ref[0].copy()
        pe[5] = bad
        with pytest.raises(AssertionError):
            K.check_logreg(pe, ref[1], X, y, Z, ref)


@pytest.mark.parametrize("N,D", K.PACK_SHAPES)
def test_expected_pack_reproduces_X(N, D):
    """expected_pack's image read back through the inverse of each layout: the GEMM1 A pieces,
    the GEMM2 B pieces and (H = 1) the combined pieces each give back the three bf16 planes of
    the zero-padded X, whose sum is X to 2^-24 relative; padded rows and columns are zero; the
    label piece holds y - 1/2 once per row."""
    rs = np.random.RandomState(N * 64 + D)
    X = (rs.randn(N, D) * np.exp(rs.randn(N, D) * 3)).astype(np.float32)
    y = (rs.rand(N) < 0.5).astype(np.float32)
    bits, planes, Xp = K.expected_pack(X, y)
    KB, DT, H, NP = K.pack_dims(D)
    nt = (N + 31) // 32
    assert bits.shape == (nt, NP, 64, 8) and NP == 3 * KB + 2 * H + 6 * DT + 1
    assert H == (1 if D in range(49, 57) else 0)
    val = (bits.astype(np.uint32) << 16).view(np.float32)
    back_a = np.zeros((3, nt * 32, 64), np.float32)
    back_b = np.zeros((3, nt * 32, 64), np.float32)
    for t in range(nt):
        for p in range(3):
            for L in range(64):
                r, h = L & 31, L >> 5
                for kb in range(KB):
                    back_a[p, 32 * t + r, 16 * kb + 8 * h:16 * kb + 8 * h + 8] = val[t, p * KB + kb, L]
                for dt in range(DT):
                    for s in range(2):
                        for j in range(8):
                            row = 32 * t + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3)
                            back_b[p, row, 32 * dt + r] = val[t, 3 * KB + 2 * H + p * 2 * DT + 2 * dt + s, L, j]
    for p in range(3):
        np.testing.assert_array_equal(back_a[p].view(np.uint32), planes[p].view(np.uint32))
        np.testing.assert_array_equal(back_b[p].view(np.uint32), planes[p].view(np.uint32))
    if H:
        for t in range(nt):
            rows = slice(32 * t, 32 * t + 32)
            for cp, (p0, p1) in enumerate([(0, 1), (2, 0)]):
                np.testing.assert_array_equal(val[t, 3 * KB + cp, :32], planes[p0][rows, 48:56])
                np.testing.assert_array_equal(val[t, 3 * KB + cp, 32:], planes[p1][rows, 48:56])
    total = back_a.astype(np.float64).sum(0)
    assert np.all(np.abs(total - Xp) <= 2.0 ** -24 * np.abs(Xp) + 1e-45)
    np.testing.assert_array_equal(Xp[:N, :D], X)
    assert not Xp[N:].any() and not Xp[:, D:].any() and not total[N:].any() and not total[:, D:].any()
    lab = bits[:, NP - 1].reshape(nt, 64 * 8).view(np.float32).reshape(nt, 64, 4)
    assert not lab[:, 8:].any()
    seen = np.full(nt * 32, np.nan, np.float32)
    for t in range(nt):
        for L in range(8):
            for k in range(4):
                row = 32 * t + k + 8 * (L & 3) + 4 * (L >> 2)
                assert np.isnan(seen[row])
                seen[row] = lab[t, L, k]
    np.testing.assert_array_equal(seen[:N], y - np.float32(0.5))
    assert not seen[N:].any()
