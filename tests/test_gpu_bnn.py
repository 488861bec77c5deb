"""The BNN kernels on the device, site by site, at tile edges and on active lists:
csrc/potential_bnn.hip (k_bnn for any shape, the register-blocked k_bnn_c3 at N = 100, Dx = 3,
H = 69, and the transposes k_cols_to_rows / k_rows_to_cols around both) and csrc/predictive.hip
k_predict_bnn.  Cases, references and the check: tests/bnn_cases.py.

Tolerance rule (tests/test_gpu_program_ops.py and tests/test_gpu_linalg_ops.py, here per site):
for U and for each of the gradient blocks of prec_obs, w1, w2 and w3, the per-chain scaled error
against float64 -- |dU| / max(1, |U64|), max |dg_site| / max(1, max |g64_site|) -- has a maximum
over the batch of at most 4 x that of a float32 restatement of the same formulas on the same rows
(oracle/batched.py BNNBatch(dtype=np.float32)) + 16 x 2^-24, no row excluded.  Every number in it
comes from references: float64 is BNNBatch's float64 evaluation before its rounding to float32;
the margin of 4 and the floor are the project's, and tests/test_bnn_cases.py shows on the CPU that
a second, independently written float32 evaluation (torch autograd on the log density) passes
the rule in both directions at every (shape, regime) here, that float64 autograd agrees with the
float64 reference to 1e-12, and that a result with one term lost at a tile or row edge, or one
gradient element 1e-4 off, fails it.  The float32 restatement's own error is 3e-8 to 8e-6 per
site, so the bounds are 1e-6 to 3e-5: 30 to 1000 times tighter than test_gpu_potentials.py
test_bnn_matches_oracle's 1e-3 of the whole chain's largest gradient, which stays as it is.

Everything else is bitwise: a chain's U and gradient do not depend on how many chains share the
launch, on which of nmx_eval_chain's modes (dense, phase array, compacted list) selected it, on
columns versus rows, or on what the workspace held; an unselected chain keeps its fill."""
import numpy as np
import pytest

import bnn_cases as B
from test_gpu_potentials import _eval, _eval_list

pytestmark = pytest.mark.gpu

C = 65            # two 64-chain groups of the transposes, the second with one chain
C_WIDE = 130      # three groups, the last with two chains
LDS_LIMIT = 160 * 1024
_LIST9 = np.array([64, 3, 129, 0, 63, 100, 32, 77, 9])  # unsorted, both sides of chain 64, the ends
_BITWISE_SHAPES = [(17, 1, 17), B.C3_SHAPE]


def _pot(N, Dx, H):
    from numpyro_amd.potentials import BNN

    X, Y = B.data(N, Dx, H)
    return BNN(X, Y, H)


def _accuracy(device, shape):
    """{(regime, C): ratios} of one shape: every regime at C chains and `unit` at one chain."""
    pot = _pot(*shape)
    out = {}
    for regime, chains in [(r, C) for r in B.REGIMES] + [("unit", 1)]:
        _, _, Z, f64, f32, _ = B.reference(*shape, chains, regime)
        out[regime, chains] = B.check_float32_level(_eval(pot, Z, device), f32, f64, shape, label=f"{regime} C={chains}")
    return out


@pytest.mark.parametrize("shape", [s for s in B.SHAPES if s != B.C3_SHAPE and s not in B.C3_NEIGHBOURS],
                         ids=lambda s: "-".join(map(str, s)))
def test_generic_kernel_stays_at_float32_level_per_site(device, shape):
    """k_bnn at each tile edge (bnn_cases.SHAPES), 65 chains in the three regimes and one chain:
    U and the four gradient blocks each within the float32 rule."""
    _accuracy(device, shape)


def test_c3_kernel_and_its_neighbours_stay_at_float32_level_per_site(device):
    """k_bnn_c3 at (100, 3, 69) and k_bnn at (99, 3, 69), (100, 3, 68), (100, 2, 69): the same rule;
    the ratios device / float32 restatement of the four printed side by side, so a difference
    between the register-blocked kernel and the generic one at the same size shows."""
    shapes = [B.C3_SHAPE] + B.C3_NEIGHBOURS
    ratios = {s: _accuracy(device, s) for s in shapes}
    print("[bnn c3 vs neighbours] device error / float32 restatement error; columns " +
          "  ".join(str(s) for s in shapes))
    for key in ratios[B.C3_SHAPE]:
        for q in ("U",) + B.SITES:
            print(f"[bnn c3 vs neighbours] {key[0]:9s} C={key[1]:<3d} {q:8s} " +
                  "  ".join(f"{ratios[s][key][q]:6.2f}" for s in shapes))


@pytest.mark.parametrize("shape", [(16, 3, 16), B.C3_SHAPE], ids=lambda s: "-".join(map(str, s)))
def test_chain_count_does_not_change_a_chain(device, shape):
    """Launches of 1, 63, 64, 65 and 130 chains give bitwise the first rows of the 130-chain
    launch: the XCD block permutation of k_bnn (pos = (b % 8) per + b / 8 over ldc blocks) and the
    transposes' 64-position tiles at their edge."""
    pot = _pot(*shape)
    Z = B.positions(*shape, C_WIDE, "unit")
    pe_a, g_a = _eval(pot, Z, device)
    assert np.all(np.isfinite(pe_a)) and np.all(np.isfinite(g_a))
    for n in (1, 63, 64, 65, 130):
        pe_b, g_b = _eval(pot, Z[:n], device)
        np.testing.assert_array_equal(pe_b, pe_a[:n], err_msg=f"{n} chains")
        np.testing.assert_array_equal(g_b, g_a[:n], err_msg=f"{n} chains")


@pytest.mark.parametrize("shape", _BITWISE_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_phase_and_list_launches_are_bitwise_the_dense_launch(device, shape):
    """nmx_eval_chain's other modes through both transposes and the kernel: a phase array with
    every third chain at PH_LEAF, a scattered unsorted list of 9 chains from all three 64-chain
    groups (chains 0, 63, 64 and 129 among them) and a list of 65 chains (a second position tile
    of one) each give bitwise the dense launch's U and gradient on the evaluated chains and leave
    the NaN fill of every other chain's U and gradient column in place."""
    from numpyro_amd import native

    pot = _pot(*shape)
    Z = B.positions(*shape, C_WIDE, "unit")
    pe_d, g_d = _eval(pot, Z, device)
    assert np.all(np.isfinite(pe_d)) and np.all(np.isfinite(g_d))
    phase = np.zeros(C_WIDE, np.int32)
    phase[::3] = native.PH_LEAF
    runs = [("phase", np.flatnonzero(phase == native.PH_LEAF), _eval(pot, Z, device, phase=phase)),
            ("list of 9", _LIST9, _eval_list(pot, Z, _LIST9, device, full=True))]
    idx65 = np.random.RandomState(65).permutation(C_WIDE)[:65]
    assert idx65.min() < 64 <= idx65.max() and np.any(idx65 >= 128)
    runs.append(("list of 65", idx65, _eval_list(pot, Z, idx65, device, full=True)))
    for what, on, (pe, g) in runs:
        np.testing.assert_array_equal(pe[on], pe_d[on], err_msg=what)
        np.testing.assert_array_equal(g[on], g_d[on], err_msg=what)
        off = np.setdiff1d(np.arange(C_WIDE), on)
        assert off.size and np.all(np.isnan(pe[off])) and np.all(np.isnan(g[off])), what


def _launch(pot, Z, device, idx=None, rows=False, bind=True):
    """One launch of `pot` over the chains of Z (idx: as a compacted list), on columns through
    BNN.evaluate or on rows through BNN.evaluate_rows (row p of z_rows: the chain at position p),
    without rebinding when bind is False (pot.workspace stays the tensor the caller prepared).
    Returns (U [C], gradient [C, D] by chain, NaN where nothing was written) as float32."""
    import torch

    from numpyro_amd import native

    n_c, D = Z.shape
    ldc = (n_c + 63) // 64 * 64
    if bind:
        pot.bind(n_c, ldc, device)
    pe = torch.full((ldc,), float("nan"), device=device)
    lst = cnt = None
    order = np.arange(n_c) if idx is None else np.asarray(idx)
    if idx is not None:
        lst = torch.zeros(ldc, dtype=torch.int32, device=device)
        lst[:len(order)] = torch.as_tensor(order.astype(np.int32), device=device)
        cnt = torch.tensor([len(order)], dtype=torch.int32, device=device)
    G = np.full((n_c, D), np.nan, np.float32)
    if rows:
        zr = torch.zeros(ldc, D, device=device)
        zr[:len(order)] = torch.from_numpy(np.ascontiguousarray(Z[order])).to(device)
        gr = torch.full((ldc, D), float("nan"), device=device)
        ev = native.EvalBatch(pe=native.ptr(pe), active_idx=native.ptr(lst), active_count=native.ptr(cnt),
                              num_chains=n_c, ldc=ldc)
        pot.evaluate_rows(ev, native.ptr(zr), native.ptr(gr), native.stream_ptr())
        torch.cuda.synchronize()
        g_rows = gr.cpu().numpy()
        assert np.all(np.isnan(g_rows[len(order):]))  # rows past the last position stay untouched
        G[order] = g_rows[:len(order)]
    else:
        z = torch.zeros(D, ldc, device=device)
        z[:, :n_c] = torch.from_numpy(np.ascontiguousarray(Z.T)).to(device)
        g = torch.full((D, ldc), float("nan"), device=device)
        ev = native.EvalBatch(z=native.ptr(z), grad=native.ptr(g), pe=native.ptr(pe), active_idx=native.ptr(lst),
                              active_count=native.ptr(cnt), num_chains=n_c, ldc=ldc)
        pot.evaluate(ev, native.stream_ptr())
        torch.cuda.synchronize()
        G = g[:, :n_c].cpu().numpy().T.copy()
    return pe[:n_c].cpu().numpy(), G


def _same_bits(a, b, what):
    for x, y, name in zip(a, b, ("U", "gradient")):
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg=f"{what}: {name}")


@pytest.mark.parametrize("shape", _BITWISE_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_rows_path_is_bitwise_the_column_path(device, shape):
    """BNN.evaluate_rows (nmx_pe_bnn_rows: the kernel on the caller's rows, no transposes) dense
    and on the list of 9: U bitwise the column path's, gradient rows bitwise its columns, and on
    the list nothing written for another chain."""
    pot = _pot(*shape)
    Z = B.positions(*shape, C_WIDE, "unit")
    cols = _launch(pot, Z, device)
    assert np.all(np.isfinite(cols[0])) and np.all(np.isfinite(cols[1]))
    _same_bits(_launch(pot, Z, device, rows=True), cols, "rows, dense")
    listed = _launch(pot, Z, device, idx=_LIST9)
    _same_bits(_launch(pot, Z, device, idx=_LIST9, rows=True), listed, "rows, list of 9")
    _same_bits((listed[0][_LIST9], listed[1][_LIST9]), (cols[0][_LIST9], cols[1][_LIST9]), "columns, list of 9")
    off = np.setdiff1d(np.arange(C_WIDE), _LIST9)
    assert np.all(np.isnan(listed[0][off])) and np.all(np.isnan(listed[1][off]))


@pytest.mark.parametrize("shape", _BITWISE_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_workspace_contents_and_repeats_do_not_matter(device, shape):
    """The row workspace of nmx_pe_bnn (positions, then gradients) is scratch: from a workspace of
    0xFF bytes (NaN in every float) the dense launch and the list-of-9 launch give bitwise what
    they give from a zeroed one, and two consecutive launches are bitwise equal."""
    pot = _pot(*shape)
    Z = B.positions(*shape, C_WIDE, "unit")
    pot.bind(C_WIDE, 192, device)
    ws = pot.workspace
    for idx, what in ((None, "dense"), (_LIST9, "list of 9")):
        ws.zero_()
        clean = _launch(pot, Z, device, idx=idx, bind=False)
        assert pot.workspace is ws
        ws.fill_(0xFF)
        _same_bits(_launch(pot, Z, device, idx=idx, bind=False), clean, f"{what}: 0xFF workspace")
        _same_bits(_launch(pot, Z, device, idx=idx, bind=False), clean, f"{what}: repeat")
        on = np.arange(C_WIDE) if idx is None else idx
        assert np.all(np.isfinite(clean[0][on])) and np.all(np.isfinite(clean[1][on]))


def _bnn_lds_bytes(N, Dx, H):
    """potential_bnn.hip lds_bytes: W1, W2, w3, X, Y, two N x H layers, gy and the 512 floats of
    the workgroup sums."""
    return 4 * (Dx * H + H * H + H + N * Dx + N + 2 * N * H + N + 512)


def test_lds_limit_of_the_potential(device):
    """k_bnn keeps a chain's weights, data and both layers in LDS; nmx_pe_bnn and nmx_pe_bnn_rows
    refuse what needs more than 160 KiB.  At H = 69, Dx = 3 the count is 4 (5549 + 143 N): N = 247
    (163480 bytes, the dynamic-LDS attribute raised through nmx_lds_limit, one workgroup per CU)
    runs and holds the float32 rule; N = 248 (164052 bytes) is refused by both entry points with a
    message naming N, H and the byte count, and the refusal leaves nothing behind: the N = 247
    launch straight after it is bitwise its earlier self."""
    import torch

    from numpyro_amd import native

    Dx, H = 3, 69
    n_fit = max(n for n in range(1, 400) if _bnn_lds_bytes(n, Dx, H) <= LDS_LIMIT)
    assert n_fit == 247 and _bnn_lds_bytes(n_fit, Dx, H) == 163480 and _bnn_lds_bytes(n_fit + 1, Dx, H) == 164052
    shape = (n_fit, Dx, H)
    pot = _pot(*shape)
    _, _, Z, f64, f32, _ = B.reference(*shape, 2, "unit")
    before = _launch(pot, Z, device)
    B.check_float32_level(before, f32, f64, shape, label="largest N under the LDS limit, C=2")
    big = _pot(n_fit + 1, Dx, H)
    wanted = rf"N={n_fit + 1}, H={H} needs {_bnn_lds_bytes(n_fit + 1, Dx, H)} bytes"
    with pytest.raises(native.NativeError, match=wanted):
        _launch(big, Z, device)
    with pytest.raises(native.NativeError, match=wanted):
        _launch(big, Z, device, rows=True)
    torch.cuda.synchronize()
    _same_bits(_launch(pot, Z, device), before, "after the refusal")
    _same_bits(_launch(pot, Z, device, rows=True), before, "rows, after the refusal")


# -------------------------------------------------------------------------------- k_predict_bnn
def _predict(device, X, smp, H, Dy, seed):
    """[S, N, Dy] float32 draws: through Predictive(P.bnn, samples) where it takes the model
    (D_Y = 1), else through nmx_predict_bnn on the flattened samples (sorted sites)."""
    import torch

    from numpyro_amd import native
    from numpyro_amd import potentials as P
    from numpyro_amd.infer import Predictive

    if Dy == 1:
        out = Predictive(P.bnn, {k: torch.from_numpy(v) for k, v in smp.items()})(seed, X, None, H)["Y"]
        return out.cpu().numpy()
    S, (N, Dx) = len(smp["prec_obs"]), X.shape
    flat = np.concatenate([smp["prec_obs"].reshape(S, 1)] + [smp[k].reshape(S, -1) for k in ("w1", "w2", "w3")], 1)
    d_x, d_flat = torch.from_numpy(X).to(device), torch.from_numpy(np.ascontiguousarray(flat, np.float32)).to(device)
    out = torch.full((S, N, Dy), float("nan"), device=device)
    native.check(native.lib().nmx_predict_bnn(native.ptr(d_x), N, Dx, H, Dy, native.ptr(d_flat), S, seed,
                                              native.ptr(out), native.stream_ptr()), "nmx_predict_bnn")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _oracle_predict(X, smp, seed):
    from oracle import predictive as OPred

    return OPred.predict_bnn(X, smp["prec_obs"], smp["w1"], smp["w2"], smp["w3"], seed)


@pytest.mark.parametrize("N,Dx,H,Dy", B.PREDICT_SHAPES)
def test_predictive_draws_at_float32_level_and_launch_shape_independent(device, N, Dx, H, Dy):
    """k_predict_bnn at one row and unit, past one tile with D_Y = 3, at H = 65 with D_Y = 2 and at
    the BASELINE shape, 16 samples: against oracle.predictive.predict_bnn on the same Philox
    stream within 4 x the float32 restatement's scaled error + 16 x 2^-24 (the forward pass in
    float32 plus the oracle's normal variates times a float32 1 / sqrt(prec)), inside the existing
    rtol = atol = 1e-4; the same seed twice bitwise equal; rows 0..15 of a 300-sample launch
    bitwise the 16-sample launch (a draw depends on (seed, sample, element) only); and per sample
    the draw minus the oracle's z / sqrt(prec) is the same mean under two seeds to 1e-4."""
    X, smp = B.predict_case(N, Dx, H, Dy)
    out = _predict(device, X, smp, H, Dy, 5)
    assert out.shape == (B.PREDICT_S, N, Dy) and out.dtype == np.float32
    ref = _oracle_predict(X, smp, 5)
    np.testing.assert_allclose(out, ref, rtol=1e-4, atol=1e-4)
    B.check_predict_float32_level(out, B.predict_float32(X, smp, N, Dy, 5), ref, label=f"{(N, Dx, H, Dy)}")
    np.testing.assert_array_equal(_predict(device, X, smp, H, Dy, 5).view(np.uint32), out.view(np.uint32))
    X300, smp300 = B.predict_case(N, Dx, H, Dy, S=300)
    out300 = _predict(device, X300, smp300, H, Dy, 5)
    np.testing.assert_array_equal(out300[:B.PREDICT_S].view(np.uint32), out.view(np.uint32))
    out9 = _predict(device, X, smp, H, Dy, 9)
    assert not np.array_equal(out9, out)
    mean5 = out.astype(np.float64) - B.predict_noise(smp, N, Dy, 5)[1]
    mean9 = out9.astype(np.float64) - B.predict_noise(smp, N, Dy, 9)[1]
    np.testing.assert_allclose(mean9, mean5, rtol=0, atol=1e-4)


def _predict_lds_bytes(N, Dx, H, Dy):
    """predictive.hip bnn_lds_bytes: the three weight blocks and two N x H layers."""
    return 4 * (Dx * H + H * H + H * Dy + 2 * N * H)


def test_lds_limit_of_the_predictive(device):
    """nmx_predict_bnn at H = 69, Dx = 3, D_Y = 1 needs 4 (5037 + 138 N) bytes of LDS: N = 260
    (163668) runs and matches the oracle at float32 level, N = 261 (164220) is refused with the
    byte count in the message, and the N = 260 launch after the refusal is bitwise its earlier
    self."""
    from numpyro_amd import native

    Dx, H, Dy = 3, 69, 1
    n_fit = max(n for n in range(1, 400) if _predict_lds_bytes(n, Dx, H, Dy) <= LDS_LIMIT)
    assert n_fit == 260 and _predict_lds_bytes(n_fit, Dx, H, Dy) == 163668
    X, smp = B.predict_case(n_fit, Dx, H, Dy, S=3)
    out = _predict(device, X, smp, H, Dy, 5)
    ref = _oracle_predict(X, smp, 5)
    np.testing.assert_allclose(out, ref, rtol=1e-4, atol=1e-4)
    B.check_predict_float32_level(out, B.predict_float32(X, smp, n_fit, Dy, 5), ref, label=f"N={n_fit} under the limit")
    Xb, smpb = B.predict_case(n_fit + 1, Dx, H, Dy, S=3)
    with pytest.raises(native.NativeError, match=rf"{_predict_lds_bytes(n_fit + 1, Dx, H, Dy)} B of LDS"):
        _predict(device, Xb, smpb, H, Dy, 5)
    np.testing.assert_array_equal(_predict(device, X, smp, H, Dy, 5).view(np.uint32), out.view(np.uint32))
