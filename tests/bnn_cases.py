"""Cases, references and the check of the BNN kernel tests (tests/test_bnn_cases.py on the CPU,
tests/test_gpu_bnn.py on the device; csrc/potential_bnn.hip k_bnn, k_bnn_c3 and the two
transposes, csrc/predictive.hip k_predict_bnn).

Model (examples/bnn.py:43-74): z = (log prec_obs, w1 [Dx, H], w2 [H, H], w3 [H, 1]) row-major,
weights ~ N(0, 1), prec_obs ~ Gamma(3, 1), Y ~ N(tanh(tanh(X w1) w2) w3, 1 / sqrt(prec_obs)).

Three references of U and dU on the same float32 inputs, all batched over the chains:
  * float64: oracle/batched.py BNNBatch(dtype=np.float64) before it rounds its result to float32
    (float64_reference) -- the truth the errors are taken from;
  * float32 restatement: BNNBatch(dtype=np.float32) -- the yardstick;
  * torch_restatement: U written from the model's log density in torch on the CPU and
    differentiated by autograd (nothing of the hand-derived adjoint), in float32 a second
    restatement, in float64 an independent derivation of the gradient.

The check (check_float32_level) is the rule of tests/test_gpu_program_ops.py and
tests/test_gpu_linalg_ops.py applied per site.  `restate` is a NumPy copy of BNNBatch's formulas
with switchable defects (CORRUPTIONS), from which tests/test_bnn_cases.py shows what the check
rejects."""
import functools

import numpy as np

from oracle.batched import BNNBatch

# (N, Dx, H): the smallest shape that reaches each edge of the generic kernel's 16 x 16 tiles, its
# K step of 4 and the 8 waves' round-robin; the register-blocked shape and its neighbours
SHAPES = [
    (1, 1, 1),      # one row, one unit, one input: every tile mask on
    (1, 3, 2),      # one row, partial tile
    (15, 2, 15),    # one short of a tile both ways; K = 15 is no multiple of 4
    (16, 3, 16),    # exact tiles; D = 321 is no multiple of the transposes' 64
    (17, 1, 17),    # one over: a second tile of one row and one column
    (33, 5, 3),     # H < 4 with Dx > 3
    (5, 3, 65),     # five column tiles, the last of one column; N < 16
    (48, 4, 33),    # 3 x 3 = 9 tiles: wave 0 takes a second one
    (100, 3, 69),   # k_bnn_c3
    (99, 3, 69), (100, 3, 68), (100, 2, 69),  # the generic kernel next to it
]
C3_SHAPE = (100, 3, 69)
C3_NEIGHBOURS = [(99, 3, 69), (100, 3, 68), (100, 2, 69)]

# regime -> (scale of the standard-normal weights, range of log prec)
REGIMES = {
    "unit": (0.5, (-1.0, 2.0)),        # typical values
    "saturated": (3.0, (-1.0, 2.0)),   # tanh near +-1, where 1 - h^2 cancels
    "far_u": (0.5, (-12.0, 6.0)),      # precision from 6e-6 to 400
}
SITES = ("prec_obs", "w1", "w2", "w3")
MARGIN = 4.0
FLOOR = 16 * 2.0 ** -24


def dim_of(N, Dx, H):
    return 1 + Dx * H + H * H + H


def site_slices(dims):
    """{site: slice of z} for dims = (N, Dx, H)."""
    _, Dx, H = dims
    o1, o2, o3 = 1, 1 + Dx * H, 1 + Dx * H + H * H
    return {"prec_obs": slice(0, 1), "w1": slice(o1, o2), "w2": slice(o2, o3), "w3": slice(o3, o3 + H)}


def shape_seed(N, Dx, H):
    return 1000003 * N + 1009 * Dx + H


def data(N, Dx, H):
    """X [N, Dx] standard normal, Y = sin(2 X[:, 0]) + 0.3 noise, float32; seeded by the shape."""
    rs = np.random.RandomState(shape_seed(N, Dx, H) % (2 ** 31))
    X = rs.randn(N, Dx).astype(np.float32)
    Y = (np.sin(2.0 * X[:, 0]) + 0.3 * rs.randn(N)).astype(np.float32)
    return X, Y


def positions(N, Dx, H, C, regime):
    """Z [C, D] float32 of a regime; seeded by the shape and the regime, the first rows of a larger
    batch are not those of a smaller one (every batch has its own references)."""
    s, (lo, hi) = REGIMES[regime]
    rs = np.random.RandomState((shape_seed(N, Dx, H) * 7 + 131 * sorted(REGIMES).index(regime) + C) % (2 ** 31))
    Z = (s * rs.randn(C, dim_of(N, Dx, H))).astype(np.float32)
    Z[:, 0] = rs.uniform(lo, hi, C)
    return Z


def _f64(out):
    return tuple(np.asarray(v, np.float64) for v in out)


def torch_restatement(X, Y, H, Z, dtype):
    """(U [C], dU [C, D]) in float64 arrays: the model's negative log density plus the
    log-Jacobian of prec = exp(u), summed over the chains and differentiated by autograd, in
    torch on the CPU at `dtype`.  Written from the density, not from BNNBatch."""
    import math

    import torch

    X = torch.tensor(np.asarray(X), dtype=dtype)
    Y = torch.tensor(np.asarray(Y), dtype=dtype).reshape(-1)
    z = torch.tensor(np.asarray(Z), dtype=dtype).requires_grad_(True)
    (N, Dx), C = X.shape, z.shape[0]
    u = z[:, 0]
    w1 = z[:, 1:1 + Dx * H].reshape(C, Dx, H)
    w2 = z[:, 1 + Dx * H:1 + Dx * H + H * H].reshape(C, H, H)
    w3 = z[:, 1 + Dx * H + H * H:].reshape(C, H, 1)
    prec = torch.exp(u)
    log_2pi = math.log(2.0 * math.pi)
    # weights ~ Normal(0, 1)
    lp = sum((-0.5 * w * w - 0.5 * log_2pi).reshape(C, -1).sum(1) for w in (w1, w2, w3))
    # prec_obs ~ Gamma(3, 1): 2 log prec - prec - lgamma(3), log prec = u; log |d prec / du| = u
    lp = lp + (2.0 * u - prec - math.lgamma(3.0)) + u
    # Y ~ Normal(yhat, prec^-1/2): -0.5 prec (Y - yhat)^2 + 0.5 u - 0.5 log 2 pi per row
    yhat = torch.tanh(torch.tanh(X @ w1) @ w2) @ w3
    r = Y[None, :] - yhat[:, :, 0]
    lp = lp + (-0.5 * prec[:, None] * r * r + 0.5 * u[:, None] - 0.5 * log_2pi).sum(1)
    U = -lp
    (G,) = torch.autograd.grad(U.sum(), z)
    return U.detach().numpy().astype(np.float64), G.numpy().astype(np.float64)


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def reference(N, Dx, H, C, regime):
    """(X, Y, Z, f64, f32, t32): the case and (U, dU) of BNNBatch(float64), BNNBatch(float32) and
    the torch float32 restatement, as float64 arrays.  Computed once, shared, read-only."""
    import torch

    X, Y = data(N, Dx, H)
    Z = positions(N, Dx, H, C, regime)
    f64 = _f64(float64_reference(X, Y, H, Z))
    f32 = _f64(BNNBatch(X, Y, H, dtype=np.float32)(Z))
    t32 = torch_restatement(X, Y, H, Z, torch.float32)
    _ro(X, Y, Z, *f64, *f32, *t32)
    return X, Y, Z, f64, f32, t32


def float64_reference(X, Y, H, Z):
    """BNNBatch(dtype=np.float64) before its last step: BNNBatch rounds what it returns to
    float32, which would put 2^-24 under every error taken against it and make the 1e-12
    agreement with autograd unobservable.  `restate` holds the same formulas and leaves the
    result in float64; test_bnn_cases checks that rounding it gives BNNBatch(float64)'s output
    bit for bit."""
    return restate(X, Y, H, Z, np.float64)


# ------------------------------------------------------------------------------ the restatement
# Defects a subtly wrong kernel could have, each a term of the evaluation at a tile or row edge
CORRUPTIONS = (
    "gw2_tile_misses_last_k",   # grad W2 without its k = N-1 term inside one 16 x 16 output tile
    "h2_w2_last_row_zero",      # h2 from W2 with row H-1 read as zero
    "ga1_last_row_clamped",     # row N-1 of ga1 taken from row N-2 (needs N >= 2)
    "g0_esq_short",             # g[0] from esq summed over N-1 rows
    "gw2_one_element_1e-4",     # one element of grad W2 off by 1e-4 of itself
)


def corruption_applies(name, dims):
    return dims[0] >= 2 if name == "ga1_last_row_clamped" else True


def restate(X, Y, H, Z, dtype, corrupt=None):
    """BNNBatch's formulas (oracle/batched.py; bitwise its results in float32, test_bnn_cases
    checks it) with one of CORRUPTIONS switched on; results at `dtype`, not rounded."""
    from scipy.special import gammaln

    F = dtype
    X, Y, Z = np.asarray(X, F), np.asarray(Y, F).reshape(-1), np.asarray(Z, F)
    (N, Dx), B = X.shape, Z.shape[0]
    dim = dim_of(N, Dx, H)
    log_2pi = float(np.log(2.0 * np.pi))
    u = Z[:, 0]
    w1 = Z[:, 1:1 + Dx * H].reshape(B, Dx, H)
    w2 = Z[:, 1 + Dx * H:1 + Dx * H + H * H].reshape(B, H, H)
    w3 = Z[:, 1 + Dx * H + H * H:].reshape(B, H, 1)
    p = np.exp(u)
    h1 = np.tanh(np.matmul(X[None], w1))
    if corrupt == "h2_w2_last_row_zero":
        h2 = np.tanh(np.matmul(h1[:, :, :H - 1], w2[:, :H - 1, :]))
    else:
        h2 = np.tanh(np.matmul(h1, w2))
    yhat = np.matmul(h2, w3)[:, :, 0]
    e = Y[None, :] - yhat
    ee = np.einsum("bn,bn->b", e, e)
    ww = np.einsum("bd,bd->b", Z[:, 1:], Z[:, 1:])
    lp = -F(0.5) * ww - F(0.5 * (dim - 1) * log_2pi)
    lp = lp + F(2) * u - p - F(gammaln(3.0)) + u
    lp = lp - F(0.5) * p * ee + F(0.5 * N) * u - F(0.5 * N * log_2pi)
    g_y = (-p[:, None] * e)[:, :, None]
    gw3 = w3 + np.matmul(h2.transpose(0, 2, 1), g_y)
    ga2 = np.matmul(g_y, w3.transpose(0, 2, 1)) * (F(1) - h2 * h2)
    gw2 = w2 + np.matmul(h1.transpose(0, 2, 1), ga2)
    if corrupt == "gw2_tile_misses_last_k":
        t = slice(0, min(16, H))  # the first output tile: full wherever H >= 16
        gw2[:, t, t] = w2[:, t, t] + np.matmul(h1[:, :N - 1, t].transpose(0, 2, 1), ga2[:, :N - 1, t])
    ga1 = np.matmul(ga2, w2.transpose(0, 2, 1)) * (F(1) - h1 * h1)
    if corrupt == "ga1_last_row_clamped":
        ga1[:, N - 1] = ga1[:, N - 2]
    gw1 = w1 + np.matmul(X.T[None], ga1)
    gu = -(F(3) - p + F(0.5 * N) - F(0.5) * p * ee)
    if corrupt == "g0_esq_short":
        gu = -(F(3) - p + F(0.5 * N) - F(0.5) * p * np.einsum("bn,bn->b", e[:, :N - 1], e[:, :N - 1]))
    G = np.concatenate([gu[:, None], gw1.reshape(B, -1), gw2.reshape(B, -1), gw3.reshape(B, -1)], axis=1)
    if corrupt == "gw2_one_element_1e-4":
        blk = G[:, 1 + Dx * H:1 + Dx * H + H * H]  # the largest element of the block, in its chain
        b, k = np.unravel_index(np.argmax(np.abs(blk)), blk.shape)
        blk[b, k] = blk[b, k] * F(1.0 + 1e-4)
    assert corrupt is None or corrupt in CORRUPTIONS, corrupt
    return -lp, G


# ------------------------------------------------------------------------------------ the check
def site_errors(got, f64, dims):
    """{quantity: per-chain scaled error [C]} of (U, dU) against float64: |dU| / max(1, |U64|)
    and, per site, max |dg_site| / max(1, max |g64_site|); inf where `got` is not finite."""
    (U, G), (U64, G64) = _f64(got), _f64(f64)
    assert U.shape == U64.shape and G.shape == G64.shape and G.shape[1] == dim_of(*dims), (U.shape, G.shape, dims)
    with np.errstate(invalid="ignore"):
        out = {"U": np.where(np.isfinite(U), np.abs(U - U64) / np.maximum(1.0, np.abs(U64)), np.inf)}
        for site, sl in site_slices(dims).items():
            err = np.abs(G[:, sl] - G64[:, sl]).max(1) / np.maximum(1.0, np.abs(G64[:, sl]).max(1))
            out[site] = np.where(np.isfinite(G[:, sl]).all(1), err, np.inf)
    return out


def float32_level(got, f32, f64, dims):
    """{quantity: (error, yardstick error, bound)}, each the maximum over the batch; the bound is
    MARGIN x the float32 restatement's error on the same rows + FLOOR.  No row is excluded."""
    assert np.all(np.isfinite(f64[0])) and np.all(np.isfinite(f64[1]))
    assert np.all(np.isfinite(f32[0])) and np.all(np.isfinite(f32[1]))
    e, r = site_errors(got, f64, dims), site_errors(f32, f64, dims)
    return {q: (float(e[q].max()), float(r[q].max()), MARGIN * float(r[q].max()) + FLOOR) for q in e}


def ratios_of(level):
    """error / max(yardstick error, 2^-24) per quantity: the figure docs/DESIGN_LOG.md tabulates."""
    return {q: e / max(r, 2.0 ** -24) for q, (e, r, _) in level.items()}


def check_float32_level(got, f32, f64, dims, label="", log=print):
    """Every quantity of `got` -- U and the gradient blocks of prec_obs, w1, w2, w3 -- within
    MARGIN x the float32 restatement's scaled error against float64 + 16 x 2^-24, each taken as
    the maximum over all chains.  The yardstick is a reference, never the thing under test.
    Prints the measured ratios and returns them."""
    level = float32_level(got, f32, f64, dims)
    ratios = ratios_of(level)
    log(f"[bnn f32 level] {label} {dims}: " + "  ".join(
        f"{q} {e:.2e} (f32 {r:.2e}, x{ratios[q]:.2f})" for q, (e, r, _) in level.items()))
    bad = {q: v for q, v in level.items() if not v[0] <= v[2]}
    assert not bad, f"{label} {dims}: " + "; ".join(
        f"{q} error {e:.3e} > bound {b:.3e} (float32 restatement {r:.3e})" for q, (e, r, b) in bad.items())
    return ratios


def existing_tolerance_accepts(got, f64):
    """Per chain [C]: whether tests/test_gpu_potentials.py test_bnn_matches_oracle's assertions
    hold on it -- U to rtol 1e-4 + 1e-2, gradient to rtol 1e-3 + 1e-3 max |g| over the whole
    chain (that test asserts chain by chain)."""
    (U, G), (U64, G64) = _f64(got), _f64(f64)
    ok_u = np.abs(U - U64) <= 1e-2 + 1e-4 * np.abs(U64)
    ok_g = np.abs(G - G64) <= 1e-3 * np.abs(G64).max(1, keepdims=True) + 1e-3 * np.abs(G64)
    return ok_u & ok_g.all(1)


# ------------------------------------------------------------------------------- the predictive
# (N, Dx, H, Dy) of k_predict_bnn
PREDICT_SHAPES = [(1, 1, 1, 1), (17, 2, 17, 3), (5, 3, 65, 2), (100, 3, 69, 1)]
PREDICT_S = 16


def predict_case(N, Dx, H, Dy, S=PREDICT_S):
    """X [N, Dx] and S posterior samples {prec_obs [S], w1 [S, Dx, H], w2 [S, H, H], w3 [S, H, Dy]},
    float32, seeded by the shape (the first 16 of a longer set are the set of 16)."""
    rs = np.random.RandomState((shape_seed(N, Dx, H) + 17 * Dy) % (2 ** 31))
    X = rs.randn(N, Dx).astype(np.float32)
    smp = {"prec_obs": np.empty(S, np.float32), "w1": np.empty((S, Dx, H), np.float32),
           "w2": np.empty((S, H, H), np.float32), "w3": np.empty((S, H, Dy), np.float32)}
    for s in range(S):  # sample by sample, so a longer set extends a shorter one
        smp["prec_obs"][s] = rs.gamma(3.0, 1.0)
        smp["w1"][s] = rs.randn(Dx, H)
        smp["w2"][s] = rs.randn(H, H) / np.sqrt(H)
        smp["w3"][s] = rs.randn(H, Dy)
    return X, smp


def predict_noise(smp, N, Dy, seed):
    """The oracle's z / sqrt(prec) [S, N, Dy] (float64) of oracle.predictive.predict_bnn."""
    from oracle import philox
    from oracle.predictive import _words

    S = len(smp["prec_obs"])
    w = _words(seed, S, N * Dy)
    z, _ = philox.box_muller(w[..., 0], w[..., 1])
    z = z.astype(np.float64).reshape(S, N, Dy)
    return z, z / np.sqrt(smp["prec_obs"].astype(np.float64))[:, None, None]


def predict_float32(X, smp, N, Dy, seed):
    """The float32 restatement of a predictive draw: the forward pass in float32 (NumPy) plus the
    oracle's own normal variates times a float32 1 / sqrt(prec)."""
    F = np.float32
    z, _ = predict_noise(smp, N, Dy, seed)
    mean = np.matmul(np.tanh(np.matmul(np.tanh(np.matmul(X[None].astype(F), smp["w1"])), smp["w2"])), smp["w3"])
    sigma = (F(1) / np.sqrt(smp["prec_obs"].astype(F)))[:, None, None]
    return (mean + sigma * z.astype(F)).astype(np.float64)


def check_predict_float32_level(got, f32, f64, label="", log=print):
    """|d| / max(1, |ref|) of a predictive draw, its maximum within MARGIN x the float32
    restatement's + 16 x 2^-24."""
    got, f32, f64 = (np.asarray(v, np.float64) for v in (got, f32, f64))
    assert got.shape == f64.shape and np.all(np.isfinite(got)), label
    e = (np.abs(got - f64) / np.maximum(1.0, np.abs(f64))).max()
    r = (np.abs(f32 - f64) / np.maximum(1.0, np.abs(f64))).max()
    log(f"[bnn predictive] {label}: error {e:.2e} (f32 {r:.2e}, x{e / max(r, 2.0 ** -24):.2f})")
    assert e <= MARGIN * r + FLOOR, f"{label}: error {e:.3e} > bound {MARGIN * r + FLOOR:.3e} (float32 {r:.3e})"
    return e / max(r, 2.0 ** -24)
