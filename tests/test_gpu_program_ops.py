"""The program kernel (csrc/nmx_program.h through nmx_pe_program and nmx_predict_program) op by
op: the hand-assembled cases of tests/program_op_cases.py against their independent float64
torch references, the workspace's stale contents, bitwise repeatability, a matvec of a drawn
site through the predictive kernel, and the compiled zoo far from the mode.

Tolerances are the project's (tests/test_gpu_program.py U_TOL / G_TOL), with test_large_likelihood's
1e-6 max|U| for the 1000-element sum.  The wide-range bound of a (case, R) is measured on the
same rows: 4 x the scaled error of the float32 NumPy restatement of the interpreter
(program_op_cases.run_host_f32) plus 16 x 2^-24; the factor covers the device's expf / logf /
lgammaf being a couple of ulp looser than NumPy's and the other order inside sums."""
import functools

import numpy as np
import pytest
import torch

import bounded_zoo as BZ
import predictive_cases as PC
import program_op_cases as OC
import program_zoo as Zoo
from numpyro_amd import native
from numpyro_amd.infer import Predictive
from numpyro_amd.program import compile_model
from test_gpu_program import G_TOL, U_TOL, _launch

pytestmark = pytest.mark.gpu


def _share(x, ref, rtol, atol):
    """The largest error as a share of its tolerance (assert_allclose's rule): passes when <= 1."""
    return float(np.max(np.abs(x - ref) / (atol + rtol * np.abs(ref))))


# ------------------------------------------------------------------ 1: every case against torch
@pytest.mark.parametrize("family", OC.FAMILIES)
def test_cases_match_the_float64_reference(device, family):
    """Every case of the family, then one assertion naming the cases that miss."""
    bad, worst_u, worst_g, share, at = [], 0.0, 0.0, 0.0, ""
    for c in OC.cases(family):
        U64, G64 = c.reference()
        pe, g = _launch(c.pot, c.Z, device)
        eU, eG = OC.scaled_errors(pe, g, U64, G64)
        u_tol, g_tol = c.tolerances(U_TOL, G_TOL)
        ok = bool(np.all(np.isfinite(pe)) and np.all(np.isfinite(g)))
        s = max(_share(pe, U64, **u_tol), _share(g, G64, **g_tol)) if ok else np.inf
        ok = ok and s <= 1.0
        if c.tanh_limit:  # 1 - tanh(+-20)^2 in float32
            ok = ok and bool(np.all(g == 0.0))
        if not ok:
            bad.append(f"{c.name}: scaled error of U {np.nanmax(eU):.3e}, of the gradient {np.nanmax(eG):.3e}, "
                       f"max |dU| {np.nanmax(np.abs(pe - U64)):.3e}, max |dG| {np.nanmax(np.abs(g - G64)):.3e}")
        else:
            worst_u, worst_g = max(worst_u, eU.max()), max(worst_g, eG.max())
            share, at = max((share, at), (s, c.name))
    print(f"{family}: {len(OC.cases(family))} cases, largest scaled error of U {worst_u:.3e}, of the gradient "
          f"{worst_g:.3e}, largest share of a tolerance {share:.3f} at {at}")
    assert not bad, f"{len(bad)} of {len(OC.cases(family))} cases:\n" + "\n".join(bad[:40])


# ------------------------------------------------------------------ 2: the workspace
_ONE_OF_EACH = (("elementwise", "pow.sslot-slot.n129"), ("limits", "softplus.at104"), ("overlap", "consecutive.n70"),
                ("reduce", "slot.n1000"), ("gather", "even.op.65from130"), ("matvec", "tanh.5x200"),
                ("fanout", "fanout.n70"))


def _evaluate_bound(pot, Z, device):
    """_launch's evaluation on the potential as it is bound (16 chains, ldc 64): its workspace is kept."""
    C, D, ldc = Z.shape[0], Z.shape[1], pot.ldc
    z = torch.zeros(D, ldc, device=device)
    z[:, :C] = torch.from_numpy(np.ascontiguousarray(Z.T.astype(np.float32))).to(device)
    g = torch.full((D, ldc), float("nan"), device=device)
    pe = torch.full((ldc,), float("nan"), device=device)
    ev = native.EvalBatch(z=native.ptr(z), grad=native.ptr(g), pe=native.ptr(pe), num_chains=C, ldc=ldc)
    pot.evaluate(ev, native.stream_ptr())
    torch.cuda.synchronize()
    return pe[:C].cpu().numpy().astype(np.float64), g[:, :C].cpu().numpy().T.astype(np.float64)


@pytest.mark.parametrize("family,name", _ONE_OF_EACH)
def test_nothing_leaks_from_the_workspace(device, family, name):
    """The workspace is torch.empty and the kernel zeroes its adjoint half alone: with every byte
    0xff (NaN) before the launch, and after a launch on other rows, the results are bitwise those
    of a zeroed workspace."""
    c = OC.case(family, name)
    other = c.Z[::-1] * 0.75 if family != "limits" else c.Z[::-1]
    c.pot.bind(OC.ROWS, 64, device)
    c.pot.workspace.zero_()
    clean = _evaluate_bound(c.pot, c.Z, device)
    assert np.all(np.isfinite(clean[0])) and np.all(np.isfinite(clean[1]))
    c.pot.workspace.fill_(0xFF)
    assert bool(torch.isnan(c.pot.workspace.view(torch.float32)).all())
    poisoned = _evaluate_bound(c.pot, c.Z, device)
    moved = _evaluate_bound(c.pot, other, device)
    again = _evaluate_bound(c.pot, c.Z, device)
    assert family == "limits" or not np.array_equal(moved[0], clean[0])
    for got in (poisoned, again):
        np.testing.assert_array_equal(got[0], clean[0])
        np.testing.assert_array_equal(got[1], clean[1])


# ------------------------------------------------------------------ 3: determinism
@pytest.mark.parametrize("family,name", [("reduce", "slot.n1000"), ("matvec", "z0.65x129")])
def test_two_launches_are_bitwise_equal(device, family, name):
    c = OC.case(family, name)
    one, two = _launch(c.pot, c.Z, device), _launch(c.pot, c.Z, device)
    np.testing.assert_array_equal(one[0], two[0])
    np.testing.assert_array_equal(one[1], two[1])


# ------------------------------------------------------------------ 4: the predictive kernel's forward
@pytest.mark.parametrize("shape", OC.PREDICTIVE_MATVEC_SHAPES, ids=["wave_per_row", "per_lane"])
def test_predictive_kernel_matvec(device, shape):
    """k_program_predict shares NmxProgram::forward: eta = X (b + e), b given and e drawn on the
    device, so that eta is an output of the kernel (a deterministic site of given sites alone is
    evaluated on the host; program_op_cases.predictive_matvec asserts that the program has the
    matvec op).  Against float64 X (b + e) of the e the device returned (the float32 sum b + e is
    exact to its rounding), by predictive_cases.compare's rule for a site without an accept /
    reject decision of its own; e itself against the float64 host interpreter by the same rule."""
    n, K = shape
    model, X, b, prog = OC.predictive_matvec(n, K)
    out = Predictive(model, {"b": torch.from_numpy(b)})(3, X)
    assert set(out) == {"e", "eta"} and out["eta"].shape == (OC.ROWS, n) and out["eta"].dtype == torch.float32
    e = out["e"].cpu().numpy()
    assert e.shape == (OC.ROWS, K) and e.dtype == np.float32 and e.std() > 0.5
    host = prog.run_host({"b": b}, 3, PC.words)
    PC.compare(f"e {n}x{K}", "monotone", e, host["e"], None, None)
    ref = (b + e).astype(np.float64) @ X.T
    PC.compare(f"eta {n}x{K}", "monotone", out["eta"].cpu().numpy(), ref, None, None)


# ------------------------------------------------------------------ 5: far from the mode
_ZOOS = {"zoo": Zoo.CASES, "bounded": BZ.CASES}
_WIDE = [(z, name) for z in sorted(_ZOOS) for name in sorted(_ZOOS[z])]


@functools.lru_cache(maxsize=None)
def _wide(zoo, name, R):
    case = _ZOOS[zoo][name]()
    pot = compile_model(case.model, case.args)
    Z = np.random.RandomState(31).uniform(-R, R, (200, case.dim)).astype(np.float32).astype(np.float64)
    U64, G64 = case.pe_grad64(Z)
    U32, G32 = OC.run_host_f32(pot.program, Z)
    return pot, Z, (U64, G64), (U32, G32)


@pytest.mark.parametrize("R", [8, 16])
@pytest.mark.parametrize("zoo,name", _WIDE)
def test_wide_range_stays_at_float32_level(device, zoo, name, R):
    """Z ~ U(-R, R), 200 rows, none excluded: reference and kernel finite on every row, and the
    kernel's scaled errors within 4 x the float32 restatement's + 16 x 2^-24."""
    pot, Z, (U64, G64), (U32, G32) = _wide(zoo, name, R)
    assert np.all(np.isfinite(U64)) and np.all(np.isfinite(G64))
    assert np.all(np.isfinite(U32)) and np.all(np.isfinite(G32))
    pe, g = _launch(pot, Z, device)
    assert np.all(np.isfinite(pe)) and np.all(np.isfinite(g)), (int((~np.isfinite(pe)).sum()), "rows not finite")
    eU32, eG32 = OC.scaled_errors(U32, G32, U64, G64)
    eU, eG = OC.scaled_errors(pe, g, U64, G64)
    bU, bG = 4.0 * eU32.max() + 16 * 2.0 ** -24, 4.0 * eG32.max() + 16 * 2.0 ** -24
    print(f"wide {zoo}.{name} R={R}: U device {eU.max():.3e} float32 {eU32.max():.3e} bound {bU:.3e} ratio "
          f"{eU.max() / eU32.max():.2f}; gradient device {eG.max():.3e} float32 {eG32.max():.3e} bound {bG:.3e} "
          f"ratio {eG.max() / eG32.max():.2f}")
    assert eU.max() <= bU, (eU.max(), bU)
    assert eG.max() <= bG, (eG.max(), bG)
