"""The op-level cases of tests/program_op_cases.py on the host: nmx_program_check accepts every
hand-assembled program, the float64 interpreter (Program.run_host) equals the independent torch
reference, and the float32 restatement of the interpreter stays within the tolerances the device
test applies (tests/test_gpu_program.py U_TOL / G_TOL), so the device test's bound is one that
float32 arithmetic can meet at these inputs.

The interpreter reads only the matrix M of a matvec's pool; the transposed copy behind it is read
by the kernel alone (per-lane forward, wave-per-row reverse).  Program therefore refuses, when it
is constructed, a pool whose halves are not transposes of each other, and the comparison of the
transposed copy's values with the reference is tests/test_gpu_program_ops.py's."""
import numpy as np
import pytest

import program_op_cases as OC
from numpyro_amd import native
from numpyro_amd.program import Program
from test_gpu_program import G_TOL, U_TOL


def test_the_forward_interpreter_knows_every_op():
    """One op per opcode name at n = 2 (a 2 x 2 matrix for the dense ops) through the one forward
    interpreter: an arithmetic op fills its slots, a draw op goes to the callback and is an error
    without one."""
    Z = np.array([[3.0, 0.5, 0.25, 1.5, 0.75, 1.25]])
    pool = [1.0, 2.0, 3.0, 4.0, 1.0, 3.0, 2.0, 4.0]  # a matvec's M, then its transpose
    layout = {"cholesky": (4, 0, 2), "trisolve": (2, 4, 0), "matvec": (2, ~0, 2), "logsumexp": (2, 0, 2),
              "concat": (2, 2, 1)}  # (n, b, aux) where they are not (2, z[2:4], 0)
    for name in native.OPCODES + native.LINALG_OPCODES + native.DRAW_OPCODES:
        n, b, aux = layout.get(name, (2, 2, 0))
        code = native.DRAW_OPCODE[name] if name in native.DRAW_OPCODE else native.OPCODE[name]
        p = Program([[code, 6, 0, b, n, 1, 1, aux]], pool, [1, 0], 10, 6)
        assert p.op_names() == [name]
        seen = []
        v = p._forward_host(Z, np.float64, p.consts64, lambda nm, op, v: seen.append((nm, op)))
        if name in native.DRAW_OPCODES:
            assert seen == [(name, p.ops[0].tolist())]
            with pytest.raises(AssertionError):
                p._forward_host(Z, np.float64, p.consts64)
        else:
            assert not seen and np.all(np.isfinite(v)) and np.any(v[0, 6:] != 0.0), (name, v)


@pytest.mark.parametrize("family", OC.FAMILIES)
def test_programs_pass_the_native_check(family):
    for c in OC.cases(family):
        st, msg = c.program.native_check()
        assert st == 0, (c.name, msg, c.program.describe())


def test_every_op_layout_and_size_is_a_case():
    names = {c.name for c in OC.cases("elementwise")}
    assert len(names) == len(OC.cases("elementwise"))
    for n in OC.WAVE_SIZES:
        for op in ("neg", "exp", "log", "sqrt", "tanh", "log1p", "square", "softplus", "lgamma"):
            assert {f"{op}.{k}.n{n}" for k in ("slot", "z3", "sslot", "zs")} <= names
        for op in ("add", "sub", "mul", "div", "pow"):
            assert {f"{op}.{k}.n{n}" for k in ("slot-slot", "z3-slot", "sslot-slot", "slot-sslot", "sslot-sslot",
                                               "slot-cvec", "slot-cscalar", "same1", "same0")} <= names
        for op in ("sub", "div", "pow"):
            assert {f"{op}.{k}.n{n}" for k in ("cvec-slot", "cscalar-slot")} <= names
    assert len(OC.cases("gather")) == len(OC.GATHER_SHAPES) * 6
    assert len(OC.cases("matvec")) == len(OC.MATVEC_SHAPES) * 3
    for family in OC.FAMILIES:
        for c in OC.cases(family):
            assert c.Z.shape == (OC.ROWS, c.dim)
            assert np.array_equal(c.Z, c.Z.astype(np.float32).astype(np.float64))
            assert np.array_equal(c.program.consts64, c.program.consts.astype(np.float64))


@pytest.mark.parametrize("family", OC.FAMILIES)
def test_interpreter_equals_the_torch_reference(family):
    worst = 0.0
    for c in OC.cases(family):
        U64, G64 = c.reference()
        assert np.all(np.isfinite(U64)) and np.all(np.isfinite(G64)), c.name
        U, G = c.program.run_host(c.Z)
        eU, eG = OC.scaled_errors(U, G, U64, G64)
        worst = max(worst, eU.max(), eG.max())
        assert eU.max() <= 1e-12 and eG.max() <= 1e-12, (c.name, eU.max(), eG.max())
    print(family, "largest scaled error of run_host against torch", worst)


@pytest.mark.parametrize("family", OC.FAMILIES)
def test_float32_restatement_is_within_the_device_tolerances(family):
    worst_u = worst_g = 0.0
    for c in OC.cases(family):
        U64, G64 = c.reference()
        U, G = OC.run_host_f32(c.program, c.Z)
        assert np.all(np.isfinite(U)) and np.all(np.isfinite(G)), c.name
        if family != "limits":  # |U| of the order of 100 (a broadcast lgamma(20) x 129 is the largest); exp(40) apart
            assert np.abs(U64).max() < 1e4, (c.name, np.abs(U64).max())
        eU, eG = OC.scaled_errors(U, G, U64, G64)
        worst_u, worst_g = max(worst_u, eU.max()), max(worst_g, eG.max())
        u_tol, g_tol = c.tolerances(U_TOL, G_TOL)
        np.testing.assert_allclose(U, U64, err_msg=c.name, **u_tol)
        np.testing.assert_allclose(G, G64, err_msg=c.name, **g_tol)
        if c.tanh_limit:
            assert np.all(G == 0.0), c.name
    print(family, "float32 restatement: largest scaled error of U", worst_u, "of the gradient", worst_g)


def test_one_op_over_overlapping_z_slices_is_refused():
    """z[0:n] with z[2:n+2], or z[3] broadcast with z[0:n], in one op: two lanes would update one
    adjoint inside one reverse op, which has no barrier.  nmx_program_check names the op; the same
    slices in two consecutive ops (family ``overlap``) and a == b pass."""
    for c in OC.overlapping_in_one_op():
        st, msg = c.program.native_check()
        assert st == 1 and msg.startswith("op 0 (mul)") and "overlap at different offsets" in msg, (c.name, st, msg)
    for c in OC.cases("overlap"):
        assert c.program.native_check() == (0, "")
    assert OC.case("elementwise", "mul.same1z.n65").program.native_check() == (0, "")


@pytest.mark.parametrize("shape", OC.PREDICTIVE_MATVEC_SHAPES)
def test_predictive_matvec_model_is_a_device_program(shape):
    """The model of the device test compiles to a program with the matvec as an op and eta as a
    device output (predictive_matvec asserts it), passes the native check, and its host run is
    X (b + e) of the e it drew."""
    import predictive_cases as PC

    n, K = shape
    model, X, b, prog = OC.predictive_matvec(n, K)
    assert prog.native_check()[0] == 0
    out = prog.run_host({"b": b}, 3, PC.words)
    ref = (b.astype(np.float64) + out["e"]) @ X.T
    assert out["eta"].shape == (OC.ROWS, n) and np.abs(out["eta"] - ref).max() <= 1e-12 * (1.0 + np.abs(ref).max())


def test_transposed_copy_is_out_of_the_interpreters_sight():
    """One element of the Mt half of a matvec's pool corrupted, M untouched.  The interpreters read
    M alone: run_host and the float32 emulation return the same bits, and nmx_program_check
    cannot know; the kernel's per-lane forward would read the corrupted element.  Program (and so
    PredictiveProgram) refuses such a pool when it is constructed, so a builder that wrote a
    wrong transposed copy fails on the host; that the device computes with the right Mt values
    is what the device comparison against torch shows (this shape runs the per-lane forward)."""
    c = OC.case("matvec", "z0.65x129")
    p = c.program
    row = next(o for o in p.ops.tolist() if o[0] == OC.OPCODE["matvec"])
    n, K, off = row[4], row[7], ~row[3]
    consts = p.consts64.copy()
    consts[off + n * K + 5 * n + 7] += 1.0  # Mt[5, 7]
    with pytest.raises(ValueError, match=r"op 0 \(matvec\).*not the transpose"):
        Program(p.ops, consts, p.index, p.num_slots, p.dim)
    # past the constructor's check: the same corruption in a copy's arrays
    bad = Program(p.ops, p.consts64, p.index, p.num_slots, p.dim)
    bad.consts64[off + n * K + 5 * n + 7] += 1.0
    bad.consts[off + n * K + 5 * n + 7] += 1.0
    assert not np.array_equal(bad.consts, p.consts) and np.array_equal(bad.consts[:off + n * K], p.consts[:off + n * K])
    assert bad.native_check()[0] == 0
    for run in (lambda q: q.run_host(c.Z), lambda q: OC.run_host_f32(q, c.Z)):
        (U, G), (Ub, Gb) = run(p), run(bad)
        assert np.array_equal(U, Ub) and np.array_equal(G, Gb)
