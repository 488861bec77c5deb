"""Hand-assembled programs for the program kernel's op-level tests (tests/test_program_ops.py on
the host interpreter, tests/test_gpu_program_ops.py on the device): every opcode of
csrc/nmx_program.h alone, at element counts around the 64 lanes and with every operand layout
nmx_program_check accepts, whether or not the compiler emits it.

A case is a ``Program`` written row by row ([opcode, dst, a, b, n, sa, sb, aux], a constant as
~offset, the pool of a matvec M then M.T), wrapped as ``ProgramPotential(prog, [("z", (D,), 0)])``,
with 16 rows of z and an independent float64 reference: the same function written as a torch
expression of Z, its gradient by autograd.  ``Program.run_host`` is never the reference.  Every
case ends in reduce_sum(w * f(...)) with w = linspace(0.5, 1.5, n): a value in the wrong lane or
an adjoint added to the wrong element changes the answer.  Constants are float32 numbers and z is
drawn as float32, so host and device see the same inputs.

Families (``cases(family)``):

elementwise  the 14 ops at n in WAVE_SIZES.  Operand layouts: ``slot`` a computed value at stride
             1; ``z3`` a z slice at offset 3; ``sslot`` a computed scalar broadcast (stride 0,
             read by every lane after a barrier, adjoint by a wave sum); ``zs`` z[3] broadcast;
             ``cvec`` / ``cscalar`` constants (as b, and as a for sub, div, pow); ``same1`` /
             ``same1z`` a == b at stride 1 (a slot, a z slice); ``same0`` a == b at stride 0.
limits       softplus at +-104, +-88, +-20, 0; tanh at +-20; log1p and exp at +-1e-6; square and
             exp at +-40.  Row r holds the points rotated by r.
overlap      two consecutive ops over z[0:n] and z[2:n+2] feeding one sum (the same adjoint slot
             updated by different lanes in consecutive reverse ops, with the barrier of touches_z
             between them).  One op with both slices is refused by nmx_program_check
             (``overlapping_in_one_op``).
reduce       reduce_sum at n in REDUCE_SIZES, of a computed vector and of a z slice at offset 3.
gather       result length n from a source of length b (GATHER_SHAPES); index patterns ``random``
             (repeats), ``zero`` (every element reads source 0: one long segment), ``even`` (half
             of the sources absent); the source a z slice at offset 3 or an op's result.
matvec       n x K (MATVEC_SHAPES) with the vector z[0:K], z[3:3+K] or tanh(z).  The kernel picks
             wave-per-row forward when n < 64 and K >= 64, wave-per-row reverse when K < 64 and
             n >= 64 (the two exclude each other), per-lane otherwise:
               (1,1) (63,63) (64,64)   per-lane forward, per-lane reverse, one element per lane
               (65,129)                per-lane both, more than one element per lane in both
               (3,64) (63,65)          wave-per-row forward (reads M), per-lane reverse
               (5,200)                 wave-per-row forward, 4 columns per lane; reverse per-lane, 4 per lane
               (64,63)                 per-lane forward (reads Mt), wave-per-row reverse (reads Mt)
               (130,3)                 per-lane forward, 3 rows per lane; wave-per-row reverse, 3 per lane
fanout       one value read by an elementwise op, a reduce_sum, a gather and a matvec at once; and
             two matvecs in a row (70 x 5 into 3 x 70: a wave-per-row reverse feeding a per-lane one).

``run_host_f32`` is the float32 NumPy restatement of ``Program.run_host`` (lgamma and digamma
torch's float32 ones): what float32 arithmetic alone costs against the float64 reference."""
import functools
import zlib

import numpy as np
import torch

from numpyro_amd import native
from numpyro_amd.native import OPCODE
from numpyro_amd.program import _BINARY, _HOST_FWD, _UNARY, Program, ProgramPotential, _host_rev

ROWS = 16
WAVE_SIZES = (1, 63, 64, 65, 129)
REDUCE_SIZES = (1, 2, 63, 64, 65, 129, 1000)
GATHER_SHAPES = ((1, 1), (63, 3), (64, 64), (65, 130), (129, 65), (300, 1))
MATVEC_SHAPES = ((1, 1), (3, 64), (63, 65), (5, 200), (63, 63), (64, 63), (130, 3), (64, 64), (65, 129))
FAMILIES = ("elementwise", "limits", "overlap", "reduce", "gather", "matvec", "fanout")

_TORCH = {
    "neg": torch.neg, "exp": torch.exp, "log": torch.log, "sqrt": torch.sqrt, "tanh": torch.tanh,
    "log1p": torch.log1p, "square": torch.square,
    "softplus": lambda x: torch.logaddexp(x, torch.zeros_like(x)),  # exact at every x, unlike F.softplus's cut
    "lgamma": torch.lgamma, "add": torch.add, "sub": torch.sub, "mul": torch.mul, "div": torch.div,
    "pow": torch.pow,
}

# input ranges (lo, hi, how): "u" uniform, "g" log-uniform, "s" uniform magnitude with a random sign
_POS = (0.05, 20.0, "g")
_UNARY_DOM = {"neg": (-2.0, 2.0, "u"), "exp": (-2.0, 2.0, "u"), "log": _POS, "sqrt": _POS, "tanh": (-2.0, 2.0, "u"),
              "log1p": (-0.9, 20.0, "u"), "square": (-2.0, 2.0, "u"), "softplus": (-4.0, 4.0, "u"), "lgamma": _POS}
_ANY = (-2.0, 2.0, "u")
_BINARY_DOM = {"add": (_ANY, _ANY), "sub": (_ANY, _ANY), "mul": (_ANY, _ANY), "div": (_ANY, (0.25, 3.0, "s")),
               "pow": ((0.1, 4.0, "g"), (-2.0, 3.0, "u"))}
# a == b: both ranges at once
_SAME_DOM = {"add": _ANY, "sub": _ANY, "mul": _ANY, "div": (0.25, 3.0, "s"), "pow": (0.1, 3.0, "g")}


def _draw(rs, dom, shape):
    lo, hi, how = dom
    if how == "g":
        return np.exp(rs.uniform(np.log(lo), np.log(hi), shape))
    x = rs.uniform(lo, hi, shape)
    return x * rs.choice([-1.0, 1.0], shape) if how == "s" else x


def weights(n):
    return np.linspace(0.5, 1.5, n).astype(np.float32).astype(np.float64)


class Val:
    """An operand or result: where it lives, its elements (1 if it is broadcast), its stride and
    its float64 form fn(Z [C, D]) -> [C, length]."""

    def __init__(self, ref, length, stride, fn):
        self.ref, self.length, self.stride, self.fn = ref, int(length), int(stride), fn

    def broadcast(self):
        assert self.length == 1
        return Val(self.ref, 1, 0, self.fn)


class Asm:
    """Assembles one program.  References stay symbolic (("z", offset), ("s", slot - dim),
    ("c", pool offset)) until ``case`` knows dim."""

    def __init__(self, name, family):
        self.name, self.family = name, family
        self.rs = np.random.RandomState(zlib.crc32(name.encode()))
        self.rows, self.consts, self.index = [], [], []
        self.nz = self.ns = self.nc = 0
        self.zcols = []  # per z allocation: values [ROWS, n]

    # ---- operands
    def z(self, n, dom, scale=1.0, stride=1, values=None):
        off = self.nz
        self.nz += n
        self.zcols.append(scale * _draw(self.rs, dom, (ROWS, n)) if values is None else np.asarray(values, np.float64))
        return Val(("z", off), n, stride, lambda Z: Z[:, off:off + n])

    def pad(self, k=3):
        """z coordinates nothing reads: their adjoint is zero."""
        self.z(k, _ANY)

    def const(self, values, stride=1):
        c = np.asarray(values, np.float64).reshape(-1).astype(np.float32).astype(np.float64)
        off = self.nc
        self.nc += c.size
        self.consts.append(c)
        t = torch.from_numpy(c.copy())[None, :]
        return Val(("c", off), c.size, stride, lambda Z: t)

    def slot(self, n, dom):
        """A computed value with the given range: 0.5 * z (exact in float32)."""
        return self.ew("mul", self.z(n, dom, scale=2.0), self.const([0.5], 0))

    # ---- ops
    def _emit(self, name, a, b, n, sa, sb, aux, length, fn):
        dst = ("s", self.ns)
        self.ns += length
        self.rows.append([OPCODE[name], dst, a, b, n, sa, sb, aux])
        return Val(dst, length, 1, fn)

    def ew(self, name, a, b=None, n=None):
        n = max(a.length, b.length if b is not None else 1) if n is None else n
        for v in (a, b):
            assert v is None or v.length == (n if v.stride else 1), (self.name, name)
        f = _TORCH[name]
        if b is None:
            fn = lambda Z: f(a.fn(Z)).expand(Z.shape[0], n)  # noqa: E731
        else:
            fn = lambda Z: f(a.fn(Z), b.fn(Z)).expand(Z.shape[0], n)  # noqa: E731
        return self._emit(name, a.ref, 0 if b is None else b.ref, n, a.stride, 0 if b is None else b.stride, 0, n, fn)

    def rsum(self, a):
        assert a.stride == 1
        return self._emit("reduce_sum", a.ref, 0, a.length, 1, 0, 0, 1, lambda Z: a.fn(Z).sum(1, keepdim=True))

    def gather(self, a, idx):
        """The index as _Builder.gather lays it out: idx, the CSR start, the stable-argsort who."""
        assert a.stride == 1
        idx = np.asarray(idx, np.int64).reshape(-1)
        who = np.argsort(idx, kind="stable")
        start = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=a.length))])
        aux = len(self.index)
        self.index += idx.tolist() + start.tolist() + who.tolist()
        sel = torch.from_numpy(idx)
        return self._emit("gather", a.ref, a.length, idx.size, 1, 0, aux, idx.size, lambda Z: a.fn(Z)[:, sel])

    def matvec(self, M, a):
        assert a.stride == 1 and M.shape[1] == a.length
        M = np.asarray(M, np.float64).astype(np.float32).astype(np.float64)
        pool = self.const(np.concatenate([M.reshape(-1), M.T.reshape(-1)]))
        Mt = torch.from_numpy(M.T.copy())
        return self._emit("matvec", a.ref, pool.ref, M.shape[0], 1, 0, M.shape[1], M.shape[0], lambda Z: a.fn(Z) @ Mt)

    # ---- the case
    def case(self, x, **kw):
        """Ends the program in reduce_sum(w * x)."""
        u = self.rsum(self.ew("mul", x, self.const(weights(x.length))))
        D = self.nz

        def res(ref):
            if not isinstance(ref, tuple):
                return ref
            kind, off = ref
            return off if kind == "z" else D + off if kind == "s" else ~off

        rows = [[r[0], res(r[1]), res(r[2]), res(r[3])] + r[4:] for r in self.rows]
        prog = Program(rows, np.concatenate(self.consts), self.index, D + self.ns, D)
        Z = np.concatenate(self.zcols, 1).astype(np.float32).astype(np.float64)
        return OpCase(self.name, self.family, prog, u.fn, Z, **kw)


class OpCase:
    def __init__(self, name, family, program, fn, Z, extra_rtol=0.0, tanh_limit=False):
        self.name, self.family, self.program, self.fn, self.Z = name, family, program, fn, Z
        self.dim = program.dim
        self.pot = ProgramPotential(program, [("z", (self.dim,), 0)])
        self.extra_rtol = extra_rtol  # the n = 1000 sum: atol += extra_rtol * max|U|
        self.tanh_limit = tanh_limit

    def reference(self, Z=None):
        """(U [C], dU/dz [C, D]) in float64 from the torch expression, gradient by autograd."""
        if Z is None:
            return self._reference
        Zt = torch.tensor(np.asarray(Z, np.float64), requires_grad=True)
        U = self.fn(Zt)[:, 0]
        (G,) = torch.autograd.grad(U.sum(), Zt)
        return U.detach().numpy().copy(), G.numpy().copy()

    @functools.cached_property
    def _reference(self):
        U, G = self.reference(self.Z)
        U.setflags(write=False)
        G.setflags(write=False)
        return U, G

    def tolerances(self, u_tol, g_tol):
        """The project's tolerances for this case (the large sum's extra as test_large_likelihood's)."""
        extra = self.extra_rtol * float(np.abs(self._reference[0]).max())
        return (dict(rtol=u_tol["rtol"], atol=u_tol["atol"] + extra),
                dict(rtol=g_tol["rtol"], atol=g_tol["atol"] + extra))


# ------------------------------------------------------------------------------------------ families
def _operand(A, kind, n, dom):
    if kind == "slot":
        return A.slot(n, dom)
    if kind == "z3":
        return A.z(n, dom)
    if kind == "sslot":
        return A.slot(1, dom).broadcast()
    if kind == "zs":
        return A.z(1, dom, stride=0)
    if kind == "cvec":
        return A.const(_draw(A.rs, dom, n))
    assert kind == "cscalar", kind
    return A.const(_draw(A.rs, dom, 1), 0)


_UNARY_LAYOUTS = ("slot", "z3", "sslot", "zs")
_BINARY_LAYOUTS = (("slot", "slot"), ("z3", "slot"), ("slot", "z3"), ("sslot", "slot"), ("slot", "sslot"),
                   ("sslot", "sslot"), ("zs", "slot"), ("slot", "cvec"), ("slot", "cscalar"), ("z3", "cscalar"))
_CONST_FIRST = (("cvec", "slot"), ("cscalar", "slot"), ("cscalar", "z3"))  # sub, div, pow
_SAME_LAYOUTS = ("same1", "same1z", "same0")


def _elementwise():
    out = []
    for n in WAVE_SIZES:
        for op in _UNARY:
            for kind in _UNARY_LAYOUTS:
                A = Asm(f"{op}.{kind}.n{n}", "elementwise")
                if kind in ("z3", "zs"):
                    A.pad()
                out.append(A.case(A.ew(op, _operand(A, kind, n, _UNARY_DOM[op]), n=n)))
        for op in _BINARY:
            layouts = _BINARY_LAYOUTS + (_CONST_FIRST if op in ("sub", "div", "pow") else ())
            for ka, kb in layouts:
                A = Asm(f"{op}.{ka}-{kb}.n{n}", "elementwise")
                da, db = _BINARY_DOM[op]
                # the z slice at offset 3 is allocated first, behind three coordinates nothing reads
                if "z3" in (ka, kb) or "zs" in (ka, kb):
                    A.pad()
                if kb in ("z3", "zs"):
                    b = _operand(A, kb, n, db)
                    a = _operand(A, ka, n, da)
                else:
                    a = _operand(A, ka, n, da)
                    b = _operand(A, kb, n, db)
                out.append(A.case(A.ew(op, a, b, n=n)))
            for kind in _SAME_LAYOUTS:
                A = Asm(f"{op}.{kind}.n{n}", "elementwise")
                if kind == "same1":
                    x = A.slot(n, _SAME_DOM[op])
                elif kind == "same1z":
                    A.pad()
                    x = A.z(n, _SAME_DOM[op])
                else:
                    x = A.slot(1, _SAME_DOM[op]).broadcast()
                out.append(A.case(A.ew(op, x, x, n=n)))
    return out


LIMIT_POINTS = (("softplus", (-104.0, -88.0, -20.0, 0.0, 20.0, 88.0, 104.0)), ("tanh", (-20.0, 20.0)),
                ("log1p", (-1e-6, 1e-6)), ("exp", (-1e-6, 1e-6)), ("square", (-40.0, 40.0)), ("exp", (-40.0, 40.0)))


def _limits():
    out = []
    for op, pts in LIMIT_POINTS:
        A = Asm(f"{op}.at{pts[-1]:g}", "limits")
        Z = np.stack([np.roll(np.asarray(pts), r) for r in range(ROWS)])
        out.append(A.case(A.ew(op, A.z(len(pts), None, values=Z)), tanh_limit=op == "tanh"))
    return out


def _overlap():
    out = []
    for n in (5, 70):
        # z[0:n] and z[2:n+2] as one allocation, referenced twice
        A = Asm(f"consecutive.n{n}", "overlap")
        A.z(n + 2, _ANY)
        lo = Val(("z", 0), n, 1, lambda Z, n=n: Z[:, 0:n])
        hi = Val(("z", 2), n, 1, lambda Z, n=n: Z[:, 2:n + 2])
        out.append(A.case(A.ew("add", A.ew("square", lo), A.ew("exp", hi))))
    return out


def overlapping_in_one_op():
    """Programs nmx_program_check must refuse (no family, never launched): one op whose two
    operands share z elements at different offsets, so that two lanes would update one adjoint
    inside one reverse op, which has no barrier.  Vector with vector, and a broadcast z[3] with a
    vector that contains it."""
    out = []
    for n in (5, 70):
        A = Asm(f"one_op.n{n}", "refused")
        A.z(n + 2, _ANY)
        out.append(A.case(A.ew("mul", Val(("z", 0), n, 1, lambda Z, n=n: Z[:, 0:n]),
                               Val(("z", 2), n, 1, lambda Z, n=n: Z[:, 2:n + 2]))))
        for first in (True, False):
            A = Asm(f"scalar_in_vector.n{n}.{'a' if first else 'b'}", "refused")
            A.z(n + 2, _ANY)
            s = Val(("z", 3), 1, 0, lambda Z: Z[:, 3:4])
            v = Val(("z", 0), n, 1, lambda Z, n=n: Z[:, 0:n])
            out.append(A.case(A.ew("mul", s, v, n=n) if first else A.ew("mul", v, s, n=n)))
    return out


def _reduce():
    out = []
    for n in REDUCE_SIZES:
        extra = 1e-6 if n == 1000 else 0.0
        A = Asm(f"slot.n{n}", "reduce")
        out.append(A.case(A.slot(n, _ANY), extra_rtol=extra))  # the case's own last op is the sum under test
        A = Asm(f"z3.n{n}", "reduce")
        A.pad()
        out.append(A.case(A.rsum(A.z(n, _ANY)), extra_rtol=extra))
    return out


def _gather():
    out = []
    for n, b in GATHER_SHAPES:
        for pattern in ("random", "zero", "even"):
            for source in ("z3", "op"):
                A = Asm(f"{pattern}.{source}.{n}from{b}", "gather")
                if pattern == "random":
                    idx = A.rs.randint(0, b, n)
                elif pattern == "zero":
                    idx = np.zeros(n, np.int64)
                else:
                    idx = 2 * A.rs.randint(0, (b + 1) // 2, n)
                if source == "z3":
                    A.pad()
                    src = A.z(b, _ANY)
                else:
                    src = A.ew("tanh", A.z(b, _ANY))
                out.append(A.case(A.gather(src, idx)))
    return out


def _matvec():
    out = []
    for n, K in MATVEC_SHAPES:
        for source in ("z0", "z3", "tanh"):
            A = Asm(f"{source}.{n}x{K}", "matvec")
            M = A.rs.randn(n, K) / np.sqrt(K)
            if source == "z3":
                A.pad()
            v = A.z(K, _ANY)
            out.append(A.case(A.matvec(M, A.ew("tanh", v) if source == "tanh" else v)))
    return out


def _fanout():
    out = []
    for n in (40, 70):  # one matvec branch each: 40 x 40 per-lane, 40 < 64; 70 x 70 per-lane with two elements per lane
        A = Asm(f"fanout.n{n}", "fanout")
        x = A.ew("tanh", A.z(n, _ANY))
        e = A.ew("mul", A.ew("square", x), A.rsum(x).broadcast())
        g = A.gather(x, A.rs.randint(0, n, n))
        m = A.matvec(A.rs.randn(n, n) / np.sqrt(n), x)
        out.append(A.case(A.ew("add", A.ew("add", e, g), m)))
    # two matvecs in a row, so that the adjoint of the first depends on z: 70 x 5 (per-lane forward,
    # wave-per-row reverse) feeding 3 x 70 (wave-per-row forward, per-lane reverse)
    A = Asm("two_layers", "fanout")
    h = A.ew("tanh", A.matvec(A.rs.randn(70, 5) / np.sqrt(5.0), A.z(5, _ANY)))
    out.append(A.case(A.ew("square", A.matvec(A.rs.randn(3, 70) / np.sqrt(70.0), h))))
    return out


_BUILD = {"elementwise": _elementwise, "limits": _limits, "overlap": _overlap, "reduce": _reduce, "gather": _gather,
          "matvec": _matvec, "fanout": _fanout}


@functools.lru_cache(maxsize=None)
def cases(family):
    return tuple(_BUILD[family]())


def case(family, name):
    return next(c for c in cases(family) if c.name == name)


PREDICTIVE_MATVEC_SHAPES = ((5, 200), (65, 129))  # wave-per-row forward, per-lane forward


def predictive_matvec(n, K):
    """(model, X [n, K], b [16, K] float32, its PredictiveProgram) of eta = X (b + e) with b given
    and e ~ Normal(0, 1) drawn.  A deterministic site of given sites alone is evaluated on the
    host and would never reach k_program_predict; eta depends on a draw, so it is a device output
    and its matvec an op of the program."""
    import numpyro_amd as numpyro
    from numpyro_amd import distributions as dist
    from numpyro_amd import jnp
    from numpyro_amd.predictive_program import compile_predictive

    rs = np.random.RandomState(n)
    X = (0.5 * rs.randn(n, K)).astype(np.float32).astype(np.float64)
    b = rs.randn(ROWS, K).astype(np.float32)

    def model(X):
        beta = numpyro.sample("b", dist.Normal(np.zeros(K), np.ones(K)))
        e = numpyro.sample("e", dist.Normal(np.zeros(K), np.ones(K)))
        numpyro.deterministic("eta", jnp.matmul(X, beta + e))

    prog = compile_predictive(model, (X,), {}, {"b"})
    rows = [o for o, nm in zip(prog.ops.tolist(), prog.op_names()) if nm == "matvec"]
    assert prog.num_ops > 0 and len(rows) == 1 and (rows[0][4], rows[0][7]) == (n, K), prog.describe()
    assert {o.name for o in prog.outputs} == {"e", "eta"} and not prog.host_deterministics
    return model, X, b, prog


def scaled_errors(U, G, U64, G64):
    """Per row: |U - U64| / max(1, |U64|) and max_d |G - G64| / max(1, max_d |G64|)."""
    eU = np.abs(U - U64) / np.maximum(1.0, np.abs(U64))
    eG = np.abs(G - G64).max(1) / np.maximum(1.0, np.abs(G64).max(1))
    return eU, eG


# ------------------------------------------------------------------------------------------ float32 emulation
def _lgamma32(x):
    return torch.lgamma(torch.from_numpy(np.ascontiguousarray(x, np.float32))).numpy()


def _digamma32(x):
    return torch.special.digamma(torch.from_numpy(np.ascontiguousarray(x, np.float32))).numpy()


def run_host_f32(program, Z):
    """Program.run_host restated in float32 NumPy: values, adjoints, constants and every
    operation in float32 (sums in NumPy's order)."""
    f4 = np.float32
    Z = np.atleast_2d(np.asarray(Z, f4))
    C, S, D = Z.shape[0], program.num_slots, program.dim
    assert Z.shape[1] == D
    cp, ix, names = program.consts, program.index, native.OPCODES
    v = np.zeros((C, S), f4)
    g = np.zeros((C, S), f4)
    v[:, :D] = Z

    def operand(ref, n, stride):
        ln = n if stride else 1
        return v[:, ref:ref + ln] if ref >= 0 else cp[None, ~ref:~ref + ln]

    def fwd(nm, x, y=None):
        if nm == "lgamma":
            return _lgamma32(x)
        r = _HOST_FWD[nm](x) if y is None else _HOST_FWD[nm](x, y)
        assert r.dtype == f4, (nm, r.dtype)
        return r

    def rev(nm, gd, x, y, out):
        if nm == "lgamma":
            return gd * _digamma32(x), None
        da, db = _host_rev(nm, gd, x, y, out)
        assert da.dtype == f4 and (db is None or db.dtype == f4), (nm, da.dtype)
        return da, db

    ops = program.ops.tolist()
    with np.errstate(all="ignore"):
        for op, dst, a, b, n, sa, sb, aux in ops:
            nm = names[op]
            if nm in _UNARY:
                v[:, dst:dst + n] = fwd(nm, operand(a, n, sa))
            elif nm in _BINARY:
                v[:, dst:dst + n] = fwd(nm, operand(a, n, sa), operand(b, n, sb))
            elif nm == "reduce_sum":
                v[:, dst] = v[:, a:a + n].sum(1)
            elif nm == "gather":
                v[:, dst:dst + n] = v[:, a + ix[aux:aux + n]]
            else:  # matvec
                M = cp[~b:~b + n * aux].reshape(n, aux)
                v[:, dst:dst + n] = v[:, a:a + aux] @ M.T
        g[:, S - 1] = 1.0
        for op, dst, a, b, n, sa, sb, aux in reversed(ops):
            nm = names[op]
            gd = g[:, dst:dst + (1 if nm == "reduce_sum" else n)]
            if nm in _UNARY or nm in _BINARY:
                x = operand(a, n, sa)
                y = operand(b, n, sb) if nm in _BINARY else None
                da, db = rev(nm, gd, x, y, v[:, dst:dst + n])
                for ref, stride, d in ((a, sa, da), (b, sb, db)):
                    if d is None or ref < 0:
                        continue
                    d = np.broadcast_to(d, (C, n))
                    if stride:
                        g[:, ref:ref + n] += d
                    else:
                        g[:, ref] += d.sum(1)
            elif nm == "reduce_sum":
                g[:, a:a + n] += gd
            elif nm == "gather":
                np.add.at(g, (slice(None), a + ix[aux:aux + n]), gd)
            else:
                M = cp[~b:~b + n * aux].reshape(n, aux)
                g[:, a:a + aux] += gd @ M
    return v[:, S - 1].astype(np.float64), g[:, :D].astype(np.float64)


