"""Log-likelihood programs: the elementwise log density of every observed site, for the generic
path of the model front end.

The reference's ``log_likelihood`` re-runs the model once per posterior sample with the latent
sites substituted and reads ``site["fn"].log_prob(site["value"])`` of every observed site
(numpyro/infer/util.py:1094-1170).  ``compile_log_likelihood`` traces the model once
(frontend.trace_model) and lowers that run to a straight-line, draw-free program of the program
compiler's format (numpyro_amd/program.py, the same builder and ``_LOGPROB`` expansions: folding,
sharing and refusals are the same) whose inputs are the given sites' constrained values, as a
predictive program's (predictive_program.py), and whose outputs are one value per observed site:
its ``log_prob`` *before* any sum over the site, constants included.  One HIP kernel
(csrc/loglik_program.hip k_program_loglik) runs the program once per posterior sample and packs
the outputs into a dense [S, columns] table; the reduce kernels of the same file turn such a
table into the pointwise lppd and p_waic without holding it whole.

``LogLikProgram.run_host`` is a NumPy interpreter of the same program (float64; float32 runs the
same arithmetic in float32, the calibration of the device tests).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import distributions as dist
from . import native
from .frontend import _base, _host, trace_model
from .predictive_program import _lgamma
from .program import (_BINARY, _BINOMIAL, _ELEMENTWISE, _HOST_FWD, _LINALG, _LOGPROB, _SCAN, _UNARY, Program, _Builder,
                      _Lowering, _Refuse, _ew_mixture, _host_linalg_fwd, _host_scan_fwd, _lp_mvn, _refuse, _V)


class LogLikOutput:
    """An observed site's log density: ``n`` tape slots from ``slot``, columns [column, column + n)
    of the dense table, of the site's batch ``shape`` (n = 1 under a wider shape: every element has
    the same value and the host expands it)."""

    def __init__(self, name, slot, n, shape, column):
        self.name, self.slot, self.n, self.shape, self.column = name, int(slot), int(n), tuple(shape), int(column)

    def __iter__(self):  # (name, slot, n, shape, column)
        return iter((self.name, self.slot, self.n, self.shape, self.column))

    def __repr__(self):
        return (f"{self.name}: slots [{self.slot}, {self.slot + self.n}) -> columns [{self.column}, "
                f"{self.column + self.n}) shape {self.shape}")


class LogLikProgram(Program):
    """A forward-only program without draws: slots [0, dim) hold the given sites (``inputs``:
    (name, offset, n, shape) in sorted name order, constrained values); ``outputs`` are the
    observed sites whose log density depends on a given site, ``constant_outputs`` (name ->
    float64 array of the site's shape) those that are host constants.  ``num_columns`` is the width
    of the dense table."""

    def __init__(self, ops, consts, index, num_slots, dim, inputs, outputs, constant_outputs):
        super().__init__(ops, consts, index, num_slots, dim)
        self.inputs, self.outputs = list(inputs), list(outputs)
        self.constant_outputs = dict(constant_outputs)
        self.num_columns = sum(o.n for o in self.outputs)

    def output_table(self):
        """int32 [num_outputs, 3]: { slot, n, column }."""
        return np.ascontiguousarray(np.asarray([[o.slot, o.n, o.column] for o in self.outputs],
                                               np.int32).reshape(-1, 3))

    def native_check(self, outputs=None, ldo=None):
        """(status, message) of nmx_loglik_program_check on the host arrays: needs no GPU."""
        lib = native.lib()
        table = self.output_table() if outputs is None else np.ascontiguousarray(np.asarray(outputs, np.int32))
        st = lib.nmx_loglik_program_check(ctypes.byref(self.native_struct()),
                                          int(table.ctypes.data) if table.size else None, table.shape[0],
                                          self.num_columns if ldo is None else int(ldo))
        return st, (lib.nmx_last_error().decode(errors="replace") if st else "")

    def op_names(self):
        return [native.op_name(o) for o in self.ops[:, 0].tolist()]

    def describe(self):
        return [f"{k}: {nm} dst={o[1]} a={o[2]} b={o[3]} n={o[4]} sa={o[5]} sb={o[6]} aux={o[7]}"
                for k, (nm, o) in enumerate(zip(self.op_names(), self.ops.tolist()))]

    def flatten_inputs(self, samples, dtype=np.float64):
        """[S, dim] from a dict name -> [S, *site shape] (or an array [S, dim])."""
        if isinstance(samples, dict):
            S = len(next(iter(samples.values())))
            cols = [np.asarray(samples[name], dtype).reshape(S, n) for name, _, n, _ in self.inputs]
            return np.concatenate(cols, 1) if cols else np.zeros((S, 0), dtype)
        return np.atleast_2d(np.asarray(samples, dtype))

    # ------------------------------------------------------------------ NumPy interpreter
    def run_host(self, samples, dtype=np.float64):
        """The program on every row of ``samples`` (see flatten_inputs), every op in ``dtype``
        arithmetic: {observed site: [S, *shape]} as ``dtype`` arrays, the constant outputs
        broadcast over S."""
        T = np.dtype(dtype).type
        Z = self.flatten_inputs(samples, dtype)
        S, NS, D = Z.shape[0], self.num_slots, self.dim
        assert Z.shape[1] == D
        cp = self.consts64.astype(dtype) if T is np.float64 else self.consts.astype(dtype)
        ix = self.index
        v = np.zeros((S, NS), dtype)
        v[:, :D] = Z

        def operand(ref, n, stride):
            ln = n if stride else 1
            return v[:, ref:ref + ln] if ref >= 0 else cp[None, ~ref:~ref + ln]

        fwd = dict(_HOST_FWD, lgamma=lambda x: _lgamma(x, dtype))
        with np.errstate(all="ignore"):
            for (op, dst, a, b, n, sa, sb, aux), nm in zip(self.ops.tolist(), self.op_names()):
                if nm in _UNARY:
                    v[:, dst:dst + n] = fwd[nm](operand(a, n, sa))
                elif nm in _BINARY:
                    v[:, dst:dst + n] = fwd[nm](operand(a, n, sa), operand(b, n, sb))
                elif nm == "reduce_sum":
                    v[:, dst] = v[:, a:a + n].sum(1)
                elif nm == "gather":
                    v[:, dst:dst + n] = v[:, a + ix[aux:aux + n]]
                elif nm == "matvec":
                    M = cp[~b:~b + n * aux].reshape(n, aux)
                    v[:, dst:dst + n] = v[:, a:a + aux] @ M.T
                elif nm in _LINALG:
                    _host_linalg_fwd(nm, v, cp, dst, a, b, n, aux)
                else:
                    assert nm in _SCAN, nm
                    _host_scan_fwd(nm, v, cp, dst, a, b, n, aux)
        out = {o.name: np.broadcast_to(v[:, o.slot:o.slot + o.n].reshape((S,) + ((o.n,) if o.shape else ())),
                                       (S,) + o.shape).copy() for o in self.outputs}
        for name, c in self.constant_outputs.items():
            out[name] = np.broadcast_to(np.asarray(c, dtype), (S,) + np.shape(c)).copy()
        return out


def _batch_shape(s, base, obs_shape):
    """Shape of log_prob at an observed site: the data's shape without the event dimensions,
    broadcast with the distribution's batch shape."""
    ev = len(base.event_shape)
    data = tuple(obs_shape[:len(obs_shape) - ev]) if ev else tuple(obs_shape)
    site = tuple(s.shape[:len(s.shape) - ev]) if ev else tuple(s.shape)
    return tuple(np.broadcast_shapes(data, site))


def compile_log_likelihood(model, args=(), kwargs=None, given=()):
    """Trace ``model(*args, **kwargs)`` and lower the log density of its observed sites to a
    LogLikProgram.  The sample sites without data whose name is in ``given`` are the inputs
    (sorted by name, constrained values).  A site that is neither observed nor given raises
    ValueError naming it (the reference would need an rng key there); a model outside the program
    compiler's class raises NotImplementedError naming the site."""
    cfg = getattr(model, "_nmx_reparam", None)
    fn = getattr(model, "_nmx_model", model)
    trace = trace_model(fn, args, kwargs, cfg)
    for name in trace.reparam:
        _refuse(name, "reparam configs are not supported")
    given = set(given)
    sizes = {}
    for s in trace.sites.values():
        base = _base(s.fn)
        if type(base) not in _LOGPROB:
            _refuse(s.name, f"{type(base).__name__} is not supported")
        if s.obs is None and s.name not in given:
            raise ValueError(f"log_likelihood: site {s.name!r} is neither observed nor in the posterior samples "
                             "(its value would have to be drawn)")
        if len(s.shape) > 1:
            _refuse(s.name, f"site of shape {s.shape}: sites of rank > 1 are not supported")
        if s.obs is not None and np.ndim(_host(s.obs)) > 1:
            _refuse(s.name, f"observations of shape {np.shape(_host(s.obs))}: rank > 1 is not supported")
        if s.obs is not None and isinstance(s.fn, dist.Independent):
            _refuse(s.name, "an observed site under to_event: its log density is not elementwise")
        n = int(np.prod(s.shape, dtype=np.int64))
        if n <= 0:
            _refuse(s.name, "empty site")
        sizes[s.name] = n
    inputs, dim = [], 0
    for s in sorted((s for s in trace.sites.values() if s.obs is None), key=lambda s: s.name):
        inputs.append((s.name, dim, sizes[s.name], tuple(s.shape)))
        dim += sizes[s.name]
    B = _Builder(dim)
    values = {name: _V(B, n, slot=off) for name, off, n, _ in inputs}
    lower = _Lowering(B, values)
    outputs, constant_outputs = [], {}
    for s in trace.sites.values():
        if s.obs is None:
            continue
        base = _base(s.fn)
        expand, pnames, _ = _LOGPROB[type(base)]
        xv = np.asarray(_host(s.obs), np.float64)
        shape = _batch_shape(s, base, xv.shape)
        n_site = int(np.prod(shape, dtype=np.int64))
        try:
            d = {p: lower.vector(getattr(base, p), s.name) for p in pnames}
            if isinstance(base, _BINOMIAL) and not d["total_count"].is_const:
                _refuse(s.name, "a total_count that depends on a latent site: it must be data")
            x = B.const(xv)
            with np.errstate(all="ignore"):
                logx = B.const(np.log(x.c)) if base.support in ("positive", "simplex") else None
            if isinstance(base, dist.MixtureSameFamily):
                terms = _ew_mixture(B, lower, base, np.asarray(x.c, np.float64).reshape(-1), s.name)
            elif isinstance(base, dist.MultivariateNormal):  # one observation per sample, as a Dirichlet vector
                terms = _lp_mvn(B, lower, base, x, s)
            else:
                terms = _ELEMENTWISE.get(type(base), expand)(B, d, x, logx)
            # the constant terms are part of the answer: summed on the host, then added once (a scalar
            # against n_site elements is a stride-0 operand)
            total, const = None, None
            for t in terms:
                t = B.const(t)
                if t.n not in (1, n_site):
                    _refuse(s.name, f"a log-density term of {t.n} elements at a site of {n_site}")
                if t.is_const:
                    const = t if const is None else const + t
                else:
                    total = t if total is None else total + t
            if total is None:
                total = const
            elif const is not None:
                total = total + const
        except _Refuse:
            raise
        except NotImplementedError as e:
            _refuse(s.name, str(e))
        if total.is_const:
            constant_outputs[s.name] = np.broadcast_to(total.c.reshape(shape if total.n > 1 else ()), shape).copy()
        else:
            outputs.append(LogLikOutput(s.name, total.slot, total.n, shape, 0))
    if not outputs:  # nothing to run on the device: every log density is a host constant
        return LogLikProgram(np.zeros((0, native.OP_WORDS)), [], [], dim, dim, inputs, [], constant_outputs)
    made = {op[1]: k for k, op in enumerate(B.ops)}
    ops, moved, num_slots = B.compact([made[o.slot] for o in outputs if o.slot >= dim])
    column = 0
    for o in outputs:
        o.slot = moved.get(o.slot, o.slot)
        o.column = column
        column += o.n
    consts = np.concatenate(B.consts) if B.consts else np.zeros(0)
    return LogLikProgram(ops, consts, B.index, num_slots, dim, inputs, outputs, constant_outputs)
