"""Log-likelihood programs: the elementwise log density of every observed site, for the generic
path of the model front end.

The reference's ``log_likelihood`` re-runs the model once per posterior sample with the latent
sites substituted and reads ``site["fn"].log_prob(site["value"])`` of every observed site
(numpyro/infer/util.py:1094-1170).  ``compile_log_likelihood`` traces the model once
(frontend.trace_model) and lowers that run to a straight-line, draw-free program of the program
compiler's format (numpyro_amd/program.py, the same builder and ``_LOGPROB`` / ``_COUNT_LOGPROB`` expansions: folding,
sharing and refusals are the same) whose inputs are the given sites' constrained values, as a
predictive program's (predictive_program.py), and whose outputs are one value per observed site:
its ``log_prob`` *before* any sum over the site, constants included.  One HIP kernel
(csrc/loglik_program.hip k_program_loglik) runs the program once per posterior sample and packs
the outputs into a dense [S, columns] table; the reduce kernels of the same file turn such a
table into the pointwise lppd and p_waic without holding it whole.

``LogLikProgram.run_host`` runs the same program on the one NumPy forward interpreter (program.py
``Program._forward_host``; float64, and float32 with the same arithmetic in float32, the
calibration of the device tests).
"""
from __future__ import annotations

import numpy as np

from . import distributions as dist
from .frontend import _base, _host
from .program import (_ELEMENTWISE, _ZERO_INFLATED, _ForwardProgram, _Refuse, _check_count_data, _ew_mixture,
                      _forward_prologue, _logprob_entry, _lp_mvn, _lp_zero_inflated, _refuse)


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


class LogLikProgram(_ForwardProgram):
    """A forward-only program without draws (program.py _ForwardProgram): ``outputs`` are the
    observed sites whose log density depends on a given site, ``constant_outputs`` (name ->
    float64 array of the site's shape) those that are host constants.  ``num_columns`` is the width
    of the dense table."""

    _CHECK = "nmx_loglik_program_check"

    def __init__(self, ops, consts, index, num_slots, dim, inputs, outputs, constant_outputs):
        super().__init__(ops, consts, index, num_slots, dim, inputs, outputs)
        self.constant_outputs = dict(constant_outputs)
        self.num_columns = sum(o.n for o in self.outputs)

    def output_table(self):
        """int32 [num_outputs, 3]: { slot, n, column }."""
        return np.ascontiguousarray(np.asarray([[o.slot, o.n, o.column] for o in self.outputs],
                                               np.int32).reshape(-1, 3))

    def native_check(self, outputs=None, ldo=None):
        """(status, message) of nmx_loglik_program_check on the host arrays: needs no GPU."""
        return super().native_check(outputs, self.num_columns if ldo is None else int(ldo))

    # ------------------------------------------------------------------ NumPy interpreter
    def run_host(self, samples, dtype=np.float64):
        """The program on every row of ``samples`` (see flatten_inputs), every op in ``dtype``
        arithmetic: {observed site: [S, *shape]} as ``dtype`` arrays, the constant outputs
        broadcast over S."""
        v = self._forward_host(self.flatten_inputs(samples, dtype), dtype, self._pool(dtype))
        S = v.shape[0]
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
    def missing(s, base):
        raise ValueError(f"log_likelihood: site {s.name!r} is neither observed nor in the posterior samples "
                         "(its value would have to be drawn)")

    def observed(s):
        if isinstance(s.fn, dist.Independent):
            _refuse(s.name, "an observed site under to_event: its log density is not elementwise")

    # every site without data is given (`missing` raises otherwise): they are the inputs
    trace, _, inputs, B, _, lower = _forward_prologue(model, args, kwargs, given, missing, observed)
    outputs, constant_outputs = [], {}
    for s in trace.sites.values():
        if s.obs is None:
            continue
        base = _base(s.fn)
        expand, pnames, _ = _logprob_entry(base)
        xv = np.asarray(_host(s.obs), np.float64)
        shape = _batch_shape(s, base, xv.shape)
        n_site = int(np.prod(shape, dtype=np.int64))
        try:
            d = {p: lower.vector(getattr(base, p), s.name) for p in pnames}
            _check_count_data(base, d, s.name)
            x = B.const(xv)
            with np.errstate(all="ignore"):
                logx = B.const(np.log(x.c)) if base.support in ("positive", "simplex") else None
            if isinstance(base, dist.MixtureSameFamily):
                terms = _ew_mixture(B, lower, base, np.asarray(x.c, np.float64).reshape(-1), s.name)
            elif isinstance(base, dist.MultivariateNormal):  # one observation per sample, as a Dirichlet vector
                terms = _lp_mvn(B, lower, base, x, s)
            elif isinstance(base, _ZERO_INFLATED):  # elementwise as it is: one value per observation
                terms = _lp_zero_inflated(B, lower, base, x, s.name)
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
        return LogLikProgram.empty(B.dim, inputs, constant_outputs)
    column = 0
    for o in outputs:
        o.column = column
        column += o.n
    return LogLikProgram(*B.forward_arrays(outputs), inputs, outputs, constant_outputs)
