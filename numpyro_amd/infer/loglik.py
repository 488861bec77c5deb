"""``log_likelihood`` and ``pointwise_predictive``: the log density of every observed site at
each posterior sample, for model functions of the program compiler's class.

Mirrors ``numpyro.infer.log_likelihood`` (numpyro/infer/util.py:1094-1170): called with the model,
a dict of posterior samples (``MCMC.get_samples()``, leading batch dims per ``batch_ndims``) and
the model's arguments, data included, it returns ``{observed site: [*batch_shape, *site_shape]}``.
The reference re-runs the model once per sample under ``substitute``; here the model is traced
once and lowered to a draw-free program (numpyro_amd/loglik_program.py compile_log_likelihood)
that one HIP kernel runs once per sample, writing a dense table (csrc/loglik_program.hip).

Nearly every use reduces that table over the samples (the log pointwise predictive density that
examples/baseball.py prints, WAIC): ``pointwise_predictive`` streams the same chunks through the
pointwise reduce kernels and returns the per-observation lppd and p_waic without holding the
table.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from .. import native
from .. import potentials as P
from ..native import check, lib, ptr
from ..pointwise import PointwiseReducer
from .predictive import common_batch_shape

# the tape of one chunk of samples stays under this many bytes
MAX_WORKSPACE_BYTES = 1 << 30
# loo holds the whole table and the PSIS kernel's column-contiguous copy of it: both under this
MAX_LOO_BYTES = 8 << 30


def _flatten(model, posterior_samples, batch_ndims, what):
    if isinstance(model, P.FusedModel):
        raise NotImplementedError(f"{what}: {model!r} is a FusedModel object, not a model function; pass the model "
                                  "written with numpyro_amd.sample (it is traced the program way)")
    if not callable(model):
        raise NotImplementedError(f"{what}: {model!r} is not a model function")
    if batch_ndims not in (0, 1, 2):
        raise ValueError(f"batch_ndims must be 0, 1 or 2, got {batch_ndims}")

    def leading():  # (site, batch shape), each checked before the sites after it are looked at
        for name, v in posterior_samples.items():
            if np.ndim(v) < batch_ndims:
                raise ValueError(f"site {name} has shape {tuple(np.shape(v))}, fewer than batch_ndims = {batch_ndims} dimensions")
            yield name, tuple(np.shape(v)[:batch_ndims])

    batch_shape = common_batch_shape(leading())
    if batch_shape is None:
        raise ValueError("No sample sites in posterior samples to infer `num_samples`.")
    S = int(math.prod(batch_shape))
    if S <= 0:
        raise ValueError(f"posterior samples of batch shape {batch_shape} hold no sample")
    flat = {k: torch.as_tensor(v if torch.is_tensor(v) else np.asarray(v)) for k, v in posterior_samples.items()}
    flat = {k: v.reshape(S, *v.shape[batch_ndims:]) for k, v in flat.items()}
    return flat, batch_shape, S


class _Run:
    """A compiled log-likelihood program bound to a device: its arrays uploaded, the samples
    flattened to [S, dim], and the chunking under MAX_WORKSPACE_BYTES."""

    def __init__(self, model, posterior_samples, args, kwargs, batch_ndims, what):
        from ..loglik_program import compile_log_likelihood

        flat, self.batch_shape, self.S = _flatten(model, posterior_samples, batch_ndims, what)
        self.prog = prog = compile_log_likelihood(model, args, kwargs, given=flat)
        self.device = prog.sample_device(flat, what)  # the CPU where every log density is a host constant
        if not prog.num_ops:
            return
        self.bound, self.x, self.chunk, self.tape = prog.bind_samples(
            flat, self.S, self.device, MAX_WORKSPACE_BYTES, what, "MAX_WORKSPACE_BYTES")
        self.d_outputs = torch.from_numpy(prog.output_table()).to(self.device)

    def chunks(self):
        return [(s0, min(self.chunk, self.S - s0)) for s0 in range(0, self.S, self.chunk)]

    def launch(self, s0, m, out):
        """Samples [s0, s0 + m) into the rows of ``out`` [>= m, num_columns]."""
        prog, x = self.prog, ptr(self.x[s0:]) if self.x is not None else None
        check(lib().nmx_loglik_program(ctypes.byref(self.bound.struct), x, m, ptr(self.d_outputs), len(prog.outputs),
                                       ptr(self.tape), ptr(out), prog.num_columns, native.stream_ptr()),
              "nmx_loglik_program")

    def constant(self, c):
        return torch.as_tensor(np.asarray(c, np.float32)).to(self.device)


def log_likelihood(model, posterior_samples, *args, parallel=False, batch_ndims=1, **kwargs):
    """numpyro.infer.log_likelihood (numpyro/infer/util.py:1094-1170) for model functions of the
    program compiler's class: {observed site: float32 tensor [*batch_shape, *site_shape]} on the
    current GPU.  ``parallel`` is accepted and ignored (every sample is one wave of one launch)."""
    run = _Run(model, posterior_samples, args, kwargs, batch_ndims, "log_likelihood")
    prog, S = run.prog, run.S
    out = {}
    if prog.num_ops:
        table = torch.empty(S, prog.num_columns, dtype=torch.float32, device=run.device)
        for s0, m in run.chunks():
            run.launch(s0, m, table[s0:])
        for o in prog.outputs:
            v = table[:, o.column:o.column + o.n]
            out[o.name] = v.reshape(S, *((o.n,) if o.shape else ())).expand(S, *o.shape).contiguous()
    for name, c in prog.constant_outputs.items():
        out[name] = run.constant(c).expand(S, *np.shape(c)).contiguous()
    return {name: v.reshape((*run.batch_shape, *v.shape[1:])) for name, v in out.items()}


def pointwise_predictive(model, posterior_samples, *args, batch_ndims=1, **kwargs):
    """{observed site: {"lppd": [*site_shape], "p_waic": [*site_shape]}}: per observation, the log
    pointwise predictive density logsumexp_s(log p(y_i | theta_s)) - log S and the variance over s
    of log p(y_i | theta_s) (S - 1 in the denominator: NaN for one sample), reduced on the device
    chunk by chunk without holding the [S, N] table."""
    run = _Run(model, posterior_samples, args, kwargs, batch_ndims, "pointwise_predictive")
    prog, S = run.prog, run.S
    out = {}
    if prog.num_ops:
        red = PointwiseReducer(prog.num_columns, run.device)
        table = torch.empty(run.chunk, prog.num_columns, dtype=torch.float32, device=run.device)
        for s0, m in run.chunks():  # stream order: the reduce reads the chunk before the next launch writes it
            run.launch(s0, m, table)
            red.accumulate(table[:m])
        lppd, p_waic = red.finish()
        for o in prog.outputs:
            out[o.name] = {k: v[o.column:o.column + o.n].reshape((o.n,) if o.shape else ()).expand(o.shape).contiguous()
                           for k, v in (("lppd", lppd), ("p_waic", p_waic))}
    for name, c in prog.constant_outputs.items():
        # S equal values: their logsumexp - log S is the value, their variance 0
        c = run.constant(c)
        out[name] = {"lppd": c, "p_waic": torch.full_like(c, 0.0 if S > 1 else float("nan"))}
    return out


def loo(model, posterior_samples, *args, batch_ndims=1, reff=1.0, **kwargs):
    """{observed site: {"elpd_loo": [*site_shape], "pareto_k": [*site_shape], "lppd": [*site_shape]}}:
    per observation, the PSIS leave-one-out log predictive density, the Pareto-k diagnostic of its
    importance ratios (numpyro_amd/psis.py; ``reff`` the relative efficiency of the draws) and the
    in-sample lppd of ``pointwise_predictive``.  The smoothing needs every sample of an observation
    at once, so the [S, N] table is held on the device, with the kernel's copy of it."""
    from .. import psis

    run = _Run(model, posterior_samples, args, kwargs, batch_ndims, "loo")
    prog, S = run.prog, run.S
    tail = psis.tail_length(S, reff)
    psis.check_sizes(S, tail)
    out = {}
    if prog.num_ops:
        N = prog.num_columns
        need = 4 * S * N + lib().nmx_psis_workspace_bytes(S, N)
        if need > MAX_LOO_BYTES:
            raise NotImplementedError(f"loo: the table of S = {S} samples x N = {N} observations and its workspace "
                                      f"need {need} bytes, above MAX_LOO_BYTES = {MAX_LOO_BYTES}; thin the draws")
        table = torch.empty(S, N, dtype=torch.float32, device=run.device)
        for s0, m in run.chunks():
            run.launch(s0, m, table[s0:])
        red = PointwiseReducer(N, run.device)
        red.accumulate(table)
        lppd, _ = red.finish()
        elpd, k = psis.psis_loo_columns(table, N, tail)
        for o in prog.outputs:
            out[o.name] = {key: v[o.column:o.column + o.n].reshape((o.n,) if o.shape else ()).expand(o.shape).contiguous()
                           for key, v in (("elpd_loo", elpd), ("pareto_k", k), ("lppd", lppd))}
    for name, c in prog.constant_outputs.items():
        # S equal ratios: no tail (T = 0), so no fit, and the estimate is the value itself
        c = run.constant(c)
        out[name] = {"elpd_loo": c, "pareto_k": torch.full_like(c, float("inf")), "lppd": c}
    return out
