"""``Predictive``: posterior predictive draws for the fused models, and posterior / prior
predictive draws for any other traced model of the program compiler's class.

Mirrors ``numpyro.infer.Predictive`` (numpyro/infer/util.py:888-1090): constructed from a
model and a dict of posterior samples (``MCMC.get_samples()``, leading batch dims per
``batch_ndims``), called with ``(rng_key, *model_args, **model_kwargs)`` where the observed
argument is ``None``, it returns ``{site: [*batch_shape, *site_shape]}`` for every sample site
not in ``posterior_samples`` (the observed sites) plus any ``return_sites`` asked for.  The
reference re-runs the traced model once per sample under ``substitute`` (:803-885); here each
model's observed-site sampler is one HIP kernel over all samples (csrc/predictive.hip).

An observed site whose data is passed (not ``None``) keeps that data, as ``numpyro.sample``
with ``obs=`` does under the reference's Predictive.  Deterministic sites (the model's
``numpyro.deterministic`` and reparameterised sites such as the non-centred funnel's ``x``,
reparam.py:140-142) are returned by default, as the reference's ``_predictive`` does
(util.py:870-877), computed from the posterior samples.  Models: covtype logistic regression
(``obs``), eight schools (``obs``), BNN (``Y``), stochastic volatility (``r``: its returns are
both the observation and the series length, examples/stochastic_volatility.py:57-65, so -- as in
the reference -- the observed data come back), funnel and its LocScaleReparam form (no observed
site: deterministic ``x`` and any ``return_sites``, as examples/funnel.py:84-87 uses it).  Out of
scope (raise): guides / params (SVI), ``infer_discrete``, prior predictive of a fused model.

Any other callable model takes the program path: at call time, when the arguments are known, the
model is traced and lowered to a forward-only program with draw ops
(numpyro_amd/predictive_program.py compile_predictive) that one HIP kernel runs once per
posterior sample (csrc/predictive_program.hip).  The sample sites named in ``posterior_samples``
are the program's inputs; every other site without data is drawn, in the model's order, so a
drawn site parameterises the later ones.  ``Predictive(model, num_samples=N)`` without posterior
samples draws every site: prior predictive.  Returned by default: the drawn sites, the observed
sites whose data was passed (as given) and the deterministic sites; Bernoulli, Binomial and Poisson
sites as int32 (an element whose parameter is outside the support, where a float site holds NaN, is
-1), the others float32.  A model outside the compiler's class raises NotImplementedError
naming the site.
"""
from __future__ import annotations

import ctypes
import math
import warnings

import numpy as np
import torch

from .. import native
from .. import potentials as P
from ..native import check, lib, ptr
from ..random import key_to_seed


def _as_device(x, device):
    return torch.as_tensor(x if torch.is_tensor(x) else np.asarray(x), dtype=torch.float32).to(device).contiguous()


def _observed(value, S, device, dtype=torch.float32):
    """An observed site keeps its data (numpyro.sample with obs=...): [S, *shape]."""
    v = torch.as_tensor(value if torch.is_tensor(value) else np.asarray(value)).to(device, dtype)
    return v.unsqueeze(0).expand(S, *v.shape)


def _predict_logreg(samples, seed, device, data, labels=None, subsample_size=None):
    if subsample_size is not None:
        raise NotImplementedError("subsample_size is out of scope here")
    X = _as_device(data, device)
    N, D = X.shape
    coefs = samples["coefs"].reshape(-1, D).to(device, torch.float32).contiguous()
    S = coefs.shape[0]
    if labels is not None:
        return {"obs": _observed(labels, S, device, torch.int32)}
    out = torch.empty(S, N, dtype=torch.int32, device=device)
    check(lib().nmx_predict_logreg(ptr(X), N, D, ptr(coefs), S, seed, ptr(out), native.stream_ptr()),
          "nmx_predict_logreg")
    return {"obs": out}


def _predict_eight_schools(samples, seed, device, J, sigma, y=None):
    theta = samples["theta"].reshape(-1, J).to(device, torch.float32).contiguous()
    if y is not None:
        return {"obs": _observed(y, theta.shape[0], device)}
    sig = _as_device(sigma, device).reshape(J)
    out = torch.empty_like(theta)
    check(lib().nmx_predict_normal(ptr(theta), ptr(sig), J, theta.shape[0], seed, ptr(out), native.stream_ptr()),
          "nmx_predict_normal")
    return {"obs": out}


def _predict_bnn(samples, seed, device, X, Y, D_H, D_Y=1):
    Xd = _as_device(X, device)
    N, Dx = Xd.shape
    S = samples["prec_obs"].reshape(-1).shape[0]
    if Y is not None:
        return {"Y": _observed(Y, S, device)}
    flat = torch.cat([samples["prec_obs"].reshape(S, 1), samples["w1"].reshape(S, -1), samples["w2"].reshape(S, -1),
                      samples["w3"].reshape(S, -1)], dim=1).to(device, torch.float32).contiguous()
    out = torch.empty(S, N, D_Y, dtype=torch.float32, device=device)
    check(lib().nmx_predict_bnn(ptr(Xd), N, Dx, D_H, D_Y, ptr(flat), S, seed, ptr(out), native.stream_ptr()),
          "nmx_predict_bnn")
    return {"Y": out}


def _predict_sv(samples, seed, device, returns):
    if returns is None:
        raise ValueError("stochastic volatility: `returns` set the series length (examples/stochastic_volatility.py:"
                         "57-65); the observed site r keeps them")
    S = samples["s"].reshape(samples["s"].shape[0], -1).shape[0]
    return {"r": _observed(returns, S, device)}


def _predict_none(samples, seed, device, *args, **kwargs):
    return {}


# FusedModel -> (observed sites, sampler(samples, seed, device, *args, **kwargs))
_PREDICTORS = {
    "logistic_regression": (("obs",), _predict_logreg),
    "eight_schools": (("obs",), _predict_eight_schools),
    "bnn": (("Y",), _predict_bnn),
    "stochastic_volatility": (("r",), _predict_sv),
    "funnel": ((), _predict_none),
    "funnel_reparam": ((), _predict_none),
}


# models whose Predictive draws nothing on the device (no free observed site)
_HOST_ONLY = {"stochastic_volatility", "funnel", "funnel_reparam"}


def common_batch_shape(shapes):
    """The batch shape that every (site, leading shape) of ``shapes`` has, None without a site."""
    batch_shape = proto = None
    for name, shp in shapes:
        if batch_shape is not None and shp != batch_shape:
            raise ValueError(f"Batch shapes at site {name} and {proto} should be the same, "
                             f"but got {shp} and {batch_shape}")
        if batch_shape is None:
            batch_shape, proto = shp, name
    return batch_shape


class Predictive:
    """numpyro.infer.Predictive (numpyro/infer/util.py:888-1090) for the fused models and for
    model functions of the program compiler's class (posterior and prior predictive)."""

    def __init__(self, model, posterior_samples=None, *, guide=None, params=None, num_samples=None,
                 return_sites=None, infer_discrete=False, parallel=False, batch_ndims=None,
                 exclude_deterministic=True, max_workspace_bytes=1 << 30):
        if posterior_samples is None and num_samples is None:
            raise ValueError("Either posterior_samples or num_samples must be specified.")
        if posterior_samples is not None and guide is not None:
            raise ValueError("Only one of guide or posterior_samples can be provided, not both.")
        if guide is not None or params:
            raise NotImplementedError("Predictive with a guide / params (SVI) is out of scope here")
        if infer_discrete:
            raise NotImplementedError("infer_discrete is out of scope here")
        fused = isinstance(model, P.FusedModel)
        if posterior_samples is None and (fused or not callable(model)):
            raise NotImplementedError("prior predictive (no posterior_samples) of a fused model is out of scope here")
        if not callable(model) or (fused and model.__name__ not in _PREDICTORS):
            raise NotImplementedError(f"no predictive sampler for {model!r} "
                                      f"(available: {sorted(_PREDICTORS)}, or a model function)")
        batch_ndims = 1 if batch_ndims is None else batch_ndims
        self._fused = fused
        self.max_workspace_bytes = int(max_workspace_bytes)
        if posterior_samples is None:  # prior predictive: every site is drawn
            if int(num_samples) <= 0:
                raise ValueError(f"num_samples must be positive, got {num_samples}")
            posterior_samples = {}
            batch_ndims = 1
        batch_shape = common_batch_shape((k, tuple(v.shape[:batch_ndims])) for k, v in posterior_samples.items())
        if batch_shape is None and (fused or num_samples is None):
            raise ValueError("No sample sites in posterior samples to infer `num_samples`.")
        if batch_shape is None:
            batch_shape = (int(num_samples),)
        batch_size = int(math.prod(batch_shape))
        if num_samples is not None and num_samples != batch_size:
            warnings.warn(f"Sample's batch dimension size {batch_size} is different from the provided "
                          f"{num_samples} num_samples argument. Defaulting to {batch_size}.", UserWarning)
        if return_sites is not None:
            assert isinstance(return_sites, (list, tuple, set))
        self.model = model
        self.posterior_samples = posterior_samples
        self.num_samples = batch_size
        self.return_sites = return_sites
        self.batch_ndims = batch_ndims
        self._batch_shape = batch_shape
        self.exclude_deterministic = exclude_deterministic
        self.parallel = parallel

    def __call__(self, rng_key, *args, **kwargs):
        if not self._fused:
            return self._call_program(rng_key, args, kwargs)
        observed, sampler = _PREDICTORS[self.model.__name__]
        nb = self.batch_ndims
        S = self.num_samples
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
        if device is None:
            if self.model.__name__ not in _HOST_ONLY:
                raise RuntimeError("Predictive needs a GPU (the samplers are HIP kernels)")
            device = torch.device("cpu")  # nothing is drawn: observed data / deterministic sites
        flat = {k: torch.as_tensor(v).reshape(S, *v.shape[nb:]) for k, v in self.posterior_samples.items()}
        draws = sampler(flat, key_to_seed(rng_key), device, *args, **kwargs)
        # deterministic sites from the (constrained) latent values: recomputed from the samples
        # (exclude_deterministic=True, the default) or taken as given
        pot = self.model.potential(*args, **kwargs)
        latent = {n: flat[n] for n, _, _ in pot.sites if n in flat}
        dets = pot.deterministic(latent) if len(latent) == len(pot.sites) else {}
        if not self.exclude_deterministic:
            dets.update({k: v for k, v in flat.items() if k in dets})
        if self.return_sites is None:
            names = [n for n in observed if n not in self.posterior_samples] + list(dets)
        else:
            names = list(self.return_sites)
        out = {}
        for n in names:
            if n in draws and n not in self.posterior_samples:
                v = draws[n]
            elif n in dets:
                v = dets[n]
            elif n in flat:  # a substituted latent site, returned as given
                v = flat[n]
            else:
                continue
            out[n] = v.reshape(*self._batch_shape, *v.shape[1:])
        return out

    # ------------------------------------------------------------------ program path
    def _call_program(self, rng_key, args, kwargs):
        from ..frontend import eval_sym
        from ..jnp import Sym, shape_of
        from ..predictive_program import compile_predictive

        nb, S = self.batch_ndims, self.num_samples
        flat = {k: torch.as_tensor(v).reshape(S, *v.shape[nb:]) for k, v in self.posterior_samples.items()}
        prog = compile_predictive(self.model, args, kwargs, given=flat)
        device = prog.sample_device(flat, "Predictive")  # the CPU where nothing is drawn: observed data / given sites
        given = {name: flat[name].to(device, torch.float32) for name, _, _, _ in prog.inputs}
        draws = self._run_program(prog, given, key_to_seed(rng_key), device) if prog.num_ops else {}
        for name, (value, integer) in prog.observed.items():
            draws[name] = _observed(value, S, device, torch.int32 if integer else torch.float32)
        dets = {o.name: draws.pop(o.name) for o in prog.outputs if not o.streams}
        for name, expr in prog.host_deterministics.items():
            if not self.exclude_deterministic and name in flat:
                dets[name] = flat[name].to(device)
                continue
            ev = tuple(shape_of(expr)) if isinstance(expr, Sym) else tuple(np.shape(expr))
            v = eval_sym(expr, given) if isinstance(expr, Sym) else torch.as_tensor(np.asarray(expr, np.float32))
            dets[name] = v.to(device).expand(S, *ev).clone() if tuple(v.shape) != (S,) + ev else v
        names = list(draws) + list(dets) if self.return_sites is None else list(self.return_sites)
        out = {}
        for n in names:
            v = draws[n] if n in draws else dets[n] if n in dets else flat[n].to(device) if n in flat else None
            if v is not None:
                out[n] = v.reshape(*self._batch_shape, *v.shape[1:])
        return out

    def _run_program(self, prog, given, seed, device):
        """{output site: [S, *shape]} of the program over all samples, in chunks whose tape stays
        under max_workspace_bytes; a draw depends on the global sample index, not on the chunk."""
        S = self.num_samples
        bound, x, chunk, tape = prog.bind_samples(given, S, device, self.max_workspace_bytes,
                                                  "predictive program", "max_workspace_bytes")
        parts = {o.name: [] for o in prog.outputs}
        for s0 in range(0, S, chunk):
            m = min(chunk, S - s0)
            check(lib().nmx_predict_program(ctypes.byref(bound.struct), ptr(x[s0:]) if x is not None else None, m, s0,
                                            seed, ptr(tape), native.stream_ptr()), "nmx_predict_program")
            for o in prog.outputs:
                v = tape[:m, o.slot:o.slot + o.n]  # a view of the tape: copied out before the next chunk
                if o.integer:  # whole numbers, or NaN where the parameter is outside the support: -1
                    v = torch.nan_to_num(v, nan=-1.0).to(torch.int32)
                else:
                    v = v.clone()
                parts[o.name].append(v.reshape(m, *o.shape))
        return {k: v[0] if len(v) == 1 else torch.cat(v) for k, v in parts.items()}
