"""numpyro.infer.autoguide for the device SVI step: mean-field normal guides over the model's
unconstrained coordinates (numpyro/infer/autoguide.py AutoNormal, AutoDiagonalNormal).

Both guides are the same device state -- ``loc[D]`` and ``rho[D]`` with ``scale = softplus(rho)``
(numpyro's ``softplus_positive`` constraint on the scale), optimised by csrc/svi.hip -- and differ
only in how the parameters are named:

  AutoNormal:          ``{site}_auto_loc`` / ``{site}_auto_scale`` per latent site, in the site's
                       unconstrained shape (a Dirichlet site of K weights has K - 1 coordinates);
  AutoDiagonalNormal:  ``auto_loc`` / ``auto_scale`` of shape [D] (ravel_pytree order: sorted sites).

``scale`` is reported constrained.  Either naming is accepted wherever parameters are passed in.
The model is resolved (traced and mapped onto its potential) by ``SVI.init`` / ``SVI.run``; the
guide's methods need that to have happened.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import native
from ..native import check, lib, ptr
from ..random import key_to_seed


class AutoGuide:
    flat_names = False  # parameters named per site

    def __init__(self, model, *, prefix="auto", init_loc_fn=None, init_scale=0.1):
        from .hmc import init_to_uniform

        if init_loc_fn is not None and init_loc_fn is not init_to_uniform:
            raise NotImplementedError(f"{type(self).__name__}: only init_loc_fn=init_to_uniform is supported (the "
                                      "engine's init_to_uniform(radius=2) draw); pass init_params to SVI.init / "
                                      "SVI.run for another start")
        if not float(init_scale) > 0.0:
            raise ValueError(f"Expected init_scale to be positive, got {init_scale}")
        self.model, self.prefix, self.init_scale = model, prefix, float(init_scale)
        self._potential = None

    # ------------------------------------------------------------------ binding and naming
    def _setup(self, potential):
        self._potential = potential

    def _pot(self):
        if self._potential is None:
            raise RuntimeError(f"{type(self).__name__}: the guide has no model structure yet; call SVI.init or "
                               "SVI.run first")
        return self._potential

    def _names(self, site=None):
        stem = self.prefix if site is None else f"{site}_{self.prefix}"
        return f"{stem}_loc", f"{stem}_scale"

    def _params(self, loc, scale):
        """Flat loc [D] and scale [D] -> the guide's parameter dict."""
        pot = self._pot()
        if self.flat_names:
            nl, ns = self._names()
            return {nl: loc, ns: scale}
        out = {}
        locs, scales = pot.unflatten(loc), pot.unflatten(scale)
        for name, _, _ in pot.sites:
            nl, ns = self._names(name)
            out[nl], out[ns] = locs[name], scales[name]
        return out

    def _flat(self, params, default_loc=None, default_scale=None):
        """A parameter dict in either naming -> (loc [D], scale [D]) float32 tensors (on the device of
        the values given); a missing entry takes the default, or is an error without one."""
        pot = self._pot()
        known = set(self._names()) | {n for s, _, _ in pot.sites for n in self._names(s)}
        unknown = sorted(set(params) - known)
        if unknown:
            raise ValueError(f"{type(self).__name__}: unknown parameter(s) {unknown}; the guide's parameters are "
                             f"{sorted(known)}")

        def get(kind, default):
            flat_name = self._names()[kind]
            if flat_name in params:
                v = torch.as_tensor(params[flat_name], dtype=torch.float32).reshape(-1)
                if v.numel() != pot.dim:
                    raise ValueError(f"{flat_name}: {v.numel()} values, the model has {pot.dim} coordinates")
                return v
            parts = []
            o = 0
            for name, shape, _ in pot.sites:
                n = int(np.prod(shape, dtype=np.int64))
                key = self._names(name)[kind]
                if key in params:
                    v = torch.as_tensor(params[key], dtype=torch.float32)
                    if tuple(v.shape) != tuple(shape):
                        raise ValueError(f"{key}: shape {tuple(v.shape)}, the site's unconstrained shape is "
                                         f"{tuple(shape)}")
                    parts.append(v.reshape(-1))
                elif default is not None:
                    parts.append(torch.as_tensor(default, dtype=torch.float32).reshape(-1)[o:o + n])
                else:
                    raise ValueError(f"{type(self).__name__}: parameter {key!r} is missing")
                o += n
            dev = next((p.device for p in parts if p.device.type != "cpu"), torch.device("cpu"))
            return torch.cat([p.to(dev) for p in parts])

        loc, scale = get(0, default_loc), get(1, default_scale)
        if not bool((scale > 0).all()):
            raise ValueError(f"{type(self).__name__}: every scale must be positive")
        return loc, scale.to(loc.device)

    def _constrained(self, flat):
        pot = self._pot()
        return pot.constrain(pot.unflatten(flat))

    # ------------------------------------------------------------------ the numpyro methods
    def median(self, params):
        """{site: constrained value at the guide's median}: the transform of ``loc``."""
        loc, _ = self._flat(params)
        return self._constrained(loc)

    def quantiles(self, params, quantiles):
        """{site: [len(quantiles), *shape]}: loc + scale * ndtri(q), constrained (every transform here
        is monotone coordinate by coordinate except the simplex's, as in the reference)."""
        loc, scale = self._flat(params)
        q = torch.as_tensor(quantiles, dtype=torch.float32, device=loc.device).reshape(-1)
        return self._constrained(loc[None, :] + scale[None, :] * torch.special.ndtri(q)[:, None])

    def sample_posterior(self, rng_key, params, sample_shape=()):
        """{site: [*sample_shape, *shape]} constrained draws from the fitted guide, drawn on the device
        (nmx_svi_draw, event NMX_EV_GUIDE: sample s is the normals of (seed, s, 0))."""
        pot = self._pot()
        loc, scale = self._flat(params)
        z = self._draw(key_to_seed(rng_key), loc, scale, int(np.prod(sample_shape, dtype=np.int64)))
        sites = pot.constrain(pot.unflatten(z))
        return {k: v.reshape(tuple(sample_shape) + tuple(v.shape[1:])) for k, v in sites.items()}

    def _draw(self, seed, loc, scale, num_samples, device=None):
        """[num_samples, D] unconstrained draws."""
        if num_samples < 1:
            raise ValueError("sample_posterior: an empty sample_shape product")
        dev = torch.device(device) if device is not None else (loc.device if loc.device.type == "cuda" else
                                                                torch.device("cuda", torch.cuda.current_device()))
        D = self._pot().dim
        ld = (num_samples + 63) // 64 * 64
        loc, scale = loc.to(dev).contiguous(), scale.to(dev).contiguous()
        z = torch.zeros(D, ld, dtype=torch.float32, device=dev)
        cfg = native.SviConfig(dim=D, num_particles=num_samples, ldc=ld, seed=seed)
        with torch.cuda.device(dev):
            check(lib().nmx_svi_draw(cfg, ptr(loc), ptr(scale), native.SVI_EVENT_GUIDE, 0, 0, ptr(z), None,
                                     native.stream_ptr()), "nmx_svi_draw")
        return z[:, :num_samples].t().contiguous()


class AutoNormal(AutoGuide):
    """numpyro/infer/autoguide.py AutoNormal: an independent normal per unconstrained coordinate,
    parameters named per site."""

    def __init__(self, model, *, prefix="auto", init_loc_fn=None, init_scale=0.1, create_plates=None):
        if create_plates is not None:
            raise NotImplementedError("AutoNormal: create_plates (data subsampling) is not supported")
        super().__init__(model, prefix=prefix, init_loc_fn=init_loc_fn, init_scale=init_scale)


class AutoDiagonalNormal(AutoGuide):
    """numpyro/infer/autoguide.py AutoDiagonalNormal: the same guide over the flattened latent
    vector, parameters ``auto_loc`` / ``auto_scale`` of shape [D]."""

    flat_names = True


def _refused(name, reason):
    def init(self, *args, **kwargs):
        raise NotImplementedError(f"{name} is not implemented: {reason}")

    return type(name, (), {"__init__": init, "__doc__": f"Refused: {reason}"})


AutoDelta = _refused(
    "AutoDelta", "a MAP estimate in constrained space needs a potential without the Jacobian of the support "
    "transforms, which Potential does not expose (U(z) includes log|J|); the device guides are AutoNormal and "
    "AutoDiagonalNormal")
AutoLaplaceApproximation = _refused(
    "AutoLaplaceApproximation", "it needs the Hessian of the potential, and the potentials give U and dU/dz only")
AutoMultivariateNormal = _refused(
    "AutoMultivariateNormal", "the device step optimises a diagonal scale; a full Cholesky factor is not implemented")
AutoLowRankMultivariateNormal = _refused(
    "AutoLowRankMultivariateNormal", "the device step optimises a diagonal scale; a low-rank factor is not implemented")

__all__ = ["AutoGuide", "AutoNormal", "AutoDiagonalNormal", "AutoDelta", "AutoLaplaceApproximation",
           "AutoMultivariateNormal", "AutoLowRankMultivariateNormal"]
