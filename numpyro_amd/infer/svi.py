"""numpyro.infer.SVI for the MI355X engine: stochastic variational inference with a mean-field
normal autoguide, the ELBO particles evaluated by the model's potential kernel and everything else
of a step -- the reduction of dU/dz over the particles, the optimiser, the next particles and the
loss -- by one further kernel (csrc/svi.hip; include/numpyro_amd.h states the arithmetic,
numpyro_amd/svi_host.py restates it in NumPy).

The guide lives in unconstrained space: q(z) = N(loc, diag(scale^2)), scale = softplus(rho).  A
reparameterised particle z_p = loc + scale * eps_p is one position of a batched potential launch
(``Potential.evaluate`` gives U(z_p) and dU/dz, the Jacobians of the support transforms included),
so every model NUTS can sample, SVI can fit.

The loss is ``mean_p U(z_p) - sum_d log scale_d - D / 2 (1 + log 2 pi)``: the negative ELBO with the
guide's entropy in closed form.  The reference's ``Trace_ELBO`` samples ``log q(z_p)`` instead; the
two have the same expectation and the same gradient -- the sampled form carries an extra
``-eps^2 / 2`` per coordinate, which holds no parameter and only adds noise to the reported loss.

Randomness is the engine's Philox stream: the noise of step t, particle p is a function of (seed,
p, t) alone (event NMX_EV_SVI), so two runs with one seed are bitwise equal and ``run(n)`` equals n
``update`` calls.  The initial ``loc`` is the engine's ``init_to_uniform(radius=2)`` draw of chain 0,
attempt 0.

Not supported, each refused by name: hand-written guides and ``param`` sites, the guides other than
AutoNormal / AutoDiagonalNormal, losses other than Trace_ELBO, optimisers other than Adam / SGD,
data subsampling, sharding the particles over devices, and ``potential_fn`` targets.
"""
from __future__ import annotations

import collections

import numpy as np
import torch

from .. import native, optim as _optim, svi_host
from ..native import check, lib, ptr
from ..potentials import FusedModel, Potential
from ..random import key_to_seed
from .autoguide import AutoGuide

SVIRunResult = collections.namedtuple("SVIRunResult", ["params", "state", "losses"])


class Trace_ELBO:
    """numpyro/infer/elbo.py Trace_ELBO: ``num_particles`` reparameterised particles per step, all in
    one potential launch.  The guide's entropy is taken in closed form (module docstring)."""

    def __init__(self, num_particles=1, vectorize_particles=True):
        if int(num_particles) < 1:
            raise ValueError(f"Trace_ELBO: num_particles = {num_particles}")
        self.num_particles = int(num_particles)


def _refused_loss(name):
    def init(self, *args, **kwargs):
        raise NotImplementedError(f"{name} is not implemented: the device SVI step estimates Trace_ELBO with a "
                                  "closed-form entropy of the mean-field normal guide")

    return type(name, (), {"__init__": init})


TraceMeanField_ELBO = _refused_loss("TraceMeanField_ELBO")
TraceGraph_ELBO = _refused_loss("TraceGraph_ELBO")
TraceEnum_ELBO = _refused_loss("TraceEnum_ELBO")
RenyiELBO = _refused_loss("RenyiELBO")


class SVIState:
    """The device state of a fit: the two parameter buffers ``par`` [2][NMX_SVI_ROWS][D] (``cur``
    indexes the copy of step ``t``), the particles ``z`` [D][ldc] of step ``t`` with their noise
    ``eps``, and the potential's outputs ``grad`` [D][ldc] and ``pe`` [ldc].  ``SVI.update`` advances
    the state it is given in place and returns it, as a donated buffer would be."""

    def __init__(self, potential, cfg, par, z, eps, grad, pe, seed, device):
        self.potential, self.cfg, self.par, self.z, self.eps, self.grad, self.pe = potential, cfg, par, z, eps, grad, pe
        self.seed, self.device = seed, device
        self.cur, self.t = 0, 0
        self.eval_batch = native.EvalBatch(z=ptr(z), grad=ptr(grad), pe=ptr(pe), num_chains=cfg.num_particles,
                                           ldc=cfg.ldc)

    def row(self, name):
        """Row ``name`` (native.SVI_ROW_NAMES: loc, rho, scale, m_loc, ...) of the current parameters."""
        return self.par[self.cur, native.SVI_ROW_NAMES.index(name)]

    loc = property(lambda self: self.row("loc"))
    rho = property(lambda self: self.row("rho"))
    scale = property(lambda self: self.row("scale"))


def _init_uniform(seed, dim, device, radius=2.0):
    """The engine's init_to_uniform draw of chain 0, attempt 0 (csrc/nuts.hip k_nuts_init_draw):
    (2 radius) u01(word) - radius over the Philox blocks (seed, 0, 0, NMX_EV_INIT, block, 0)."""
    nblk = (dim + 3) // 4
    ck = np.zeros((nblk, 6), np.uint32)
    ck[:, 2] = (5 << 24) | np.arange(nblk)  # NMX_EV_INIT
    ck[:, 4], ck[:, 5] = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    d_ck = torch.from_numpy(ck.view(np.int32)).to(device)
    out = torch.zeros(nblk, 4, dtype=torch.int32, device=device)
    check(lib().nmx_selftest_philox(ptr(d_ck), ptr(out), nblk, native.stream_ptr()), "nmx_selftest_philox")
    words = out.cpu().numpy().view(np.uint32).reshape(-1)[:dim]
    u = (words >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return np.float32(2.0 * radius) * u - np.float32(radius)


class SVI:
    """numpyro/infer/svi.py SVI(model, guide, optim, loss): ``init`` / ``update`` / ``evaluate`` /
    ``get_params`` / ``run`` with the reference's call shapes.  The model's data is bound by ``init``
    (or ``run``): the arguments ``update`` and ``evaluate`` take are accepted for the call shape and
    must be the ones the state was initialised with (there is no data subsampling)."""

    def __init__(self, model, guide, optim, loss, **static_kwargs):
        if not isinstance(guide, AutoGuide):
            what = getattr(guide, "__name__", type(guide).__name__)
            raise NotImplementedError(
                f"SVI: the guide {what!r} is not an autoguide of this package; hand-written guide functions (and "
                "`param` sites) are not supported -- pass autoguide.AutoNormal(model) or "
                "autoguide.AutoDiagonalNormal(model)")
        if not isinstance(loss, Trace_ELBO):
            raise NotImplementedError(f"SVI: the loss {type(loss).__name__!r} is not supported; pass Trace_ELBO()")
        if guide.model is not model:
            raise ValueError("SVI: the guide was built for another model")
        if not (callable(model) or isinstance(model, (FusedModel, Potential))):
            raise NotImplementedError("SVI: the model must be a model function, a FusedModel or a Potential "
                                      "(potential_fn targets written in torch are not supported)")
        self.model, self.guide, self.loss = model, guide, loss
        self.optim = _optim.resolve(optim)
        self.static_kwargs = static_kwargs

    # ------------------------------------------------------------------ init
    def _potential(self, args, kwargs):
        if isinstance(self.model, Potential):
            return self.model
        from .hmc import NUTS

        kwargs = {**self.static_kwargs, **kwargs}
        if kwargs.get("subsample_size") is not None:
            raise NotImplementedError("SVI: data subsampling (subsample_size) is not supported")
        return NUTS(self.model).potential(args, kwargs)  # the fused kernel, else the program kernel

    def initial_params(self, loc, init_params=None):
        """(loc, rho, scale) [D] float32 that ``init`` uploads: the drawn ``loc`` and rho =
        softplus^-1(init_scale), each overridden by ``init_params`` (in either guide's naming; what it
        leaves out keeps the default).  A given scale is kept as given, beside rho = softplus^-1 of it."""
        loc = np.asarray(loc, np.float32)
        rho, scale = svi_host.init_rho_scale(self.guide.init_scale, loc.size, np.float32)
        if init_params:
            loc_t, scale_t = self.guide._flat(init_params, loc, scale)
            loc = loc_t.cpu().numpy().astype(np.float32)
            given = scale_t.cpu().numpy().astype(np.float32)
            rho = np.where(given != scale, svi_host.softplus_inv(given.astype(np.float64)).astype(np.float32), rho)
            scale = given
        return loc, rho, scale

    def init(self, rng_key, *args, init_params=None, device=None, **kwargs):
        seed = key_to_seed(rng_key)
        pot = self._potential(args, kwargs)
        self.guide._setup(pot)
        if device is None:
            if not torch.cuda.is_available():
                raise native.NativeError("SVI needs a GPU: the step runs as HIP kernels and has no host path")
            device = torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        D, P = pot.dim, self.loss.num_particles
        ldc = (P + 63) // 64 * 64
        o = self.optim
        cfg = native.SviConfig(dim=D, num_particles=P, ldc=ldc, optimizer=o.code, step_size=o.step_size, b1=o.b1,
                               b2=o.b2, eps=o.eps, seed=seed)
        with torch.cuda.device(device):
            pot.bind(P, ldc, device)
            loc, rho, scale = self.initial_params(_init_uniform(seed, D, device), init_params)
            par = torch.zeros(2, native.SVI_ROWS, D, dtype=torch.float32, device=device)
            par[0, :3] = torch.from_numpy(np.stack([loc, rho, scale])).to(device)
            z, eps, grad = (torch.zeros(D, ldc, dtype=torch.float32, device=device) for _ in range(3))
            pe = torch.zeros(ldc, dtype=torch.float32, device=device)
            state = SVIState(pot, cfg, par, z, eps, grad, pe, seed, device)
            check(lib().nmx_svi_draw(cfg, ptr(state.loc), ptr(state.scale), native.SVI_EVENT_STEP, 0, 0, ptr(z),
                                     ptr(eps), native.stream_ptr()), "nmx_svi_draw")
        return state

    # ------------------------------------------------------------------ steps
    def _step(self, state, loss_ptr, stream):
        state.potential.evaluate(state.eval_batch, stream)
        c = state.cur
        check(lib().nmx_svi_step(state.cfg, state.t, ptr(state.par[c]), ptr(state.par[1 - c]), ptr(state.grad),
                                 ptr(state.pe), ptr(state.z), ptr(state.eps), loss_ptr, stream), "nmx_svi_step")
        state.cur, state.t = 1 - c, state.t + 1

    def update(self, state, *args, **kwargs):
        """One step: (state, loss), the loss a 0-d device tensor of the parameters before the step."""
        with torch.cuda.device(state.device):
            loss = torch.empty(1, dtype=torch.float32, device=state.device)
            self._step(state, ptr(loss), native.stream_ptr())
        return state, loss[0]

    stable_update = update

    def evaluate(self, state, *args, **kwargs):
        """The loss at the state's parameters and particles (the one the next ``update`` returns); the
        parameters, the particles and the step counter are left as they are."""
        with torch.cuda.device(state.device):
            loss = torch.empty(1, dtype=torch.float32, device=state.device)
            stream = native.stream_ptr()
            state.potential.evaluate(state.eval_batch, stream)
            check(lib().nmx_svi_loss(state.cfg, ptr(state.par[state.cur]), ptr(state.pe), ptr(loss), stream),
                  "nmx_svi_loss")
        return loss[0]

    def get_params(self, state):
        """The guide's parameters (copies, on the device), ``scale`` constrained."""
        return self.guide._params(state.loc.clone(), state.scale.clone())

    def run(self, rng_key, num_steps, *args, progress_bar=False, stable_update=False, init_state=None,
            init_params=None, **kwargs):
        """``num_steps`` steps enqueued back to back without a host synchronisation; ``losses`` is a
        [num_steps] device tensor, entry t written by step t's launch."""
        num_steps = int(num_steps)
        if num_steps < 1:
            raise ValueError("num_steps must be a positive integer.")
        state = init_state if init_state is not None else self.init(rng_key, *args, init_params=init_params, **kwargs)
        with torch.cuda.device(state.device):
            losses = torch.empty(num_steps, dtype=torch.float32, device=state.device)
            stream = native.stream_ptr()
            base = ptr(losses)
            for i in range(num_steps):
                self._step(state, base + 4 * i, stream)
        return SVIRunResult(self.get_params(state), state, losses)
