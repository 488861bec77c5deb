"""The SVI step of csrc/svi.hip restated in NumPy: the particle draw, the reparameterised ELBO
gradient of a mean-field normal guide, Adam / SGD and the loss (include/numpyro_amd.h "stochastic
variational inference" states the arithmetic).

``HostSVI`` takes any ``pe_grad(Z [P, D]) -> (U [P], dU/dz [P, D])`` and the device's seed.  With
``dtype=np.float64`` it is the oracle the device is tested against; with ``dtype=np.float32`` every
operation (the Box-Muller normals included) rounds to float32, in NumPy's order of summation and
not the kernel's: a second float32 implementation, whose distance from the float64 one is the
yardstick the device tolerances are taken from.

The Philox block function is an argument (``rng(seed, chain, it, event, idx, sub) -> [..., 4]``
uint32, the signature of ``oracle.philox.rng``): the package holds no NumPy Philox.
"""
from __future__ import annotations

import math

import numpy as np

EV_SVI, EV_GUIDE = 9, 10  # NMX_EV_SVI, NMX_EV_GUIDE (csrc/nmx_common.h)
HALF_LOG_2PI_E = 0.5 * (1.0 + math.log(2.0 * math.pi))


def softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def softplus_inv(y):
    return y + np.log(-np.expm1(-y))


def sigmoid(x):
    return 1 / (1 + np.exp(-x))


def init_rho_scale(init_scale, dim, dtype=np.float64):
    """rho = softplus^-1(init_scale) rounded to ``dtype``, and scale = softplus(rho) of that rounded
    rho (formed in float64, rounded once): what SVI.init uploads."""
    rho = np.full(dim, softplus_inv(np.float64(init_scale))).astype(dtype)
    return rho, softplus(rho.astype(np.float64)).astype(dtype)


def normals(rng, seed, particles, it, event, dim, dtype=np.float64):
    """eps [len(particles), dim]: coordinate d is normal number d % 4 of the block
    rng(seed, p, it, event, d // 4, 0) -- Box-Muller cos and sin of the words (x, y), then of (z, w);
    the uniforms are exact in float32, the rest is computed in ``dtype``."""
    particles = np.asarray(particles, np.uint64).reshape(-1)
    nblk = (dim + 3) // 4
    w = rng(seed, particles[:, None], it, event, np.arange(nblk)[None, :], 0)  # [P, nblk, 4]
    dt = np.dtype(dtype).type
    u = (w >> np.uint32(8)).astype(np.float32)
    out = np.empty(w.shape, dtype)
    for k in (0, 2):
        u1 = ((u[..., k] + np.float32(1.0)) * np.float32(2.0 ** -24)).astype(dtype)  # (0, 1]
        u2 = (u[..., k + 1] * np.float32(2.0 ** -24)).astype(dtype)  # [0, 1)
        rad = np.sqrt(dt(-2.0) * np.log(u1))
        ang = dt(2.0 * math.pi) * u2
        out[..., k], out[..., k + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return out.reshape(len(particles), 4 * nblk)[:, :dim]


class HostSVI:
    """The state is a dict {loc, rho, scale, m_loc, v_loc, m_rho, v_rho: [D]; t: int}."""

    def __init__(self, pe_grad, dim, num_particles, seed, rng, optim, dtype=np.float64):
        self.pe_grad, self.dim, self.P, self.seed, self.rng = pe_grad, int(dim), int(num_particles), int(seed), rng
        self.optim, self.dtype = optim, np.dtype(dtype).type

    def init(self, loc, init_scale=0.1, scale=None):
        D, dt = self.dim, self.dtype
        if scale is None:
            rho, scale = init_rho_scale(init_scale, D, dt)
        else:
            scale = np.broadcast_to(np.asarray(scale, dt), (D,)).copy()
            rho = softplus_inv(scale.astype(np.float64)).astype(dt)
        st = {"loc": np.asarray(loc, dt).reshape(D).copy(), "rho": rho, "scale": scale, "t": 0}
        for k in ("m_loc", "v_loc", "m_rho", "v_rho"):
            st[k] = np.zeros(D, dt)
        return st

    def noise(self, t):
        """eps [P, D] of step t."""
        return normals(self.rng, self.seed, np.arange(self.P), t, EV_SVI, self.dim, self.dtype)

    def loss_at(self, loc, rho, t):
        """The loss as a function of (loc, rho) with the noise of step t held fixed."""
        dt = self.dtype
        loc, scale = np.asarray(loc, dt), softplus(np.asarray(rho, dt))
        U, _ = self.pe_grad(loc[None, :] + scale[None, :] * self.noise(t))
        return self._loss(np.asarray(U, dt), scale)

    def _loss(self, U, scale):
        dt = self.dtype
        return (U.sum(dtype=dt) / dt(self.P) - np.log(scale).sum(dtype=dt)) - dt(self.dim) * dt(HALF_LOG_2PI_E)

    def grads(self, st, Z=None, eps=None):
        """(loss, g_loc, g_rho) at the state; Z and eps [P, D] default to the draw of step st['t']
        (the device tests pass the device's own)."""
        dt = self.dtype
        eps = self.noise(st["t"]) if eps is None else np.asarray(eps, dt)
        Z = (st["loc"][None, :] + st["scale"][None, :] * eps) if Z is None else np.asarray(Z, dt)
        U, G = self.pe_grad(Z)
        U, G = np.asarray(U, dt), np.asarray(G, dt)
        g_loc = G.sum(0, dtype=dt) / dt(self.P)
        g_scale = (G * eps).sum(0, dtype=dt) / dt(self.P) - dt(1.0) / st["scale"]
        return self._loss(U, st["scale"]), g_loc, g_scale * sigmoid(st["rho"])

    def update(self, st, Z=None, eps=None):
        dt, o = self.dtype, self.optim
        loss, g_loc, g_rho = self.grads(st, Z, eps)
        new = dict(st)
        t = st["t"]
        for x, g in (("loc", g_loc), ("rho", g_rho)):
            if type(o).__name__ == "Adam":
                b1, b2 = dt(o.b1), dt(o.b2)
                c1, c2 = dt(1.0 - float(b1) ** (t + 1)), dt(1.0 - float(b2) ** (t + 1))
                m = (dt(1.0) - b1) * g + b1 * st["m_" + x]
                v = (dt(1.0) - b2) * (g * g) + b2 * st["v_" + x]
                new["m_" + x], new["v_" + x] = m, v
                new[x] = st[x] - dt(o.step_size) * (m / c1) / (np.sqrt(v / c2) + dt(o.eps))
            else:
                new[x] = st[x] - dt(o.step_size) * g
        new["scale"] = softplus(new["rho"])
        new["t"] = t + 1
        assert all(np.asarray(v).dtype == np.dtype(dt) for k, v in new.items() if k != "t")
        return new, loss

    def run(self, st, num_steps):
        losses = np.zeros(num_steps, self.dtype)
        for i in range(num_steps):
            st, losses[i] = self.update(st)
        return st, losses
