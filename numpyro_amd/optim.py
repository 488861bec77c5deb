"""numpyro.optim for the device SVI step: the optimisers are descriptions (a code and its
hyper-parameters) that ``infer.SVI`` hands to the step kernel (csrc/svi.hip), which applies them
to the guide's ``loc`` and ``rho`` on the device.  ``numpyro_amd.svi_host`` restates both.

  Adam (jax.example_libraries.optimizers.adam, numpyro/optim.py Adam), step t = 0, 1, ...:
      m = (1 - b1) g + b1 m;  v = (1 - b2) g^2 + b2 v
      x -= step_size * (m / (1 - b1^(t+1))) / (sqrt(v / (1 - b2^(t+1))) + eps)
  SGD:  x -= step_size * g

Every other optimiser of numpyro.optim is refused by name.
"""
from __future__ import annotations

from . import native


class _Optimizer:
    code = None

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{k}={v!r}' for k, v in self.__dict__.items())})"


def _step_size(step_size, who):
    if callable(step_size):
        raise NotImplementedError(f"optim.{who}: a step-size schedule (a callable step_size) is not supported; "
                                  "pass a number")
    step_size = float(step_size)
    if not step_size > 0.0:
        raise ValueError(f"optim.{who}: step_size = {step_size}, need a positive number")
    return step_size


class Adam(_Optimizer):
    code = native.SVI_ADAM

    def __init__(self, step_size, b1=0.9, b2=0.999, eps=1e-8):
        self.step_size = _step_size(step_size, "Adam")
        self.b1, self.b2, self.eps = float(b1), float(b2), float(eps)
        if not (0.0 <= self.b1 < 1.0 and 0.0 <= self.b2 < 1.0):
            raise ValueError(f"optim.Adam: b1 = {b1}, b2 = {b2} outside [0, 1)")


class SGD(_Optimizer):
    code = native.SVI_SGD

    def __init__(self, step_size):
        self.step_size = _step_size(step_size, "SGD")
        self.b1 = self.b2 = self.eps = 0.0


def _refused(name):
    def init(self, *args, **kwargs):
        raise NotImplementedError(f"optim.{name} is not implemented: the device SVI step applies Adam or SGD "
                                  "(numpyro_amd.optim.Adam, numpyro_amd.optim.SGD)")

    return type(name, (_Optimizer,), {"__init__": init})


Adagrad = _refused("Adagrad")
ClippedAdam = _refused("ClippedAdam")
Minimize = _refused("Minimize")
Momentum = _refused("Momentum")
RMSProp = _refused("RMSProp")
RMSPropMomentum = _refused("RMSPropMomentum")
SM3 = _refused("SM3")


def resolve(optim):
    """The Adam / SGD description of ``optim``, or a refusal that names what was given."""
    if isinstance(optim, (Adam, SGD)):
        return optim
    name = getattr(optim, "__name__", None) or type(optim).__name__
    raise NotImplementedError(f"SVI: unknown optimiser {name!r} ({optim!r}); pass numpyro_amd.optim.Adam(step_size) "
                              "or numpyro_amd.optim.SGD(step_size)")
