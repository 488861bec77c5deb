"""Distribution descriptors of the hot path (numpyro/distributions), for models written against
numpyro's API and run through the model front end (numpyro_amd/frontend.py).

They hold their parameters (numbers, arrays, or symbolic values of latent sites while a model
is traced) and shapes; the arithmetic runs in the fused kernels the front end maps a traced
model onto, or in the program the front end lowers it to (numpyro_amd/program.py expands each
log_prob into primitive operations), so there is no log_prob here.  Names and signatures follow numpyro:
Normal (continuous.py:2171), HalfCauchy (:700), Exponential (:455), Gamma (:490), StudentT
(:2344), Bernoulli / BernoulliLogits (discrete.py:108-139), GaussianRandomWalk (continuous.py:
658), MultivariateNormal (:1487), HalfNormal (:829), LogNormal (:1166), Cauchy (:217), Poisson
(discrete.py:748; observed sites only), Uniform (continuous.py:2431), Beta (:165), Pareto (:2230),
BinomialProbs / BinomialLogits / Binomial (discrete.py:172, :243, :298; observed sites only),
Dirichlet (continuous.py), CategoricalProbs / CategoricalLogits / Categorical (discrete.py) and
MixtureSameFamily (mixtures.py), the last two kinds as observed sites only; the count likelihoods
GammaPoisson, NegativeBinomialProbs / NegativeBinomialLogits / NegativeBinomial, NegativeBinomial2,
BetaBinomial (conjugate.py), GeometricProbs / GeometricLogits / Geometric, ZeroInflatedProbs /
ZeroInflatedLogits / ZeroInflatedDistribution, ZeroInflatedPoisson (discrete.py) and
ZeroInflatedNegativeBinomial2 (conjugate.py), observed sites only; MultivariateNormal keeps a
symbolic covariance_matrix or scale_tril for the program compiler;
``.to_event`` / ``.expand`` (distribution.py:377-420).
"""
from __future__ import annotations

import numpy as np

from .jnp import Sym, shape_of


def _bshape(*params):
    shapes = [shape_of(p) for p in params if p is not None]
    return tuple(np.broadcast_shapes(*shapes)) if shapes else ()


class Distribution:
    support = "real"

    def __init__(self, batch_shape=(), event_shape=()):
        self.batch_shape = tuple(batch_shape)
        self.event_shape = tuple(event_shape)

    @property
    def shape(self):
        return self.batch_shape + self.event_shape

    def to_event(self, reinterpreted_batch_ndims=None):
        n = len(self.batch_shape) if reinterpreted_batch_ndims is None else int(reinterpreted_batch_ndims)
        return Independent(self, n)

    def expand(self, batch_shape):
        return ExpandedDistribution(self, tuple(batch_shape))

    def params(self):
        return {}

    def __repr__(self):
        return f"{type(self).__name__}(batch_shape={self.batch_shape}, event_shape={self.event_shape})"


class Independent(Distribution):
    def __init__(self, base, reinterpreted_batch_ndims):
        n = reinterpreted_batch_ndims
        bs = base.batch_shape
        super().__init__(bs[:len(bs) - n], bs[len(bs) - n:] + base.event_shape)
        self.base_dist = base
        self.support = base.support

    def params(self):
        return self.base_dist.params()


class ExpandedDistribution(Distribution):
    def __init__(self, base, batch_shape):
        super().__init__(batch_shape, base.event_shape)
        self.base_dist = base
        self.support = base.support

    def params(self):
        return self.base_dist.params()


class Normal(Distribution):
    def __init__(self, loc=0.0, scale=1.0):
        super().__init__(_bshape(loc, scale))
        self.loc, self.scale = loc, scale

    def params(self):
        return {"loc": self.loc, "scale": self.scale}


class HalfCauchy(Distribution):
    support = "positive"

    def __init__(self, scale=1.0):
        super().__init__(_bshape(scale))
        self.scale = scale

    def params(self):
        return {"scale": self.scale}


class HalfNormal(Distribution):
    support = "positive"

    def __init__(self, scale=1.0):
        super().__init__(_bshape(scale))
        self.scale = scale

    def params(self):
        return {"scale": self.scale}


class LogNormal(Distribution):
    support = "positive"

    def __init__(self, loc=0.0, scale=1.0):
        super().__init__(_bshape(loc, scale))
        self.loc, self.scale = loc, scale

    def params(self):
        return {"loc": self.loc, "scale": self.scale}


class Cauchy(Distribution):
    def __init__(self, loc=0.0, scale=1.0):
        super().__init__(_bshape(loc, scale))
        self.loc, self.scale = loc, scale

    def params(self):
        return {"loc": self.loc, "scale": self.scale}


class Poisson(Distribution):
    """Observed sites only (a discrete latent cannot be sampled by HMC)."""

    support = "nonnegative_integer"

    def __init__(self, rate):
        super().__init__(_bshape(rate))
        self.rate = rate

    def params(self):
        return {"rate": self.rate}


class Exponential(Distribution):
    support = "positive"

    def __init__(self, rate=1.0):
        super().__init__(_bshape(rate))
        self.rate = rate

    def params(self):
        return {"rate": self.rate}


class Gamma(Distribution):
    support = "positive"

    def __init__(self, concentration, rate=1.0):
        super().__init__(_bshape(concentration, rate))
        self.concentration, self.rate = concentration, rate

    def params(self):
        return {"concentration": self.concentration, "rate": self.rate}


class StudentT(Distribution):
    def __init__(self, df, loc=0.0, scale=1.0):
        super().__init__(_bshape(df, loc, scale))
        self.df, self.loc, self.scale = df, loc, scale

    def params(self):
        return {"df": self.df, "loc": self.loc, "scale": self.scale}


class BernoulliLogits(Distribution):
    support = "boolean"

    def __init__(self, logits):
        super().__init__(_bshape(logits))
        self.logits = logits

    def params(self):
        return {"logits": self.logits}


class BernoulliProbs(Distribution):
    support = "boolean"

    def __init__(self, probs):
        super().__init__(_bshape(probs))
        self.probs = probs

    def params(self):
        return {"probs": self.probs}


def Bernoulli(probs=None, logits=None):
    """numpyro/distributions/discrete.py:142-151 dispatch on probs / logits."""
    if (probs is None) == (logits is None):
        raise ValueError("One of `probs` or `logits` must be specified.")
    return BernoulliLogits(logits) if logits is not None else BernoulliProbs(probs)


class Uniform(Distribution):
    """``support`` is "interval"; the bounds are ``low`` and ``high``."""

    support = "interval"

    def __init__(self, low=0.0, high=1.0):
        super().__init__(_bshape(low, high))
        self.low, self.high = low, high

    def params(self):
        return {"low": self.low, "high": self.high}


class Beta(Distribution):
    support = "unit_interval"

    def __init__(self, concentration1, concentration0):
        super().__init__(_bshape(concentration1, concentration0))
        self.concentration1, self.concentration0 = concentration1, concentration0

    def params(self):
        return {"concentration1": self.concentration1, "concentration0": self.concentration0}


class Pareto(Distribution):
    """``support`` is "greater_than"; the lower bound is ``scale``."""

    support = "greater_than"

    def __init__(self, scale, alpha):
        super().__init__(_bshape(scale, alpha))
        self.scale, self.alpha = scale, alpha

    def params(self):
        return {"scale": self.scale, "alpha": self.alpha}


class BinomialProbs(Distribution):
    """Observed sites only (a discrete latent cannot be sampled by HMC)."""

    support = "integer_interval"

    def __init__(self, probs, total_count=1):
        super().__init__(_bshape(probs, total_count))
        self.probs, self.total_count = probs, total_count

    def params(self):
        return {"probs": self.probs, "total_count": self.total_count}


class BinomialLogits(Distribution):
    """Observed sites only (a discrete latent cannot be sampled by HMC)."""

    support = "integer_interval"

    def __init__(self, logits, total_count=1):
        super().__init__(_bshape(logits, total_count))
        self.logits, self.total_count = logits, total_count

    def params(self):
        return {"logits": self.logits, "total_count": self.total_count}


def Binomial(total_count=1, probs=None, logits=None):
    """numpyro/distributions/discrete.py:298-303 dispatch on probs / logits."""
    if (probs is None) == (logits is None):
        raise ValueError("One of `probs` or `logits` must be specified.")
    return BinomialLogits(logits, total_count) if logits is not None else BinomialProbs(probs, total_count)


def _one_of(**kw):
    if sum(v is not None for v in kw.values()) != 1:
        raise ValueError("One of " + " or ".join(f"`{k}`" for k in kw) + " must be specified.")


class GammaPoisson(Distribution):
    """numpyro/distributions/conjugate.py:177 GammaPoisson: a Poisson whose rate is
    Gamma(concentration, rate).  This and the count likelihoods below are observed sites only (a
    discrete latent cannot be sampled by HMC); every parameter may depend on latent sites."""

    support = "nonnegative_integer"

    def __init__(self, concentration, rate=1.0):
        super().__init__(_bshape(concentration, rate))
        self.concentration, self.rate = concentration, rate

    def params(self):
        return {"concentration": self.concentration, "rate": self.rate}


class NegativeBinomialProbs(Distribution):
    """conjugate.py:240: GammaPoisson(total_count, 1 / probs - 1); probs is the chance that counts."""

    support = "nonnegative_integer"

    def __init__(self, total_count, probs):
        super().__init__(_bshape(total_count, probs))
        self.total_count, self.probs = total_count, probs

    def params(self):
        return {"total_count": self.total_count, "probs": self.probs}


class NegativeBinomialLogits(Distribution):
    """conjugate.py:254: GammaPoisson(total_count, exp(-logits))."""

    support = "nonnegative_integer"

    def __init__(self, total_count, logits):
        super().__init__(_bshape(total_count, logits))
        self.total_count, self.logits = total_count, logits

    def params(self):
        return {"total_count": self.total_count, "logits": self.logits}


def NegativeBinomial(total_count, probs=None, logits=None):
    """conjugate.py:231 dispatch on probs / logits."""
    if probs is not None:
        return NegativeBinomialProbs(total_count, probs)
    if logits is not None:
        return NegativeBinomialLogits(total_count, logits)
    raise ValueError("One of `probs` or `logits` must be specified.")


class NegativeBinomial2(Distribution):
    """conjugate.py:276: GammaPoisson(concentration, concentration / mean)."""

    support = "nonnegative_integer"

    def __init__(self, mean, concentration):
        super().__init__(_bshape(mean, concentration))
        self.mean, self.concentration = mean, concentration

    def params(self):
        return {"mean": self.mean, "concentration": self.concentration}


class BetaBinomial(Distribution):
    """conjugate.py:26: a Binomial whose probability is Beta(concentration1, concentration0);
    ``total_count`` is data, as Binomial's."""

    support = "integer_interval"

    def __init__(self, concentration1, concentration0, total_count=1):
        super().__init__(_bshape(concentration1, concentration0, total_count))
        self.concentration1, self.concentration0, self.total_count = concentration1, concentration0, total_count

    def params(self):
        return {"concentration1": self.concentration1, "concentration0": self.concentration0,
                "total_count": self.total_count}


class GeometricProbs(Distribution):
    """discrete.py:868: failures before the first success, pmf (1 - probs)^k probs."""

    support = "nonnegative_integer"

    def __init__(self, probs):
        super().__init__(_bshape(probs))
        self.probs = probs

    def params(self):
        return {"probs": self.probs}


class GeometricLogits(Distribution):
    """discrete.py:909."""

    support = "nonnegative_integer"

    def __init__(self, logits):
        super().__init__(_bshape(logits))
        self.logits = logits

    def params(self):
        return {"logits": self.logits}


def Geometric(probs=None, logits=None):
    """discrete.py:951 dispatch on probs / logits."""
    _one_of(probs=probs, logits=logits)
    return GeometricProbs(probs) if probs is not None else GeometricLogits(logits)


class ZeroInflatedProbs(Distribution):
    """discrete.py:758: with probability ``gate`` a zero, else a draw of ``base_dist`` (a count
    likelihood: Poisson, the negative binomial family, Geometric, Binomial or BetaBinomial)."""

    def __init__(self, base_dist, gate):
        if base_dist.event_shape:
            raise ValueError(f"ZeroInflatedProbs expected empty base_dist.event_shape but got {base_dist.event_shape}")
        super().__init__(tuple(np.broadcast_shapes(shape_of(gate), base_dist.batch_shape)))
        self.base_dist, self.gate = base_dist, gate
        self.support = base_dist.support

    def params(self):
        return {"base_dist": self.base_dist, "gate": self.gate}


class ZeroInflatedLogits(Distribution):
    """discrete.py:814: ZeroInflatedProbs with gate = sigmoid(gate_logits)."""

    def __init__(self, base_dist, gate_logits):
        if base_dist.event_shape:
            raise ValueError(f"ZeroInflatedLogits expected empty base_dist.event_shape but got {base_dist.event_shape}")
        super().__init__(tuple(np.broadcast_shapes(shape_of(gate_logits), base_dist.batch_shape)))
        self.base_dist, self.gate_logits = base_dist, gate_logits
        self.support = base_dist.support

    def params(self):
        return {"base_dist": self.base_dist, "gate_logits": self.gate_logits}


def ZeroInflatedDistribution(base_dist, *, gate=None, gate_logits=None):
    """discrete.py:832 dispatch on gate / gate_logits."""
    _one_of(gate=gate, gate_logits=gate_logits)
    return ZeroInflatedProbs(base_dist, gate) if gate is not None else ZeroInflatedLogits(base_dist, gate_logits)


class ZeroInflatedPoisson(ZeroInflatedProbs):
    """discrete.py:849 (the gate comes first, as there)."""

    def __init__(self, gate, rate=1.0):
        super().__init__(Poisson(rate), gate)
        self.rate = rate


def ZeroInflatedNegativeBinomial2(mean, concentration, *, gate=None, gate_logits=None):
    """conjugate.py:293."""
    return ZeroInflatedDistribution(NegativeBinomial2(mean, concentration), gate=gate, gate_logits=gate_logits)


class Dirichlet(Distribution):
    """numpyro/distributions/continuous.py Dirichlet: event shape (K,), support the simplex.  The
    program compiler takes a concentration of rank 1 (constant or symbolic)."""

    support = "simplex"

    def __init__(self, concentration):
        shape = shape_of(concentration)
        if len(shape) < 1:
            raise ValueError("`concentration` parameter must be at least one-dimensional.")
        super().__init__(shape[:-1], shape[-1:])
        self.concentration = concentration

    def params(self):
        return {"concentration": self.concentration}


class CategoricalProbs(Distribution):
    """Observed sites only (a discrete latent cannot be sampled by HMC).  The last axis of
    ``probs`` is the category axis (discrete.py CategoricalProbs)."""

    support = "integer_interval"

    def __init__(self, probs):
        shape = shape_of(probs)
        if len(shape) < 1:
            raise ValueError("`probs` parameter must be at least one-dimensional.")
        super().__init__(shape[:-1])
        self.probs = probs

    def params(self):
        return {"probs": self.probs}


class CategoricalLogits(Distribution):
    """Observed sites only; the last axis of ``logits`` is the category axis."""

    support = "integer_interval"

    def __init__(self, logits):
        shape = shape_of(logits)
        if len(shape) < 1:
            raise ValueError("`logits` parameter must be at least one-dimensional.")
        super().__init__(shape[:-1])
        self.logits = logits

    def params(self):
        return {"logits": self.logits}


def Categorical(probs=None, logits=None):
    """numpyro/distributions/discrete.py Categorical: dispatch on probs / logits."""
    if (probs is None) == (logits is None):
        raise ValueError("One of `probs` or `logits` must be specified.")
    return CategoricalLogits(logits) if logits is not None else CategoricalProbs(probs)


class MixtureSameFamily(Distribution):
    """numpyro/distributions/mixtures.py MixtureSameFamily: the component distribution's last
    batch axis is the mixture axis.  Observed sites only: the program compiler marginalises the
    component index (log-sum-exp over the components)."""

    def __init__(self, mixing_distribution, component_distribution):
        cb = tuple(component_distribution.batch_shape)
        super().__init__(cb[:-1], component_distribution.event_shape)
        self.mixing_distribution = mixing_distribution
        self.component_distribution = component_distribution
        self.support = component_distribution.support

    def params(self):
        return {"mixing_distribution": self.mixing_distribution,
                "component_distribution": self.component_distribution}


class GaussianRandomWalk(Distribution):
    def __init__(self, scale=1.0, num_steps=1):
        super().__init__(_bshape(scale), (int(num_steps),))
        self.scale, self.num_steps = scale, int(num_steps)

    def params(self):
        return {"scale": self.scale, "num_steps": self.num_steps}


class MultivariateNormal(Distribution):
    """numpyro/distributions/continuous.py MultivariateNormal.  A constant ``scale_tril`` is kept as
    the covariance it stands for; a symbolic ``covariance_matrix`` or ``scale_tril`` (an expression
    of latent sites) is kept as it is, for the program compiler (``matrix_shape`` is its full
    shape: batch dimensions are the compiler's to refuse)."""

    def __init__(self, loc=0.0, covariance_matrix=None, precision_matrix=None, scale_tril=None):
        self.scale_tril = None
        if scale_tril is not None and isinstance(scale_tril, Sym):
            self.scale_tril = scale_tril
        elif scale_tril is not None:
            st = np.asarray(scale_tril, np.float64)
            covariance_matrix = st @ np.swapaxes(st, -1, -2)
        mats = [m for m in (covariance_matrix, precision_matrix, self.scale_tril) if m is not None]
        if len(mats) != 1:
            raise ValueError("One of `covariance_matrix`, `precision_matrix`, `scale_tril` must be specified.")
        self.matrix_shape = tuple(shape_of(mats[0]))
        d = self.matrix_shape[-1]
        super().__init__((), (d,))
        self.loc = loc
        self.covariance_matrix, self.precision_matrix = covariance_matrix, precision_matrix

    def params(self):
        return {"loc": self.loc, "covariance_matrix": self.covariance_matrix,
                "precision_matrix": self.precision_matrix, "scale_tril": self.scale_tril}
