"""numpyro.infer drop-in surface for the MI355X engine (MCMC, NUTS, HMC, SVI)."""
from . import autoguide  # noqa: F401
from .hmc import HMC, NUTS, HMCAdaptState, HMCState, MCMCKernel, init_to_uniform, pooled  # noqa: F401
from .loglik import log_likelihood, loo, pointwise_predictive  # noqa: F401
from .mcmc import MCMC, shard_chains  # noqa: F401
from .predictive import Predictive  # noqa: F401
from .svi import (SVI, RenyiELBO, SVIRunResult, SVIState, Trace_ELBO, TraceEnum_ELBO,  # noqa: F401
                  TraceGraph_ELBO, TraceMeanField_ELBO)

__all__ = ["HMC", "NUTS", "MCMC", "MCMCKernel", "HMCState", "HMCAdaptState", "init_to_uniform", "Predictive", "pooled",
           "log_likelihood", "pointwise_predictive", "loo", "SVI", "SVIState", "SVIRunResult", "Trace_ELBO",
           "autoguide"]
