"""Logistic and Poisson regression after sampling (csrc/predictive_glm.hip): the pointwise
log-likelihood table of obs ~ Bernoulli(logits = X @ W_s) or Poisson(exp(X @ W_s + offset)) and the
Poisson posterior predictive counts, for posterior samples W [S, D], 1 <= D <= 1024.
``GlmPredictive`` holds the data matrix split into the kernel's bf16 planes with the rows' side data,
made once; ``infer.log_likelihood`` / ``pointwise_predictive`` / ``loo`` reach it for a model of
that structure, ``infer.Predictive`` for ``potentials.poisson_regression``."""
from __future__ import annotations

import numpy as np
import torch

from . import native
from .native import check, lib, ptr
from .softmax_predictive import _dev

MAX_FEATURES = 1024


class GlmPredictive:
    """X [N, D] on ``device`` with y [N] (None: draws only) and an offset [N] (None: zero), split once
    for any number of launches; a launch takes up to ``max_samples`` samples (the W scratch of the
    workspace), more are run in chunks."""

    def __init__(self, X, device, family, y=None, offset=None, max_samples=4096):
        if family not in native.GLM_FAMILY:
            raise ValueError(f"family {family!r}: one of {sorted(native.GLM_FAMILY)}")
        self.device, self.family = torch.device(device), native.GLM_FAMILY[family]
        X = _dev(X, self.device, torch.float32)
        if X.dim() != 2 or not 1 <= X.shape[1] <= MAX_FEATURES:
            raise ValueError(f"{family} regression needs data [N, D], 1 <= D <= {MAX_FEATURES} (got {tuple(X.shape)})")
        self.N, self.D = X.shape
        side = [None if v is None else _dev(v, self.device, torch.float32) for v in (y, offset)]
        for name, v in zip(("y", "offset"), side):
            if v is not None and tuple(v.shape) != (self.N,):
                raise ValueError(f"{name} of shape {tuple(v.shape)} for {self.N} rows")
        self.has_y, self.max_samples = y is not None, int(max_samples)
        self.workspace = torch.empty(lib().nmx_glm_predictive_workspace_bytes(self.N, self.D, self.max_samples),
                                     dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().nmx_glm_predictive_pack(ptr(X), ptr(side[0]), ptr(side[1]), self.N, self.D, self.family,
                                                ptr(self.workspace), native.stream_ptr()), "nmx_glm_predictive_pack")

    def _samples(self, W):
        W = _dev(W, self.device, torch.float32)
        if W.dim() != 2 or W.shape[1] != self.D:
            raise ValueError(f"posterior samples of shape {tuple(W.shape[1:])} per draw, the data has {self.D} features")
        return W

    def log_likelihood(self, W, out=None):
        """log p(y_n | W_s) for samples W [S, D]: float32 [S, N], or written into the first S rows and
        N columns of ``out`` (float32, unit column stride)."""
        if not self.has_y:
            raise ValueError("this GlmPredictive was made without y: it serves draws only")
        W = self._samples(W)
        S = W.shape[0]
        if out is None:
            out = torch.empty(S, self.N, dtype=torch.float32, device=self.device)
        if out.dim() != 2 or out.dtype != torch.float32 or out.device != self.device or out.shape[0] < S or \
                out.shape[1] < self.N or (out.shape[1] > 1 and out.stride(1) != 1):
            raise ValueError(f"a table of shape {tuple(out.shape)}, strides {out.stride()}, {out.dtype} on {out.device}: "
                             f"need float32 [>= {S}, >= {self.N}] rows on {self.device}")
        ld = out.stride(0) if out.shape[0] > 1 else out.shape[1]
        with torch.cuda.device(self.device):
            for s0 in range(0, S, self.max_samples):
                m = min(self.max_samples, S - s0)
                check(lib().nmx_glm_loglik(ptr(self.workspace), self.N, self.D, self.family, ptr(W[s0:]), m,
                                           ptr(out[s0:]), ld, native.stream_ptr()), "nmx_glm_loglik")
        return out

    def draw(self, W, seed, sample0=0):
        """Counts drawn from Poisson(exp(X @ W_s + offset)): int32 [S, N]; the draw of sample s depends
        on (seed, sample0 + s, n) only."""
        W = self._samples(W)
        S = W.shape[0]
        out = torch.empty(S, self.N, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            for s0 in range(0, S, self.max_samples):
                m = min(self.max_samples, S - s0)
                check(lib().nmx_glm_predict(ptr(self.workspace), self.N, self.D, self.family, ptr(W[s0:]), m,
                                            sample0 + s0, seed, ptr(out[s0:]), self.N, native.stream_ptr()),
                      "nmx_glm_predict")
        return out
