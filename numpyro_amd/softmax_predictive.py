"""Softmax regression after sampling (csrc/predictive_softmax.hip): the pointwise log-likelihood
table and posterior predictive labels of obs ~ Categorical(logits = X @ W_s) for posterior samples
W [S, D, K].  ``SoftmaxPredictive`` holds the data matrix split into the kernel's bf16 planes, made
once; ``infer.log_likelihood`` / ``pointwise_predictive`` / ``loo`` and ``infer.Predictive`` reach
it for a model of that structure."""
from __future__ import annotations

import numpy as np
import torch

from . import native
from .native import check, lib, ptr


def _dev(x, device, dtype):
    return torch.as_tensor(x if torch.is_tensor(x) else np.asarray(x)).to(device, dtype).contiguous()


class SoftmaxPredictive:
    """X [N, D] on ``device``, split once for any number of launches."""

    def __init__(self, X, device):
        self.device = torch.device(device)
        X = _dev(X, self.device, torch.float32)
        if X.dim() != 2:
            raise ValueError(f"softmax regression needs data [N, D] (got {tuple(X.shape)})")
        self.N, self.D = X.shape
        self.packed = torch.empty(lib().nmx_softmax_predictive_workspace_bytes(self.N, self.D), dtype=torch.uint8,
                                  device=self.device)
        with torch.cuda.device(self.device):
            check(lib().nmx_softmax_predictive_pack(ptr(X), self.N, self.D, ptr(self.packed), native.stream_ptr()),
                  "nmx_softmax_predictive_pack")

    def _samples(self, W):
        W = _dev(W, self.device, torch.float32)
        if W.dim() != 3 or W.shape[1] != self.D:
            raise ValueError(f"posterior samples of shape {tuple(W.shape[1:])} per draw, the data has {self.D} features")
        return W

    def log_likelihood(self, y, W, out=None):
        """log p(y_n | W_s) for labels y [N] and samples W [S, D, K]: float32 [S, N], or written into
        the first S rows and N columns of ``out`` (float32, unit column stride).  NaN where a label
        is outside [0, K)."""
        W, y = self._samples(W), _dev(y, self.device, torch.int32)
        S, K = W.shape[0], W.shape[2]
        if tuple(y.shape) != (self.N,):
            raise ValueError(f"labels of shape {tuple(y.shape)} for {self.N} rows")
        if out is None:
            out = torch.empty(S, self.N, dtype=torch.float32, device=self.device)
        if out.dim() != 2 or out.dtype != torch.float32 or out.device != self.device or out.shape[0] < S or \
                out.shape[1] < self.N or (out.shape[1] > 1 and out.stride(1) != 1):
            raise ValueError(f"a table of shape {tuple(out.shape)}, strides {out.stride()}, {out.dtype} on {out.device}: "
                             f"need float32 [>= {S}, >= {self.N}] rows on {self.device}")
        ld = out.stride(0) if out.shape[0] > 1 else out.shape[1]
        with torch.cuda.device(self.device):
            check(lib().nmx_softmax_loglik(ptr(self.packed), ptr(y), self.N, self.D, K, ptr(W), S, ptr(out), ld,
                                           native.stream_ptr()), "nmx_softmax_loglik")
        return out

    def draw(self, W, seed):
        """Labels drawn from softmax(X @ W_s): int32 [S, N]; a draw depends on (seed, s, n) only."""
        W = self._samples(W)
        S, K = W.shape[0], W.shape[2]
        out = torch.empty(S, self.N, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().nmx_softmax_predict(ptr(self.packed), self.N, self.D, K, ptr(W), S, seed, ptr(out), self.N,
                                            native.stream_ptr()), "nmx_softmax_predict")
        return out
