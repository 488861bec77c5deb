"""Pointwise reductions of a log-likelihood table on the device: per column of a table [S, N],
lppd = logsumexp over S - log S and p_waic = the unbiased variance over S (csrc/loglik_program.hip
k_pointwise_partial / k_pointwise_merge / k_pointwise_finish; include/numpyro_amd.h
"log-likelihood programs" states the arithmetic, the orders and the special columns).  The state
is a running one: chunks of rows are accumulated one call after another, so the table never has
to be held whole."""
from __future__ import annotations

import torch

from . import native
from .native import check, lib, ptr


class PointwiseReducer:
    """Running lppd / p_waic state over ``num_columns`` columns on ``device``."""

    def __init__(self, num_columns, device):
        self.num_columns = int(num_columns)
        if self.num_columns <= 0:
            raise ValueError(f"a pointwise reduction needs columns, got {num_columns}")
        self.device = device
        self.state = torch.empty(lib().nmx_pointwise_state_bytes(self.num_columns), dtype=torch.uint8, device=device)
        self.num_rows = 0

    def accumulate(self, table):
        """Add the rows of ``table`` [rows, >= num_columns] (float32, on the device, unit column
        stride; the first num_columns columns are read)."""
        if table.dim() != 2 or table.dtype != torch.float32 or table.shape[1] < self.num_columns or \
                (table.shape[1] > 1 and table.stride(1) != 1) or table.device != self.state.device:
            raise ValueError(f"pointwise table of shape {tuple(table.shape)}, strides {table.stride()}, {table.dtype} "
                             f"on {table.device}: need float32 [rows, >= {self.num_columns}] rows on {self.device}")
        if table.shape[0] == 0:
            return
        ld = table.stride(0) if table.shape[0] > 1 else max(table.shape[1], 1)
        check(lib().nmx_pointwise_accumulate(ptr(table), table.shape[0], ld, self.num_columns, ptr(self.state),
                                             int(self.num_rows == 0), native.stream_ptr()), "nmx_pointwise_accumulate")
        self.num_rows += table.shape[0]

    def finish(self):
        """(lppd [num_columns], p_waic [num_columns]) of the rows accumulated so far."""
        if self.num_rows == 0:
            raise ValueError("no rows were accumulated")
        lppd = torch.empty(self.num_columns, dtype=torch.float32, device=self.state.device)
        p_waic = torch.empty_like(lppd)
        check(lib().nmx_pointwise_finish(ptr(self.state), self.num_columns, ptr(lppd), ptr(p_waic),
                                         native.stream_ptr()), "nmx_pointwise_finish")
        return lppd, p_waic


def reduce_table(table):
    """(lppd, p_waic), each of shape table.shape[1:], of a table [S, ...] (a tensor or array; moved
    to the current GPU as float32)."""
    if not torch.cuda.is_available():
        raise RuntimeError("the pointwise reductions need a GPU (they are HIP kernels)")
    device = torch.device("cuda", torch.cuda.current_device())
    t = torch.as_tensor(table).to(device, torch.float32)
    if t.dim() < 1 or t.shape[0] == 0:
        raise ValueError(f"a log-likelihood table needs a leading sample dimension, got shape {tuple(t.shape)}")
    flat = t.reshape(t.shape[0], -1).contiguous()
    red = PointwiseReducer(flat.shape[1], device)
    red.accumulate(flat)
    lppd, p_waic = red.finish()
    return lppd.reshape(t.shape[1:]), p_waic.reshape(t.shape[1:])
