"""PSIS-LOO of a log-likelihood table on the device: per column of a table [S, N], the
Pareto-smoothed importance-sampling estimate of the leave-one-out log predictive density and the
Pareto-k diagnostic of its importance ratios (csrc/psis.hip k_psis_transpose / k_psis_column;
include/numpyro_amd.h "PSIS-LOO" states the arithmetic, the orders and the special columns).
Unlike the pointwise reductions the smoothing needs every sample of a column at once, so the table
is held whole, and the kernel works on a column-contiguous copy of it (the workspace)."""
from __future__ import annotations

import math

import torch

from . import native
from .native import check, lib, ptr


def tail_length(num_rows, reff=1.0):
    """M = ceil(min(S / 5, 3 sqrt(S / reff))): the number of largest ratios the generalised Pareto
    distribution is fitted to (Vehtari, Gelman and Gabry 2017; reff the relative efficiency of the
    draws, 1 for independent ones)."""
    S = int(num_rows)
    reff = float(reff)
    if not (reff > 0.0 and math.isfinite(reff)):
        raise ValueError(f"reff must be positive and finite, got {reff}")
    return int(math.ceil(min(S / 5.0, 3.0 * math.sqrt(S / reff))))


def check_sizes(num_rows, tail):
    """Refuse what nmx_psis_loo would refuse, with the sizes named."""
    if num_rows < 2:
        raise ValueError(f"PSIS-LOO needs at least 2 samples, got S = {num_rows}")
    if num_rows > native.PSIS_MAX_ROWS:
        raise NotImplementedError(f"PSIS-LOO of S = {num_rows} samples: above NMX_PSIS_MAX_ROWS = "
                                  f"{native.PSIS_MAX_ROWS}; thin the draws")
    if tail > native.PSIS_MAX_TAIL:
        raise NotImplementedError(f"PSIS-LOO of S = {num_rows} samples: the tail of M = {tail} ratios is above "
                                  f"NMX_PSIS_MAX_TAIL = {native.PSIS_MAX_TAIL} (it is sorted in LDS); thin the draws")
    if not 1 <= tail < num_rows:
        raise ValueError(f"PSIS-LOO tail of M = {tail} ratios outside [1, S = {num_rows})")


def psis_loo_columns(table, num_columns, tail):
    """(elpd_loo [num_columns], pareto_k [num_columns]) of the first num_columns columns of ``table``
    [S, >= num_columns] (float32, on the device, unit column stride) with the tail length ``tail``."""
    num_columns = int(num_columns)
    if table.dim() != 2 or table.dtype != torch.float32 or not table.is_cuda or num_columns <= 0 or \
            table.shape[1] < num_columns or (table.shape[1] > 1 and table.stride(1) != 1):
        raise ValueError(f"PSIS table of shape {tuple(table.shape)}, strides {table.stride()}, {table.dtype} on "
                         f"{table.device}: need float32 [S, >= {num_columns}] rows on a GPU")
    S = table.shape[0]
    check_sizes(S, tail)
    ld = table.stride(0)
    if ld < num_columns:
        raise ValueError(f"PSIS table of shape {tuple(table.shape)} with row stride {ld}: rows overlap")
    with torch.cuda.device(table.device):
        work = torch.empty(lib().nmx_psis_workspace_bytes(S, num_columns), dtype=torch.uint8, device=table.device)
        elpd = torch.empty(num_columns, dtype=torch.float32, device=table.device)
        k = torch.empty_like(elpd)
        check(lib().nmx_psis_loo(ptr(table), S, ld, num_columns, int(tail), ptr(work), ptr(elpd), ptr(k),
                                 native.stream_ptr()), "nmx_psis_loo")
    return elpd, k


def psis_loo_table(table, reff=1.0):
    """(elpd_loo, pareto_k), each of shape table.shape[1:], of a table [S, ...] (a tensor or array;
    moved to the current GPU as float32)."""
    if not torch.cuda.is_available():
        raise RuntimeError("PSIS-LOO needs a GPU (it is a HIP kernel)")
    device = torch.device("cuda", torch.cuda.current_device())
    t = torch.as_tensor(table).to(device, torch.float32)
    if t.dim() < 1 or t.shape[0] == 0:
        raise ValueError(f"a log-likelihood table needs a leading sample dimension, got shape {tuple(t.shape)}")
    S = t.shape[0]
    tail = tail_length(S, reff)
    check_sizes(S, tail)
    flat = t.reshape(S, -1).contiguous()
    if flat.shape[1] == 0:
        raise ValueError(f"a log-likelihood table needs observations, got shape {tuple(t.shape)}")
    elpd, k = psis_loo_columns(flat, flat.shape[1], tail)
    return elpd.reshape(t.shape[1:]), k.reshape(t.shape[1:])
