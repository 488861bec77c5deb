"""PSIS-LOO of a log-likelihood table on the device: seconds per call of psis.psis_loo_table
(csrc/psis.hip: the transpose into the workspace, then one workgroup per column), beside the time
of the pointwise reduction (nmx_pointwise_accumulate + nmx_pointwise_finish, one pass over the same
table) and of a torch transpose of the table (what the column-contiguous copy costs on its own).

Nothing else in the project computes PSIS, so the yardstick is the number of passes the algorithm
makes over the table (the transpose's read and write, the minimum, four select rounds, the
compaction: eight table-sized streams) times the measured one-pass reduction:
`ratio_over_one_pass` is printed for comparison with that count.

Tables: the one-parameter normal model of tests/psis_cases.py (spread 0.7: k of about 0.4 - 1.2),
drawn on the device.  Protocol: `--warmup` untimed calls of each route, then `--runs` timed calls of
each, the routes alternating, each call between device events; the record holds the median and the
spread (max - min) / median.

usage: python scripts/bench_loo.py [--sizes 4096x1000,262144x1000,1048576x256] [--runs 20] [--warmup 3]
Needs a GPU: there is no CPU fall-back."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import torch  # noqa: E402

from numpyro_amd.pointwise import PointwiseReducer  # noqa: E402
from numpyro_amd.psis import psis_loo_table, tail_length  # noqa: E402


def normal_table(S, N, spread, device):
    g = torch.Generator(device=device).manual_seed(0)
    mu = spread * torch.randn(S, generator=g, device=device)
    y = torch.linspace(-3.0, 3.0, N, device=device)
    table = y[None, :] - mu[:, None]
    table.square_().mul_(-0.5).sub_(0.5 * math.log(2.0 * math.pi))
    return table


def event_time(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096x1000,262144x1000,1048576x256")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--spread", type=float, default=0.7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_loo.py needs a GPU")
    device = torch.device("cuda:0")
    for size in a.sizes.split(","):
        S, N = (int(v) for v in size.split("x"))
        table = normal_table(S, N, a.spread, device)

        def one_pass():
            red = PointwiseReducer(N, device)
            red.accumulate(table)
            return red.finish()

        routes = {"psis_loo": lambda: psis_loo_table(table),
                  "one_pass_reduction": one_pass,
                  "torch_transpose": lambda: table.t().contiguous()}
        for _ in range(a.warmup):
            for fn in routes.values():
                fn()
        torch.cuda.synchronize()
        times = {r: [] for r in routes}
        for _ in range(a.runs):
            for route, fn in routes.items():
                times[route].append(event_time(fn))
        elpd, k = psis_loo_table(table)
        mid = {r: sorted(t)[len(t) // 2] for r, t in times.items()}
        rec = {"samples": S, "observations": N, "tail": tail_length(S), "table_bytes": 4 * S * N, "runs": a.runs,
               "pareto_k_range": [float(k.min()), float(k.max())], "elpd_loo": float(elpd.double().sum())}
        for r in routes:
            rec[r + "_s"] = mid[r]
            rec[r + "_spread"] = (max(times[r]) - min(times[r])) / mid[r]
            rec[r + "_table_bytes_per_s"] = 4 * S * N / mid[r]
        rec["ratio_over_one_pass"] = mid["psis_loo"] / mid["one_pass_reduction"]
        print(json.dumps(rec), flush=True)
        del table


if __name__ == "__main__":
    main()
