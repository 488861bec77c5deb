"""log_likelihood and pointwise_predictive on the program kernel against a torch restatement:
seconds per call at 4096 posterior samples.

Three routes to the log pointwise predictive density of a model's observed site:
  log_likelihood:        infer.log_likelihood(model, samples, *args) -- the model is traced and
                         lowered to a log-likelihood program at the call, one HIP kernel runs it
                         once per sample and writes the [S, N] table
                         (numpyro_amd/loglik_program.py, csrc/loglik_program.hip);
  pointwise_predictive:  the same program, its chunks streamed through the reduce kernels: lppd
                         and p_waic per observation, no table;
  torch:                 the same log densities from float32 torch operations on the device, then
                         torch.logsumexp over the samples: what a user would write by hand.
Sizes: the poisson model at N = 2000, G = 50, K = 8 (tests/program_zoo.py) and partially_pooled
(tests/bounded_zoo.py, 18 observations).  Protocol: one untimed call of each route, then the
routes alternate `--repeats` times in this process; each repeat times `--calls` calls between
device synchronisations.  The two program routes include tracing and lowering the model on the
host; `compile_s` times that part alone, `table_device_s` the program launch alone and
`reduce_device_s` the reduce kernels alone on the finished table.

usage: python scripts/bench_loglik.py [--samples 4096] [--calls 20] [--repeats 3]
Needs a GPU: there is no CPU fall-back."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bounded_zoo as BZ  # noqa: E402
import program_zoo as Zoo  # noqa: E402
from numpyro_amd.infer import log_likelihood, pointwise_predictive  # noqa: E402
from numpyro_amd.infer import loglik as LL  # noqa: E402
from numpyro_amd.loglik_program import compile_log_likelihood  # noqa: E402
from numpyro_amd.pointwise import PointwiseReducer  # noqa: E402


def poisson_samples(case, S, device):
    rs = np.random.RandomState(0)
    return {name: torch.as_tensor((0.5 + np.abs(z)) if positive else 0.3 * z, dtype=torch.float32, device=device)
            for name, shape, positive in case.sites for z in [rs.randn(S, *shape)]}


def baseball_samples(case, S, device):
    rs = np.random.RandomState(0)
    out = {"m": rs.uniform(0.2, 0.35, S), "kappa": 1.0 + rs.pareto(1.5, S), "phi": rs.beta(12.0, 33.0, (S, 18))}
    return {k: torch.as_tensor(v, dtype=torch.float32, device=device) for k, v in out.items()}


def torch_poisson(case, samples, device):
    X, group, y, _ = case.args
    Xd = torch.as_tensor(X, dtype=torch.float32, device=device)
    gd = torch.as_tensor(group, device=device)
    yd = torch.as_tensor(y, dtype=torch.float32, device=device)
    lg = torch.lgamma(yd + 1.0)

    def table():
        eta = samples["a"][:, gd] + samples["b"] @ Xd.T
        return yd * eta - torch.exp(eta) - lg

    return table


def torch_baseball(case, samples, device):
    n = torch.as_tensor(case.args[0], dtype=torch.float32, device=device)
    k = torch.as_tensor(case.args[1], dtype=torch.float32, device=device)
    coef = torch.lgamma(n + 1.0) - torch.lgamma(k + 1.0) - torch.lgamma(n - k + 1.0)
    return lambda: k * torch.log(samples["phi"]) + (n - k) * torch.log1p(-samples["phi"]) + coef


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", default="poisson2000,partially_pooled")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_loglik.py needs a GPU")
    device = torch.device("cuda:0")
    cases = {"poisson2000": (Zoo.poisson_large, "y", poisson_samples, torch_poisson),
             "partially_pooled": (BZ.CASES["partially_pooled"], "obs", baseball_samples, torch_baseball)}
    log_s = math.log(a.samples)
    for size in a.sizes.split(","):
        make, site, draw, restate = cases[size]
        case = make()
        samples = draw(case, a.samples, device)
        table = restate(case, samples, device)
        routes = {"log_likelihood": lambda: log_likelihood(case.model, samples, *case.args)[site],
                  "pointwise_predictive": lambda: pointwise_predictive(case.model, samples, *case.args)[site]["lppd"],
                  "torch": lambda: torch.logsumexp(table(), 0) - log_s}
        prog = compile_log_likelihood(case.model, case.args, {}, samples)
        rec = {"size": size, "samples": a.samples, "site_elements": prog.num_columns, "ops": prog.num_ops,
               "slots": prog.num_slots, "tape_bytes": 4 * prog.num_slots * a.samples,
               "table_bytes": 4 * prog.num_columns * a.samples}
        first = {r: fn() for r, fn in routes.items()}  # untimed: code objects, allocator
        ref = first["torch"].double()
        rec["max_abs_lppd_difference_from_torch"] = {
            "pointwise_predictive": float((first["pointwise_predictive"].double() - ref).abs().max()),
            "log_likelihood": float((torch.logsumexp(first["log_likelihood"].double(), 0) - log_s - ref).abs().max())}
        times = {r: [] for r in routes}
        for _ in range(a.repeats):
            for route, fn in routes.items():
                t = timed(fn, a.calls)
                times[route].append(t)
                print(f"{size} {route}: {t * 1e3:.3f} ms per call", flush=True)
        t0 = time.perf_counter()
        for _ in range(a.calls):
            compile_log_likelihood(case.model, case.args, {}, samples)
        rec["compile_s"] = (time.perf_counter() - t0) / a.calls
        run = LL._Run(case.model, samples, case.args, {}, 1, "bench")
        out = torch.empty(a.samples, prog.num_columns, dtype=torch.float32, device=device)
        rec["table_device_s"] = timed(lambda: [run.launch(s0, m, out[s0:]) for s0, m in run.chunks()], a.calls)

        def reduce():
            red = PointwiseReducer(prog.num_columns, device)
            red.accumulate(out)
            return red.finish()

        rec["reduce_device_s"] = timed(reduce, a.calls)
        rec["torch_table_s"] = timed(table, a.calls)
        for route, t in times.items():
            rec[route + "_s_per_call"] = t
        mid = {r: sorted(t)[len(t) // 2] for r, t in times.items()}
        rec["ratio_torch_over_log_likelihood_median"] = mid["torch"] / mid["log_likelihood"]
        rec["ratio_torch_over_pointwise_predictive_median"] = mid["torch"] / mid["pointwise_predictive"]
        rec["spread"] = {r: (max(t) - min(t)) / mid[r] for r, t in times.items()}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
