"""Predictive on the program kernel against a torch restatement: seconds per call at 4096
posterior samples.

Two ways to draw the observed site of a model without a fused predictive kernel:
  program: Predictive(model, samples)(key, *args) -- the model is traced and lowered to a
           predictive program at the call, one HIP kernel runs it once per sample
           (numpyro_amd/predictive_program.py, csrc/predictive_program.hip);
  torch:   the same parameters from torch operations on the device and torch's own samplers
           (torch.poisson, torch.distributions.StudentT): what a user would write by hand.
Sizes: the poisson model at N = 2000, G = 50, K = 8 (one draw_poisson of 2000 elements per
sample) and robust8 (a StudentT site of 8), both from tests/program_zoo.py.  Protocol: one
untimed call of each path, then the two paths alternate `--repeats` times in this process; each
repeat times `--calls` calls between device synchronisations.  The program path's call includes
tracing and lowering the model on the host; `program_compile_s` times that part alone and
`program_device_s` the launches alone (the rest is uploading the program and slicing the tape).

usage: python scripts/bench_predictive.py [--samples 4096] [--calls 20] [--repeats 3]
Needs a GPU: there is no CPU fall-back."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import program_zoo as Zoo  # noqa: E402
from numpyro_amd.infer import Predictive  # noqa: E402
from numpyro_amd.predictive_program import compile_predictive  # noqa: E402
from numpyro_amd.random import key_to_seed  # noqa: E402


def posterior_like(case, S, device):
    rs = np.random.RandomState(0)
    return {name: torch.as_tensor((0.5 + np.abs(z)) if positive else 0.3 * z, dtype=torch.float32, device=device)
            for name, shape, positive in case.sites for z in [rs.randn(S, *shape)]}


def torch_poisson(case, samples, device):
    X, group, _, _ = case.args
    Xd = torch.as_tensor(X, dtype=torch.float32, device=device)
    gd = torch.as_tensor(group, device=device)
    return lambda: torch.poisson(torch.exp(samples["a"][:, gd] + samples["b"] @ Xd.T)).to(torch.int32)


def torch_robust8(case, samples, device):
    sigma = torch.as_tensor(case.args[1], dtype=torch.float32, device=device)
    return lambda: torch.distributions.StudentT(4.0, samples["theta"], sigma).sample()


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
    ap.add_argument("--sizes", default="poisson2000,robust8")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_predictive.py needs a GPU")
    device = torch.device("cuda:0")
    cases = {"robust8": (Zoo.CASES["robust8"], (2,), "obs", torch_robust8),
             "poisson2000": (Zoo.poisson_large, (2,), "y", torch_poisson)}
    for size in a.sizes.split(","):
        make, observed, site, restate = cases[size]
        case = make()
        args = tuple(None if i in observed else x for i, x in enumerate(case.args))
        samples = posterior_like(case, a.samples, device)
        pred = Predictive(case.model, samples)
        paths = {"program": lambda: pred(3, *args)[site], "torch": restate(case, samples, device)}
        prog = compile_predictive(case.model, args, {}, samples)
        rec = {"size": size, "samples": a.samples, "site_elements": prog.outputs[0].n, "ops": prog.num_ops,
               "slots": prog.num_slots, "tape_bytes": 4 * prog.num_slots * a.samples}
        for fn in paths.values():  # untimed: code objects, allocator
            fn()
        times = {"program": [], "torch": []}
        for _ in range(a.repeats):
            for path, fn in paths.items():
                t = timed(fn, a.calls)
                times[path].append(t)
                print(f"{size} {path}: {t * 1e3:.3f} ms per call", flush=True)
        t0 = time.perf_counter()
        for _ in range(a.calls):
            compile_predictive(case.model, args, {}, samples)
        rec["program_compile_s"] = (time.perf_counter() - t0) / a.calls
        given = {name: samples[name] for name, _, _, _ in prog.inputs}
        rec["program_device_s"] = timed(lambda: pred._run_program(prog, given, key_to_seed(3), device), a.calls)
        for path, t in times.items():
            rec[path + "_s_per_call"] = t
        mid = {p: sorted(t)[len(t) // 2] for p, t in times.items()}
        rec["ratio_torch_over_program_median"] = mid["torch"] / mid["program"]
        rec["spread"] = {p: (max(t) - min(t)) / mid[p] for p, t in times.items()}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
