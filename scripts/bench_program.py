"""Program potential against the torch generic path: NUTS leapfrog/s at 4096 chains.

Two ways to sample a model without a fused kernel:
  program: NUTS(model) -- the front end lowers the model to a program, one HIP kernel per
           evaluation (numpyro_amd/program.py, csrc/potential_program.hip);
  torch:   NUTS(potential_fn=<hand-written float32 torch potential>, init_params=...) -- what
           the project offered before (potentials.TorchPotential, vmap(grad_and_value)).
Sizes: robust8 (D = 10) and the poisson model at N = 2000, G = 50, K = 8 (D = 60), both from
tests/program_zoo.py.  Protocol: one short untimed run of each path, then the two paths
alternate three times in this process; each repeat adapts for `--warmup` transitions and times
`--samples` transitions between device synchronisations; leapfrog/s = sum(num_steps) / wall.
Also prints the program's cost model (bytes_per_eval) for the kernel figures: kernel time comes
from a separate `rocprofv3 --kernel-trace --stats -- python scripts/bench_program.py --profile`.

usage: python scripts/bench_program.py [--chains 4096] [--warmup 200] [--samples 100] [--profile]
Needs a GPU: there is no CPU fall-back."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import program_zoo as Zoo  # noqa: E402
from numpyro_amd.infer import MCMC, NUTS  # noqa: E402
from numpyro_amd.program import ProgramPotential  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, spec (6.3e12 achievable by a streaming copy)


def timed_run(case, path, chains, warmup, samples, device):
    """(leapfrog/s, timed leapfrogs, wall seconds) of one adapted run."""
    if path == "program":
        kernel, kw = NUTS(case.model), {}
        args = case.args
    else:
        kernel = NUTS(potential_fn=case.torch_fn(torch.float32, device))
        kw, args = {"init_params": case.init_params(chains, torch.float32, device)}, ()
    mcmc = MCMC(kernel, num_warmup=warmup, num_samples=samples, num_chains=chains, progress_bar=False)
    mcmc.warmup(7, *args, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mcmc.run(8, *args, extra_fields=("num_steps",), **kw)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    if path == "program":
        assert isinstance(kernel._potential, ProgramPotential)
    leap = float(mcmc.get_extra_fields()["num_steps"].to(torch.float64).sum())
    return leap / wall, leap, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", default="robust8,poisson2000")
    ap.add_argument("--profile", action="store_true", help="program path only, one short run (for rocprofv3)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_program.py needs a GPU")
    device = torch.device("cuda:0")
    cases = {"robust8": Zoo.CASES["robust8"], "poisson2000": Zoo.poisson_large}
    for size in a.sizes.split(","):
        case = cases[size]()
        pot = NUTS(case.model).potential(case.args)
        rec = {"size": size, "dim": case.dim, "chains": a.chains, "ops": pot.program.num_ops,
               "slots": pot.program.num_slots, "bytes_per_eval": pot.bytes_per_eval(),
               "flops_per_eval": pot.flops_per_eval(1)}
        if a.profile:
            rate, leap, wall = timed_run(case, "program", a.chains, 20, 20, device)
            rec.update(program_leapfrog_per_s=rate, leapfrogs=leap)
            print(json.dumps(rec), flush=True)
            continue
        for path in ("program", "torch"):  # untimed: code objects, vmap tracing, allocator
            timed_run(case, path, a.chains, 10, 5, device)
        rates = {"program": [], "torch": []}
        for _ in range(a.repeats):
            for path in ("program", "torch"):
                rate, leap, wall = timed_run(case, path, a.chains, a.warmup, a.samples, device)
                rates[path].append(rate)
                print(f"{size} {path}: {rate:.4g} leapfrog/s ({leap:.0f} leapfrogs in {wall:.2f} s)", flush=True)
        for path, r in rates.items():
            rec[path + "_leapfrog_per_s"] = r
        mid = {p: sorted(r)[len(r) // 2] for p, r in rates.items()}
        rec["ratio_program_over_torch_median"] = mid["program"] / mid["torch"]
        rec["ratio_worst_case"] = min(rates["program"]) / max(rates["torch"])
        rec["spread"] = {p: (max(r) - min(r)) / mid[p] for p, r in rates.items()}
        # end-to-end: the tape bytes of the program's evaluations per second (not the kernel's share)
        rec["program_tape_bytes_per_s_end_to_end"] = mid["program"] * rec["bytes_per_eval"]
        rec["share_of_hbm_peak_end_to_end"] = rec["program_tape_bytes_per_s_end_to_end"] / HBM_PEAK
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
