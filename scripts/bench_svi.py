"""SVI steps per second at 4096 particles: the device step against the same algorithm in torch.

Two ways to take one Adam step of a mean-field normal guide:
  device: numpyro_amd.infer.SVI -- the model's potential kernel over the particles, then the one
          kernel of csrc/svi.hip (gradient reduction, Adam, the next particles, the loss);
  torch:  the same arithmetic written with torch operations on the same device: eps = randn,
          z = loc + scale * eps, torch.func.vmap(grad_and_value) of the hand-written float32
          potential (tests/program_zoo.py Case.torch_fn; for covtype the logistic-regression
          potential below), the means over particles, Adam and the loss, nothing synchronised.
Sizes: robust8 (D = 10), the poisson model at N = 2000, G = 50, K = 8 (D = 60), both from
tests/program_zoo.py, and covtype (datasets.covtype_synthetic, D = 55).  Protocol: one untimed
run of each path, then the two paths alternate `--repeats` times in this process; each repeat
initialises a fit and times `--steps` steps between device synchronisations.  The new kernel's
share of a step comes from a separate
`rocprofv3 --kernel-trace --stats -- python scripts/bench_svi.py --profile`.

usage: python scripts/bench_svi.py [--particles 4096] [--steps 200] [--repeats 3] [--sizes ...]
                                   [--covtype-rows 581012] [--profile]
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

import program_zoo as Zoo  # noqa: E402
from numpyro_amd import datasets, optim  # noqa: E402
from numpyro_amd import potentials as P  # noqa: E402
from numpyro_amd.infer import SVI, Trace_ELBO  # noqa: E402
from numpyro_amd.infer.autoguide import AutoDiagonalNormal  # noqa: E402

STEP_SIZE, INIT_SCALE = 0.01, 0.1


class Covtype:
    """examples/covtype.py:66-71 on the synthetic covtype: the fused model and its torch potential."""

    def __init__(self, rows):
        self.X, self.y = datasets.covtype_synthetic(rows)
        self.model, self.args, self.dim = P.logistic_regression, (self.X, self.y), self.X.shape[1]
        self.sites = [("coefs", (self.dim,), False)]

    def torch_fn(self, dtype, device):
        X, y = torch.as_tensor(self.X, dtype=dtype, device=device), torch.as_tensor(self.y, dtype=dtype, device=device)

        def u(s):
            c = s["coefs"]
            logits = X @ c
            prior = 0.5 * (c * c).sum() + 0.5 * self.dim * math.log(2 * math.pi)
            return prior + (torch.nn.functional.softplus(logits) - y * logits).sum()

        return u


def device_steps(case, particles, steps, device):
    svi = SVI(case.model, AutoDiagonalNormal(case.model, init_scale=INIT_SCALE), optim.Adam(STEP_SIZE),
              Trace_ELBO(particles))
    state = svi.init(1, *case.args, device=device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = svi.run(1, steps, init_state=state)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return steps / wall, float(res.losses[-1])


def torch_steps(case, particles, steps, device):
    fn = case.torch_fn(torch.float32, device)
    D = case.dim

    def unflatten(z):
        out, o = {}, 0
        for name, shape, _ in case.sites:
            n = int(np.prod(shape))
            out[name] = z[o:o + n].reshape(shape)
            o += n
        return out

    grad_and_value = torch.func.vmap(torch.func.grad_and_value(lambda z: fn(unflatten(z))))
    gen = torch.Generator(device=device).manual_seed(1)
    loc = 4.0 * torch.rand(D, device=device, generator=gen) - 2.0
    rho = torch.full((D,), math.log(math.expm1(INIT_SCALE)), device=device)
    m = torch.zeros(2, D, device=device)
    v = torch.zeros(2, D, device=device)
    losses = torch.empty(steps, device=device)
    b1, b2, eps_adam = 0.9, 0.999, 1e-8
    const = 0.5 * D * (1.0 + math.log(2 * math.pi))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(steps):
        scale = torch.nn.functional.softplus(rho)
        eps = torch.randn(particles, D, device=device, generator=gen)
        g, u = grad_and_value(loc + scale * eps)
        g_loc = g.mean(0)
        g_rho = ((g * eps).mean(0) - 1.0 / scale) * torch.sigmoid(rho)
        losses[t] = u.mean() - torch.log(scale).sum() - const
        grads = torch.stack([g_loc, g_rho])
        m = (1 - b1) * grads + b1 * m
        v = (1 - b2) * grads * grads + b2 * v
        upd = STEP_SIZE * (m / (1 - b1 ** (t + 1))) / (torch.sqrt(v / (1 - b2 ** (t + 1))) + eps_adam)
        loc, rho = loc - upd[0], rho - upd[1]
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return steps / wall, float(losses[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", default="robust8,poisson2000,covtype")
    ap.add_argument("--covtype-rows", type=int, default=datasets.COVTYPE_N)
    ap.add_argument("--covtype-steps", type=int, default=20, help="steps per repeat of the covtype size")
    ap.add_argument("--profile", action="store_true", help="device path only, one short run (for rocprofv3)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_svi.py needs a GPU")
    device = torch.device("cuda:0")
    cases = {"robust8": Zoo.CASES["robust8"], "poisson2000": Zoo.poisson_large,
             "covtype": lambda: Covtype(a.covtype_rows)}
    for size in a.sizes.split(","):
        case = cases[size]()
        steps = a.covtype_steps if size == "covtype" else a.steps
        rec = {"size": size, "dim": case.dim, "particles": a.particles, "steps": steps}
        if a.profile:
            rec["device_steps_per_s"] = device_steps(case, a.particles, steps, device)[0]
            print(json.dumps(rec), flush=True)
            continue
        paths = {"device": device_steps, "torch": torch_steps}
        for fn in paths.values():  # untimed: code objects, vmap tracing, allocator
            fn(case, a.particles, 3, device)
        rates = {p: [] for p in paths}
        for _ in range(a.repeats):
            for path, fn in paths.items():
                rate, last = fn(case, a.particles, steps, device)
                rates[path].append(rate)
                print(f"{size} {path}: {rate:.4g} steps/s (last loss {last:.6g})", flush=True)
        for path, r in rates.items():
            rec[path + "_steps_per_s"] = r
        mid = {p: sorted(r)[len(r) // 2] for p, r in rates.items()}
        rec["ratio_device_over_torch_median"] = mid["device"] / mid["torch"]
        rec["ratio_worst_case"] = min(rates["device"]) / max(rates["torch"])
        rec["spread"] = {p: (max(r) - min(r)) / mid[p] for p, r in rates.items()}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
