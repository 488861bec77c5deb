"""torch.distributed worker of tests/test_gpu_init.py: one rank of a 2-rank run (gloo, both ranks
on cuda:0) of num_chains = 2 with a callable potential_fn and batched init_params, so each rank
holds one chain.  Rank 0 saves every rank's potential dimension, chain shard and draws.
usage: torchrun ... dist_init_worker.py OUT"""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_gpu_init import banana_run  # noqa: E402

dist.init_process_group("gloo")
torch.cuda.set_device(0)
dim, x, mcmc = banana_run()
world = dist.get_world_size()
info = [None] * world
dist.all_gather_object(info, (int(dim), [mcmc.chain_lo, mcmc.chain_hi, mcmc.local_chains]))
x = x.contiguous()
xs = [torch.zeros_like(x) for _ in range(world)]
dist.all_gather(xs, x)
if dist.get_rank() == 0:
    torch.save({"x": torch.cat(xs), "dims": [i[0] for i in info], "chains": [i[1] for i in info]}, sys.argv[1])
dist.destroy_process_group()
