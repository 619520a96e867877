#!/usr/bin/env python3
"""Step time of the NTU model (bs=64, fwd + bwd + SGD) under torch's data-parallel wrappers
on ONE GPU, next to the plain step of the same process:

  plain    the unwrapped model (side stream on, deferred gradient writes)
  replica  torch.nn.parallel.replicate(model, [0])[0], re-made every step as
           nn.DataParallel does (in-order backward: replica tensors are not leaves)
  ddp      DistributedDataParallel, world 1 over RCCL (in-order backward)

Each leg: 5 warm-up steps, then 20 steps between two HIP events. Prints one JSON line per
leg and a closing line with the ratios to the mean of the two plain legs.

    python tools/wrapper_cost.py [--steps 20] [--warmup 5] [--batch 64]
"""
import argparse
import json
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "shift-gcn_amd"))

import torch  # noqa: E402


def build(dev):
    import shiftgcn
    from shiftgcn import train
    torch.manual_seed(1)
    model = shiftgcn.Model(num_class=60, num_point=25, num_person=2,
                           graph="graph.ntu_rgb_d.Graph").to(dev).train()
    return model, train.build_optimizer(model, base_lr=0.1)


def timed(forward, opt, x, y, steps, warmup):
    def step():
        loss = torch.nn.functional.cross_entropy(forward(x), y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()

    for _ in range(warmup):
        step()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args()
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel, replicate
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    gen = torch.Generator().manual_seed(1000)
    x = torch.randn(args.batch, 3, 300, 25, 2, generator=gen).to(dev)
    y = torch.randint(0, 60, (args.batch,), generator=gen).to(dev)
    res = {}

    def leg(name, make):
        model, opt = build(dev)
        forward, done = make(model)
        try:
            ms = timed(forward, opt, x, y, args.steps, args.warmup)
        finally:
            done()
        res[name] = ms
        print(json.dumps({"leg": name, "step_ms": round(ms, 3), "steps": args.steps,
                          "warmup": args.warmup, "batch": args.batch}), flush=True)

    def plain(model):
        return model, lambda: None

    def replica(model):
        return (lambda inp: replicate(model, [0])[0](inp)), lambda: None

    def ddp(model):
        store = tempfile.mkdtemp()
        dist.init_process_group("nccl", init_method=f"file://{store}/store", rank=0,
                                world_size=1, device_id=dev)
        return DistributedDataParallel(model, device_ids=[0]), dist.destroy_process_group

    leg("plain", plain)
    leg("replica", replica)
    leg("ddp", ddp)
    leg("plain_again", plain)
    base = 0.5 * (res["plain"] + res["plain_again"])
    print(json.dumps({"plain_ms": round(base, 3),
                      "replica_over_plain": round(res["replica"] / base, 4),
                      "ddp_over_plain": round(res["ddp"] / base, 4),
                      "device": torch.cuda.get_device_name(0),
                      "gpus_visible": torch.cuda.device_count()}))


if __name__ == "__main__":
    main()
