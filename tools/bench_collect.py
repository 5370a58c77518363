#!/usr/bin/env python
"""Collect-path measurement of the graph-captured PPO collect (PPOConfig.graph_collect: one captured graph per ring
block holding act, step, mgx_policy_bootstrap, the episode statistics, the last values and the GAE) against the path
it replaces, the eager fused_act collect of the same build.

  collect    one CompactRolloutCollector.collect() of each kind, two collectors of the same seeds and weights, in
             alternating repeats after a warm-up that captures every block's graph; at two shapes: config 3's (65,536
             envs, horizon 16, n_stack 4, multi / 'pick up' / 8x8 / 4 objects) and the reference recipe's (16 envs,
             horizon 1024)
  bootstrap  FusedActor.bootstrap alone against the nonzero() + values + index_put_ sequence it replaced (the torch
             policy's collect still runs that sequence; both fused collects run the kernel) on one step of a
             65,536-env buffer with 1/64 of the envs truncated, and both with no env truncated (what every step pays)
Device events and host wall time (a collect ends with its one host read, so the wall time is the whole rollout);
median and range (min, max).

  python tools/bench_collect.py [--out profiles/r15_graph_collect] [--sha BUILD] [--repeats 12] [--part all]
writes OUT/collect.json (parts run one after another in this process; --part runs one and merges it into the file).
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "minigrid-rl_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)

ENV3 = dict(problem="multi", mission=2, size=8, num_objects=4)
SHAPES = {"config3_65536x16": (65536, 16), "recipe_16x1024": (16, 1024)}


def _stat(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), repeats=len(ms))


def _timed(fn, torch):
    """(device ms between two events around fn, host wall ms until the device is idle)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def _collectors(n, horizon, torch):
    from mgx import MgxEngine
    from mgx.policy import ActorCriticPolicy
    from mgx.ppo import CompactRolloutCollector, PPOConfig, graph_refill_every
    torch.manual_seed(0)
    out = {}
    pol = None
    for graph in (False, True):
        eng = MgxEngine(n_envs=n, seed=42, n_stack=4, terminal_mode="truncated", mission_dtype=torch.uint8,
                        reward64=True, refill_every=graph_refill_every(horizon), **ENV3)
        pol = ActorCriticPolicy(n_stack=4).to(eng.device) if pol is None else copy.deepcopy(pol)
        cfg = PPOConfig(n_envs=n, horizon=horizon, n_frames_stack=4, env=ENV3, fused_act=True, graph_collect=graph)
        out[graph] = CompactRolloutCollector(eng, pol, cfg)
        out[graph].start()
    return out


def part_collect(args, torch):
    res = {}
    for name, (n, horizon) in SHAPES.items():
        cols = _collectors(n, horizon, torch)
        for _ in range(cols[True].rollout.buf.blocks + 1):           # every block's graph captured and replayed once
            cols[False].collect(), cols[True].collect()
        dev, wall = {False: [], True: []}, {False: [], True: []}
        for _ in range(args.repeats):
            for g in (False, True):
                d, w = _timed(cols[g].collect, torch)
                dev[g].append(d)
                wall[g].append(w)
        for c in cols.values():
            c.engine.poll_error()
        e, g = statistics.median(wall[False]), statistics.median(wall[True])
        res[name] = dict(n_envs=n, horizon=horizon, refill_every=cols[True].engine.refill_every,
                         eager=dict(device=_stat(dev[False]), wall=_stat(wall[False])),
                         graph=dict(device=_stat(dev[True]), wall=_stat(wall[True])),
                         wall_ratio_eager_over_graph=e / g,
                         device_ratio_eager_over_graph=statistics.median(dev[False]) / statistics.median(dev[True]),
                         every_graph_run_below_every_eager_run=max(wall[True]) < min(wall[False]),
                         ranges_overlap=max(wall[True]) >= min(wall[False]))
        del cols
        torch.cuda.empty_cache()
    return res


def part_bootstrap(args, torch):
    n, horizon = SHAPES["config3_65536x16"]
    col = _collectors(n, horizon, torch)[False]
    col.collect()
    buf, fused, cfg = col.rollout.buf, col.fused, col.cfg
    dev = buf.engine.device
    t = horizon - 1
    gamma32 = torch.tensor(cfg.gamma, dtype=torch.float32).to(dev)
    g = torch.Generator().manual_seed(1)
    buf.terminal_rows.copy_(buf.rows[buf.row(t + 1)])                # a defined terminal row for every env

    def eager():
        boot = (buf.truncated[t].bool() & ~buf.terminated[t].bool()).nonzero().flatten()
        if boot.numel():
            tv = fused.values(buf, t, terminal=True, envs=boot)
            r = buf.rewards[t]
            r.index_put_((boot,), r.index_select(0, boot) + gamma32 * tv)

    def kernel():
        fused.bootstrap(buf, t, cfg.gamma)

    res = {}
    for name, k in (("one_in_64_truncated", n // 64), ("none_truncated", 0)):
        flags = torch.zeros(n, dtype=torch.uint8)
        flags[torch.randperm(n, generator=g)[:k]] = 1
        buf.truncated[t].copy_(flags)
        buf.terminated[t].zero_()
        for _ in range(3):
            eager(), kernel()
        ms = {"eager": ([], []), "mgx_policy_bootstrap": ([], [])}
        for _ in range(max(args.repeats, 20)):
            for key, fn in (("eager", eager), ("mgx_policy_bootstrap", kernel)):
                d, w = _timed(fn, torch)
                ms[key][0].append(d)
                ms[key][1].append(w)
        assert int(fused.boot_count) == k
        res[name] = dict(selected=k, **{key: dict(device=_stat(v[0]), wall=_stat(v[1])) for key, v in ms.items()})
    buf.engine.poll_error()
    return res


PARTS = {"collect": part_collect, "bootstrap": part_bootstrap}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_graph_collect"))
    ap.add_argument("--sha", default="")
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--part", default="all", choices=["all"] + list(PARTS))
    args = ap.parse_args()
    import torch
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "collect.json")
    doc = {}
    if args.part != "all" and os.path.exists(path):
        doc = json.load(open(path))
    doc.update(build=args.sha, device=torch.cuda.get_device_name(0), torch=torch.__version__,
               method="alternating repeats in one process after a warm-up; device = events around the call, wall = "
                      "host time until the device is idle; median (min, max) in ms")
    for name, fn in PARTS.items():
        if args.part in ("all", name):
            doc[name] = fn(args, torch)
            print(name, json.dumps(doc[name]))
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
