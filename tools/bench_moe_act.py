#!/usr/bin/env python
"""Act-path measurement of the mission-routed mixture of experts (mgx_policy_act_moe, mgx/moe.py).

At 65,536 envs, n_stack 4, multi / every mission / 8x8 / 4 objects, four experts routed by task:
  (a) what was possible before: four FusedActor.act launches over ALL samples, then the torch select by
      route[mission id] of actions, values and log-probs
  (b) FusedMoEActor.act: the route launch and one policy pass over the partition
  (c) one FusedActor.act: the floor (one policy over all samples)
(a), (b) and (c) alternate in one loop; device events after a warm-up, median of >= 12 repeats with the spread (min,
max) beside it.  `launches`: the route launch and the policy launch of (b) separately, in device time, from a
rocprofv3 kernel trace of a child process that runs (b) alone.  `evaluate`: one 4,096-env x 4,096-episode graph
evaluation (GraphEvaluator, refill_every 16) of the mixture and of a single policy on engines of equal seed,
alternating, host wall time of the whole call.

Every part runs in a child process of its own under a time limit; the first failure ends the run.
  python tools/bench_moe_act.py [--out profiles/r19_moe_act] [--sha BUILD] [--envs 65536] [--repeats 12]
writes OUT/act.json.
"""
import argparse
import csv
import glob
import hashlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "minigrid-rl_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)

ENV = dict(problem="multi", mission=None, size=8, num_objects=4)
TASKS = {"GTO": 0, "TGL": 1, "PKP": 2, "GTG": 3}
K = 4


def _stat(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), repeats=len(ms))


def _timed(fn, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _experts(torch, device):
    from mgx.policy import ActorCriticPolicy
    pols = []
    for s in range(len(TASKS)):
        torch.manual_seed(s)
        pols.append(ActorCriticPolicy(n_stack=K).to(device).train(False))
    return pols


def _setup(args, torch):
    """The engine after 8 random steps, the mixture's actor, the four experts' own actors and the route."""
    from mgx import MgxEngine
    from mgx.compact import CompactBuffer
    from mgx.fused_policy import FusedActor
    from mgx.moe import FusedMoEActor, MoEPolicy, route_by_task
    n = args.envs
    eng = MgxEngine(n_envs=n, n_stack=K, terminal_mode="truncated", mission_dtype=torch.uint8, **ENV)
    pols = _experts(torch, eng.device)
    buf = CompactBuffer(eng, 16, ring=True)
    eng.reset()
    buf.observe(0)
    torch.manual_seed(0)
    for t in range(8):                                                         # populated stacks, episode starts
        buf.step(t, torch.randint(0, 7, (n,), device=eng.device))
    moe = MoEPolicy(pols, route_by_task(TASKS, ids=range(128)))
    actor = FusedMoEActor(moe, eng, seed=1)
    singles = [FusedActor(p, eng, seed=1) for p in pols]
    for a in [actor] + singles:
        a.index_table(buf)
    return eng, buf, moe, actor, singles, 8


def part_act(args):
    import torch
    eng, buf, moe, actor, singles, t = _setup(args, torch)
    route = moe.route.to(eng.device).to(torch.int64)

    def four_and_select():
        outs = [s.act(buf, t) for s in singles]
        which = route[buf.mids[buf.row(t)].to(torch.int64)][None]
        return tuple(torch.stack([o[j] for o in outs]).gather(0, which)[0] for j in range(3))

    def mixture():
        return actor.act(buf, t)

    def single():
        return singles[0].act(buf, t)

    # the select picks the routed expert's outputs: check it once against the mixture, deterministic
    want = [s.act(buf, t, deterministic=True) for s in singles]
    which = route[buf.mids[buf.row(t)].to(torch.int64)][None]
    got = actor.act(buf, t, deterministic=True)
    for j in range(3):
        assert torch.equal(torch.stack([o[j] for o in want]).gather(0, which)[0], got[j])
    for _ in range(5):
        four_and_select(), mixture(), single()
    torch.cuda.synchronize()
    ta, tb, tc = [], [], []
    for _ in range(args.repeats):
        ta.append(_timed(four_and_select, torch))
        tb.append(_timed(mixture, torch))
        tc.append(_timed(single, torch))
    eng.poll_error()
    rec = actor.last_route.cpu().tolist()
    a, b, c = _stat(ta), _stat(tb), _stat(tc)
    return dict(n_envs=args.envs, n_stack=K, env=ENV, experts=len(singles), route="by task " + json.dumps(TASKS),
                counts_per_expert=rec[1:8:2], live_tiles=rec[16], grid_tiles=(args.envs + 63 * len(singles)) // 64,
                a_four_acts_plus_select=a, b_moe_act=b, c_one_act=c,
                ratio_a_over_b=a["median_ms"] / b["median_ms"], ratio_b_over_c=b["median_ms"] / c["median_ms"],
                every_b_run_below_every_a_run=max(tb) < min(ta))


def part_loop(args):
    """(b) alone, for the kernel trace: warm-up, then `repeats` calls."""
    import torch
    eng, buf, moe, actor, singles, t = _setup(args, torch)
    for _ in range(5 + args.repeats):
        actor.act(buf, t)
    torch.cuda.synchronize()
    eng.poll_error()
    return dict(calls=5 + args.repeats)


def part_launches(args):
    """The two launches of (b) in device time: a rocprofv3 kernel trace of part_loop in a child process."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out = tempfile.mkdtemp(prefix="moe_trace_")
    try:
        cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", out, "-o", "run", "--", sys.executable,
               os.path.abspath(__file__), "--part", "loop", "--envs", str(args.envs), "--repeats", str(args.repeats)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        files = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if p.returncode != 0 or not files:
            sys.stderr.write(p.stdout.decode(errors="replace")[-4000:])
            raise RuntimeError("the kernel trace failed (exit %d)" % p.returncode)
        ms = {"mgx_moe_route_kernel": [], "mgx_policy_moe_kernel": []}
        with open(files[0]) as f:
            for r in csv.DictReader(f):
                for name in ms:
                    if name in r["Kernel_Name"]:
                        ms[name].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    finally:
        shutil.rmtree(out, ignore_errors=True)
    if any(len(v) != 5 + args.repeats for v in ms.values()):
        raise RuntimeError("expected %d launches of each kernel, found %s"
                           % (5 + args.repeats, {k: len(v) for k, v in ms.items()}))
    return dict(n_envs=args.envs, route_launch=_stat(ms["mgx_moe_route_kernel"][5:]),
                policy_launch=_stat(ms["mgx_policy_moe_kernel"][5:]),
                method="kernel durations of a rocprofv3 kernel trace, the first 5 calls dropped")


def part_evaluate(args):
    import torch
    from mgx import GraphEvaluator, MgxEngine, summarize_missions
    from mgx.fused_policy import FusedActor
    from mgx.moe import FusedMoEActor, MoEPolicy, route_by_task
    n = n_eval = 4096
    engs = [MgxEngine(n_envs=n, seed=42, n_stack=K, terminal_mode="truncated", mission_dtype=torch.uint8,
                      reward64=True, refill_every=16, **ENV) for _ in range(2)]
    pols = _experts(torch, engs[0].device)
    moe = MoEPolicy(pols, route_by_task(TASKS, ids=range(128)))
    ev_m = GraphEvaluator(FusedMoEActor(moe, engs[0], seed=1))
    ev_s = GraphEvaluator(FusedActor(pols[0], engs[1], seed=1))
    ev_m.evaluate(n_eval), ev_s.evaluate(n_eval)                               # warm-up: captures every graph
    runs = {"mixture": [], "single": []}
    for _ in range(args.repeats):
        for key, ev in (("mixture", ev_m), ("single", ev_s)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev.evaluate(n_eval)
            runs[key].append(dict(ms=(time.perf_counter() - t0) * 1e3, steps=ev.last["steps"]))
    # every evaluate() starts with the actor's sync (the blob and the mission table of every expert): its share
    sync = {"mixture": [], "single": []}
    for _ in range(args.repeats):
        for key, ev in (("mixture", ev_m), ("single", ev_s)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev.actor.sync()
            torch.cuda.synchronize()
            sync[key].append((time.perf_counter() - t0) * 1e3)
    r, l = ev_m.evaluate(n_eval, return_episode_rewards=True)
    cols = summarize_missions(r, l, ev_m.last["mission_ids"])
    for e in engs:
        e.poll_error()
    doc = dict(n_envs=n, n_eval_episodes=n_eval, refill_every=16, env=ENV,
               per_task_episodes={k: v["episodes"] for k, v in cols["per_task"].items()})
    for key, rs in runs.items():
        doc[key] = dict(wall=_stat([x["ms"] for x in rs]), steps=[x["steps"] for x in rs],
                        actor_sync_alone=_stat(sync[key]))
    doc["wall_ratio_mixture_over_single"] = doc["mixture"]["wall"]["median_ms"] / doc["single"]["wall"]["median_ms"]
    ref = os.path.join(ROOT, "profiles", "r17_graph_eval", "eval.json")
    if os.path.exists(ref):                                                    # the earlier single-policy figure
        g = json.load(open(ref))["evaluate"]["4096x4096"]["graph"]
        doc["r17_graph_eval_single_policy_pick_up"] = dict(wall=g["wall"], steps=g["steps"])
    return doc


PARTS = {"act": (part_act, 420), "loop": (part_loop, 300), "launches": (part_launches, 420),
         "evaluate": (part_evaluate, 420)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_moe_act"))
    ap.add_argument("--sha", default=None, help="build id to record (default: git rev-parse HEAD)")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--part", choices=sorted(PARTS), default=None, help="(internal) run one part in this process")
    args = ap.parse_args()
    if args.part:
        print("RESULT " + json.dumps(PARTS[args.part][0](args)))
        return 0
    if args.repeats < 12:
        ap.error("--repeats must be >= 12")
    sha = args.sha
    if sha is None:
        try:
            sha = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            sha = "unknown"
    lib = os.path.join(ROOT, "minigrid-rl_amd", "mgx", "libmgx.so")
    doc = dict(build_sha=sha, libmgx_sha256=hashlib.sha256(open(lib, "rb").read()).hexdigest(),
               method="alternating repeats in one process after a warm-up; act: device events around each call; "
                      "evaluate: host wall time of the whole call; median (min, max) in ms")
    os.makedirs(args.out, exist_ok=True)
    for name in ("act", "launches", "evaluate"):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", name, "--envs", str(args.envs),
               "--repeats", str(args.repeats)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=PARTS[name][1])
        text = p.stdout.decode(errors="replace")
        lines = [ln for ln in text.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(text[-4000:])
            sys.stderr.write("\n%s failed (exit %d): stopping\n" % (name, p.returncode))
            return 1
        doc[name] = json.loads(lines[-1][7:])
        print(name, json.dumps(doc[name]))
    with open(os.path.join(args.out, "act.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
