#!/usr/bin/env python
"""Evaluation-path measurement of the graph-captured evaluator (mgx.evaluation.GraphEvaluator: blocks of act, step
and mgx_eval_record as captured graphs, one host read per block) against the path it replaces, the eager
evaluate_policy(..., fused=actor) loop of the same build (one host read and about eight small torch ops per step).

  evaluate   one evaluation of each kind on two engines of equal seed and one policy, in alternating repeats after a
             warm-up evaluation that captures every graph; host wall time of the whole call, the actor's sync in
             front and the final read of the records included.  Every repeat is the next evaluation on its engine (a reset continues the engine's
             streams), so the episodes differ from repeat to repeat and, after the first over-run, between the two
             paths: the steps each repeat executed and needed are recorded with its time.  Two shapes: the reference
             recipe's (16 envs, 100 episodes, multi / 'pick up' / 8x8, refill_every 16) and 4,096 envs x 4,096
             episodes
  record     mgx_eval_record alone against the eager loop's accounting lines, per step, at both env counts: 256
             back-to-back launches between two device events

  python tools/bench_eval.py [--out profiles/r17_graph_eval] [--sha BUILD] [--repeats 12] [--part all]
writes OUT/eval.json (parts run one after another in this process; --part runs one and merges it into the file).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "minigrid-rl_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)

ENV = dict(problem="multi", mission=2, size=8, num_objects=4)
SHAPES = {"recipe_16x100": (16, 100), "4096x4096": (4096, 4096)}
REFILL_EVERY = 16


def _stat(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), repeats=len(ms))


def _engine(n, torch):
    from mgx import MgxEngine
    return MgxEngine(n_envs=n, seed=42, n_stack=4, terminal_mode="truncated", mission_dtype=torch.uint8,
                     reward64=True, refill_every=REFILL_EVERY, **ENV)


def part_evaluate(args, torch):
    from mgx import GraphEvaluator, evaluate_policy
    from mgx.fused_policy import FusedActor
    from mgx.policy import ActorCriticPolicy
    res = {}
    for name, (n, n_eval) in SHAPES.items():
        torch.manual_seed(0)
        eng_e, eng_g = _engine(n, torch), _engine(n, torch)
        pol = ActorCriticPolicy(n_stack=4).to(eng_e.device)
        act_e, act_g = FusedActor(pol, eng_e, seed=1), FusedActor(pol, eng_g, seed=1)
        ev = GraphEvaluator(act_g)

        def eager():
            act_e.sync()                                       # as EvalCallback does before every evaluation
            out = evaluate_policy(pol, eng_e, n_eval, fused=act_e)
            return out, eng_e.calls, eng_e.calls

        def graph():
            out = ev.evaluate(n_eval)                          # syncs the actor itself
            return out, ev.last["steps"], ev.last["steps_needed"]

        first = eager()[0], graph()[0]                         # warm-up; the graph evaluation captures its blocks
        assert first[0] == first[1], first                     # equal seeds, first evaluation: the same episodes
        runs = {"eager": [], "graph": []}
        for _ in range(args.repeats):
            for key, fn in (("eager", eager), ("graph", graph)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out, steps, needed = fn()
                runs[key].append(dict(ms=(time.perf_counter() - t0) * 1e3, steps=steps, steps_needed=needed,
                                      mean_reward=out[0]))
        eng_e.poll_error()
        eng_g.poll_error()
        doc = dict(n_envs=n, n_eval_episodes=n_eval, refill_every=REFILL_EVERY, block_steps=ev.K,
                   graphs_captured=len(ev.graphs))
        per = {}
        for key, rs in runs.items():
            ms = [r["ms"] for r in rs]
            per[key] = [1e3 * r["ms"] / r["steps_needed"] for r in rs]       # the repeats differ in their episodes
            doc[key] = dict(wall=_stat(ms), steps=[r["steps"] for r in rs],
                            steps_needed=[r["steps_needed"] for r in rs],
                            us_per_needed_step=dict(median=statistics.median(per[key]), min=min(per[key]),
                                                    max=max(per[key])))
        e, g = [r["ms"] for r in runs["eager"]], [r["ms"] for r in runs["graph"]]
        doc.update(wall_ratio_eager_over_graph=statistics.median(e) / statistics.median(g),
                   every_graph_run_below_every_eager_run=max(g) < min(e), ranges_overlap=max(g) >= min(e),
                   per_needed_step_ratio_eager_over_graph=statistics.median(per["eager"]) /
                   statistics.median(per["graph"]),
                   per_needed_step_ranges_overlap=max(per["graph"]) >= min(per["eager"]))
        res[name] = doc
        del ev, act_e, act_g, eng_e, eng_g
        torch.cuda.empty_cache()
    return res


def part_record(args, torch):
    from mgx.evaluation import EvalRecords
    res, launches = {}, 256
    dev = torch.device("cuda", torch.cuda.current_device())
    for n, n_eval in SHAPES.values():
        cap = max(1, -(-n_eval // n))
        g = torch.Generator().manual_seed(n)
        done = (torch.rand(n, generator=g) < 0.02).to(torch.uint8).to(dev)
        r = torch.rand(n, generator=g, dtype=torch.float64).to(dev)
        ln = torch.randint(1, 65, (n,), generator=g, dtype=torch.int32).to(dev)
        mid = torch.randint(0, 256, (n,), generator=g).to(torch.uint8).to(dev)
        rec = EvalRecords(n, cap, dev)
        idx = torch.arange(n, device=dev)
        targets = (n_eval + idx) // n
        counts = torch.zeros(n, dtype=torch.int64, device=dev)
        rew = torch.zeros((n, cap), dtype=torch.float64, device=dev)
        lens = torch.zeros((n, cap), dtype=torch.int64, device=dev)
        when = torch.full((n, cap), -1, dtype=torch.int64, device=dev)

        def kernel(t):
            rec.record(done, r, None, ln, mid, n_eval, step_offset=t)

        def eager(t):                                          # evaluate_policy's accounting lines, its host read too
            if not bool((counts < targets).any()):
                return
            rc = done.bool() & (counts < targets)
            slot = counts.clamp(max=cap - 1)
            rew[idx, slot] = torch.where(rc, r, rew[idx, slot])
            lens[idx, slot] = torch.where(rc, ln.long(), lens[idx, slot])
            when[idx, slot] = torch.where(rc, torch.full_like(counts, t), when[idx, slot])
            counts.add_(rc.long())

        out = {}
        for key, fn in (("mgx_eval_record", kernel), ("eager_accounting", eager)):
            us = []
            for _ in range(max(args.repeats, 12)):
                rec.begin(n_eval)
                counts.zero_()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                a.record()
                for t in range(launches):
                    fn(t)
                b.record()
                b.synchronize()
                us.append((1e3 * a.elapsed_time(b) / launches, 1e6 * (time.perf_counter() - t0) / launches))
            out[key] = dict(device_us_per_step=dict(median=statistics.median(u[0] for u in us),
                                                    min=min(u[0] for u in us), max=max(u[0] for u in us)),
                            wall_us_per_step=dict(median=statistics.median(u[1] for u in us),
                                                  min=min(u[1] for u in us), max=max(u[1] for u in us)))
        res["%d_envs" % n] = dict(n_envs=n, n_eval_episodes=n_eval, launches=launches, **out)
    return res


PARTS = {"evaluate": part_evaluate, "record": part_record}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_graph_eval"))
    ap.add_argument("--sha", default="")
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--part", default="all", choices=["all"] + list(PARTS))
    args = ap.parse_args()
    if args.repeats < 12:
        ap.error("--repeats must be at least 12")
    import torch
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "eval.json")
    doc = {}
    if args.part != "all" and os.path.exists(path):
        doc = json.load(open(path))
    doc.update(build=args.sha, device=torch.cuda.get_device_name(0), torch=torch.__version__,
               method="alternating repeats in one process after a warm-up evaluation; wall = host time of the whole "
                      "call, the final read included; median (min, max) in ms; record: 256 launches between two "
                      "device events, per launch")
    for name, fn in PARTS.items():
        if args.part in ("all", name):
            doc[name] = fn(args, torch)
            print(name, json.dumps(doc[name]))
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
