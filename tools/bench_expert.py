#!/usr/bin/env python
"""Device time of the shortest-path expert (mgx_expert_act, mgx/expert.py) and the expert's episode statistics.

Per config -- multi / every mission / locked doors at 8x8 and 16x16, gtg 8x8 -- at 65,536 envs, n_stack 4:
  (a) one mgx_expert_act (int64 actions and costs)
  (b) one mgx_step_compact of the same engine (the expert's own actions)
  (c) one FusedActor.act (mgx_policy_act, sampled) over the same rows: the act the expert labels for
(a), (b) and (c) alternate in one loop after 24 expert-played steps (mid-episode states: carried keys, opened
doors); device events around each call, median of >= 12 repeats with the spread (min, max) beside it.  The step
changes the state, so every repeat's expert call sees another state of the same distribution: the spread of (a)
includes that.  `states`: the share of envs per cost class at the last timed call.
`episodes`: one GraphEvaluator(expert) run of 16,384 episodes over 1,024 envs (refill_every 16; 16 episodes per env:
every env's FIRST episode draws its mission from the same position of the shared MT19937 stream, so one episode per
env would be one task only): mean episode length, solved share (reward > 0) and mean reward, overall and per task --
the project's optimal-length column.

Every config runs in a child process of its own under a time limit; the first failure ends the run.
  python tools/bench_expert.py [--out profiles/rNN_expert] [--sha BUILD] [--envs 65536] [--repeats 12]
writes OUT/expert.json (default OUT: the next free profiles/rNN_expert).
"""
import argparse
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "minigrid-rl_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)

CONFIGS = {
    "multi8": dict(problem="multi", mission=None, size=8, num_objects=4),
    "multi16": dict(problem="multi", mission=None, size=16, num_objects=4),
    "gtg8": dict(problem="gtg", mission=5, size=8, num_objects=4),
}
K, WARM_STEPS, EVAL_ENVS, N_EVAL = 4, 24, 1024, 16384


def _stat(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), repeats=len(ms))


def _timed(fn, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def part_config(args):
    import torch
    from mgx import ExpertActor, GraphEvaluator, MgxEngine, summarize_missions
    from mgx.compact import CompactBuffer
    from mgx.fused_policy import FusedActor
    from mgx.policy import ActorCriticPolicy
    env, n = CONFIGS[args.config], args.envs
    eng = MgxEngine(n_envs=n, n_stack=K, terminal_mode="truncated", mission_dtype=torch.uint8, **env)
    T = WARM_STEPS + 8 + 3 * args.repeats
    buf = CompactBuffer(eng, T)
    eng.reset()
    buf.observe(0)
    expert = ExpertActor(eng)
    torch.manual_seed(0)
    actor = FusedActor(ActorCriticPolicy(n_stack=K).to(eng.device).train(False), eng, seed=1)
    actor.index_table(buf)
    acts = torch.zeros(n, dtype=torch.int64, device=eng.device)
    t = 0

    def label():
        expert.expert_act(out=acts)

    def step():
        nonlocal t
        buf.step(t, acts)
        t += 1

    def policy():
        actor.act(buf, t)

    for _ in range(WARM_STEPS):
        label(), step()
    for _ in range(5):
        label(), step(), policy()
    torch.cuda.synchronize()
    ta, tb, tc = [], [], []
    for _ in range(args.repeats):
        ta.append(_timed(label, torch))
        tb.append(_timed(step, torch))
        tc.append(_timed(policy, torch))
    eng.poll_error()
    cost = expert.last_cost.cpu()
    states = {name: float((cost == c).float().mean()) if c <= 0 else float((cost > 0).float().mean())
              for name, c in (("routed", 1), ("mission_done", 0), ("unsupported", -1), ("drop_routine", -2),
                              ("key_routine", -3), ("gave_up", -4))}
    a, b, c = _stat(ta), _stat(tb), _stat(tc)
    doc = dict(n_envs=n, n_stack=K, env=env, steps_before=WARM_STEPS + 5, expert_act=a, step_compact=b,
               fused_actor_act=c, states=states, ratio_expert_over_act=a["median_ms"] / c["median_ms"],
               ratio_expert_over_step=a["median_ms"] / b["median_ms"],
               expert_costs_more_than_the_act=a["median_ms"] > c["median_ms"])
    eng.close()
    # the optimal-length column: one graph evaluation of the expert
    ee = MgxEngine(n_envs=EVAL_ENVS, n_stack=K, terminal_mode="truncated", mission_dtype=torch.uint8, reward64=True,
                   refill_every=16, **env)
    ev = GraphEvaluator(ExpertActor(ee))
    r, l = ev.evaluate(N_EVAL, return_episode_rewards=True)
    ee.poll_error()
    cols = summarize_missions(r, l, ev.last["mission_ids"])
    doc["episodes"] = dict(n_envs=EVAL_ENVS, n_eval_episodes=N_EVAL, refill_every=16, steps=ev.last["steps"],
                           overall=cols["overall"], per_task=cols["per_task"],
                           length_quartiles=[float(x) for x in statistics.quantiles(l, n=4)],
                           length_min=int(min(l)), length_max=int(max(l)))
    return doc


def _next_out():
    prof = os.path.join(ROOT, "profiles")
    used = [int(m.group(1)) for m in (re.match(r"r(\d+)_", f) for f in os.listdir(prof)) if m]
    return os.path.join(prof, "r%02d_expert" % (max(used, default=0) + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: the next free profiles/rNN_expert")
    ap.add_argument("--sha", default=None, help="build id to record (default: git rev-parse HEAD)")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--config", choices=sorted(CONFIGS), default=None, help="(internal) run one config in this process")
    args = ap.parse_args()
    if args.config:
        print("RESULT " + json.dumps(part_config(args)))
        return 0
    if args.repeats < 12:
        ap.error("--repeats must be >= 12")
    out = args.out or _next_out()
    sha = args.sha
    if sha is None:
        try:
            sha = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            sha = "unknown"
    lib = os.path.join(ROOT, "minigrid-rl_amd", "mgx", "libmgx.so")
    doc = dict(build_sha=sha, libmgx_sha256=hashlib.sha256(open(lib, "rb").read()).hexdigest(),
               method="alternating repeats in one process after a warm-up; device events around each call; median "
                      "(min, max) in ms; episodes: one GraphEvaluator(expert) run per config")
    os.makedirs(out, exist_ok=True)
    for name in ("multi8", "multi16", "gtg8"):
        cmd = [sys.executable, os.path.abspath(__file__), "--config", name, "--envs", str(args.envs),
               "--repeats", str(args.repeats)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
        text = p.stdout.decode(errors="replace")
        lines = [ln for ln in text.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(text[-4000:])
            sys.stderr.write("\n%s failed (exit %d): stopping\n" % (name, p.returncode))
            return 1
        doc[name] = json.loads(lines[-1][7:])
        print(name, json.dumps(doc[name]))
    with open(os.path.join(out, "expert.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
