#!/usr/bin/env python
"""Act-path measurement of the fused actor-critic kernel (mgx_policy_act) against the path it replaces.

At 65,536 envs, n_stack 4, BASELINE config 3's env (multi / 'pick up' / 8x8 / 4 objects):
  (a) gather_step + pol(obs): the stacked fp32 observation, the torch module, the Categorical sample
  (b) FusedActor.act: one launch over the compact rows
  (c) one full CompactRolloutCollector.collect of horizon 16 with fused_act off and on
(a) and (b) alternate in one loop, (c)'s two collectors too; device events after a warm-up, median of >= 20
repeats, the spread (min, max) beside it.  `parity` records the forward-parity figures of
tests/test_fused_policy_gpu.py (kernel and torch fp32 against the fp64 module) per n_stack.

Every part runs in a child process of its own under a time limit; the first failure ends the run.
  python tools/bench_policy_act.py [--out profiles/r08_policy_act] [--sha BUILD] [--envs 65536] [--repeats 20]
writes OUT/act.json and OUT/parity.json.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "minigrid-rl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

ENV3 = dict(problem="multi", mission=2, size=8, num_objects=4)
GFLOP_PER_STEP_65536 = 10.4            # 2 x ~79.4k MAC per sample x 65,536
FP32_VECTOR_PEAK_TFLOPS = 157.3


def _stat(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), repeats=len(ms))


def _timed(fn, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def part_act(args):
    import torch
    from mgx import MgxEngine
    from mgx.compact import CompactBuffer
    from mgx.fused_policy import FusedActor
    from mgx.policy import ActorCriticPolicy
    n, k = args.envs, 4
    torch.manual_seed(0)
    eng = MgxEngine(n_envs=n, n_stack=k, terminal_mode="truncated", mission_dtype=torch.uint8, **ENV3)
    pol = ActorCriticPolicy(n_stack=k, mission_cache=True).to(eng.device)      # learn()'s policy (PPOConfig.mission_cache)
    pol.train(False)
    buf = CompactBuffer(eng, 16, ring=True)
    eng.reset()
    buf.observe(0)
    for t in range(8):                                                         # populated stacks, episode starts
        buf.step(t, torch.randint(0, 7, (n,), device=eng.device))
    actor = FusedActor(pol, eng, seed=1)
    t = 8
    obs = buf.gather_step(t, f32=True)

    def parent():
        with torch.no_grad():
            return pol(buf.gather_step(t, f32=True, out=obs))

    def fused():
        return actor.act(buf, t)

    for _ in range(5):
        parent(), fused()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(args.repeats):
        ta.append(_timed(parent, torch))
        tb.append(_timed(fused, torch))
    eng.poll_error()
    a, b = _stat(ta), _stat(tb)
    tf = GFLOP_PER_STEP_65536 * (n / 65536.0) / b["median_ms"]                  # GFLOP / ms = TFLOP/s
    return dict(n_envs=n, n_stack=k, env=ENV3, parent_gather_plus_policy=a, fused_act=b,
                ratio_parent_over_fused=a["median_ms"] / b["median_ms"],
                fused_tflops=tf, fused_fraction_of_fp32_vector_peak=tf / FP32_VECTOR_PEAK_TFLOPS)


def part_collect(args):
    import torch
    from mgx import MgxEngine
    from mgx.policy import ActorCriticPolicy
    from mgx.ppo import PPOConfig, make_collector
    n = args.envs
    cols = {}
    for fused in (False, True):
        cfg = PPOConfig(n_envs=n, horizon=16, n_frames_stack=4, env=ENV3, fused_act=fused)
        torch.manual_seed(0)
        eng = MgxEngine(n_envs=n, seed=cfg.seed, n_stack=4, terminal_mode="truncated", mission_dtype=torch.uint8,
                        reward64=True, **ENV3)
        pol = ActorCriticPolicy(n_stack=4, mission_cache=cfg.mission_cache).to(eng.device)
        col = make_collector(eng, pol, cfg)
        col.start()
        cols[fused] = (col, eng)
    for _ in range(2):
        for fused in (False, True):
            cols[fused][0].collect()
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for _ in range(args.repeats):
        for fused in (False, True):
            ms[fused].append(_timed(cols[fused][0].collect, torch))
    for col, eng in cols.values():
        eng.poll_error()
    off, on = _stat(ms[False]), _stat(ms[True])
    return dict(n_envs=n, horizon=16, collect_fused_off=off, collect_fused_on=on,
                ratio_off_over_on=off["median_ms"] / on["median_ms"])


def part_parity(args):
    import test_fused_policy_gpu as T
    out = {}
    for k in (1, 3, 4):
        r = T._run(k)
        lp_ref = r.ref_logp.gather(1, r.actions[:, None])[:, 0]
        dev = dict(logits=float((r.logits - r.ref_logits).abs().max()),
                   values=float((r.values - r.ref_values).abs().max()),
                   log_probs=float((r.log_probs - lp_ref).abs().max()))
        out["n_stack_%d" % k] = dict(samples=int(r.logits.shape[0]), kernel_max_abs_dev_vs_fp64=dev,
                                     torch_fp32_gpu_max_abs_dev_vs_fp64=r.e_torch,
                                     bound_4x=r.tol, logit_scale=float(r.ref_logits.abs().max()))
        print("n_stack %d: kernel %s | torch fp32 %s" % (k, dev, r.e_torch))
    return out


PARTS = {"act": (part_act, 420), "collect": (part_collect, 420), "parity": (part_parity, 300)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_policy_act"))
    ap.add_argument("--sha", default=None, help="build id to record (default: git rev-parse HEAD)")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--part", choices=sorted(PARTS), default=None, help="(internal) run one part in this process")
    args = ap.parse_args()
    if args.part:
        print("RESULT " + json.dumps(PARTS[args.part][0](args)))
        return 0
    if args.repeats < 20:
        ap.error("--repeats must be >= 20")
    sha = args.sha
    if sha is None:
        try:
            sha = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            sha = "unknown"
    lib = os.path.join(ROOT, "minigrid-rl_amd", "mgx", "libmgx.so")
    meta = dict(build_sha=sha, libmgx_sha256=hashlib.sha256(open(lib, "rb").read()).hexdigest())
    os.makedirs(args.out, exist_ok=True)
    res = {}
    for name in ("parity", "act", "collect"):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", name, "--envs", str(args.envs),
               "--repeats", str(args.repeats)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=PARTS[name][1])
        text = p.stdout.decode(errors="replace")
        lines = [ln for ln in text.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(text[-4000:])
            sys.stderr.write("\n%s failed (exit %d): stopping\n" % (name, p.returncode))
            return 1
        res[name] = json.loads(lines[-1][7:])
        print(name, json.dumps(res[name]))
    with open(os.path.join(args.out, "parity.json"), "w") as f:
        json.dump(dict(meta, **res["parity"]), f, indent=1, sort_keys=True)
        f.write("\n")
    with open(os.path.join(args.out, "act.json"), "w") as f:
        json.dump(dict(meta, act=res["act"], collect=res["collect"]), f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
