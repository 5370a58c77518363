#!/usr/bin/env python
"""Two builds of libmgx.so against each other on the fused policy path: exact bits and speed.

A refactor of the kernels behind mgx_gather_ring, mgx_policy_act, mgx_policy_bootstrap, mgx_policy_act_moe and
mgx_policy_backward must change neither a bit of what they compute nor their speed.  Build the parent commit's library to a second path (`make OUT=...`) and run
  python tools/ab_policy_libs.py --parent PATH/libmgx_parent.so [--new minigrid-rl_amd/mgx/libmgx.so] [--out DIR]
Each library is loaded through MGX_LIB_PATH in child processes of its own, every child under its own time limit;
the first failure ends the run.

bits  tests/test_fused_policy_gpu.py's fixture (70 envs, a ring of 3 rows, 40 random steps; seeded, so both children
      see the same buffer) at n_stack 1, 4, 5, 8 x without / with terminal rows x 1, 64, 65, 200 samples: the gather's
      image, direction and mission in u8 and f32; mgx_policy_act's logits and values (mode 0), actions and log-probs
      (mode 1, and mode 2 with one seed and a zeroed counter); mgx_policy_act_moe's the same in the three modes and
      words 0..17 of its route record, for mixtures of 1 and 4 experts (mission id m -> expert m % E);
      mgx_policy_backward's grad_blob at max_groups 2, and grad_mission_feat where the samples fit one tile (<= 64:
      across tiles its atomic order is run-dependent even for one library).  Per n_stack also mgx_policy_bootstrap
      of the fixture's last step: the rewards, the list, the count and the values.  Random actions end this
      fixture's episodes long before max_steps, so no step of it truncates an env: the step's flags are drawn from
      the seeded generator (truncated for half of the envs, terminated for a quarter) and the terminal rows are
      random bytes, as tests/test_graph_collect_gpu.py does; a count of 0 fails the child, the parent's counts are
      recorded.  Compared byte for byte -> OUT/bits.json; any differing tensor makes the run fail.
time  config 3's env, 65,536 envs, n_stack 4: FusedActor.act, FusedEvaluator.forward_raw and backward_raw (+ fold),
      FusedMoEActor.act (4 experts) and FusedActor.bootstrap (every 4th env flagged truncated),
      device events after a warm-up, 20 repeats per child; children in the order parent, new, parent, new, so that
      the parent's spread over two loads of the same library is measured in the same run.  Per timing: the medians
      and ranges of every child and of each library's 40 pooled repeats; `within_parent_range` = the new library's
      pooled median exceeds the parent's by no more than the parent's pooled range (max - min).  The first child of
      each library also times whole Trainer.train calls with fused_update on.  -> OUT/time.json; a timing outside
      the parent's range makes the run fail.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "minigrid-rl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

ENV3 = dict(problem="multi", mission=2, size=8, num_objects=4)
FIXTURE = dict(problem="gtg", mission=5, size=6, num_objects=2)      # tests/test_fused_policy_gpu.py: ENV
N_ENVS, T_RING, STEPS = 70, 3, 40
STACKS, COUNTS, MAX_GROUPS = (1, 4, 5, 8), (1, 64, 65, 200), 2
EXPERTS = (1, 4)                                                     # mixtures; mission id m goes to expert m % E
GAMMA = 0.99
TIMINGS = ("act", "forward_raw", "backward_raw_and_fold", "moe_act", "bootstrap")


def _stat(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), repeats=len(ms))


def _timed(fn, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def part_bits(args):
    import numpy as np
    import torch
    import test_fused_policy_gpu as T
    from mgx import MgxEngine
    from mgx.compact import CompactBuffer
    from mgx.fused_policy import FusedActor
    from mgx.fused_train import FusedEvaluator
    from mgx.moe import FusedMoEActor, MoEPolicy
    out, counts = {}, {}
    for k in STACKS:
        pol = T._policy(k).cuda()
        eng = MgxEngine(n_envs=N_ENVS, n_stack=k, terminal_mode="truncated", mission_dtype=torch.uint8, **FIXTURE)
        buf = CompactBuffer(eng, T_RING, ring=True)
        actor = FusedActor(pol, eng, seed=1234)
        ev = FusedEvaluator(pol, eng, max_groups=MAX_GROUPS)
        experts = [pol] + [T._policy(k, seed).cuda() for seed in range(1, max(EXPERTS))]
        mixtures = {n_exp: FusedMoEActor(MoEPolicy(experts[:n_exp], torch.arange(256) % n_exp), eng, seed=1234)
                    for n_exp in EXPERTS}
        eng.reset()
        buf.observe(0)
        g = torch.Generator().manual_seed(5)
        t = 0
        for _ in range(STEPS):
            buf.step(t, torch.randint(0, 7, (N_ENVS,), generator=g).cuda())
            t += 1
            if t == T_RING:
                buf.carry_over()
                t = 0
        for n in COUNTS:                                   # observations 0..t of the current rollout, with repeats
            obs_t = torch.randint(0, t + 1, (n,), generator=g)
            env = torch.randint(0, N_ENVS, (n,), generator=g)
            index = buf.index(obs_t, env).to(torch.int64).cuda().contiguous()
            gl, gv = torch.randn((n, 7), generator=g).cuda(), torch.randn(n, generator=g).cuda()
            for term in (False, True):
                tag = "k%d/terminal%d/n%d/" % (k, term, n)
                for f32 in (False, True):
                    for name, v in buf.gather(index, terminal=term, f32=f32).items():
                        out[tag + "gather_%s_%s" % ("f32" if f32 else "u8", name)] = v
                _, values, _, logits = actor._run(buf, index, 0, terminal=term, logits=True)
                out[tag + "mode0_logits"], out[tag + "mode0_values"] = logits, values
                a1, _, lp1, _ = actor._run(buf, index, 1, terminal=term)
                out[tag + "mode1_actions"], out[tag + "mode1_log_probs"] = a1, lp1
                actor.counter.zero_()
                a2, _, lp2, _ = actor._run(buf, index, 2, terminal=term)
                out[tag + "mode2_actions"], out[tag + "mode2_log_probs"] = a2, lp2
                for n_exp, mix in mixtures.items():
                    mtag = tag + "moe%d_" % n_exp
                    _, values, _, logits = mix._run(buf, index, 0, terminal=term, logits=True)
                    out[mtag + "mode0_logits"], out[mtag + "mode0_values"] = logits, values
                    out[mtag + "route_record"] = mix.last_route[:18].clone()
                    a1, _, lp1, _ = mix._run(buf, index, 1, terminal=term)
                    out[mtag + "mode1_actions"], out[mtag + "mode1_log_probs"] = a1, lp1
                    mix.counter.zero_()
                    a2, _, lp2, _ = mix._run(buf, index, 2, terminal=term)
                    out[mtag + "mode2_actions"], out[mtag + "mode2_log_probs"] = a2, lp2
            tag = "k%d/n%d/" % (k, n)
            gb, gm = ev.backward_raw(buf, index, actor.blob, actor.mission_feat, gl, gv)
            out[tag + "grad_blob"] = gb
            if n <= 64:
                out[tag + "grad_mission_feat"] = gm
        # the bootstrap of the last step (last, because it draws the step's flags and the terminal rows)
        buf.truncated[t - 1].copy_(torch.rand(N_ENVS, generator=g) < 0.5)
        buf.terminated[t - 1].copy_(torch.rand(N_ENVS, generator=g) < 0.25)
        rows = torch.randint(0, 256, buf.terminal_rows.shape, generator=g).to(torch.uint8)
        rows[:, 0] %= 4
        buf.terminal_rows.copy_(rows)
        rew, val = torch.linspace(-1.0, 1.0, N_ENVS).cuda(), torch.full((N_ENVS,), 7.0).cuda()
        actor.boot_list.fill_(-1)
        actor.bootstrap(buf, t - 1, GAMMA, rewards=rew, values=val)
        counts[k] = int(actor.boot_count)
        if not 0 < counts[k] < N_ENVS:
            raise SystemExit("bootstrap: %d of %d envs selected" % (counts[k], N_ENVS))
        tag = "k%d/bootstrap/" % k
        out[tag + "rewards"], out[tag + "values"] = rew, val
        out[tag + "list"], out[tag + "count"] = actor.boot_list.clone(), actor.boot_count.clone()
        eng.poll_error()
    np.savez(args.save, **{name: v.cpu().numpy() for name, v in out.items()})
    return dict(tensors=len(out), bootstrap_counts=counts)


def part_time(args):
    import torch
    from mgx import MgxEngine
    from mgx.compact import CompactBuffer
    from mgx.fused_policy import FusedActor
    from mgx.fused_train import FusedEvaluator
    from mgx.moe import FusedMoEActor, MoEPolicy
    from mgx.policy import ActorCriticPolicy
    n, k = args.envs, 4
    torch.manual_seed(0)
    eng = MgxEngine(n_envs=n, n_stack=k, terminal_mode="truncated", mission_dtype=torch.uint8, **ENV3)
    pol = ActorCriticPolicy(n_stack=k, mission_cache=True).to(eng.device)
    pol.train(False)
    buf = CompactBuffer(eng, 16, ring=True)
    eng.reset()
    buf.observe(0)
    for t in range(8):                                                         # populated stacks, episode starts
        buf.step(t, torch.randint(0, 7, (n,), device=eng.device))
    actor = FusedActor(pol, eng, seed=1)
    ev = FusedEvaluator(pol, eng)
    index = buf.index(8, buf._arange).to(torch.int64).contiguous()
    gl, gv = torch.randn((n, 7), device=eng.device), torch.randn(n, device=eng.device)
    experts = [pol] + [ActorCriticPolicy(n_stack=k, mission_cache=True).to(eng.device) for _ in range(3)]
    mix = FusedMoEActor(MoEPolicy(experts, torch.arange(256) % 4), eng, seed=1)
    buf.truncated[7].copy_(torch.arange(n, device=eng.device) % 4 == 0)        # the bootstrap's work: every 4th env
    buf.terminated[7].zero_()
    rew = torch.zeros(n, device=eng.device)
    fns = dict(act=lambda: actor.act(buf, 8),
               forward_raw=lambda: ev.forward_raw(buf, index, actor.blob, actor.mission_feat),
               backward_raw_and_fold=lambda: ev.backward_raw(buf, index, actor.blob, actor.mission_feat, gl, gv),
               moe_act=lambda: mix.act(buf, 8),
               bootstrap=lambda: actor.bootstrap(buf, 7, GAMMA, rewards=rew))
    for _ in range(5):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(args.repeats):
        for name, fn in fns.items():
            ms[name].append(_timed(fn, torch))
    eng.poll_error()
    res = dict(n_envs=n, n_stack=k, env=ENV3, ms=ms)
    if args.train:
        res["train_fused_update_ms"] = _train(args, torch)
    return res


def _train(args, torch):
    """Whole Trainer.train calls (fused_train, fused_mission and fused_update on) on one collected rollout."""
    from mgx import MgxEngine
    from mgx.policy import ActorCriticPolicy
    from mgx.ppo import PPOConfig, Trainer, make_collector
    n = args.envs
    cfg = PPOConfig(n_envs=n, horizon=16, batch_size=65536, n_frames_stack=4, env=ENV3, fused_act=True,
                    fused_train=True, fused_mission=True, fused_update=True)
    torch.manual_seed(0)
    eng = MgxEngine(n_envs=n, seed=42, n_stack=4, terminal_mode="truncated", mission_dtype=torch.uint8,
                    reward64=True, **ENV3)
    pol = ActorCriticPolicy(n_stack=4, mission_cache=True).to(eng.device)
    col = make_collector(eng, pol, cfg)
    col.start()
    ro = col.collect()
    pol.optimizer = torch.optim.Adam(pol.parameters(), lr=3e-4, eps=cfg.optim_eps)
    trainer = Trainer(pol, cfg)
    trainer.train(ro, 1.0)
    torch.cuda.synchronize()
    ms = [_timed(lambda: trainer.train(ro, 1.0), torch) for _ in range(3)]
    eng.poll_error()
    return ms


PARTS = {"bits": (part_bits, 540), "time": (part_time, 540)}


def _child(args, part, lib, extra):
    cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--envs", str(args.envs),
           "--repeats", str(args.repeats)] + extra
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=PARTS[part][1],
                       env=dict(os.environ, MGX_LIB_PATH=lib))
    text = p.stdout.decode(errors="replace")
    lines = [ln for ln in text.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        sys.stderr.write(text[-4000:])
        sys.stderr.write("\n%s with %s failed (exit %d): stopping\n" % (part, lib, p.returncode))
        return None
    return json.loads(lines[-1][7:])


def _write(path, obj):
    with open(path, "w") as f:
        json.dump(obj, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the parent commit's library (make OUT=...)")
    ap.add_argument("--new", default=os.path.join(ROOT, "minigrid-rl_amd", "mgx", "libmgx.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_policy_shared"))
    ap.add_argument("--only", choices=sorted(PARTS), default=None, help="run one of the two comparisons")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--part", choices=sorted(PARTS), default=None, help="(internal) run one part in this process")
    ap.add_argument("--save", default=None, help="(internal) bits: the .npz to write")
    ap.add_argument("--train", action="store_true", help="(internal) time: also time Trainer.train")
    args = ap.parse_args()
    if args.part:
        print("RESULT " + json.dumps(PARTS[args.part][0](args)))
        return 0
    if not args.parent:
        ap.error("--parent is required")
    if args.repeats < 20:
        ap.error("--repeats must be >= 20")
    libs = dict(parent=os.path.abspath(args.parent), new=os.path.abspath(args.new))
    meta = {"libmgx_sha256_" + name: hashlib.sha256(open(path, "rb").read()).hexdigest() for name, path in libs.items()}
    os.makedirs(args.out, exist_ok=True)
    ok = True
    if args.only in (None, "bits"):
        import numpy as np
        with tempfile.TemporaryDirectory() as tmp:
            counts = {}
            for name, path in libs.items():
                r = _child(args, "bits", path, ["--save", os.path.join(tmp, name + ".npz")])
                if r is None:
                    return 1
                counts[name] = r["bootstrap_counts"]
            a, b = (np.load(os.path.join(tmp, name + ".npz")) for name in ("parent", "new"))
            names = sorted(a.files)
            differing = [nm for nm in names if nm not in b.files or a[nm].dtype != b[nm].dtype or
                         a[nm].shape != b[nm].shape or a[nm].tobytes() != b[nm].tobytes()]
            differing += [nm for nm in b.files if nm not in a.files]
        _write(os.path.join(args.out, "bits.json"),
               dict(meta, fixture=dict(FIXTURE, n_envs=N_ENVS, ring_rows=T_RING, steps=STEPS), n_stack=list(STACKS),
                    sample_counts=list(COUNTS), max_groups=MAX_GROUPS, experts=list(EXPERTS),
                    bootstrap=dict(gamma=GAMMA, parent_count_by_n_stack=counts["parent"]),
                    tensors_compared=len(names),
                    tensors_differing=differing, bitwise_equal=not differing))
        print("bits: %d tensors compared, %d differ %s" % (len(names), len(differing), differing[:10]))
        ok = ok and not differing
    if args.only in (None, "time"):
        runs = []
        for i, name in enumerate(("parent", "new", "parent", "new")):
            r = _child(args, "time", libs[name], ["--train"] if i < 2 else [])
            if r is None:
                return 1
            runs.append(dict(r, lib=name))
            print("time", name, {q: round(statistics.median(r["ms"][q]), 4) for q in TIMINGS})
        res = dict(meta, n_envs=runs[0]["n_envs"], n_stack=runs[0]["n_stack"], env=ENV3, order=[r["lib"] for r in runs])
        for q in TIMINGS:
            pooled = {name: _stat([x for r in runs if r["lib"] == name for x in r["ms"][q]]) for name in libs}
            par = pooled["parent"]
            res[q] = dict(per_child=[dict(_stat(r["ms"][q]), lib=r["lib"]) for r in runs], pooled=pooled,
                          parent_range_ms=par["max_ms"] - par["min_ms"],
                          new_minus_parent_median_ms=pooled["new"]["median_ms"] - par["median_ms"],
                          within_parent_range=pooled["new"]["median_ms"] - par["median_ms"] <= par["max_ms"] - par["min_ms"])
            ok = ok and res[q]["within_parent_range"]
        res["train_fused_update"] = {r["lib"]: _stat(r["train_fused_update_ms"]) for r in runs[:2]}
        _write(os.path.join(args.out, "time.json"), res)
        print("time:", {q: res[q]["within_parent_range"] for q in TIMINGS}, res["train_fused_update"])
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
