#!/usr/bin/env python
"""Update-path measurement of the fused policy gradient (mgx_policy_act + mgx_policy_backward through
mgx/fused_train.py) against the path it replaces (gather + pol.evaluate_actions + torch autograd).

At 65,536 envs, n_stack 4, horizon 16, BASELINE config 3's env (multi / 'pick up' / 8x8 / 4 objects):
  step    one minibatch step of 65,536 rows (evaluate -> loss -> backward -> grad-norm clip -> Adam) with
          PPOConfig.fused_train off and on, two policies of the same initial weights over one rollout; the
          fused step's pieces (differentiable blob + table, forward kernel, backward kernels) timed on their own
  train   one whole Trainer.train (4 epochs x 16 minibatches) off and on, and one collect (fused_act on)
  parity  the per-tensor deviations of tests/test_fused_train_gpu.py's yardstick on one full minibatch:
          kernel path and torch fp32 (GPU) against the fp64 CPU module, N(0, 1) cotangents
The two legs alternate in one loop; device events after a warm-up; median and range (min, max).

Every part runs in a child process of its own under a time limit; the first failure ends the run.
  python tools/bench_policy_train.py [--out profiles/r10_policy_train] [--sha BUILD] [--envs 65536] [--repeats 20]
writes OUT/train.json and OUT/parity.json.

--fused-mission measures the fused mission encoder (mgx_mission_forward / mgx_mission_backward through
mgx/fused_mission.py) instead, into profiles/r12_mission_gru: the same minibatch step with fused_train on and
fused_mission off and on in alternation (flag off is the path above, unchanged), inputs() and its backward alone
for both, and the per-tensor parity ratios of tests/test_fused_mission_gpu.py's yardstick on the rollout's
(mission id, v) table rows.
"""
import argparse
import copy
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
GFLOP_BACKWARD_65536 = 38.0            # 2 x ~0.29 M multiply-adds per sample x 65,536 (forward recompute included)


def _stat(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), repeats=len(ms))


def _timed(fn, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _setup(args, torch):
    """One collected rollout of config 3 and two (policy, Trainer) pairs of the same initial weights: flag off, on."""
    from mgx import MgxEngine
    from mgx.policy import ActorCriticPolicy
    from mgx.ppo import PPOConfig, Trainer, make_collector
    n = args.envs
    cfgs = {f: PPOConfig(n_envs=n, horizon=16, batch_size=65536, n_frames_stack=4, env=ENV3, fused_act=True,
                         fused_train=f) for f in (False, True)}
    torch.manual_seed(0)
    eng = MgxEngine(n_envs=n, seed=42, n_stack=4, terminal_mode="truncated", mission_dtype=torch.uint8,
                    reward64=True, **ENV3)
    pol = ActorCriticPolicy(n_stack=4, mission_cache=True).to(eng.device)
    col = make_collector(eng, pol, cfgs[True])
    col.start()
    ro = col.collect()
    pols = {False: copy.deepcopy(pol), True: pol}
    for f in pols:                                                   # deepcopy keeps the optimizer on the old tensors
        pols[f].optimizer = torch.optim.Adam(pols[f].parameters(), lr=3e-4, eps=cfgs[f].optim_eps)
    trainers = {f: Trainer(pols[f], cfgs[f]) for f in pols}
    return eng, col, ro, cfgs, pols, trainers


def part_step(args):
    import torch
    from mgx.fused_train import FusedEvaluator
    eng, col, ro, cfgs, pols, trainers = _setup(args, torch)
    cfg = cfgs[True]
    perm = torch.randperm(ro.T * ro.N, device=eng.device)
    ev = FusedEvaluator(pols[True], eng)
    ev.prepare(ro.buf)
    batch = {False: next(ro.minibatches(cfg.batch_size, perm)), True: next(ro.minibatch_indices(cfg.batch_size, perm))}
    rows = int(batch[True][0].numel())

    def step(fused):
        pol = pols[fused]
        obs, actions, old_v, old_lp, adv, ret = batch[fused]
        if fused:
            values, log_prob, entropy = ev.evaluate_actions(ro.buf, obs, actions)
        else:
            values, log_prob, entropy = pol.evaluate_actions(obs, actions)
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        ratio = torch.exp(log_prob - old_lp)
        policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - cfg.clip_range, 1 + cfg.clip_range)).mean()
        vp = old_v + torch.clamp(values - old_v, -cfg.clip_range_vf, cfg.clip_range_vf)
        loss = policy_loss - cfg.ent_coef * entropy.mean() + cfg.vf_coef * torch.nn.functional.mse_loss(ret, vp)
        pol.optimizer.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(pol.parameters(), cfg.max_grad_norm)
        pol.optimizer.step()

    for f in pols:
        pols[f].train(True)
    for _ in range(3):
        step(False), step(True)
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for _ in range(args.repeats):
        for f in (False, True):
            ms[f].append(_timed(lambda: step(f), torch))
    # the fused step's pieces
    gl = torch.randn((rows, 7), device=eng.device)
    gv = torch.randn(rows, device=eng.device)
    index = batch[True][0].to(torch.int64).contiguous()
    state = {}

    def inputs():
        state["blob"], state["table"] = ev.inputs()

    def table_backward():
        inputs()
        (state["table"].sum() + state["blob"].sum()).backward()

    inputs()
    blob, table = state["blob"].detach().contiguous(), state["table"].detach().contiguous()
    pieces = dict(inputs_forward=inputs, inputs_forward_and_backward=table_backward,
                  forward_kernel=lambda: ev.forward_raw(ro.buf, index, blob, table),
                  backward_kernels=lambda: ev.backward_raw(ro.buf, index, blob, table, gl, gv))
    out = {}
    for name, fn in pieces.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        out[name] = _stat([_timed(fn, torch) for _ in range(args.repeats)])
    eng.poll_error()
    off, on = _stat(ms[False]), _stat(ms[True])
    bk = out["backward_kernels"]["median_ms"]
    return dict(n_envs=args.envs, rows=rows, n_stack=4, env=ENV3, table_rows=int(ev._rows.numel()),
                step_fused_off=off, step_fused_on=on, ratio_off_over_on=off["median_ms"] / on["median_ms"],
                every_fused_below_every_torch=on["max_ms"] < off["min_ms"], fused_pieces=out,
                backward_tflops=GFLOP_BACKWARD_65536 * (rows / 65536.0) / bk,
                mission_inputs_share_of_fused_step=out["inputs_forward_and_backward"]["median_ms"] / on["median_ms"])


def part_train(args):
    import torch
    eng, col, ro, cfgs, pols, trainers = _setup(args, torch)
    reps = max(3, args.repeats // 4)
    for f in (False, True):
        trainers[f].train(ro, 1.0)
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for _ in range(reps):
        for f in (False, True):
            ms[f].append(_timed(lambda: trainers[f].train(ro, 1.0), torch))
    collect = _stat([_timed(col.collect, torch) for _ in range(reps)])
    eng.poll_error()
    off, on = _stat(ms[False]), _stat(ms[True])
    steps = args.envs * 16
    return dict(n_envs=args.envs, horizon=16, n_epochs=cfgs[True].n_epochs, batch_size=65536,
                train_fused_off=off, train_fused_on=on, ratio_off_over_on=off["median_ms"] / on["median_ms"],
                collect_fused_act=collect,
                iteration_env_steps_per_s=dict(off=steps / (collect["median_ms"] + off["median_ms"]) * 1e3,
                                               on=steps / (collect["median_ms"] + on["median_ms"]) * 1e3))


def part_parity(args):
    import torch
    import test_fused_train_gpu as T
    eng, col, ro, cfgs, pols, trainers = _setup(args, torch)
    pol = pols[True]
    pol.train(True)
    from mgx.fused_train import FusedEvaluator
    n = args.parity_samples
    perm = torch.randperm(ro.T * ro.N, device=eng.device)[:n]
    index = next(ro.minibatch_indices(n, perm))[0].to(torch.int64).contiguous()
    r = T.Run()
    r.k, r.pol, r.buf, r.eng = 4, pol, ro.buf, eng
    r.pol64 = copy.deepcopy(pol).cpu().double()
    obs = {kk: v.clone() for kk, v in ro.buf.gather(index, f32=False).items()}
    gen = torch.Generator().manual_seed(17)
    gl, gv = torch.randn((n, 7), generator=gen), torch.randn(n, generator=gen)
    loss = T._linear_loss(gl, gv)
    ref = T._module_grads(r.pol64, T._out64, obs, loss)
    t32 = T._module_grads(pol, T._out32, obs, loss)
    ev = FusedEvaluator(pol, eng)
    ev.prepare(ro.buf)
    got, _, _ = T._kernel_grads(r, ev, index, gl, gv)
    out = {}
    for name in ref:
        e_torch = float((t32[name] - ref[name]).abs().max())
        scale = float(ref[name].abs().max())
        bound = max(4.0 * e_torch, 4.0 * T.EPS32 * scale)
        dev = float((got[name] - ref[name]).abs().max())
        out[name] = dict(kernel_max_abs_dev_vs_fp64=dev, torch_fp32_gpu_max_abs_dev_vs_fp64=e_torch, bound=bound,
                         ratio=dev / bound, max_abs_ref=scale)
        print("%s: kernel %.3e torch %.3e ratio %.2f" % (name, dev, e_torch, dev / bound))
    eng.poll_error()
    return dict(samples=n, n_stack=4, tensors=out, worst_ratio=max(v["ratio"] for v in out.values()))


def _mission_setup(args, torch):
    """_setup's rollout and policy, and two FusedEvaluators over it: fused_mission off and on."""
    from mgx.fused_train import FusedEvaluator
    eng, col, ro, cfgs, pols, trainers = _setup(args, torch)
    pol = pols[True]
    pol.train(True)
    evs = {f: FusedEvaluator(pol, eng, fused_mission=f) for f in (False, True)}
    for ev in evs.values():
        ev.prepare(ro.buf)
    return eng, ro, cfgs[True], pol, evs


def part_mission_step(args):
    import torch
    eng, ro, cfg, pol, evs = _mission_setup(args, torch)
    perm = torch.randperm(ro.T * ro.N, device=eng.device)
    index, actions, old_v, old_lp, adv, ret = next(ro.minibatch_indices(cfg.batch_size, perm))
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)

    def step(f):
        values, log_prob, entropy = evs[f].evaluate_actions(ro.buf, index, actions)
        ratio = torch.exp(log_prob - old_lp)
        policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - cfg.clip_range, 1 + cfg.clip_range)).mean()
        vp = old_v + torch.clamp(values - old_v, -cfg.clip_range_vf, cfg.clip_range_vf)
        loss = policy_loss - cfg.ent_coef * entropy.mean() + cfg.vf_coef * torch.nn.functional.mse_loss(ret, vp)
        pol.optimizer.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(pol.parameters(), cfg.max_grad_norm)
        pol.optimizer.step()

    def inputs(f):
        blob, table = evs[f].inputs()
        (table.sum() + blob.sum()).backward()

    out = {}
    for name, fn in (("step", step), ("inputs_forward_and_backward", inputs)):
        for _ in range(3):
            fn(False), fn(True)
        torch.cuda.synchronize()
        ms = {False: [], True: []}
        for _ in range(args.repeats):
            for f in (False, True):
                ms[f].append(_timed(lambda: fn(f), torch))
        off, on = _stat(ms[False]), _stat(ms[True])
        out[name] = dict(fused_mission_off=off, fused_mission_on=on, ratio_off_over_on=off["median_ms"] / on["median_ms"],
                         every_on_below_every_off=on["max_ms"] < off["min_ms"])
    eng.poll_error()
    return dict(n_envs=args.envs, rows=int(index.numel()), n_stack=4, env=ENV3, table_rows=int(evs[True]._rows.numel()),
                seq_len=int(evs[True]._stacks.shape[1]), **out)


def part_mission_parity(args):
    import torch
    import test_fused_mission_gpu as M
    from mgx.fused_mission import mission_params
    eng, ro, cfg, pol, evs = _mission_setup(args, torch)
    seq32 = pol.features_extractor.extractors["mission"]
    seq64 = copy.deepcopy(seq32).cpu().double()
    tok = evs[True]._stacks.cpu()
    g = torch.randn((tok.shape[0], 128), generator=torch.Generator().manual_seed(17))
    ref = M._module(seq64, tok.long(), g)
    t32 = M._module(seq32, tok.long().to(eng.device), g.to(eng.device))
    c = M.Ctx()
    c.enc, c.params = evs[True].mission, mission_params(pol)
    got = M._kernel(c, tok, g)
    tensors = dict(ref[1], features=ref[0])
    t32 = dict(t32[1], features=t32[0])
    got = dict(got[1], features=got[0])
    out = {}
    for name in tensors:
        e_torch = float((t32[name] - tensors[name]).abs().max())
        scale = float(tensors[name].abs().max())
        bound = max(4.0 * e_torch, 4.0 * M.EPS32 * scale)
        dev = float((got[name].double().cpu() - tensors[name]).abs().max())
        out[name] = dict(kernel_max_abs_dev_vs_fp64=dev, torch_fp32_gpu_max_abs_dev_vs_fp64=e_torch, bound=bound,
                         ratio=dev / bound, max_abs_ref=scale)
        print("%s: kernel %.3e torch %.3e ratio %.2f" % (name, dev, e_torch, dev / bound))
    return dict(table_rows=int(tok.shape[0]), seq_len=int(tok.shape[1]), tensors=out,
                worst_ratio=max(v["ratio"] for v in out.values()))


PARTS = {"step": (part_step, 420), "train": (part_train, 540), "parity": (part_parity, 540),
         "mission_step": (part_mission_step, 420), "mission_parity": (part_mission_parity, 300)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/r10_policy_train (r12_mission_gru with --fused-mission)")
    ap.add_argument("--fused-mission", action="store_true", help="measure the fused mission encoder instead")
    ap.add_argument("--sha", default=None, help="build id to record (default: git rev-parse HEAD)")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--parity-samples", type=int, default=65536)
    ap.add_argument("--parts", default=None, help="default: parity,step,train (mission_parity,mission_step)")
    ap.add_argument("--part", choices=sorted(PARTS), default=None, help="(internal) run one part in this process")
    args = ap.parse_args()
    if args.part:
        print("RESULT " + json.dumps(PARTS[args.part][0](args)))
        return 0
    if args.repeats < 20:
        ap.error("--repeats must be >= 20")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "r12_mission_gru" if args.fused_mission else "r10_policy_train")
    if args.parts is None:
        args.parts = "mission_parity,mission_step" if args.fused_mission else "parity,step,train"
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
    for name in args.parts.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", name, "--envs", str(args.envs),
               "--repeats", str(args.repeats), "--parity-samples", str(args.parity_samples)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=PARTS[name][1])
        text = p.stdout.decode(errors="replace")
        lines = [ln for ln in text.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(text[-4000:])
            sys.stderr.write("\n%s failed (exit %d): stopping\n" % (name, p.returncode))
            return 1
        res[name] = json.loads(lines[-1][7:])
        print(name, json.dumps(res[name]))
    if "mission_parity" in res:
        with open(os.path.join(args.out, "parity.json"), "w") as f:
            json.dump(dict(meta, **res["mission_parity"]), f, indent=1, sort_keys=True)
            f.write("\n")
    if "mission_step" in res:
        with open(os.path.join(args.out, "train.json"), "w") as f:
            json.dump(dict(meta, **res["mission_step"]), f, indent=1, sort_keys=True)
            f.write("\n")
    if "parity" in res:
        with open(os.path.join(args.out, "parity.json"), "w") as f:
            json.dump(dict(meta, **res["parity"]), f, indent=1, sort_keys=True)
            f.write("\n")
    if "step" in res or "train" in res:
        with open(os.path.join(args.out, "train.json"), "w") as f:
            json.dump(dict(meta, step=res.get("step"), train=res.get("train")), f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
