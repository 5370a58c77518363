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

--fused-update measures the fused PPO update (mgx_ppo_loss / mgx_adam_step on a flat parameter arena through
mgx/fused_update.py) instead, into profiles/r13_ppo_update: the same minibatch step with fused_train and fused_mission
on and fused_update off and on in alternation (flag off is the path above, unchanged), the pieces of the on-step
each on its own, one whole Trainer.train (4 epochs x 16 minibatches) off and on, and the parity ratios of
tests/test_fused_update_gpu.py's yardstick at the minibatch's and the arena's size.

--graph-train measures the graph-captured update (PPOConfig.graph_train) instead, into
profiles/r16_graph_train/train.json: one whole Trainer.train with fused_train, fused_mission and fused_update on and
graph_train off and on, the same build, 12 alternating repeats after the capture, host wall time and device events,
median (min - max), at (a) the recipe's 16 envs x 1,024 steps, batch 256, 4 epochs and (b) config 3's 65,536 x 16,
batch 65,536; the six calls of one 256-sample step at (a), each timed on its own; and one learn() iteration
(collect + train) at (a) with graph_collect and graph_train both on against both off.  No threshold is set: the figures and whether the ranges overlap are recorded as measured.
"""
import argparse
import copy
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

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


def _update_setup(args, torch):
    """_setup's rollout and two (policy, Trainer) pairs of the same initial weights, fused_train + fused_mission on
    both: fused_update off (the path above, unchanged) and on."""
    import dataclasses
    from mgx.ppo import Trainer
    eng, col, ro, cfgs, pols, _ = _setup(args, torch)
    base = dataclasses.replace(cfgs[True], fused_mission=True)
    cfgs = {False: base, True: dataclasses.replace(base, fused_update=True)}
    trainers = {f: Trainer(pols[f], cfgs[f]) for f in pols}
    return eng, ro, cfgs, pols, trainers


def part_update_step(args):
    import torch
    from mgx.fused_train import FusedEvaluator
    from mgx.fused_update import FusedUpdate, adam_step, ppo_loss
    eng, ro, cfgs, pols, trainers = _update_setup(args, torch)
    cfg = cfgs[True]
    clip, clip_vf = cfg.clip_range, cfg.clip_range_vf
    perm = torch.randperm(ro.T * ro.N, device=eng.device)[:cfg.batch_size]
    index, actions, old_v, old_lp, adv0, ret = next(ro.minibatch_indices(cfg.batch_size, perm))
    index = index.to(torch.int64).contiguous()
    env, t = perm // ro.T, perm % ro.T
    sel = (t * ro.N + env).contiguous()
    rollout = (ro.actions, ro.values, ro.log_probs, ro.advantages, ro.returns)
    rows = int(index.numel())
    ev = FusedEvaluator(pols[False], eng, fused_mission=True)
    ev.prepare(ro.buf)
    up = FusedUpdate(pols[True], eng)
    up.prepare(ro.buf)
    stats_row = torch.zeros(8, device=eng.device)
    stats = dict(pg=[], vf=[], ent=[], kl=[], clipfrac=[])

    def off():                         # Trainer.train's loop body with fused_train + fused_mission, line for line
        pol = pols[False]
        values, log_prob, entropy = ev.evaluate_actions(ro.buf, index, actions)
        adv = (adv0 - adv0.mean()) / (adv0.std() + 1e-8)
        ratio = torch.exp(log_prob - old_lp)
        pl1 = adv * ratio
        pl2 = adv * torch.clamp(ratio, 1 - clip, 1 + clip)
        policy_loss = -torch.min(pl1, pl2).mean()
        values_pred = old_v + torch.clamp(values - old_v, -clip_vf, clip_vf)
        value_loss = torch.nn.functional.mse_loss(ret, values_pred)
        entropy_loss = -torch.mean(entropy)
        loss = policy_loss + cfg.ent_coef * entropy_loss + cfg.vf_coef * value_loss
        with torch.no_grad():
            log_ratio = log_prob - old_lp
            stats["kl"] = [torch.mean((torch.exp(log_ratio) - 1) - log_ratio)]
            stats["clipfrac"] = [torch.mean((torch.abs(ratio - 1) > clip).float())]
        stats["pg"], stats["vf"], stats["ent"] = [policy_loss.detach()], [value_loss.detach()], [entropy_loss.detach()]
        pol.optimizer.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(pol.parameters(), cfg.max_grad_norm)
        pol.optimizer.step()

    def on():
        up.step(ro.buf, index, sel, rollout, cfg, 3e-4, stats_row, adv_mode=1)

    for p in pols.values():
        p.train(True)
    for _ in range(3):
        off(), on()
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for _ in range(args.repeats):
        ms[False].append(_timed(off, torch))
        ms[True].append(_timed(on, torch))
    # the on-step's pieces, each on its own
    a, enc = up.arena, up.ev.mission
    stacks, trows = up.ev._stacks, up.ev._rows
    ws = enc._workspace(stacks.shape[0], stacks.shape[1])
    logits, values, g_logits, g_values = up._buffers(rows)           # the step's own per-size buffers
    state = dict(step=a.step)

    def mission_forward():
        enc.forward_rows(stacks, up._mission, up.table, trows, ws)

    def mission_backward():
        enc.backward_rows(stacks, up._mission, up.g_table.view(-1, 128), trows, ws, out=up._g_mission)

    def adam():
        state["step"] += 1
        adam_step(a.param, a.grad, a.exp_avg, a.exp_avg_sq, 3e-4, state["step"], eps=cfg.optim_eps,
                  max_grad_norm=cfg.max_grad_norm, scratch=up._adam_scratch)

    pieces = dict(
        mission_forward_and_table=mission_forward,
        forward_kernel=lambda: up.ev.forward_raw(ro.buf, index, up._blob, up.table),
        ppo_loss=lambda: ppo_loss(logits, values, *rollout, clip, clip_vf, cfg.ent_coef, cfg.vf_coef, adv_mode=1, sel=sel,
                                  out=(g_logits, g_values, stats_row), scratch=up._loss_scratch),
        backward_kernels=lambda: up.ev.backward_raw(ro.buf, index, up._blob, up.table, g_logits, g_values,
                                                    out=(up._g_blob, up.g_table)),
        # the backward consumes the forward's records: the pair is timed
        mission_forward_and_backward=lambda: (mission_forward(), mission_backward()), adam_step=adam)
    out = {}
    for name, fn in pieces.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        out[name] = _stat([_timed(fn, torch) for _ in range(args.repeats)])
    eng.poll_error()
    s_off, s_on = _stat(ms[False]), _stat(ms[True])
    return dict(n_envs=args.envs, rows=rows, n_stack=4, env=ENV3, table_rows=int(trows.numel()), arena_words=a.words,
                off_leg="Trainer.train's loop body, fused_train + fused_mission, on a pre-indexed minibatch",
                step_fused_update_off=s_off, step_fused_update_on=s_on,
                ranges_overlap=not (s_on["max_ms"] < s_off["min_ms"]),
                on_median_below_off_median=s_on["median_ms"] < s_off["median_ms"],
                ratio_off_over_on=s_off["median_ms"] / s_on["median_ms"], on_pieces=out)


def part_update_train(args):
    import torch
    eng, ro, cfgs, pols, trainers = _update_setup(args, torch)
    for f in (False, True):
        trainers[f].train(ro, 1.0)
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for _ in range(args.repeats):
        for f in (False, True):
            ms[f].append(_timed(lambda: trainers[f].train(ro, 1.0), torch))
    eng.poll_error()
    off, on = _stat(ms[False]), _stat(ms[True])
    cfg = cfgs[True]
    return dict(n_envs=args.envs, horizon=16, n_epochs=cfg.n_epochs, batch_size=cfg.batch_size,
                minibatches=cfg.n_epochs * ((args.envs * 16 + cfg.batch_size - 1) // cfg.batch_size),
                train_fused_update_off=off, train_fused_update_on=on,
                ranges_overlap=not (on["max_ms"] < off["min_ms"]),
                on_median_below_off_median=on["median_ms"] < off["median_ms"],
                ratio_off_over_on=off["median_ms"] / on["median_ms"])


def part_update_parity(args):
    """tests/test_fused_update_gpu.py's yardstick on its synthetic batch at the minibatch's size (every adv_mode, value
    clipping on and off, through sel) and on three Adam steps at the arena's size."""
    import torch
    import test_fused_update_gpu as U
    if not torch.cuda.is_available():
        raise SystemExit("no GPU")
    n = args.parity_samples

    def pack(rows):
        return {name: dict(kernel_abs_dev_vs_fp64=dev, torch_fp32_gpu_abs_dev_vs_fp64=e, bound=bound,
                           ratio=dev / bound if bound else 0.0) for name, dev, e, bound in rows}

    loss = {}
    for adv_mode in (0, 1, 2):
        for vclip in (True, False):
            rows, _, _ = U._loss_compare(n, adv_mode, vclip, True)
            loss["adv_mode %d value_clip %d" % (adv_mode, vclip)] = pack(rows)
    from mgx.fused_update import arena_layout
    words = arena_layout(4)[1]
    adam = {case: pack(U._adam_compare(words, case)[0]) for case in ("clip", "noclip", "off")}
    worst = lambda d: max(v["ratio"] for c in d.values() for v in c.values())  # noqa: E731
    return dict(samples=n, arena_words=words, ppo_loss=loss, adam_step=adam, worst_ratio_ppo_loss=worst(loss),
                worst_ratio_adam_step=worst(adam))


GRAPH_REPEATS = 12
GRAPH_SHAPES = {"a_recipe_16x1024_batch256": dict(n_envs=16, horizon=1024, batch_size=256),
                "b_config3_65536x16_batch65536": dict(n_envs=65536, horizon=16, batch_size=65536)}


def _wall_and_device(fn, torch):
    """(host wall ms between two device synchronisations, device-event ms) of one fn()."""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, a.elapsed_time(b)


def _off_on(off, on):
    return dict(off=off, on=on, ranges_overlap=not (on["max_ms"] < off["min_ms"] or off["max_ms"] < on["min_ms"]),
                on_median_below_off_median=on["median_ms"] < off["median_ms"],
                ratio_off_over_on=off["median_ms"] / on["median_ms"])


def _graph_cfg(shape, **kw):
    from mgx.ppo import PPOConfig
    return PPOConfig(n_frames_stack=4, n_epochs=4, env=ENV3, fused_act=True, fused_train=True, fused_mission=True,
                     fused_update=True, **shape, **kw)


def _graph_leg(cfg, torch, refill_every=0):
    from mgx import MgxEngine
    from mgx.policy import ActorCriticPolicy
    from mgx.ppo import Trainer, make_collector
    torch.manual_seed(0)
    eng = MgxEngine(n_envs=cfg.n_envs, seed=42, n_stack=4, terminal_mode="truncated", mission_dtype=torch.uint8,
                    reward64=True, refill_every=refill_every, **ENV3)
    pol = ActorCriticPolicy(n_stack=4, optim_eps=cfg.optim_eps, mission_cache=True).to(eng.device)
    col = make_collector(eng, pol, cfg)
    col.start()
    return eng, col, Trainer(pol, cfg)


def part_graph_train(args):
    """One Trainer.train on one collected rollout, graph_train off and on in alternation, at both shapes."""
    import torch
    out = {}
    for name, shape in GRAPH_SHAPES.items():
        legs = {f: _graph_leg(_graph_cfg(shape, graph_train=f), torch) for f in (False, True)}
        ros = {f: legs[f][1].collect() for f in legs}
        for _ in range(2):                                           # the first graph leg captures
            for f in legs:
                legs[f][2].train(ros[f], 1.0)
        ms = {f: ([], []) for f in legs}
        for _ in range(GRAPH_REPEATS):
            for f in (False, True):
                w, d = _wall_and_device(lambda: legs[f][2].train(ros[f], 1.0), torch)
                ms[f][0].append(w)
                ms[f][1].append(d)
        for f in legs:
            legs[f][0].poll_error()
        up = legs[True][2].update
        n = shape["n_envs"] * shape["horizon"]
        out[name] = dict(shape, n_epochs=4, minibatch_steps=4 * ((n + shape["batch_size"] - 1) // shape["batch_size"]),
                         graphs_captured=len(up._graphs), mission_table_rows=int(up.ev._rows.numel()),
                         host_wall=_off_on(_stat(ms[False][0]), _stat(ms[True][0])),
                         device_events=_off_on(_stat(ms[False][1]), _stat(ms[True][1])))
        del legs, ros
        torch.cuda.empty_cache()
    return out


def part_graph_pieces(args):
    """Where a minibatch step of the recipe's shape (256 samples) spends its device time: the six calls of the
    captured step launched eagerly one at a time on the graph's own buffers, device events, 20 repeats each."""
    import torch
    from mgx.fused_update import adam_step_sched, ppo_loss
    shape = GRAPH_SHAPES["a_recipe_16x1024_batch256"]
    eng, col, tr = _graph_leg(_graph_cfg(shape, graph_train=True), torch)
    ro = col.collect()
    tr.train(ro, 1.0)                                                # captures; index / sel hold the last permutation
    up, cfg, m = tr.update, tr.cfg, shape["batch_size"]
    b, enc, ev = up._gbuf, up.ev.mission, up.ev
    _, stacks, rows, ws = next(iter(up._graphs.values()))
    index, sel = b["index"][:m], b["sel"][:m]
    logits, values, g_logits, g_values = up._buffers(m)
    rollout = (ro.actions, ro.values, ro.log_probs, ro.advantages, ro.returns)
    a, pg = up.arena, tr.policy.optimizer.param_groups[0]
    b["cursor"].zero_()                                              # 256 entries: enough for every call below

    def mission_forward():
        enc.forward_rows(stacks, up._mission, up.table, rows, ws)

    pieces = dict(
        mission_forward_rows=mission_forward,
        policy_act=lambda: ev.forward_raw(ro.buf, index, up._blob, up.table, out=(logits, values)),
        ppo_loss=lambda: ppo_loss(logits, values, *rollout, cfg.clip_range, cfg.clip_range_vf, cfg.ent_coef, cfg.vf_coef,
                                  adv_mode=1, sel=sel, out=(g_logits, g_values, b["stats"][0]),
                                  scratch=up._loss_scratch),
        policy_backward=lambda: ev.backward_raw(ro.buf, index, up._blob, up.table, g_logits, g_values,
                                                scratch=b["scratch"], out=(up._g_blob, up.g_table)),
        # the backward consumes the forward's records: the pair is timed
        mission_forward_and_backward_rows=lambda: (
            mission_forward(), enc.backward_rows(stacks, up._mission, up.g_table.view(-1, 128), rows, ws,
                                                 out=up._g_mission)),
        adam_step_sched=lambda: adam_step_sched(a.param, a.grad, a.exp_avg, a.exp_avg_sq, b["sched"], b["cursor"],
                                                betas=pg["betas"], eps=pg["eps"], max_grad_norm=cfg.max_grad_norm,
                                                scratch=up._adam_scratch))
    out = {}
    for name, fn in pieces.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        out[name] = _stat([_timed(fn, torch) for _ in range(20)])
    eng.poll_error()
    return dict(shape, mission_table_rows=int(rows.numel()), seq_len=int(stacks.shape[1]), pieces=out)


def part_graph_learn(args):
    """One learn() iteration (collect + train) at the recipe's shape: graph_collect + graph_train both off and both
    on, the engines alike (the graph collect's refill epoch on both), in alternation after three warm iterations."""
    import torch
    from mgx.ppo import graph_refill_every
    shape = GRAPH_SHAPES["a_recipe_16x1024_batch256"]
    every = graph_refill_every(shape["horizon"])
    legs = {f: _graph_leg(_graph_cfg(shape, graph_collect=f, graph_train=f), torch, refill_every=every)
            for f in (False, True)}

    def iteration(f):
        _, col, tr = legs[f]
        tr.train(col.collect(), 1.0)

    for _ in range(3):
        for f in legs:
            iteration(f)
    ms = {f: [] for f in legs}
    for _ in range(GRAPH_REPEATS):
        for f in (False, True):
            ms[f].append(_wall_and_device(lambda: iteration(f), torch)[0])
    for f in legs:
        legs[f][0].poll_error()
    return dict(shape, n_epochs=4, refill_every=every, warm_iterations=3,
                train_graphs_captured=len(legs[True][2].update._graphs),
                collect_graphs_captured=len(legs[True][1].graphs),
                iteration_host_wall=_off_on(_stat(ms[False]), _stat(ms[True])))


PARTS = {"step": (part_step, 420), "train": (part_train, 540), "parity": (part_parity, 540),
         "mission_step": (part_mission_step, 420), "mission_parity": (part_mission_parity, 300),
         "update_step": (part_update_step, 300), "update_train": (part_update_train, 420),
         "update_parity": (part_update_parity, 300), "graph_train": (part_graph_train, 420),
         "graph_learn": (part_graph_learn, 300), "graph_pieces": (part_graph_pieces, 240)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/r10_policy_train (r12_mission_gru with --fused-mission)")
    ap.add_argument("--fused-mission", action="store_true", help="measure the fused mission encoder instead")
    ap.add_argument("--fused-update", action="store_true", help="measure the fused PPO update instead")
    ap.add_argument("--graph-train", action="store_true", help="measure the graph-captured update instead")
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
        args.out = os.path.join(ROOT, "profiles", "r16_graph_train" if args.graph_train else
                                "r13_ppo_update" if args.fused_update else
                                "r12_mission_gru" if args.fused_mission else "r10_policy_train")
    if args.parts is None:
        args.parts = ("graph_train,graph_pieces,graph_learn" if args.graph_train else
                      "update_parity,update_step,update_train" if args.fused_update else
                      "mission_parity,mission_step" if args.fused_mission else "parity,step,train")
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
    if "graph_train" in res or "graph_learn" in res:
        with open(os.path.join(args.out, "train.json"), "w") as f:
            json.dump(dict(meta, repeats=GRAPH_REPEATS, train=res.get("graph_train"), learn=res.get("graph_learn"),
                           step_pieces=res.get("graph_pieces")), f, indent=1, sort_keys=True)
            f.write("\n")
    if "update_parity" in res:
        with open(os.path.join(args.out, "parity.json"), "w") as f:
            json.dump(dict(meta, **res["update_parity"]), f, indent=1, sort_keys=True)
            f.write("\n")
    if "update_step" in res or "update_train" in res:
        with open(os.path.join(args.out, "train.json"), "w") as f:
            json.dump(dict(meta, step=res.get("update_step"), train=res.get("update_train")), f, indent=1,
                      sort_keys=True)
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
