#!/usr/bin/env python3
"""The refill kernel's wave-cost model: union trip counts x static instruction counts.

tools/refill_wave_model.cpp runs the generator on the host and prints, per attempt round, the lane-mean and the
wave-union trip count of every generator loop.  This script builds it (g++, -DMGX_HOST_SIM), runs it for a config
and prices the union counts with the static VALU / SALU counts of the same blocks in `mgx_refill_s8_kernel<64>`
(hipcc -O3 --offload-arch=gfx950 -S, the kernel's loops by their back edges; each block's OWN instructions, its
inner loops taken out).  Modelled instructions per attempt round = sum over blocks of own count x union trips.

  python tools/refill_wave_model.py [--build r18|r07|r06] [--mission 5] [--envs 4096] [--episodes 11] [--wave 64]
                                    [--llw 4096] [--binary PATH] [--out FILE]

The static counts are a table in this file, per build: update it (the comment beside each entry names the loop)
when the generator's code changes.  What the model leaves out: the prefix (looked up in records by the kernel),
the attempt's set-up, the record write and the kernel's prologue -- about a quarter of the wave's instructions.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# block -> (own VALU, own SALU, union count it is multiplied by)
STATIC = {
    # parent of round 7: ten-word passes restarted after a draw that straddles them, word-by-word tail
    "r06": {
        "task loop own":            (564 - 278, 331 - 219, "tasks"),          # while (todo) body less the pass loop
        "draw_cell pass own":       (278 - 40 - 61 - 63, 219 - 35 - 34 - 34, "draw_passes"),
        "draw_cell candidate loop": (40, 35, "cand_iters"),
        "tail randbelow_c loops":   (62, 34, "tail_rb_passes"),               # two inlined loops, 61 and 63 VALU
        "goal/agent loop":          (78, 44, "goal_agent_iters"),             # one PCG64 step: 12 32-bit multiplies
    },
    # round 7: decoder state carried across passes, 10-bit guard masks, goal / agent loop without its stores
    "r07": {
        "task loop own":            (415 - 123, 186 - 63, "tasks"),
        "draw_cell pass own":       (123 - 26, 63 - 23, "draw_passes"),
        "draw_cell candidate loop": (26, 23, "cand_iters"),
        "goal/agent loop":          (65, 26, "goal_agent_iters"),
    },
    # round 18: one loop over the passes of all tasks (task set-up and commit inside it, single exit), per-room
    # constants selected from constants of S.  Priced with the flattened union counts
    "r18": {
        "task + pass loop own":     (317 - 27, 94 - 16, "flat_passes"),       # while (todo) body less the candidate loop
        "candidate loop":           (27, 16, "flat_cand_iters"),
        "goal/agent loop":          (65, 26, "goal_agent_iters"),
    },
}


def build_binary(extra=()):
    out = os.path.join(tempfile.mkdtemp(prefix="refill_wave_model_"), "refill_wave_model")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-DMGX_HOST_SIM",
                           "-I", os.path.join(ROOT, "tests", "host_gen"), "-I", os.path.join(ROOT, "tests", "host_wave"),
                           "-I", os.path.join(ROOT, "minigrid-rl_amd", "csrc"), *extra, "-o", out,
                           os.path.join(ROOT, "tools", "refill_wave_model.cpp")])
    return out


def run_model(binary, mission, size, envs, episodes, wave, llw, cursors=None):
    cmd = [binary, "--mission", str(mission), "--size", str(size), "--envs", str(envs), "--episodes", str(episodes),
           "--wave", str(wave), "--llw", str(llw)]
    if cursors:
        cmd += ["--cursors", cursors]
    return json.loads(subprocess.check_output(cmd).decode())


def price(counts, build):
    rows, tv, ts = [], 0.0, 0.0
    for name, (v, s, key) in STATIC[build].items():
        u = counts["wave_union"][key]
        rows.append(dict(block=name, own_valu=v, own_salu=s, union_trips=u, lane_mean_trips=counts["lane_mean"][key],
                         valu=round(v * u, 1), salu=round(s * u, 1)))
        tv += v * u
        ts += s * u
    return dict(blocks=rows, valu_per_round=round(tv, 1), salu_per_round=round(ts, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", default="r18", choices=sorted(STATIC))
    ap.add_argument("--mission", type=int, default=5, help="-1: drawn (config 4)")
    ap.add_argument("--size", type=int, default=8)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--episodes", type=int, default=11)
    ap.add_argument("--wave", type=int, default=64)
    ap.add_argument("--llw", type=int, default=4096)
    ap.add_argument("--binary", default=None, help="a built refill_wave_model (default: build the tree's)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    binary = a.binary or build_binary()
    counts = run_model(binary, a.mission, a.size, a.envs, a.episodes, a.wave, a.llw)
    res = dict(build=a.build, counts=counts, model=price(counts, a.build))
    txt = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    print(txt)
    return 0


if __name__ == "__main__":
    sys.exit(main())
