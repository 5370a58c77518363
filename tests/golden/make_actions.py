"""Generate the action scripts under tests/golden/actions/: the scripted agent (scripted_agent.py) run over
the C oracle at block scale -- hundreds of envs, so that many envs of one workgroup dirty their grids, pop
episodes and truncate on the same step.  A script stores the actions (int8 [T][n]) and the config alone; the
tests replay it through the oracle and the kernels.  No reference needed: the oracle is pinned to the
reference by the fixtures, and tests/test_scripted_agent.py ties the agent's oracle runs to its reference runs.

Usage:  python tests/golden/make_actions.py [--only NAME]
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)

import oracle as O  # noqa: E402
import scripted_agent as SA  # noqa: E402

SEED, AGENT_SEED = 42, 1234
# n = 520: eight 64-env blocks and eight envs (sixteen 32-env blocks and eight in the fused rollout at S = 16);
# T: a multiple of 32 above 2 * size^2 (above size^2 at S = 16)
SCRIPTS = [("multi_all_s8", dict(problem="multi", mission=None, size=8), 520, 160),
           ("multi_tgl_s16", dict(problem="multi", mission=1, size=16), 520, 288),
           ("full_s8", dict(problem="full", mission=None, size=8), 200, 160)]


def make(cfg, n, T):
    ov = O.OracleVec(cfg["problem"], cfg["mission"], cfg["size"], 4, n, SEED)
    ov.reset()
    acts = SA.run(ov, SA.ScriptedAgent(n, AGENT_SEED), T)
    m = cfg["mission"]
    return dict(actions=acts, problem=np.array(cfg["problem"]), mission=np.array(-1 if m is None else m, np.int64),
                size=np.array(cfg["size"], np.int64), num_objects=np.array(4, np.int64), seed=np.array(SEED, np.int64),
                agent_seed=np.array(AGENT_SEED, np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    out_dir = os.path.join(HERE, "actions")
    os.makedirs(out_dir, exist_ok=True)
    for name, cfg, n, T in SCRIPTS:
        if args.only and args.only != name:
            continue
        t0 = time.time()
        d = make(cfg, n, T)
        np.savez_compressed(os.path.join(out_dir, name + ".npz"), **d)
        print("%-16s n=%d T=%d %6.1fs" % (name, n, T, time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
