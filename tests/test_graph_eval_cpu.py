"""Graph-captured evaluation (mgx.evaluation.GraphEvaluator, mgx_eval_record): everything that can be checked
without a GPU -- the numpy restatement of the kernel against the loop body of evaluate_policy, the schedule of a
deferred callback, summarize_missions, the argument checks of the entry point and the ValueError paths."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mgx import _lib  # noqa: E402
from mgx.evaluation import (EvalCallback, StopTrainingOnRewardThreshold, eval_record_reference,  # noqa: E402
                            evaluate_policy, summarize_missions)
from mgx.ppo import check_graph_callback, deferred_on_steps  # noqa: E402


# ---------------------------------------------------------------- 1. the reference against evaluate_policy's loop body
def _eager_body(st, done, r, ep_len, n_eval, t):
    """The accounting lines of evaluate_policy's loop (rec = done & (counts < targets) ... counts += rec) on CPU
    tensors, verbatim but for the names of the inputs."""
    counts, rew, lens, when = st["counts"], st["rew"], st["lens"], st["when"]
    n, cap = rew.shape
    idx = torch.arange(n)
    targets = (n_eval + idx) // n
    rec = done & (counts < targets)
    slot = counts.clamp(max=cap - 1)
    rew[idx, slot] = torch.where(rec, r, rew[idx, slot])
    lens[idx, slot] = torch.where(rec, ep_len.long(), lens[idx, slot])
    when[idx, slot] = torch.where(rec, torch.full_like(counts, t), when[idx, slot])
    counts += rec.long()


@pytest.mark.parametrize("n,n_eval", [(1, 3), (5, 0), (5, 3), (5, 5), (7, 23), (64, 63), (65, 200)])
def test_reference_equals_the_eager_loop_body(n, n_eval):
    """Random done / reward / length sequences, 40 steps: counts and the three tables of the eager loop equal the
    reference's after every step; n_eval < n leaves envs with target 0, n_eval = 0 records nothing at all."""
    g = np.random.default_rng(100 * n + n_eval)
    cap = max(1, (n_eval + n - 1) // n)
    st = dict(counts=torch.zeros(n, dtype=torch.int64), rew=torch.zeros((n, cap), dtype=torch.float64),
              lens=torch.zeros((n, cap), dtype=torch.int64), when=torch.full((n, cap), -1, dtype=torch.int64))
    ref = dict(counts=np.zeros(n, np.int32), rewards=np.zeros((n, cap)), lengths=np.zeros((n, cap), np.int32),
               when=np.full((n, cap), -1, np.int64), missions=np.full((n, cap), 255, np.uint8), remaining=n_eval)
    seen = []
    for t in range(40):
        done = g.random(n) < 0.35
        r = np.where(g.random(n) < 0.5, 0.0, g.random(n))
        ep_len = g.integers(1, 65, n).astype(np.int32)
        mids = g.integers(0, 256, n).astype(np.uint8)
        _eager_body(st, torch.as_tensor(done), torch.as_tensor(r), torch.as_tensor(ep_len), n_eval, t)
        before = ref["counts"].copy()
        eval_record_reference(ref, done, r, ep_len, mids, n_eval, t)
        seen += [(t, e, int(mids[e])) for e in range(n) if ref["counts"][e] != before[e]]
        assert np.array_equal(st["counts"].numpy(), ref["counts"]), t
        assert np.array_equal(st["rew"].numpy(), ref["rewards"]), t
        assert np.array_equal(st["lens"].numpy(), ref["lengths"]), t
        assert np.array_equal(st["when"].numpy(), ref["when"]), t
        assert ref["remaining"] == n_eval - int(ref["counts"].sum()), t
    targets = (n_eval + np.arange(n)) // n
    assert int(targets.sum()) == n_eval                      # what the host sets `remaining` to
    assert np.all(ref["counts"] <= targets)
    if n_eval < n:
        assert np.all(ref["counts"][:n - n_eval] == 0)        # target 0: never recorded
    if n_eval == 0:
        assert not seen and np.all(ref["when"] == -1) and np.all(ref["missions"] == 255)
    for t, e, m in seen:                                      # the mission of the step that recorded, in its slot
        k = int(np.nonzero(ref["when"][e] == t)[0][0])
        assert ref["missions"][e, k] == m
    assert np.all(ref["missions"][ref["when"] < 0] == 255)    # empty slots untouched


# ---------------------------------------------------------------- 2. the deferred callback schedule
class _Policy:
    training = False

    def train(self, mode=True):
        self.training = mode


class _Every:
    """EvalCallback's trigger rule without an evaluation: every eval_freq calls; False at the stop_at-th trigger."""
    deferrable = True

    def __init__(self, eval_freq, stop_at=None):
        self.eval_freq, self.stop_at, self.n_calls, self.calls, self.triggers = eval_freq, stop_at, 0, [], []

    def on_step(self, policy, num_timesteps):
        self.n_calls += 1
        self.calls.append(num_timesteps)
        if self.n_calls % self.eval_freq:
            return True
        self.triggers.append(num_timesteps)
        return len(self.triggers) != self.stop_at


@pytest.mark.parametrize("horizon,n_envs,eval_freq", [(16, 8, 24), (16, 8, 5), (4, 70, 1), (12, 3, 12)])
def test_deferred_schedule_equals_the_per_step_schedule(horizon, n_envs, eval_freq):
    """Three rollouts: a deferred callback sees one call per step, in order, each with that step's num_timesteps --
    the calls and triggers of a callback stepped inside the loop."""
    cb, pol = _Every(eval_freq), _Policy()
    ts = 0
    for _ in range(3):
        assert deferred_on_steps(cb, pol, ts, n_envs, horizon) is None
        ts += horizon * n_envs
    want = [(k + 1) * n_envs for k in range(3 * horizon)]
    assert cb.calls == want
    assert cb.triggers == [x for k, x in enumerate(want) if (k + 1) % eval_freq == 0]
    assert pol.training is False


def test_deferred_stop_reports_the_step_that_stopped():
    """False at the second trigger (call 10 of eval_freq 5, step 2 of the second 8-step rollout): the helper returns
    that step's count and calls nothing after it."""
    cb, pol = _Every(5, stop_at=2), _Policy()
    assert deferred_on_steps(cb, pol, 0, 4, 8) is None
    assert deferred_on_steps(cb, pol, 32, 4, 8) == 32 + 2 * 4
    assert cb.n_calls == 10 and cb.calls[-1] == 40 and cb.triggers == [20, 40]


def test_stop_threshold_through_eval_callback_attributes():
    """EvalCallback is deferrable, keeps its default path, and refuses graph without fused."""
    cb = EvalCallback(None, eval_freq=3)
    assert cb.deferrable is True and cb.fused is False and cb.graph is False
    assert EvalCallback.deferrable is True
    with pytest.raises(ValueError):
        EvalCallback(None, graph=True)
    cb = EvalCallback(None, fused=True, graph=True, callback_on_new_best=StopTrainingOnRewardThreshold(0.5))
    assert cb.fused and cb.graph and cb.actor is None and cb.evaluator is None
    assert cb.on_step(_Policy(), 8) is True                   # eval_freq 10000: no evaluation, no engine touched


# ---------------------------------------------------------------- 3. summarize_missions
def test_summarize_missions_by_hand():
    ids = {"GTG": 3, "GTO": 0 | (0 << 2) | (0 << 5), "PKP": 2 | (5 << 2) | (3 << 5), "TGL": 1 | (3 << 2) | (0 << 5)}
    assert _lib.mission_text(ids["GTG"]) == "go to goal" and _lib.mission_text(ids["PKP"]) == "pick up yellow box"
    rewards = [0.5, 0.0, 0.25, 0.0, 0.75, 1.0]
    lengths = [10, 64, 30, 64, 5, 1]
    missions = [ids["GTG"], ids["GTG"], ids["PKP"], ids["TGL"], ids["GTO"], ids["GTO"]]
    s = summarize_missions(rewards, lengths, missions)
    assert set(s) == {"overall", "per_task"}
    assert s["overall"] == dict(episodes=6, success_rate=4 / 6, mean_reward=float(np.mean(rewards)),
                                mean_length=float(np.mean(lengths)))
    assert list(s["per_task"]) == ["GTG", "GTO", "PKP", "TGL"]
    assert s["per_task"]["GTG"] == dict(episodes=2, success_rate=0.5, mean_reward=0.25, mean_length=37.0)
    assert s["per_task"]["GTO"] == dict(episodes=2, success_rate=1.0, mean_reward=0.875, mean_length=3.0)
    assert s["per_task"]["PKP"] == dict(episodes=1, success_rate=1.0, mean_reward=0.25, mean_length=30.0)
    assert s["per_task"]["TGL"] == dict(episodes=1, success_rate=0.0, mean_reward=0.0, mean_length=64.0)
    empty = summarize_missions([], [], [])
    assert empty["overall"]["episodes"] == 0 and empty["per_task"] == {}
    with pytest.raises(ValueError):
        summarize_missions([1.0], [1, 2], [3])


# ---------------------------------------------------------------- 4. ValueError paths, no engine
class _WithPredict:
    def predict(self, obs, deterministic=True):
        raise AssertionError("never called")


def test_graph_argument_errors_without_an_engine():
    with pytest.raises(ValueError, match="fused"):            # graph= without fused
        evaluate_policy(_WithPredict(), None, graph=True)
    with pytest.raises(ValueError, match="callable"):         # a callable over stacked observations
        evaluate_policy(lambda obs: obs, None, fused=object(), graph=True)

    class Actor:
        engine = policy = None

    class Ev:
        actor = Actor()

    with pytest.raises(ValueError, match="another FusedActor"):
        evaluate_policy(_WithPredict(), None, fused=Actor(), graph=Ev())


def test_graph_collect_accepts_only_deferrable_callbacks():
    class Plain:
        def on_step(self, policy, num_timesteps):
            return True

    class Deferrable(Plain):
        deferrable = True

    class NotDeferrable(Plain):
        deferrable = False

    check_graph_callback(None)
    check_graph_callback(Deferrable())
    check_graph_callback(EvalCallback(None))
    for cb in (Plain(), NotDeferrable()):
        with pytest.raises(ValueError, match="deferrable") as ei:
            check_graph_callback(cb)
        assert "graph_collect: a callback needs a host decision every step" in str(ei.value)


# ---------------------------------------------------------------- 5. the entry point's argument checks
def test_eval_record_rejects_bad_arguments_without_gpu():
    """MGX_ERR_INVALID before any HIP call and before any pointer is dereferenced."""
    lib = _lib.load()
    fields = [f for f, _ in _lib.MgxEvalRecordArgs._fields_]

    def args(**kw):
        a = _lib.MgxEvalRecordArgs(**{f: 0x1000 for f in fields})     # never dereferenced: the checks come first
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def call(n=64, n_eval=10, cap=1, off=0, a=args()):
        return lib.mgx_eval_record(n, n_eval, cap, off, None if a is None else ctypes.byref(a), None)

    cases = [dict(a=None), dict(n=0), dict(n=-3), dict(cap=0), dict(cap=-1), dict(n_eval=-1),
             dict(n_eval=65, cap=1),                                  # the largest target is 2
             dict(a=args(reward64_dev=None, ep_return_dev=None))]
    cases += [dict(a=args(**{f: None})) for f in fields if f not in ("reward64_dev", "ep_return_dev")]
    for kw in cases:
        st = call(**kw)
        assert st == 1, (kw, st)                                     # MGX_ERR_INVALID
        assert b"mgx_eval_record" in lib.mgx_last_error()
