"""Checkpoint resume on the parameter arena (ParamArena.import_state, mgx/fused_update.py), on CPU tensors.

nn.Module.load_state_dict copies into the parameters in place, so they stay arena views; Optimizer.load_state_dict
REPLACES the state's tensors, so after it exp_avg / exp_avg_sq are the checkpoint's own tensors and the arena's moments
are stale.  import_state() -- which FusedUpdate.prepare runs before every train() -- copies such a foreign state in
and exports views again.  Every checkpoint goes through torch.save and torch.load(weights_only=True), as
tools/ppo_learn.py's --save / --resume do.  Every comparison is bit for bit."""
import copy
import os

import pytest
import torch

from mgx.fused_update import ParamArena
from mgx.policy import ActorCriticPolicy

STACKS = [1, 4, 8]


def _policy(k, seed=0):
    torch.manual_seed(seed)
    return ActorCriticPolicy(n_stack=k)


def _layout_tensors(pol):
    """The 25 parameters in arena-layout order (policy.parameters() is in module order)."""
    from mgx.fused_mission import mission_params
    from mgx.fused_policy import _params
    return list(_params(pol)[1]) + list(mission_params(pol))


def _same(a, b):
    a, b = a.detach().contiguous(), b.detach().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and \
        torch.equal(a.view(torch.int32), b.view(torch.int32))


def _grads(pol, n, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(p.shape, generator=g) for p in pol.parameters()] for _ in range(n)]


def _torch_steps(pol, grads):
    for g in grads:
        for p, gg in zip(pol.parameters(), g):
            p.grad = gg.clone()
        pol.optimizer.step()


def _through_a_file(pol, path, **extra):
    """The checkpoint of tools/ppo_learn.py, written and read back the way it does -> (checkpoint, file size)."""
    torch.save(dict(policy=pol.state_dict(), optimizer=pol.optimizer.state_dict(), **extra), path)
    return torch.load(path, map_location="cpu", weights_only=True), os.path.getsize(path)


def _is_view_state(arena):
    """Whether policy.optimizer's state holds all 25 entries and every moment is the arena's view at its offset."""
    state = arena.policy.optimizer.state
    for p, (_, o, shape) in zip(arena.tensors, arena.layout):
        st = state.get(p)
        if not st or set(st) != {"step", "exp_avg", "exp_avg_sq"}:
            return False
        for key, flat in (("exp_avg", arena.exp_avg), ("exp_avg_sq", arena.exp_avg_sq)):
            if st[key].data_ptr() != flat.data_ptr() + 4 * o or tuple(st[key].shape) != tuple(shape):
                return False
    return len(state) == 25


def _fill_moments(arena, seed):
    """Known non-zero moments in every word (exp_avg_sq >= 0), through the flat buffers."""
    g = torch.Generator().manual_seed(seed)
    arena.exp_avg.copy_(torch.randn(arena.words, generator=g))
    arena.exp_avg_sq.copy_(torch.rand(arena.words, generator=g) + 0.125)


@pytest.mark.parametrize("k", STACKS)
def test_live_load_into_an_arena_backed_policy(k, tmp_path):
    """A donor's checkpoint after three torch Adam steps, loaded in place into a policy that already lives in an
    arena with an exported state: the parameters stay views, the optimizer's moments do not and the arena's are stale
    (the state of affairs import_state exists for).  After import_state() the arena's moments and step are the
    donor's, the optimizer's state is views again, and two further torch Adam steps on fixed gradients give what the
    donor gives -- in the parameters, in the optimizer's state and in the arena's buffers."""
    donor = _policy(k, seed=1)
    grads = _grads(donor, 5)
    _torch_steps(donor, grads[:3])
    ck, _ = _through_a_file(donor, tmp_path / "donor.pt")
    pol = _policy(k, seed=0)
    arena = ParamArena(pol)
    arena.export_state()
    assert _is_view_state(arena) and arena.step == 0
    pol.load_state_dict(ck["policy"])
    pol.optimizer.load_state_dict(ck["optimizer"])
    for p, (_, o, _) in zip(arena.tensors, arena.layout):             # parameters: copied in place
        assert p.data_ptr() == arena.param.data_ptr() + 4 * o
    for p, q in zip(pol.parameters(), donor.parameters()):
        assert _same(p, q)
    assert not _is_view_state(arena)                                   # moments: replaced
    assert arena.step == 0 and not arena.exp_avg.any() and not arena.exp_avg_sq.any()
    assert arena.import_state() is True
    assert arena.step == 3 and _is_view_state(arena)
    want = [donor.optimizer.state[q] for q in _layout_tensors(donor)]
    for st, m, v in zip(want, arena.views(arena.exp_avg), arena.views(arena.exp_avg_sq)):
        assert _same(m, st["exp_avg"]) and _same(v, st["exp_avg_sq"]) and m.any() and v.any()
        assert int(st["step"]) == 3
    assert all(int(pol.optimizer.state[p]["step"]) == 3 for p in arena.tensors)
    assert arena.import_state() is False                               # views now: nothing to do
    _torch_steps(pol, grads[3:])
    _torch_steps(donor, grads[3:])
    for (name, p), q in zip(pol.named_parameters(), donor.parameters()):
        assert _same(p, q), name
    for p, q, m, v in zip(arena.tensors, _layout_tensors(donor), arena.views(arena.exp_avg),
                          arena.views(arena.exp_avg_sq)):
        a, b = pol.optimizer.state[p], donor.optimizer.state[q]
        assert _same(a["exp_avg"], b["exp_avg"]) and _same(a["exp_avg_sq"], b["exp_avg_sq"])
        assert _same(m, b["exp_avg"]) and _same(v, b["exp_avg_sq"])    # torch stepped on the arena's own memory
        assert int(a["step"]) == int(b["step"]) == 5
    assert arena.import_state() is False and arena.step == 5           # the step count follows torch's


@pytest.mark.parametrize("k", STACKS)
def test_arena_backed_checkpoint_round_trip(k, tmp_path):
    """A checkpoint of a policy whose parameters and optimizer state are arena views, at step 7 with known moments:
    loaded into a fresh policy, a fresh ParamArena imports step 7, the moments and the parameters bit for bit and
    owns the state as views.  The file holds each of the three arenas once, not 75 views with a storage each:
    below 3 x 4 x words bytes + 64 KiB (n_stack 4: 1,338,895 bytes for 110,216 words)."""
    pol = _policy(k, seed=0)
    arena = ParamArena(pol)
    _fill_moments(arena, 70 + k)
    arena.step = 7
    arena.export_state()
    ck, size = _through_a_file(pol, tmp_path / "arena.pt", timesteps=1234)
    print("n_stack %d: %d words, checkpoint %d bytes" % (k, arena.words, size))
    assert size < 3 * 4 * arena.words + 64 * 1024
    assert ck["timesteps"] == 1234 and len(ck["optimizer"]["state"]) == 25
    fresh = _policy(k, seed=9)
    assert not any(_same(p, q) for p, q in zip(fresh.parameters(), pol.parameters()) if p.dim() > 1)
    fresh.load_state_dict(ck["policy"])
    fresh.optimizer.load_state_dict(ck["optimizer"])
    again = ParamArena(fresh)
    assert again.step == 7 and _is_view_state(again) and again.attached()
    assert all(int(fresh.optimizer.state[p]["step"]) == 7 for p in again.tensors)
    for name in ("param", "exp_avg", "exp_avg_sq"):
        for (tname, _, _), x, y in zip(arena.layout, again.views(getattr(again, name)),
                                       arena.views(getattr(arena, name))):
            assert _same(x, y) and (x.any() or name == "param"), (name, tname)    # biases start at zero
    for p, q in zip(fresh.parameters(), pol.parameters()):
        assert _same(p, q)


@pytest.mark.parametrize("k", STACKS)
def test_empty_state_leaves_the_arena_as_it_is(k):
    """No optimizer state at all: the arena is authoritative -- moments and step stay, nothing is exported."""
    pol = _policy(k)
    arena = ParamArena(pol)
    _fill_moments(arena, 1)
    arena.step = 5
    arena.export_state()
    pol.optimizer.state.clear()
    m, v = arena.exp_avg.clone(), arena.exp_avg_sq.clone()
    assert arena.import_state() is False
    assert arena.step == 5 and _same(arena.exp_avg, m) and _same(arena.exp_avg_sq, v)
    assert len(pol.optimizer.state) == 0


@pytest.mark.parametrize("k", STACKS)
def test_view_state_leaves_the_moments_and_takes_the_step(k):
    """A state made only of the arena's views: the moments -- whatever was written to the arena since the export --
    are untouched, and the step count is the state's (torch's Adam advances it there)."""
    pol = _policy(k)
    arena = ParamArena(pol)
    arena.export_state()
    _fill_moments(arena, 2)
    m, v = arena.exp_avg.clone(), arena.exp_avg_sq.clone()
    for st in pol.optimizer.state.values():
        st["step"] = torch.tensor(11.0)
    assert arena.import_state() is False
    assert arena.step == 11 and _same(arena.exp_avg, m) and _same(arena.exp_avg_sq, v)
    assert _is_view_state(arena)
    del pol.optimizer.state[arena.tensors[3]]                          # a proper subset of views is still views
    assert arena.import_state() is False
    assert arena.step == 11 and _same(arena.exp_avg, m) and _same(arena.exp_avg_sq, v)


SUBSET = {0: 4, 7: 9, 19: 2, 21: 6}                # tensor in layout order -> its step count


@pytest.mark.parametrize("k", STACKS)
def test_foreign_subset_is_imported_and_the_rest_zeroed(k):
    """Foreign entries for four of the 25 tensors (blob and mission ones) over an arena full of other values: those
    four are imported, every other tensor's moments are zero, the step is the largest of the entries', and all 25
    entries are views afterwards."""
    pol = _policy(k)
    arena = ParamArena(pol)
    _fill_moments(arena, 3)
    arena.step = 99
    arena.export_state()
    g = torch.Generator().manual_seed(4)
    state = pol.optimizer.state
    state.clear()
    want = {}
    for i, step in SUBSET.items():
        p = arena.tensors[i]
        want[i] = (torch.randn(p.shape, generator=g), torch.rand(p.shape, generator=g))
        state[p] = {"step": torch.tensor(float(step)), "exp_avg": want[i][0].clone(),
                    "exp_avg_sq": want[i][1].clone()}
    assert arena.import_state() is True
    assert arena.step == 9 and _is_view_state(arena)
    for i, (m, v) in enumerate(zip(arena.views(arena.exp_avg), arena.views(arena.exp_avg_sq))):
        if i in want:
            assert _same(m, want[i][0]) and _same(v, want[i][1]), i
        else:
            assert not m.any() and not v.any(), i
    assert all(int(state[p]["step"]) == 9 for p in arena.tensors)


@pytest.mark.parametrize("k", STACKS)
@pytest.mark.parametrize("what", ["shape", "dtype", "sq_shape"])
def test_wrong_foreign_moment_is_a_value_error(k, what):
    """A foreign moment of another shape (same element count included) or dtype: ValueError, from import_state and
    from the constructor, before anything was copied or moved."""
    pol = _policy(k)
    donor = copy.deepcopy(pol)
    _torch_steps(donor, _grads(donor, 1))
    arena = ParamArena(pol)
    _fill_moments(arena, 5)
    arena.step = 2
    arena.export_state()
    m, v = arena.exp_avg.clone(), arena.exp_avg_sq.clone()

    def spoil(policy, tensors):
        policy.optimizer.load_state_dict(donor.optimizer.state_dict())
        st = policy.optimizer.state[tensors[22]]                      # mission.weight_hh_l0, [384, 128]
        if what == "shape":
            st["exp_avg"] = torch.zeros(385, 128)
        elif what == "dtype":
            st["exp_avg"] = st["exp_avg"].double()
        else:
            st["exp_avg_sq"] = st["exp_avg_sq"].reshape(128, 384)

    spoil(pol, arena.tensors)
    with pytest.raises(ValueError, match="mission.weight_hh_l0"):
        arena.import_state()
    assert _same(arena.exp_avg, m) and _same(arena.exp_avg_sq, v)
    other = _policy(k, seed=2)
    ptrs = [p.data_ptr() for p in other.parameters()]
    spoil(other, _layout_tensors(other))
    with pytest.raises(ValueError, match="mission.weight_hh_l0"):
        ParamArena(other)
    assert ptrs == [p.data_ptr() for p in other.parameters()]
