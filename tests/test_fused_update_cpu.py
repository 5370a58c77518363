"""Fused PPO update (mgx_ppo_loss / mgx_adam_step, mgx/fused_update.py, added within ABI 9): everything that can
be checked without a GPU -- the exports, the scratch sizes, the argument checks, the parameter arena and the
Python-side validation."""
import copy
import ctypes

import pytest
import torch

from mgx import _lib
from mgx import fused_policy as fp
from mgx.policy import DEFAULT_ARCH, ActorCriticPolicy

NEW = ("mgx_ppo_loss_scratch_words", "mgx_ppo_loss", "mgx_adam_scratch_words", "mgx_adam_step")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_exports_and_abi_version(lib):
    assert _lib.ABI_VERSION == 9 and lib.mgx_abi_version() == 9
    for name in NEW:
        assert name in _lib.EXPORTS and getattr(lib, name) is not None


@pytest.mark.parametrize("name", ["mgx_ppo_loss_scratch_words", "mgx_adam_scratch_words"])
def test_scratch_words(lib, name):
    """-1 for sizes <= 0; positive, even (the partials are doubles) and non-decreasing otherwise."""
    f = getattr(lib, name)
    for n in (0, -1, -(1 << 40)):
        assert int(f(n)) == -1, n
    prev = 0
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099, 65536, 65537, 110000, 1 << 20, 1 << 31, 1 << 40):
        w = int(f(n))
        assert w >= prev and w > 0 and w % 2 == 0, (n, w)
        prev = w


LOSS_PTRS = ("logits_dev", "values_dev", "actions_dev", "old_values_dev", "old_log_probs_dev", "advantages_dev",
             "returns_dev", "g_logits_dev", "g_values_dev", "stats_dev", "scratch_dev")


def test_ppo_loss_rejects_bad_arguments_without_gpu(lib):
    """Every bad-argument case is MGX_ERR_INVALID before any HIP call and before any pointer is dereferenced (the
    pointers are fake), and mgx_last_error() names the call."""
    n = 257
    need = int(lib.mgx_ppo_loss_scratch_words(n))

    def call(n=n, args="ok", stream=None, **kw):
        a = _lib.MgxPpoLossArgs(sel_dev=0x1000, adv_stats_dev=0x1000, scratch_words=need, clip_range=0.1,
                                clip_range_vf=0.08, ent_coef=0.04, vf_coef=0.8, adv_mode=1,
                                **{name: 0x1000 for name in LOSS_PTRS})
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.mgx_ppo_loss(n, None if args is None else ctypes.byref(a), stream)

    cases = [dict(args=None)] + [{name: None} for name in LOSS_PTRS]
    cases += [dict(n=0), dict(n=-3), dict(adv_mode=-1), dict(adv_mode=3), dict(adv_mode=2, adv_stats_dev=None),
              dict(clip_range=0.0), dict(clip_range=-0.1), dict(clip_range=float("nan")),
              dict(scratch_words=need - 1), dict(scratch_words=0), dict(scratch_words=-1), dict(scratch_dev=0x1004)]
    for i, kw in enumerate(cases):
        st = call(**kw)
        assert st == 1, (i, kw, st)                  # MGX_ERR_INVALID
        assert b"mgx_ppo_loss" in lib.mgx_last_error()


def test_adam_step_rejects_bad_arguments_without_gpu(lib):
    n = 1025
    need = int(lib.mgx_adam_scratch_words(n))
    d = ctypes.c_void_p(0x1000)

    def call(param=d, grad=d, m=d, v=d, n=n, args="ok", norm=d, scratch=d, words=need, **kw):
        a = _lib.MgxAdamArgs(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, step=1, max_grad_norm=0.5, grad_scale=1.0)
        for k, val in kw.items():
            setattr(a, k, val)
        return lib.mgx_adam_step(param, grad, m, v, n, None if args is None else ctypes.byref(a), norm, scratch,
                                 words, None)

    cases = [dict(param=None), dict(grad=None), dict(m=None), dict(v=None), dict(args=None), dict(scratch=None),
             dict(n=0), dict(n=-1), dict(step=0), dict(step=-2), dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0),
             dict(beta2=1.5), dict(beta2=float("nan")), dict(eps=-1e-8), dict(words=need - 1), dict(words=0),
             dict(scratch=ctypes.c_void_p(0x1004))]
    for i, kw in enumerate(cases):
        st = call(**kw)
        assert st == 1, (i, kw, st)                  # MGX_ERR_INVALID
        assert b"mgx_adam_step" in lib.mgx_last_error()


def _policy(k, seed=0):
    torch.manual_seed(seed)
    return ActorCriticPolicy(n_stack=k)


def _obs(k, n=5, seed=1):
    g = torch.Generator().manual_seed(seed)
    return {"image": torch.randint(0, 11, (n, 3 * k, 7, 7), generator=g).to(torch.uint8),
            "direction": torch.randint(0, 2, (n, 4 * k), generator=g).to(torch.uint8),
            "mission": torch.randint(0, 32, (n, 32 * k), generator=g).to(torch.uint8)}


@pytest.mark.parametrize("k", [1, 4, 8])
def test_param_arena_layout(k):
    """The blob tensors sit at blob_offsets without padding (arena.param[:blob_words] is pack_blob), the five
    mission tensors follow on 16-byte boundaries, every parameter and gradient is a view at its offset, the values
    and a policy forward are unchanged by the move, and p.grad sees a write to arena.grad."""
    from mgx.fused_mission import mission_params
    from mgx.fused_update import ParamArena, arena_layout
    pol = _policy(k)
    pol.train(False)
    before = {n: p.detach().clone() for n, p in pol.named_parameters()}
    blob_before = fp.pack_blob(pol).clone()
    obs = _obs(k)
    with torch.no_grad():
        out_before = pol(obs, deterministic=True)
    arena = ParamArena(pol)
    layout, words = arena_layout(k)
    assert len(layout) == 25 and arena.words == words == arena.param.numel() == arena.grad.numel() \
        == arena.exp_avg.numel() == arena.exp_avg_sq.numel()
    assert arena.blob_words == fp.blob_words(k)
    for (name, o, shape), (bname, (bo, bshape)) in zip(layout[:20], fp.blob_offsets(k).items()):
        assert (name, o, tuple(shape)) == (bname, bo, tuple(bshape))
    assert torch.equal(arena.param[:arena.blob_words], blob_before)
    _, blob_tensors = fp._params(pol)
    tensors = list(blob_tensors) + list(mission_params(pol))
    assert {id(p) for p in tensors} == {id(p) for p in pol.parameters()}
    end = 0
    for p, (name, o, shape) in zip(tensors, layout):
        assert o >= end and tuple(p.shape) == tuple(shape)
        assert p.data_ptr() == arena.param.data_ptr() + 4 * o, name
        assert p.grad is not None and p.grad.data_ptr() == arena.grad.data_ptr() + 4 * o, name
        assert p.is_contiguous() and p.grad.shape == p.shape
        end = o + p.numel()
    assert end <= words
    for p, (name, o, _) in zip(tensors[20:], layout[20:]):
        assert o % 4 == 0 and p.data_ptr() % 16 == 0 and p.grad.data_ptr() % 16 == 0, name
    for n, p in pol.named_parameters():
        assert torch.equal(p.detach(), before[n]), n
    with torch.no_grad():
        out_after = pol(obs, deterministic=True)
    for x, y in zip(out_before, out_after):
        assert torch.equal(x, y)
    assert arena.attached() and arena.step == 0
    assert not arena.grad.any() and not arena.exp_avg.any() and not arena.exp_avg_sq.any()
    arena.grad.copy_(torch.arange(words, dtype=torch.float32))
    for p, (name, o, shape) in zip(tensors, layout):
        assert torch.equal(p.grad.reshape(-1), torch.arange(o, o + p.numel(), dtype=torch.float32)), name
    arena.param[:arena.blob_words].mul_(2.0)
    assert torch.equal(fp.pack_blob(pol), 2.0 * blob_before)             # the parameters see a write to the arena


def _torch_steps(pol, grads):
    for g in grads:
        for p, gg in zip(pol.parameters(), g):
            p.grad = gg.clone()
        pol.optimizer.step()


@pytest.mark.parametrize("k", [1, 4, 8])
def test_param_arena_optimizer_state_round_trip(k):
    """An arena built on a policy whose optimizer has taken three steps imports the moments and the step count;
    export_state() then two torch Adam steps give bit for bit what torch alone gives from the same moments, and
    optimizer.state_dict() holds all 25 entries."""
    from mgx.fused_update import ParamArena
    pol = _policy(k)
    g = torch.Generator().manual_seed(3)
    grads = [[torch.randn(p.shape, generator=g) for p in pol.parameters()] for _ in range(5)]
    _torch_steps(pol, grads[:3])
    ref = copy.deepcopy(pol)
    _torch_steps(ref, grads[3:])
    arena = ParamArena(pol)
    assert arena.step == 3
    for p, m, v in zip(arena.tensors, arena.views(arena.exp_avg), arena.views(arena.exp_avg_sq)):
        st = pol.optimizer.state[p]
        assert torch.equal(m, st["exp_avg"]) and torch.equal(v, st["exp_avg_sq"]) and m.any() and v.any()
    pol.optimizer.state.clear()
    arena.export_state()
    sd = pol.optimizer.state_dict()
    assert len(sd["state"]) == 25 and all(int(s["step"]) == 3 for s in sd["state"].values())
    _torch_steps(pol, grads[3:])
    for (n, p), q in zip(pol.named_parameters(), ref.parameters()):
        assert torch.equal(p.detach(), q.detach()), n
    for p, q in zip(pol.parameters(), ref.parameters()):
        a, b = pol.optimizer.state[p], ref.optimizer.state[q]
        assert torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])
        assert int(a["step"]) == int(b["step"]) == 5


def test_param_arena_fresh_export():
    """Without an optimizer state the arena starts at step 0 with zero moments; export_state() then a torch step
    equals torch's own first step."""
    from mgx.fused_update import ParamArena
    pol = _policy(4)
    ref = copy.deepcopy(pol)
    g = torch.Generator().manual_seed(4)
    grads = [[torch.randn(p.shape, generator=g) for p in pol.parameters()]]
    arena = ParamArena(pol)
    arena.export_state()
    _torch_steps(pol, grads)
    _torch_steps(ref, grads)
    for p, q in zip(pol.parameters(), ref.parameters()):
        assert torch.equal(p.detach(), q.detach())
    for p, (_, o, _) in zip(arena.tensors, arena.layout):              # torch's step updated the arena in place
        assert p.data_ptr() == arena.param.data_ptr() + 4 * o
    assert not arena.attached()                                        # _torch_steps replaced every p.grad
    arena.attach_grads()
    assert arena.attached()
    pol.optimizer.zero_grad()
    assert not arena.attached()
    arena.attach_grads()
    assert arena.attached()


def test_fused_update_flag_validation():
    from mgx.ppo import PPOConfig
    assert PPOConfig().fused_update is False
    for kw in (dict(), dict(fused_train=True), dict(fused_mission=True, fused_act=True),
               dict(fused_train=True, fused_mission=True, layout="sb3")):
        with pytest.raises(ValueError):
            PPOConfig(fused_update=True, **kw)
    cfg = PPOConfig(fused_update=True, fused_train=True, fused_mission=True)
    assert cfg.fused_update and cfg.layout == "compact"
    PPOConfig(fused_update=True, fused_train=True, fused_mission=True, fused_act=True)


def test_arena_rejects_other_architectures():
    """Whatever _params / mission_params reject is the same ValueError, before a parameter is moved; so is a policy
    with a parameter outside the 25."""
    from mgx.fused_update import FusedUpdate, ParamArena
    bad = [ActorCriticPolicy(n_stack=2, net_arch=dict(pi=[32, 32], vf=[64, 64])),
           ActorCriticPolicy(n_stack=2, arch=dict(DEFAULT_ARCH, mission=[["Embedding", [32, 32]],
                                                                         ["GRU", [32, 64, 1, True, True]]])),
           ActorCriticPolicy(n_stack=2, arch=dict(DEFAULT_ARCH, mission=[["Embedding", [40, 32]],
                                                                         ["GRU", [32, 128, 1, True, True]]]))]
    for pol in bad:
        ptrs = [p.data_ptr() for p in pol.parameters()]
        with pytest.raises(ValueError, match="reference architecture"):
            ParamArena(pol)
        with pytest.raises(ValueError, match="reference architecture"):
            FusedUpdate(pol, None)
        assert ptrs == [p.data_ptr() for p in pol.parameters()]
    pol = ActorCriticPolicy(n_stack=2)
    pol.extra = torch.nn.Parameter(torch.zeros(3))
    ptrs = [p.data_ptr() for p in pol.parameters()]
    with pytest.raises(ValueError, match="outside"):
        ParamArena(pol)
    assert ptrs == [p.data_ptr() for p in pol.parameters()]
