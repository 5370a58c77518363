"""Fused actor-critic inference (mgx_policy_act, ABI 8): everything that can be checked without a GPU --
the weight blob's layout, the mission-feature table and the argument checks."""
import ctypes

import pytest
import torch

from mgx import _lib
from mgx import fused_policy as fp
from mgx.policy import ActorCriticPolicy


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("k", [1, 4, 5, 6, 7, 8])
def test_blob_layout(lib, k):
    """mgx_policy_blob_words(K) is the packer's length (46,984 at K = 4) and slicing the blob by the documented
    offsets returns every parameter tensor bit for bit."""
    torch.manual_seed(k)
    pol = ActorCriticPolicy(n_stack=k)
    for p in pol.parameters():                       # biases are zero after init: make every word distinct
        p.data.normal_()
    blob = fp.pack_blob(pol)
    assert blob.dtype == torch.float32 and blob.dim() == 1
    assert int(lib.mgx_policy_blob_words(k)) == blob.numel() == fp.blob_words(k)
    if k == 4:
        assert blob.numel() == 46984
    fe = pol.features_extractor.extractors
    convs = [m for m in fe["image"] if isinstance(m, torch.nn.Conv2d)]
    mods = {"direction": fe["direction"][0], "conv1": convs[0], "conv2": convs[1], "conv3": convs[2],
            "policy_net.0": pol.policy_net[0], "policy_net.1": pol.policy_net[2],
            "value_net_body.0": pol.value_net_body[0], "value_net_body.1": pol.value_net_body[2],
            "action_net": pol.action_net, "value_net": pol.value_net}
    offs = fp.blob_offsets(k)
    assert list(offs) == [n for n, _ in fp.blob_layout(k)]
    end = 0
    for name, (o, shape) in offs.items():
        assert o == end                                # contiguous, in the documented order
        mod, attr = name.rsplit(".", 1)
        t = getattr(mods[mod], attr).detach()
        assert tuple(t.shape) == shape
        assert torch.equal(blob[o:o + t.numel()].reshape(shape), t), name
        end = o + t.numel()
    assert end == blob.numel()


def test_blob_words_rejects_other_stacks(lib):
    for k in (0, -1, 9, 100):
        assert int(lib.mgx_policy_blob_words(k)) == -1


@pytest.mark.parametrize("k", [1, 3, 4, 5, 8])
def test_mission_table_matches_extractor(lib, k):
    """mission_feat[mid][v-1] = the extractor's mission features of K - v zero frames followed by v copies of
    the mission's tokens, for 'go to goal', an object mission and 'drop', every v."""
    torch.manual_seed(7)
    pol = ActorCriticPolicy(n_stack=k)
    pol.train(False)
    tab = fp.mission_table(pol)
    assert tab.shape == (256, k, 128) and tab.dtype == torch.float32
    tokens = torch.as_tensor(_lib.mission_tokens()).long()
    fe = pol.features_extractor
    for mid in (3, 2 | (5 << 2) | (3 << 5), 128):
        assert _lib.mission_text(mid) in ("go to goal", "pick up yellow box", "drop")
        for v in range(1, k + 1):
            stack = torch.cat([torch.zeros(32 * (k - v), dtype=torch.int64), tokens[mid].repeat(v)])[None]
            assert stack.shape == (1, 32 * k)
            obs = {"image": torch.zeros((1, 3 * k, 7, 7)), "direction": torch.zeros((1, 4 * k)), "mission": stack}
            with torch.no_grad():
                want = fe(obs)[0, 80:]
            assert want.shape == (128,)
            assert torch.allclose(tab[mid, v - 1], want, rtol=0, atol=4 * torch.finfo(torch.float32).eps), (mid, v)


def test_policy_act_rejects_bad_arguments_without_gpu(lib):
    """Every bad-argument case that needs no live handle returns MGX_ERR_INVALID before any HIP call (0 <
    ring_rows < n_stack reads the handle's n_stack: tests/test_fused_policy_gpu.py)."""
    d = ctypes.c_void_p(0x1000)                      # never dereferenced: the checks come first

    def call(pol, out, n=16):
        return lib.mgx_policy_act(d, d, d, d, 64, 0, d, n, None,
                                  None if pol is None else ctypes.byref(pol),
                                  None if out is None else ctypes.byref(out), None)

    def policy(**kw):
        p = _lib.MgxPolicy(blob_dev=0x1000, mission_feat_dev=0x1000, mode=1, seed=1, counter_dev=0x1000)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def outs(**kw):
        o = _lib.MgxActOut(actions_dev=0x1000, values_dev=0x1000, log_probs_dev=0x1000, logits_dev=0x1000)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    cases = [(None, outs(), 16), (policy(), None, 16), (policy(blob_dev=None), outs(), 16),
             (policy(mission_feat_dev=None), outs(), 16), (policy(), outs(), 0), (policy(), outs(), -3),
             (policy(mode=-1), outs(), 16), (policy(mode=3), outs(), 16),
             (policy(mode=2, counter_dev=None), outs(), 16),
             (policy(mode=1), outs(actions_dev=None), 16), (policy(mode=2), outs(log_probs_dev=None), 16)]
    for i, (p, o, n) in enumerate(cases):
        st = call(p, o, n)
        assert st == 1, (i, st)                      # MGX_ERR_INVALID
        assert b"mgx_policy_act" in lib.mgx_last_error()


def test_fused_actor_rejects_other_architectures():
    """ValueError before the engine is touched: custom net_arch, custom arch, n_actions != 7."""
    from mgx.policy import DEFAULT_ARCH
    arch = {k: [list(l) for l in v] for k, v in DEFAULT_ARCH.items()}
    arch["direction"] = [["Linear", [4, 8]]]
    for pol in (ActorCriticPolicy(n_stack=2, net_arch={"pi": [32, 32], "vf": [64, 64]}),
                ActorCriticPolicy(n_stack=2, net_arch={"pi": [64], "vf": [64]}),
                ActorCriticPolicy(n_stack=2, arch=arch),
                ActorCriticPolicy(n_stack=2, n_actions=6)):
        with pytest.raises(ValueError):
            fp.FusedActor(pol, None)
    fp.pack_blob(ActorCriticPolicy(n_stack=2))       # the default architecture packs
