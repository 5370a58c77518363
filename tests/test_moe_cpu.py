"""Mission-routed mixture of experts (mgx_policy_act_moe, mgx/moe.py): everything that can be checked without a
GPU -- the argument checks, the scratch size, the route builders, the numpy restatement of the route launch and
MoEPolicy.predict on a stacked CPU batch."""
import ctypes

import numpy as np
import pytest
import torch

from mgx import _lib
from mgx import moe as M
from mgx.evaluation import task_of
from mgx.policy import ActorCriticPolicy


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_policy_act_moe_rejects_bad_arguments_without_gpu(lib):
    """Every bad-argument case that needs no live handle returns MGX_ERR_INVALID before any HIP call."""
    d = ctypes.c_void_p(0x1000)                      # never dereferenced: the checks come first
    need = int(lib.mgx_policy_moe_scratch_words(16, 4))

    def call(pol, out, n=16, index=d, rows=d):
        return lib.mgx_policy_act_moe(d, rows, d, d, 64, 0, index, n, None,
                                      None if pol is None else ctypes.byref(pol),
                                      None if out is None else ctypes.byref(out), None)

    def policy(blob=None, feat=None, **kw):
        p = _lib.MgxPolicyMoe(n_experts=4, mode=1, route_dev=0x1000, seed=1, counter_dev=0x1000,
                              scratch_dev=0x1000, scratch_words=need)
        for x in range(4):
            p.blob_dev[x] = p.mission_feat_dev[x] = 0x1000
        if blob is not None:
            p.blob_dev[blob] = None
        if feat is not None:
            p.mission_feat_dev[feat] = None
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def outs(**kw):
        o = _lib.MgxActOut(actions_dev=0x1000, values_dev=0x1000, log_probs_dev=0x1000, logits_dev=0x1000)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    cases = [(None, outs(), {}), (policy(), None, {}),
             (policy(route_dev=None), outs(), {}), (policy(scratch_dev=None), outs(), {}),
             (policy(blob=0), outs(), {}), (policy(blob=3), outs(), {}),
             (policy(feat=0), outs(), {}), (policy(feat=3), outs(), {}),
             (policy(n_experts=0), outs(), {}), (policy(n_experts=9), outs(), {}), (policy(n_experts=-1), outs(), {}),
             (policy(n_experts=5), outs(), {}),                      # expert 4's pointers are null
             (policy(scratch_words=need - 1), outs(), {}), (policy(scratch_words=0), outs(), {}),
             (policy(scratch_dev=0x1004), outs(), {}),               # the i64 list needs 8-byte alignment
             (policy(), outs(), dict(n=17)),                         # the scratch is sized for 16 samples
             # every case mgx_policy_act rejects
             (policy(), outs(), dict(n=0)), (policy(), outs(), dict(n=-3)),
             (policy(mode=-1), outs(), {}), (policy(mode=3), outs(), {}),
             (policy(mode=2, counter_dev=None), outs(), {}),
             (policy(mode=1), outs(actions_dev=None), {}), (policy(mode=2), outs(log_probs_dev=None), {}),
             (policy(), outs(), dict(index=None)), (policy(), outs(), dict(rows=None))]
    for i, (p, o, kw) in enumerate(cases):
        st = call(p, o, **kw)
        assert st == 1, (i, st)                      # MGX_ERR_INVALID
        assert b"mgx_policy_act_moe" in lib.mgx_last_error()
    # pointers past n_experts are not looked at: the remaining refusal of this call is the null handle's
    p = policy(n_experts=2, blob=3, feat=2)
    st = lib.mgx_policy_act_moe(None, d, d, d, 64, 0, d, 16, None, ctypes.byref(p), ctypes.byref(outs()), None)
    assert st == 1 and b"bad sample addressing" in lib.mgx_last_error()


def test_scratch_words_is_the_stated_bound(lib):
    """32 record words + an i64 and an i32 list of n + 63 E entries; -1 outside the documented range."""
    for n in (1, 63, 64, 65, 200, 65536, 10 ** 7):
        for e in range(1, 9):
            cap = n + 63 * e
            assert int(lib.mgx_policy_moe_scratch_words(n, e)) == 32 + 3 * cap == M.scratch_words(n, e)
            assert cap // 64 >= -(-n // 64)          # the grid covers n samples of a single expert
    for n, e in ((0, 4), (-1, 4), (16, 0), (16, 9), (16, -2), (2 ** 31 - 1, 1), (2 ** 31 - 63 * 8, 8)):
        assert int(lib.mgx_policy_moe_scratch_words(n, e)) == -1
    assert int(lib.mgx_policy_moe_scratch_words(2 ** 31 - 1 - 63 * 8, 8)) == 32 + 3 * (2 ** 31 - 1)
    with pytest.raises(ValueError):
        M.scratch_words(0, 4)


def test_route_by_task_follows_the_mission_texts(lib):
    mapping = {"GTG": 3, "GTO": 0, "TGL": 1, "PKP": 2, "DRP": 4, "MOV": 5}
    route = M.route_by_task(mapping)
    assert route.dtype == torch.uint8 and tuple(route.shape) == (256,)
    used = M.used_mission_ids()
    assert 3 in used and 128 in used and len(used) > 50
    seen = set()
    for m in range(256):
        if m in used:
            task = task_of(_lib.mission_text(m))
            assert int(route[m]) == mapping[task], (m, task)
            seen.add(task)
        else:
            assert int(route[m]) == 0
    assert seen == set(mapping)
    four = {"GTG": 3, "GTO": 0, "TGL": 1, "PKP": 2}
    with pytest.raises(ValueError, match="DRP|MOV"):
        M.route_by_task(four)                         # 'drop' and 'move ...' are used ids too
    r4 = M.route_by_task(four, ids=range(128))        # the ids of `multi`
    assert torch.equal(r4[:128], route[:128]) and int(r4[128:].max()) == 0
    with pytest.raises(ValueError, match="GTG"):
        M.route_by_task({"GTO": 0, "TGL": 1, "PKP": 2}, ids=range(128))


def test_route_from_gate_takes_the_first_argmax_under_ties(lib):
    tokens = torch.as_tensor(_lib.mission_tokens()).long()
    used = M.used_mission_ids()
    tied_all, tied_13, tied_last = used[0], used[5], used[9]

    def gate(tok):
        """Logits [B, 4]: a peak at (first token + length) % 4, exact ties for three chosen ids."""
        assert tok.dtype == torch.int64 and tuple(tok.shape) == (256, 32)
        out = torch.zeros((tok.shape[0], 4))
        peak = (tok[:, 0] + (tok != 0).sum(1)) % 4
        out[torch.arange(tok.shape[0]), peak] = 1.0
        for b in range(tok.shape[0]):
            if torch.equal(tok[b], tokens[tied_all]):
                out[b] = 0.5
            elif torch.equal(tok[b], tokens[tied_13]):
                out[b] = torch.tensor([0.0, 2.0, 0.0, 2.0])
            elif torch.equal(tok[b], tokens[tied_last]):
                out[b] = torch.tensor([-1.0, -1.0, 7.0, 7.0])
        return out

    route = M.route_from_gate(gate)
    assert route.dtype == torch.uint8 and tuple(route.shape) == (256,)
    assert int(route[tied_all]) == 0 and int(route[tied_13]) == 1 and int(route[tied_last]) == 2
    want = (tokens[:, 0] + (tokens != 0).sum(1)) % 4
    for m in used:
        if m not in (tied_all, tied_13, tied_last):
            assert int(route[m]) == int(want[m])
    with pytest.raises(ValueError):
        M.route_from_gate(lambda tok: torch.zeros((tok.shape[0], 9)))
    # a module: Embedding + GRU + Linear on the tokens, the shape of the reference's gate
    class Gate(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.emb, self.gru, self.out = torch.nn.Embedding(32, 8), torch.nn.GRU(8, 16, batch_first=True), \
                torch.nn.Linear(16, 3)

        def forward(self, tok):
            return self.out(self.gru(self.emb(tok))[1][0])

    torch.manual_seed(0)
    g = Gate()
    with torch.no_grad():
        assert torch.equal(M.route_from_gate(g).long(), g(tokens).argmax(1))


def test_moe_policy_rejects_bad_mixtures(lib):
    p2, p4 = ActorCriticPolicy(n_stack=2), ActorCriticPolicy(n_stack=4)
    zero = torch.zeros(256, dtype=torch.uint8)
    with pytest.raises(ValueError, match="n_stack"):
        M.MoEPolicy([p2, p4], zero)
    with pytest.raises(ValueError, match="experts"):
        M.MoEPolicy([p2] * 9, zero)
    with pytest.raises(ValueError, match="experts"):
        M.MoEPolicy([], zero)
    bad = zero.clone()
    bad[77] = 2
    with pytest.raises(ValueError, match="expert 2"):
        M.MoEPolicy([p2, p2], bad)
    with pytest.raises(ValueError):
        M.MoEPolicy([p2, p2], zero[:255])
    assert M.MoEPolicy([p2] * 8, torch.arange(256) % 8).n_stack == 2


def _check_route(mids, route, n_experts):
    """The properties every route must have; returns the reference's result."""
    r = M.moe_route_reference(mids, route, n_experts)
    n = len(mids)
    which = np.asarray(route)[np.asarray(mids, dtype=np.int64)] if n else np.zeros(0, np.int64)
    seg, pos = r["segments"], r["pos"]
    assert r["cap"] == n + 63 * n_experts == pos.size
    end = tiles = 0
    seen = []
    for e in range(8):
        start, count = int(seg[e, 0]), int(seg[e, 1])
        assert start % 64 == 0 and start == end                       # 64-aligned, in expert order, disjoint
        assert count == (int((which == e).sum()) if e < n_experts else 0)
        mine = pos[start:start + count]
        assert (np.diff(mine) > 0).all() and (mine >= 0).all()        # ascending positions
        assert (which[mine] == e).all()
        pad = -(-count // 64) * 64
        assert (pos[start + count:start + pad] == -1).all()           # the padding is never written
        seen += mine.tolist()
        end, tiles = start + pad, tiles + pad // 64
    assert end <= r["cap"] and (pos[end:] == -1).all()
    assert r["tiles"] == tiles <= r["cap"] // 64                      # the grid bound
    routable = np.nonzero(which < n_experts)[0]
    assert sorted(seen) == routable.tolist() and len(set(seen)) == len(seen)    # each exactly once
    assert r["unroutable"] == n - routable.size
    return r


def test_moe_route_reference_random_and_adversarial():
    rng = np.random.default_rng(0)
    for n in list(range(1, 10)) + [63, 64, 65, 127, 128, 129, 200, 255, 256, 300]:
        for n_experts in (1, 2, 3, 4, 8):
            _check_route(rng.integers(0, 256, n), rng.integers(0, n_experts, 256), n_experts)
            _check_route(rng.integers(0, 256, n), rng.integers(0, 12, 256), n_experts)     # unroutable bytes
    ident = np.arange(256)
    for only in range(8):                                             # every expert empty but one
        for n in (1, 63, 64, 65, 128, 300):
            r = _check_route(np.full(n, only), ident, 8)
            assert r["tiles"] == -(-n // 64) and int(r["segments"][only, 1]) == n
            assert int(r["segments"][only, 0]) == 0                   # empty segments take no room
    # counts of exactly 0, 1, 63, 64, 65 and 128 at once, interleaved
    counts = {0: 0, 1: 1, 2: 63, 3: 64, 4: 65, 5: 128, 6: 0, 7: 2}
    mids = np.concatenate([np.full(c, e) for e, c in counts.items()])
    rng.shuffle(mids)
    r = _check_route(mids, ident, 8)
    assert [int(c) for c in r["segments"][:, 1]] == list(counts.values())
    assert [int(s) for s in r["segments"][:, 0]] == [0, 0, 64, 128, 192, 320, 448, 448]
    assert r["tiles"] == 0 + 1 + 1 + 1 + 2 + 2 + 0 + 1
    # everything unroutable
    r = _check_route(np.full(70, 9), ident, 8)
    assert r["tiles"] == 0 and r["unroutable"] == 70 and (r["pos"] == -1).all()
    # with an index, the list is index[pos]
    idx = rng.integers(0, 10 ** 12, mids.size)
    r = M.moe_route_reference(mids, ident, 8, index=idx)
    live = r["pos"] >= 0
    assert (r["list"][live] == idx[r["pos"][live]]).all() and (r["list"][~live] == -1).all()


def test_moe_policy_predict_is_the_chosen_experts(lib):
    """On a stacked CPU batch: row b's action is experts[route[mission id of its newest frame]].predict(row)."""
    k, n_experts, B = 3, 4, 48
    experts = []
    for s in range(n_experts):
        torch.manual_seed(10 + s)
        p = ActorCriticPolicy(n_stack=k)
        with torch.no_grad():
            p.action_net.weight.normal_()
            p.action_net.bias.normal_()
        p.train(False)
        experts.append(p)
    used = M.used_mission_ids()
    route = torch.tensor([(m * 7 + 1) % n_experts for m in range(256)], dtype=torch.uint8)
    moe = M.MoEPolicy(experts, route)
    tokens = torch.as_tensor(_lib.mission_tokens())
    g = torch.Generator().manual_seed(3)
    mids = torch.tensor(used)[torch.randint(0, len(used), (B,), generator=g)]
    older = torch.tensor(used)[torch.randint(0, len(used), (B,), generator=g)]      # older frames: another mission
    mission = torch.cat([tokens[older], torch.zeros((B, 32), dtype=torch.uint8), tokens[mids]], 1)
    obs = {"image": torch.randint(0, 256, (B, 3 * k, 7, 7), generator=g, dtype=torch.uint8),
           "direction": torch.nn.functional.one_hot(torch.randint(0, 4, (B, k), generator=g), 4).reshape(B, 4 * k)
           .to(torch.uint8), "mission": mission}
    assert torch.equal(moe.mission_ids(obs), mids)
    assert torch.equal(moe.experts_of(obs), route.long()[mids])
    got = moe.predict(obs, deterministic=True)
    assert got.dtype == torch.int64 and tuple(got.shape) == (B,)
    per_expert = [p.predict(obs, deterministic=True) for p in experts]
    assert len({tuple(a.tolist()) for a in per_expert}) > 1           # the experts disagree: the choice matters
    assert len(set(route.long()[mids].tolist())) == n_experts
    for b in range(B):
        e = int(route[mids[b]])
        row = {kk: v[b:b + 1] for kk, v in obs.items()}
        assert int(got[b]) == int(experts[e].predict(row, deterministic=True)[0]) == int(per_expert[e][b]), b
    bad = dict(obs, mission=torch.full_like(mission, 31))
    with pytest.raises(ValueError):
        moe.predict(bad)
    assert moe.predict(obs).shape == (B,)                              # sampled: runs
