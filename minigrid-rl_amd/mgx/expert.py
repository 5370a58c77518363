"""The shortest-path expert: its normative definition (expert_reference, numpy) and the device actor over
mgx_expert_act (ExpertActor).

The reference's expert (src/experts.py) is a per-env Python A* over a full-grid symbolic observation that knows
nothing of locked doors; imitation.yaml (`algo: bc`) clones it.  This one is a function of the env's current state
alone -- the dict MgxEngine.dump_state() / OracleVec.dump() return -- and is defined by the rules below; the kernel
(csrc/mgx_expert.h) must return the same action and cost for every env, in integers.

Cells: grid[x][y] = (type, colour, state, box-holds-key); door state 0 open, 1 closed, 2 locked.

Cost model over states (x, y, dir): LEFT / RIGHT cost 1; FORWARD into an empty cell or an open door costs 1; entering
a closed door costs 2 (TOGGLE, then FORWARD); entering a locked door costs 2, but only while carrying the key of its
colour; everything else is impassable (lava, walls, objects, any goal that is not the final cell).  The agent's own
cell is always a valid start.  D(s) is the cost-to-go to a goal set G.  The first action is the argmin over [the
forward move, LEFT, RIGHT] of edge cost + D(successor), ties in that order; the forward move is TOGGLE when the front
cell is a door that must be opened first.

Rules -- the first that applies decides (action, cost):
 1. mission_done: DONE, 0.
 2. no target cell (tx == 255): the target action if there is one, cost 1 ('drop' completes on the action alone);
    else ('move' missions: the target range is not part of the state dump) DONE, -1 -- unsupported.
 3. needed = the hand holds a key whose colour some locked door of the grid has.  ta == PICKUP with a full hand
    that is not needed: the drop routine, -2.
 4. route to the mission.  At-cell missions (ta in {255, 0}): G = the target cell in any direction, which may be
    entered as the final move; cost D (standing on it already: DONE, 0).  Facing missions: G = every neighbour of
    the target, facing it; cost D + 1; at D == 0 the action is ta, or (PICKUP with a full hand) the drop routine, -2.
 5. unreachable with a full hand that is not needed: the drop routine, -2.
 6. unreachable with an empty hand: G = every state facing a key, or a key-holding box, whose colour some locked
    door has; the route's first action, at D == 0 PICKUP for a key and TOGGLE for a box; cost -3.
 7. otherwise DONE, -4: give up.
Drop routine: the first empty cell among front, right, left, behind decides: DROP, RIGHT, LEFT, RIGHT; none: DONE.
"""
import ctypes
import weakref

import numpy as np

LEFT, RIGHT, FORWARD, PICKUP, DROP, TOGGLE, DONE = range(7)
EMPTY, WALL, DOOR, KEY, BALL, BOX, GOAL, LAVA = 1, 2, 4, 5, 6, 7, 8, 9
NONE = 255
DV = ((1, 0), (0, 1), (-1, 0), (0, -1))
INF = 1 << 20
COST_UNSUPPORTED, COST_DROP, COST_KEY, COST_GIVE_UP = -1, -2, -3, -4


def _pred_cells(b, d):
    """r[c - DV[d]] = b[c] over bool [N, S, S] boards (x, y): the cells a forward move in direction d enters b from."""
    r = np.zeros_like(b)
    if d == 0:
        r[:, :-1, :] = b[:, 1:, :]
    elif d == 1:
        r[:, :, :-1] = b[:, :, 1:]
    elif d == 2:
        r[:, 1:, :] = b[:, :-1, :]
    else:
        r[:, :, 1:] = b[:, :, :-1]
    return r


def _cost_to_go(e1, e2, seeds, agent):
    """D int32 [N, 4, S, S] (dir, x, y), INF where G cannot be reached: a layered backward search from `seeds`
    (bool [N, 4, S, S]).  e1 / e2: bool [N, S, S], the cells a forward move enters at cost 1 / 2.  The search stops
    once every env's agent state (agent: [N, 3] x, y, dir) is labelled or its frontier is empty: states further
    from G than the agent stay INF, which no first action depends on."""
    N, _, S, _ = seeds.shape
    n = np.arange(N)
    at = (n, agent[:, 2].astype(np.int64), agent[:, 0].astype(np.int64), agent[:, 1].astype(np.int64))
    D = np.full(seeds.shape, INF, np.int32)
    D[seeds] = 0
    new, held = seeds.copy(), np.zeros_like(seeds)
    for k in range(1, 8 * S * S + 1):
        open_ = (D[at] == INF) & (new.any(axis=(1, 2, 3)) | held.any(axis=(1, 2, 3)))
        if not open_.any():
            break
        cand = np.roll(new, 1, axis=1) | np.roll(new, -1, axis=1)        # a turn: direction d +- 1, same cell
        for d in range(4):
            cand[:, d] |= _pred_cells((new[:, d] & e1) | held[:, d], d)
        held = new & e2[:, None]                                         # door cells: their entry costs 2
        new = cand & (D == INF)
        D[new] = k
    return D


def _first_action(D, e1, e2, agent):
    """(cost D(agent state), first action) per env; cost INF where unreachable, action FORWARD / TOGGLE / LEFT /
    RIGHT (undefined where cost is 0 or INF)."""
    N, _, S, _ = D.shape
    n = np.arange(N)
    ax, ay, dr = (agent[:, i].astype(np.int64) for i in range(3))
    dv = np.array(DV)
    fx, fy = ax + dv[dr, 0], ay + dv[dr, 1]
    inb = (fx >= 0) & (fx < S) & (fy >= 0) & (fy < S)
    fxc, fyc = np.clip(fx, 0, S - 1), np.clip(fy, 0, S - 1)
    ec = np.where(inb & e1[n, fxc, fyc], 1, np.where(inb & e2[n, fxc, fyc], 2, INF))
    cf = np.minimum(ec + D[n, dr, fxc, fyc].astype(np.int64), INF)
    cl = np.minimum(1 + D[n, (dr + 3) % 4, ax, ay].astype(np.int64), INF)
    cr = np.minimum(1 + D[n, (dr + 1) % 4, ax, ay].astype(np.int64), INF)
    here = D[n, dr, ax, ay].astype(np.int64)
    fwd = np.where(ec == 2, TOGGLE, FORWARD)
    act = np.where((cf <= cl) & (cf <= cr), fwd, np.where(cl <= cr, LEFT, RIGHT))
    return here, act


def _facing_seeds(cells):
    """bool [N, 4, S, S]: every state that faces a cell of `cells` (bool [N, S, S])."""
    return np.stack([_pred_cells(cells, d) for d in range(4)], axis=1)


def expert_reference(state):
    """(actions int32 [N], cost int32 [N]) of the expert for a state dict of arrays (module docstring)."""
    grid, agent = np.asarray(state["grid"]), np.asarray(state["agent"])
    carry, target = np.asarray(state["carrying"]), np.asarray(state["target"])
    done = np.asarray(state["mission_done"])
    N, S = grid.shape[0], grid.shape[1]
    n = np.arange(N)
    typ, col, st, aux = (grid[..., i] for i in range(4))
    tx, ty, ta = (target[:, i].astype(np.int64) for i in range(3))
    has_t = tx != NONE
    txc, tyc = np.where(has_t, tx, 0), np.where(has_t, ty, 0)
    hand = carry[:, 0] != 0
    locked = (typ == DOOR) & (st == 2)
    lcol = np.zeros((N, 8), bool)                                         # colours of the locked doors
    for c in range(8):
        lcol[:, c] = (locked & (col == c)).any(axis=(1, 2))
    needed = (carry[:, 0] == KEY) & lcol[n, carry[:, 1] & 7]
    mine = locked & (carry[:, 0] == KEY)[:, None, None] & (col == carry[:, 1][:, None, None])
    e1 = (typ == EMPTY) | ((typ == DOOR) & (st == 0))
    e2 = ((typ == DOOR) & (st == 1)) | mine
    at_cell = (ta == NONE) | (ta == 0)
    tcell = np.zeros((N, S, S), bool)
    tcell[n[has_t], txc[has_t], tyc[has_t]] = True
    final = tcell & at_cell[:, None, None]
    seeds = np.where(at_cell[:, None, None, None], np.repeat(tcell[:, None], 4, axis=1), _facing_seeds(tcell))
    e1m, e2m = e1 | final, e2 & ~final
    rule3 = (ta == PICKUP) & hand & ~needed
    d1, a1 = np.full(N, INF, np.int64), np.full(N, DONE, np.int64)
    m = np.nonzero((done == 0) & has_t & ~rule3)[0]                       # the envs rule 4 is reached for
    if m.size:
        d1[m], a1[m] = _first_action(_cost_to_go(e1m[m], e2m[m], seeds[m], agent[m]), e1m[m], e2m[m], agent[m])
    kcell = ((typ == KEY) | ((typ == BOX) & (aux != 0))) & np.take_along_axis(
        lcol, (col & 7).reshape(N, -1).astype(np.int64), axis=1).reshape(N, S, S)
    d2, a2 = np.full(N, INF, np.int64), np.full(N, DONE, np.int64)
    m = m[(d1[m] == INF) & ~hand[m]]                                      # ... and rule 6
    if m.size:
        d2[m], a2[m] = _first_action(_cost_to_go(e1[m], e2[m], _facing_seeds(kcell[m]), agent[m]), e1[m], e2[m],
                                     agent[m])
    # the drop routine and the front cell
    ax, ay, dr = (agent[:, i].astype(np.int64) for i in range(3))
    dv = np.array(DV)
    drop = np.full(N, DONE, np.int64)
    for k, a in ((2, RIGHT), (3, LEFT), (1, RIGHT), (0, DROP)):           # later entries take precedence
        d = (dr + k) % 4
        x, y = ax + dv[d, 0], ay + dv[d, 1]
        ok = (x >= 0) & (x < S) & (y >= 0) & (y < S)
        ok &= typ[n, np.clip(x, 0, S - 1), np.clip(y, 0, S - 1)] == EMPTY
        drop = np.where(ok, a, drop)
    fx, fy = np.clip(ax + dv[dr, 0], 0, S - 1), np.clip(ay + dv[dr, 1], 0, S - 1)
    front_key = typ[n, fx, fy] == KEY
    actions, cost = np.zeros(N, np.int32), np.zeros(N, np.int32)
    for i in range(N):
        if done[i]:
            a, c = DONE, 0
        elif not has_t[i]:
            a, c = (int(ta[i]), 1) if ta[i] != NONE else (DONE, COST_UNSUPPORTED)
        elif rule3[i]:
            a, c = drop[i], COST_DROP
        elif d1[i] < INF:
            if at_cell[i]:
                a, c = (a1[i], d1[i]) if d1[i] > 0 else (DONE, 0)
            elif d1[i] == 0:
                a, c = (drop[i], COST_DROP) if ta[i] == PICKUP and hand[i] else (int(ta[i]), 1)
            else:
                a, c = a1[i], d1[i] + 1
        elif hand[i] and not needed[i]:
            a, c = drop[i], COST_DROP
        elif not hand[i] and d2[i] < INF:
            a = a2[i] if d2[i] > 0 else (PICKUP if front_key[i] else TOGGLE)
            c = COST_KEY
        else:
            a, c = DONE, COST_GIVE_UP
        actions[i], cost[i] = a, c
    return actions, cost


class ExpertActor:
    """The expert as an actor over `engine` (mgx_expert_act): it quacks like a FusedActor for inference --
    evaluate_policy(expert, engine, n, fused=expert) and GraphEvaluator(expert) run it unchanged -- but it acts on the
    engine's CURRENT state, not on rows of a buffer: `t` must be the buffer's newest observation.  That is checked
    where the host can see it (act(): the buffer's rollout position against the engine's call count); _run, which
    gets bare indices, only checks the buffer's engine.  last_cost: the cost tensor (i32 [N]) of the last call.
    A duck type, not a CompactActor: it has no values or logits, and its act reads no rows."""

    def __init__(self, engine):
        import torch
        from . import _lib
        self.engine = engine
        self.policy = self
        self.training = False
        self.last_cost = torch.zeros(engine.n, dtype=torch.int32, device=engine.device)
        self._lib = _lib
        self._base = {}            # id(buffer) -> (weak ref, call count mod T of its observation 0, last call count)

    def sync(self):
        """Nothing to sync: the expert has no weights."""

    def train(self, mode=True):
        return self

    def predict(self, obs, deterministic=True):
        raise TypeError("ExpertActor.predict: the expert needs the engine's state, not an observation -- use "
                        "act(buf, t) (evaluate_policy(expert, engine, n, fused=expert))")

    def expert_act(self, out=None, cost=True):
        """mgx_expert_act on the current stream -> actions (int32 / int64 [N]; `out` or a fresh int64 tensor); the
        costs go to last_cost unless cost=False."""
        import torch
        e, _lib = self.engine, self._lib
        if out is None:
            out = torch.empty(e.n, dtype=torch.int64, device=e.device)
        elif out.dtype not in (torch.int32, torch.int64) or out.numel() != e.n or not out.is_contiguous() \
                or out.device != e.device:
            raise ValueError("out must be a contiguous int32/int64 [%d] tensor on %s" % (e.n, e.device))
        _lib.check(e.L.mgx_expert_act(e.h, ctypes.c_void_p(out.data_ptr()), out.element_size(),
                                      ctypes.c_void_p(self.last_cost.data_ptr()) if cost else None, e._stream()),
                   "mgx_expert_act")
        return out

    def _run(self, buf, index, mode, terminal=False, logits=False, out=None):
        if buf.engine is not self.engine:
            raise ValueError("the buffer belongs to another engine")
        if terminal or logits or mode == 0:
            raise ValueError("ExpertActor has actions only: no values, logits or terminal observations")
        if index.numel() != self.engine.n:
            raise ValueError("ExpertActor acts for every env of the engine at once")
        actions = self.expert_act(None if out is None else out[0])
        return actions, None, None, None

    def act(self, buf, t, deterministic=True, envs=None, logits=False, out=None):
        """(actions, None, None) for observation t of `buf`, which must be the newest: the engine's state is what
        the expert reads."""
        if envs is not None:
            raise ValueError("ExpertActor acts for every env of the engine at once")
        if buf.engine is not self.engine:
            raise ValueError("the buffer belongs to another engine")
        if isinstance(t, int):
            # a buffer stepped in lockstep with the engine starts rollout c at call base + c * T; the base is taken
            # from the first act on the buffer since the engine's last reset (that one cannot be checked)
            calls = self.engine.calls
            key = self._base.get(id(buf))
            if key is None or key[0]() is not buf or calls < key[2]:
                key = self._base[id(buf)] = (weakref.ref(buf), (calls - t) % buf.T, calls)
            if not 0 <= t <= buf.T or (calls - t - key[1]) % buf.T != 0:
                raise ValueError("ExpertActor.act: observation %d is not the engine's current state (engine call count "
                                 "%d, buffer rollouts of %d steps)" % (t, calls, buf.T))
            self._base[id(buf)] = (key[0], key[1], calls)
        a = self._run(buf, buf._arange, 1, out=out)[0]
        return a, None, None
