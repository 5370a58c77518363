"""A deterministic scripted agent that plays episodes to their end: it solves missions, fetches keys
and unlocks doors, runs into the time limit, and ends episodes on their very last step -- the states
a trained policy lives in and uniform random actions (which play `done` one step in seven) never reach.

The agent sees one env's state in the dump layout both the reference runner (make_golden.py) and the C
oracle (OracleVec.dump()) produce:

  grid      u8 [S][S][4], x-major: (type, colour, state, box-holds-key); door state 0 open / 1 closed /
            2 locked; types 1 empty, 2 wall, 4 door, 5 key, 6 ball, 7 box, 8 goal, 9 lava
  agent     (x, y, dir), dir 0..3 = +x, +y, -x, -y
  carrying  the same four bytes as a grid cell, type 0 = empty hand
  target    (tx, ty, target action); 255 = None
  mission_done, step_count

plus a context per env (AgentCtx): a numpy Generator seeded from (agent seed, env index) and two small
memories that are cleared at every step_count == 0.  Equal states give equal actions, so a run over the
oracle reproduces a run over the reference as long as the two agree.

Mode = env index % 5: 0, 1 solver; 2 keyer; 3 wanderer; 4 last-step.  Every mode first takes a uniform
action from 0..5 with probability 0.05.

  solver     shortest path (BFS over empty cells, open doors, closed doors, locked doors while carrying
             their key; the goal only as the final cell) to the target cell, or to a neighbour of the
             target facing it, then the target action; empties its hand before a pickup; falls back to
             the key routine when the target is out of reach, then to wandering; a mission without a
             target position: its target action with probability 0.3, else wanders.  With the mission
             complete it waits 0..3 steps and plays `done`.
  keyer      while a locked door stands: fetch the key of its colour (toggling the box that holds it),
             carry it to the door, toggle; drop any other carried object first.  In three episodes of
             ten it first carries a key of another colour to a locked door and toggles that (the door
             stays locked).  With no locked door left it is a solver.
  wanderer   left / right / forward x4 / pickup / drop / toggle, never `done`; refuses to step into lava
             or onto the goal with probability 0.98 -- it runs into the time limit.
  last-step  a solver that holds the completed mission until step_count == size^2 - 1 and plays `done`
             on that step; on `go to goal` it stands beside the goal, looking away, and turns and steps onto
             it on that step: the episode terminates and truncates on one step.
"""
import numpy as np

LEFT, RIGHT, FORWARD, PICKUP, DROP, TOGGLE, DONE = range(7)
EMPTY, WALL, DOOR, KEY, BALL, BOX, GOAL, LAVA = 1, 2, 4, 5, 6, 7, 8, 9
NONE = 255
DV = ((1, 0), (0, 1), (-1, 0), (0, -1))
MODES = ("solver", "solver", "keyer", "wanderer", "laststep")
P_RANDOM, P_TARGET_ACTION, P_REFUSE, P_WRONG_KEY = 0.05, 0.3, 0.98, 0.3
_WANDER = (LEFT, RIGHT, FORWARD, FORWARD, FORWARD, FORWARD, PICKUP, DROP, TOGGLE)
_HERE, _FACING = -1, -2


class AgentCtx:
    """What the agent keeps per env beside the env's own state."""

    def __init__(self, seed, index):
        self.mode = MODES[index % 5]
        self.rng = np.random.default_rng([int(seed), int(index)])
        self.wait = -1              # steps left before `done`, -1 = not drawn yet
        self.wrong_key = False      # keyer: this episode starts with the wrong key


class View:
    """One env's state as plain Python lists."""
    __slots__ = ("S", "grid", "x", "y", "dir", "carry", "target", "mission_done", "step_count", "_things")

    def __init__(self, S, grid, agent, carry, target, mission_done, step_count):
        self.S, self.grid = S, grid
        self.x, self.y, self.dir = agent
        self.carry, self.target = carry, target
        self.mission_done, self.step_count = mission_done, step_count
        self._things = None

    def things(self):
        """((x, y), cell) of every cell that is neither empty nor wall, in x-major order."""
        if self._things is None:
            self._things = [((x, y), c) for x, col in enumerate(self.grid) for y, c in enumerate(col) if c[0] > WALL]
        return self._things


def views(st):
    """Views of every env of a state dict of arrays (OracleVec.dump(), or the same keys of a fixture)."""
    grid, agent, carry = st["grid"].tolist(), st["agent"].tolist(), st["carrying"].tolist()
    target, md, sc = st["target"].tolist(), st["mission_done"].tolist(), st["step_count"].tolist()
    S = st["grid"].shape[1]
    return [View(S, grid[i], agent[i], carry[i], target[i], md[i], sc[i]) for i in range(len(agent))]


def _passable(cell, carry):
    t = cell[0]
    if t == EMPTY:
        return True
    if t == DOOR:
        return cell[2] != 2 or (carry[0] == KEY and carry[1] == cell[1])
    return False


def _turn(cur, want):
    return RIGHT if (want - cur) % 4 == 1 else LEFT


def _route(v, dests):
    """First action of a shortest path from the agent's cell to any cell of `dests` (each an admissible end
    cell), _HERE when it stands on one, None when none can be reached."""
    start = (v.x, v.y)
    if start in dests:
        return _HERE
    grid, carry = v.grid, v.carry
    parent = {start: None}
    queue, head, found = [start], 0, None
    while head < len(queue) and found is None:
        c = queue[head]
        head += 1
        for dx, dy in DV:
            n = (c[0] + dx, c[1] + dy)
            if n in parent:
                continue
            if n in dests:
                parent[n] = c
                found = n
                break
            if _passable(grid[n[0]][n[1]], carry):
                parent[n] = c
                queue.append(n)
    if found is None:
        return None
    while parent[found] != start:
        found = parent[found]
    want = DV.index((found[0] - v.x, found[1] - v.y))
    if v.dir != want:
        return _turn(v.dir, want)
    cell = grid[found[0]][found[1]]
    return TOGGLE if cell[0] == DOOR and cell[2] != 0 else FORWARD


def _approach(v, cell):
    """Towards a neighbour of `cell`, then turn to face it: an action, _FACING, or None (out of reach)."""
    dests = set()
    for dx, dy in DV:
        n = (cell[0] + dx, cell[1] + dy)
        if 0 <= n[0] < v.S and 0 <= n[1] < v.S and (n == (v.x, v.y) or _passable(v.grid[n[0]][n[1]], v.carry)):
            dests.add(n)
    r = _route(v, dests)
    if r != _HERE:
        return r
    want = DV.index((cell[0] - v.x, cell[1] - v.y))
    return _FACING if v.dir == want else _turn(v.dir, want)


def _front(v):
    dx, dy = DV[v.dir]
    return v.grid[v.x + dx][v.y + dy]


def _drop(v):
    """Empty the hand onto an empty front cell, turning towards one first."""
    if _front(v)[0] == EMPTY:
        return DROP
    for d, (dx, dy) in enumerate(DV):
        if v.grid[v.x + dx][v.y + dy][0] == EMPTY:
            return _turn(v.dir, d)
    return RIGHT


def _idle(v):
    """Pass a step without changing anything that matters: bump a wall, else turn."""
    return FORWARD if _front(v)[0] == WALL else RIGHT


def _wander(v, ctx):
    a = _WANDER[int(ctx.rng.integers(0, 9))]
    if a == FORWARD and _front(v)[0] in (GOAL, LAVA) and ctx.rng.random() < P_REFUSE:
        a = LEFT
    return a


def _cells(v, pred):
    return [p for p, c in v.things() if pred(c)]


def _fetch(v, cells):
    """Towards the first reachable of `cells`, then pick it up (a key) or toggle it (a box)."""
    for c in cells:
        r = _approach(v, c)
        if r == _FACING:
            return PICKUP if v.grid[c[0]][c[1]][0] == KEY else TOGGLE
        if r is not None:
            return r
    return None


def _keys(v, ctx):
    """The key routine: an action, or None when no locked door is left or nothing can be done about one."""
    locked = _cells(v, lambda c: c[0] == DOOR and c[2] == 2)
    if not locked:
        return None
    colours = [v.grid[x][y][1] for x, y in locked]
    carry = v.carry
    if carry[0] == KEY:
        if carry[1] in colours:
            r = _approach(v, locked[colours.index(carry[1])])
            if r == _FACING:
                return TOGGLE
            if r is not None:
                return r
        elif ctx.wrong_key:
            for c in locked:
                r = _approach(v, c)
                if r == _FACING:
                    ctx.wrong_key = False
                    return TOGGLE
                if r is not None:
                    return r
            ctx.wrong_key = False
    if carry[0] != 0:
        return _drop(v)
    if ctx.wrong_key:
        r = _fetch(v, _cells(v, lambda c: c[0] == KEY and c[1] not in colours))
        if r is not None:
            return r
        ctx.wrong_key = False
    for col in colours:
        r = _fetch(v, _cells(v, lambda c: c[1] == col and (c[0] == KEY or (c[0] == BOX and c[3] == 1))))
        if r is not None:
            return r
    return None


def _solve(v, ctx, hold):
    last = v.step_count == v.S * v.S - 1
    if v.mission_done:
        if hold:
            return DONE if last else _idle(v)
        if ctx.wait < 0:
            ctx.wait = int(ctx.rng.integers(0, 4))
        if ctx.wait == 0:
            ctx.wait = -1
            return DONE
        ctx.wait -= 1
        return _idle(v)
    tx, ty, ta = v.target
    if tx == NONE:
        if ta != NONE and ctx.rng.random() < P_TARGET_ACTION:
            return ta
        return _wander(v, ctx)
    if ta == NONE:                                  # go to goal: the goal cell itself
        if hold:
            r = _approach(v, (tx, ty))
            if abs(tx - v.x) + abs(ty - v.y) == 1:  # beside the goal: look away until the turns left are due
                turns = (0, 1, 2, 1)[(DV.index((tx - v.x, ty - v.y)) - v.dir) % 4]
                if v.S * v.S - 1 - v.step_count > turns:
                    if turns == 0:
                        return RIGHT
                    return PICKUP if v.carry[0] != 0 else DROP      # (neither does anything)
                return FORWARD if r == _FACING else r
        else:
            r = _route(v, {(tx, ty)})
        if r is not None and r != _HERE:
            return r
    else:
        if ta == PICKUP and v.carry[0] != 0:
            return _drop(v)
        r = _approach(v, (tx, ty))
        if r == _FACING:
            if ta == DONE and hold and not last:    # `go to`: its `done` completes and ends at once
                return DROP if _front(v)[0] != EMPTY else _idle(v)
            return ta
        if r is not None:
            return r
    r = _keys(v, ctx)
    return _wander(v, ctx) if r is None else r


def act(v, ctx):
    """The action of one env: `v` its View, `ctx` its AgentCtx."""
    if v.step_count == 0:
        ctx.wait = -1
        ctx.wrong_key = ctx.mode == "keyer" and ctx.rng.random() < P_WRONG_KEY
    if ctx.rng.random() < P_RANDOM:
        return int(ctx.rng.integers(0, 6))
    if ctx.mode == "wanderer":
        return _wander(v, ctx)
    if ctx.mode == "keyer":
        r = _keys(v, ctx)
        if r is not None:
            return r
    return _solve(v, ctx, ctx.mode == "laststep")


class ScriptedAgent:
    """The agent over n envs: act(state dict of arrays) -> int8 [n]."""

    def __init__(self, n, seed):
        self.ctx = [AgentCtx(seed, i) for i in range(n)]

    def act(self, st):
        return np.array([act(v, c) for v, c in zip(views(st), self.ctx)], np.int8)


def run(vec, agent, T):
    """The agent over `vec` (an OracleVec after reset(), or anything with dump() and step(actions)) for T steps, one
    dump() per step -> the actions, int8 [T][n]."""
    acts = np.zeros((T, len(agent.ctx)), np.int8)
    for t in range(T):
        acts[t] = agent.act(vec.dump())
        vec.step(acts[t].astype(np.int32))
    return acts
