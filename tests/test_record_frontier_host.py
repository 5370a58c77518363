"""The arithmetic of the prefix-record frontier (minigrid-rl_amd/csrc/mgx_device.h: pfx_window, the window of
records one MT slide launch computes and the frontier it leaves, and mt_slide_superblocks, what the launch then
generates) compiled for the HOST (tests/host_gen, -DMGX_HOST_SIM) and driven over synthetic growth sequences of
the stream -- the functions mgx_mt_slide_kernel calls, without a GPU.  Per launch, with hi the groups generated
before it and ring_words the words the ring holds:

  a. no position of [rec_lo, rec_hi) is below hi * 10 - ring_words (no record is computed from a recycled slot);
  b. rec_hi <= hi * 10 - PFX_LOOK (no record reads words not generated yet);
  c. the frontier never decreases;
  d. after the launch the frontier is behind the stream by at most PFX_LOOK + max(what the launch generated,
     PFX_LOOK) -- and so by less than one ring for everything a slide can generate (whole super-blocks, at most
     MT_SLIDE_MAX_SB, never into live groups);
  e. a model of the record slots (one per ring word, the position whose record it holds): after every launch every
     slot holds a position from the ring length below the frontier, or nothing -- a lookup in the live window can
     only meet its own record or the one a single pass before it, which the pass tag tells apart; under (d) the
     frontier skips nothing and the slots hold exactly the ring length below it.

Growth beyond what a slide generates (whole rings per launch) is driven too: the window then skips positions, and
(a), (b), (c), (e) and the first half of (d) must hold all the same.  Test infrastructure only."""
import ctypes

import numpy as np
import pytest

from test_generator_host import _lib


class Sim:
    """MtCtl's hi / rec_done over slide launches, from mgx_create's initial state."""

    def __init__(self, ring_groups, threads, slots):
        self.L = _lib()
        self.look, self.fields, self.sbg, self.maxsb = (self.L.hg_const(k) for k in range(4))
        assert (self.look, self.fields, self.sbg * self.fields) == (320, 10, 3120)
        self.rg, self.rw, self.threads = ring_groups, ring_groups * self.fields, threads
        # mgx_create: the host fills whole super-blocks of min(ring, 2^20 words) (more where ring_depth x livelock_words
        # asks for it: the same state further up the stream), records for all but the last PFX_LOOK
        self.hi = min(self.rw, 1 << 20) // (self.sbg * self.fields) * self.sbg
        self.done = self.hi * self.fields - self.look
        self.slots = None
        if slots:
            self.slots = np.full(self.rw, -1, np.int64)
            self._store(0, self.done)
        self.clean = True                    # no launch has skipped a position yet

    def _store(self, lo, hi):
        lo = max(lo, hi - self.rw)
        pos = np.arange(lo, hi, dtype=np.int64)
        self.slots[pos % self.rw] = pos

    def launch(self, grow_groups, legal=True, may_skip=False):
        """One slide: records first (the window), then `grow_groups` groups generated.  legal: a growth the slide can
        produce; may_skip: the launch before was not."""
        out = (ctypes.c_uint64 * 5)()
        self.L.hg_pfx_window(self.done, self.hi, self.rw, self.threads, self.look, out)
        zero_lo, lo, hi, nxt, strides = (int(v) for v in out)
        top = self.hi * self.fields
        assert zero_lo <= lo <= hi
        assert lo >= top - self.rw, "a: window below the words the ring holds"
        assert hi <= top - self.look, "b: a record would read past the words generated"
        assert nxt >= self.done and nxt == hi, "c: the frontier went back / is not the window's end"
        assert (strides - 1) * self.threads < hi - lo <= strides * self.threads or (hi == lo and strides == 0)
        assert lo >= self.done and zero_lo >= self.done and lo - zero_lo <= self.look   # cleared: skipped positions only
        if not may_skip:
            assert lo == self.done and zero_lo == lo, "a position below the new frontier got no record"
        self.clean = self.clean and lo == self.done
        if self.slots is not None:
            if lo > zero_lo:
                z = np.arange(zero_lo, lo, dtype=np.int64) % self.rw
                w = np.arange(lo, hi, dtype=np.int64) % self.rw
                assert not np.intersect1d(z, w).size, "a cleared slot is also computed by this launch"
                self.slots[z] = -1
            self._store(lo, hi)
        self.done = nxt
        self.hi += grow_groups
        lag = self.hi * self.fields - self.done
        assert lag <= self.look + max(grow_groups * self.fields, self.look), "d: lag beyond what the launch generated"
        if legal:
            assert lag <= self.rw, "d: lag beyond one ring"
        if self.slots is not None:
            held = self.slots[self.slots >= 0]
            assert (held >= self.done - self.rw).all(), "e: a slot holds a position a ring or more below the frontier"
            if self.clean:
                pos = np.arange(max(0, self.done - self.rw), self.done, dtype=np.int64)
                assert np.array_equal(self.slots[pos % self.rw], pos), "e: slots are not the ring below the frontier"

    def slide(self, min_cursor_words, max_cursor_words, ahead=1 << 19):
        """What mgx_mt_slide_kernel generates for these cursors (MT_AHEAD past the furthest, within the ring)."""
        nsb = self.L.hg_slide_superblocks(self.hi, min_cursor_words // self.fields,
                                          (max_cursor_words + ahead) // self.fields, self.rg)
        assert 0 <= nsb <= self.maxsb
        return nsb * self.sbg


RINGS = [512, 1024, 2048, 4096, 1 << 13, 1 << 14, 1 << 15, 1 << 20, 1 << 23, 1 << 26]   # groups (x 10 words)
THREADS = [256, 512, 4096]                       # one slide workgroup, two, the 65,536-env grid


def _slots(rg):
    return rg <= 1 << 15


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("rg", RINGS)
def test_frontier_follows_legal_growth(rg, threads):
    """Zero growth, one super-block per launch (below one position per thread at 4,096 threads, 12 per thread at
    256), the most a slide can generate (every cursor at the stream's end: the whole ring less a remainder, or
    MT_SLIDE_MAX_SB super-blocks), a reset's jump of D x 43 words (D = 256 and 4,096), and random cursors."""
    s = Sim(rg, threads, _slots(rg))
    for _ in range(3):
        s.launch(0)
    for _ in range(8):
        s.launch(s.sbg)
    for _ in range(2 if rg > 1 << 15 else 6):
        top = s.hi * s.fields
        g = s.slide(top, top)                       # nothing live below the end: all the ring may be rewritten
        assert g > 0 and g * s.fields <= s.rw - 400   # (whole super-blocks: never a whole ring, mgx_device.h)
        s.launch(g)
    for D in (256, 4096):
        s.launch(0)
        top = s.hi * s.fields
        g = s.slide(top - 2 * s.look, top - 2 * s.look + D * 43, ahead=0)
        if rg >= 1 << 15:
            assert g * s.fields >= D * 43 - 2 * s.look
        s.launch(g)
    rng = np.random.default_rng(rg + threads)
    for _ in range(40 if rg > 1 << 15 else 200):
        top = s.hi * s.fields
        mn = top - int(rng.integers(0, s.rw))
        mx = min(top, mn + int(rng.integers(0, s.rw)))
        s.launch(s.slide(max(mn, 0), mx, ahead=int(rng.choice([0, 4000, 1 << 19]))))


@pytest.mark.parametrize("threads", [256, 4096])
@pytest.mark.parametrize("rg", [512, 4096, 1 << 15, 1 << 26])
def test_frontier_survives_growth_beyond_a_ring(rg, threads):
    """Growth no slide produces -- a ring less PFX_LOOK plus one group, a whole ring, 2.5 rings, 300 rings per
    launch, between launches of legal growth: the window is clamped to the words the ring holds, the skipped
    positions' records are cleared where the launch does not rewrite them, and the frontier is back behind the
    stream by what the last launch generated one launch later."""
    s = Sim(rg, threads, _slots(rg))
    for g in (rg - s.look // s.fields + 1, rg, rg * 5 // 2, 300 * rg, rg + 7, rg * 256, rg * 256 + 1):
        s.launch(s.sbg)
        s.launch(g, legal=False)           # the launch that over-generates is itself in order ...
        s.launch(s.sbg, may_skip=True)     # ... the next one skips
        s.launch(0)
        s.launch(s.sbg)
