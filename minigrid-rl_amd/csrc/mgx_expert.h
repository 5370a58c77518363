// mgx_expert_act (include/mgx.h, added within ABI 9): the shortest-path expert of mgx/expert.py
// (expert_reference is the normative definition; the rules are restated in include/mgx.h) for every env of a handle,
// from the engine's own state -- EnvState and the one-byte-per-cell grid -- in one launch.
//
// Lane = env, one wave per workgroup of 64 envs.  The wave copies its 64 grids from HBM into LDS with 16-B loads
// (consecutive lanes on consecutive pieces; a lane's grid starts at an odd number of 16-B slots, so the lanes' own
// 16-B reads do not share banks), each lane folds its grid into BOARDS -- one bit per cell, row y of the grid in
// half y of eight 32-bit words (a fixed 16-bit row stride, whatever S is: bit x + 16 (y & 1) of word y >> 1) --
// and the search runs on boards in registers: four boards, one per direction, hold the labelled states.
//
// The search is a backward breadth-first search from the goal set G.  Layer k holds the states with cost-to-go k.
// A state's predecessors are the two turns (the same cell on the boards of d - 1 and d + 1) and the cell behind it
// (one shift of board d against DV[d]), the latter only when the state's own cell can be entered; a cell entered
// through a door that has to be toggled first costs 2, so what such cells contribute is held back one layer.  A
// lane stops caring once its agent's state is labelled (layer L) or its frontier is empty (unreachable); the
// layers at which the agent's three successors were labelled decide the first action: the first of [forward, left,
// right] with edge cost + layer == L.  The loop ends when every lane of the wave has stopped, and after 8 S^2
// layers at the latest (4 S^2 states, edge costs <= 2): a lane that gets there reports "unreachable", so no
// board, however wrong, can hang a wave.  The key routine is a second run with other seeds, entered only when some
// lane of the wave needs it (wave-uniform).  Integers only; no atomics; nothing of the handle is written.
//
// MGX_HOST_SIM: ex_lane and everything under it compile for the host (one lane at a time, the wave votes being
// the lane's own flag) -- the CPU check of the boards and the search against expert_reference.
#pragma once

#define EX_THREADS 64                    // one wave
constexpr int EX_INF = 0x3FFF;           // "not labelled" (every real layer is <= 8 * 16 * 16 = 2048)
constexpr int EX_GRID_SLOTS = 17;        // 16-B slots per env grid in LDS: GS / 16 <= 16, made odd
constexpr int EX_BOARD_WORDS = 28;       // per lane: three boards of 8 words (E1, E2, key cells) + 4 words: 7 slots, odd

#ifdef MGX_HOST_SIM
#define EX_ALL(x) (x)
#define EX_ANY(x) (x)
#else
#define EX_ALL(x) __all(x)
#define EX_ANY(x) __any(x)
#endif

// the cells a forward move in direction D enters the cells of `b` from: r[c - DV[D]] = b[c]
template <int D>
__device__ __forceinline__ void ex_pred(const uint32_t (&b)[8], uint32_t (&r)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (D == 0) r[i] = (b[i] >> 1) & 0x7FFF7FFFu;                          // x - 1 (bit 16 must not reach bit 15)
        else if (D == 2) r[i] = (b[i] << 1) & 0xFFFEFFFEu;                     // x + 1
        else if (D == 1) r[i] = (b[i] >> 16) | (i < 7 ? b[i < 7 ? i + 1 : 7] << 16 : 0u);   // y - 1
        else r[i] = (b[i] << 16) | (i > 0 ? b[i > 0 ? i - 1 : 0] >> 16 : 0u);               // y + 1
    }
}

// word w of a board, w a per-lane value (a select chain: a register array is never indexed dynamically)
__device__ __forceinline__ uint32_t ex_pick(const uint32_t (&b)[8], int w) {
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) r = (w == i) ? b[i] : r;
    return r;
}

// the predecessors of layer `N` on board D: both turns, and the cells behind those of N[D] that can be entered at
// cost 1 and behind what was held back (cost 2)
template <int D>
__device__ __forceinline__ void ex_expand(const uint32_t (&N)[4][8], const uint32_t (&H)[4][8], const uint32_t (&E1)[8],
                                          uint32_t (&C)[8]) {
    uint32_t src[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) src[i] = (N[D][i] & E1[i]) | H[D][i];
    ex_pred<D>(src, C);
#pragma unroll
    for (int i = 0; i < 8; ++i) C[i] |= N[(D + 1) & 3][i] | N[(D + 3) & 3][i];
}

struct ExRoute {
    int L;          // cost-to-go of the agent's state, EX_INF = unreachable
    int act;        // its first action (FORWARD / TOGGLE / LEFT / RIGHT); meaningless unless 0 < L < EX_INF
};

// T: the target cells.  at_cell: G = the cells of T in every direction; else G = every state facing a cell of T.
__device__ __forceinline__ ExRoute ex_search(const uint32_t (&E1)[8], const uint32_t (&E2)[8], const uint32_t (&T)[8],
                                             bool at_cell, int ax, int ay, int dir, int S, int maxl) {
    uint32_t R[4][8], N[4][8], H[4][8];
    {
        uint32_t f0[8], f1[8], f2[8], f3[8];
        ex_pred<0>(T, f0); ex_pred<1>(T, f1); ex_pred<2>(T, f2); ex_pred<3>(T, f3);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            N[0][i] = at_cell ? T[i] : f0[i];
            N[1][i] = at_cell ? T[i] : f1[i];
            N[2][i] = at_cell ? T[i] : f2[i];
            N[3][i] = at_cell ? T[i] : f3[i];
        }
    }
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int i = 0; i < 8; ++i) { R[d][i] = N[d][i]; H[d][i] = 0u; }
    // the agent's cell and the cell in front of it, as (word, bit); a position outside the board matches nothing
    const int aw = ay >> 1;
    const uint32_t ab = (ax < 16 && ay < 16) ? 1u << (ax + 16 * (ay & 1)) : 0u;
    const int fx = ax + ((dir == 0) - (dir == 2)), fy = ay + ((dir == 1) - (dir == 3));
    const bool fok = (unsigned)fx < (unsigned)S && (unsigned)fy < (unsigned)S;
    const int fw = fok ? fy >> 1 : 8;
    const uint32_t fb = fok ? 1u << (fx + 16 * (fy & 1)) : 0u;
    const int ec = (ex_pick(E1, fw) & fb) ? 1 : (ex_pick(E2, fw) & fb) ? 2 : EX_INF;
    const int dl = (dir + 3) & 3, dr = (dir + 1) & 3;
    int LA = EX_INF, lf = EX_INF, ll = EX_INF, lr = EX_INF;
    bool fin = false;
    for (int k = 0; k <= maxl; ++k) {
        if (k > 0) {
            uint32_t C[4][8];
            ex_expand<0>(N, H, E1, C[0]);
            ex_expand<1>(N, H, E1, C[1]);
            ex_expand<2>(N, H, E1, C[2]);
            ex_expand<3>(N, H, E1, C[3]);
#pragma unroll
            for (int d = 0; d < 4; ++d)
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    H[d][i] = N[d][i] & E2[i];
                    const uint32_t nn = C[d][i] & ~R[d][i];
                    N[d][i] = nn;
                    R[d][i] |= nn;
                }
        }
        // which of the four states of the agent's cell, and of the front cell, this layer labelled
        uint32_t hit_a = 0, hit_f = 0, live = 0;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            hit_a |= ((ex_pick(N[d], aw) & ab) ? 1u : 0u) << d;
            hit_f |= ((ex_pick(N[d], fw) & fb) ? 1u : 0u) << d;
#pragma unroll
            for (int i = 0; i < 8; ++i) live |= N[d][i] | H[d][i];
        }
        if (LA == EX_INF && ((hit_a >> dir) & 1u)) LA = k;
        if (ll == EX_INF && ((hit_a >> dl) & 1u)) ll = k;
        if (lr == EX_INF && ((hit_a >> dr) & 1u)) lr = k;
        if (lf == EX_INF && ((hit_f >> dir) & 1u)) lf = k;
        fin = fin || LA != EX_INF || live == 0u;
        if (EX_ALL(fin)) break;
    }
    ExRoute r;
    r.L = LA;
    r.act = (ec + lf == LA) ? (ec == 2 ? A_TOGGLE : A_FORWARD) : (ll + 1 == LA) ? A_LEFT : A_RIGHT;
    return r;
}

// One pass over the lane's grid `g` (S * S cell codes, y-major, 16-B aligned), two boards out through `brd`.  PASS 1: brd[0..8) = E1, the cells entered at cost 1 (empty, open door); brd[8..16) = E2, at
// cost 2 (closed door; locked door of the carried key's colour `keycol`, 8 = no key); returns the set of the
// locked doors' colours.  PASS 2: brd[16..24) = the keys and key-holding boxes whose colour is in `lcol`.
// The loop's control (cell index, x, y) is the same in every lane.
template <int PASS>
__device__ __forceinline__ uint32_t ex_scan(const uint8_t *g, uint32_t *brd, int S, int keycol, uint32_t lcol) {
    uint32_t *rows = brd + (PASS == 1 ? 0 : 16);       // row y: half y & 1 of word y >> 1 (the words are zeroed first)
#pragma unroll
    for (int i = 0; i < (PASS == 1 ? 16 : 8); ++i) brd[(PASS == 1 ? 0 : 16) + i] = 0u;
    const int cells = S * S, chunks = (cells + 15) >> 4;
    uint32_t ra = 0, rb = 0, seen = 0;
    int x = 0, y = 0;
    for (int c = 0; c < chunks; ++c) {
        const uint4 q = *reinterpret_cast<const uint4 *>(g + 16 * c);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (16 * c + j < cells) {
                const uint32_t code = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
                const int t = code & 15, col = (code >> 4) & 7, aux = code >> 7;
                if (PASS == 1) {
                    const bool door = t == T_DOOR;
                    ra |= (uint32_t)(t == T_EMPTY || t == T_OPEN) << x;
                    rb |= (uint32_t)(door && (!aux || col == keycol)) << x;
                    seen |= (uint32_t)(door && aux) << col;
                } else {
                    ra |= (uint32_t)((t == T_KEY || (t == T_BOX && aux)) && ((lcol >> col) & 1u)) << x;
                }
                if (++x == S) {
                    rows[y >> 1] |= ra << (16 * (y & 1));
                    if (PASS == 1) rows[8 + (y >> 1)] |= rb << (16 * (y & 1));
                    ra = rb = 0;
                    x = 0;
                    ++y;
                }
            }
        }
    }
    return seen;
}

__device__ __forceinline__ uint8_t ex_cell(const uint8_t *g, int S, int x, int y) {
    return ((unsigned)x < (unsigned)S && (unsigned)y < (unsigned)S) ? g[y * S + x] : CODE_WALL;
}

// The expert of one env (mgx/expert.py's rules, in their order).  live: the lane holds an env.
__device__ __forceinline__ void ex_lane(const EnvState &st, bool live, const uint8_t *g, uint32_t *brd, int S,
                                        int &action, int &cost) {
    const int ax = st.ax, ay = st.ay, dir = st.dir & 3, ta = st.target_action;
    const bool hand = st.carry != 0, has_key = (st.carry & 15) == T_KEY;
    const int keycol = has_key ? (st.carry >> 4) & 7 : 8;
    const uint32_t lcol = ex_scan<1>(g, brd, S, keycol, 0u);
    const bool needed = has_key && ((lcol >> keycol) & 1u);
    const bool has_t = st.tx != NONE8;
    const bool rule3 = ta == A_PICKUP && hand && !needed;
    const bool at_cell = ta == NONE8 || ta == 0;
    const bool need1 = live && !st.mission_done && has_t && !rule3;
    const int maxl = 8 * S * S;
    ExRoute r1, r2;
    {
        const int tw = st.ty >> 1;
        const uint32_t tb = (need1 && st.tx < 16 && st.ty < 16) ? 1u << (st.tx + 16 * (st.ty & 1)) : 0u;
        uint32_t T[8], E1[8], E2[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            T[i] = (i == tw) ? tb : 0u;
            const uint32_t fin = at_cell ? T[i] : 0u;          // the final cell may be entered, at cost 1
            E1[i] = brd[i] | fin;
            E2[i] = brd[8 + i] & ~fin;
        }
        r1 = ex_search(E1, E2, T, at_cell, ax, ay, dir, S, maxl);
    }
    const bool reach1 = need1 && r1.L < EX_INF;
    const bool need2 = need1 && !reach1 && !hand;
    r2.L = EX_INF;
    r2.act = A_DONE;
    if (EX_ANY(need2)) {
        ex_scan<2>(g, brd, S, keycol, lcol);
        uint32_t T[8], E1[8], E2[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            T[i] = need2 ? brd[16 + i] : 0u;
            E1[i] = brd[i];
            E2[i] = brd[8 + i];
        }
        r2 = ex_search(E1, E2, T, false, ax, ay, dir, S, maxl);
    }
    // the drop routine: the first empty cell among front, right, left, behind
    const int dx = (dir == 0) - (dir == 2), dy = (dir == 1) - (dir == 3);
    const uint8_t cf = ex_cell(g, S, ax + dx, ay + dy), cr = ex_cell(g, S, ax - dy, ay + dx);
    const uint8_t cl = ex_cell(g, S, ax + dy, ay - dx), cb = ex_cell(g, S, ax - dx, ay - dy);
    const int drop = cf == CODE_EMPTY ? A_DROP : cr == CODE_EMPTY ? A_RIGHT : cl == CODE_EMPTY ? A_LEFT
                     : cb == CODE_EMPTY ? A_RIGHT : A_DONE;
    int a, c;
    if (st.mission_done) { a = A_DONE; c = 0; }
    else if (!has_t) { a = ta != NONE8 ? ta : A_DONE; c = ta != NONE8 ? 1 : -1; }
    else if (rule3) { a = drop; c = -2; }
    else if (reach1) {
        if (at_cell) { a = r1.L > 0 ? r1.act : A_DONE; c = r1.L; }
        else if (r1.L == 0) { const bool full = ta == A_PICKUP && hand; a = full ? drop : ta; c = full ? -2 : 1; }
        else { a = r1.act; c = r1.L + 1; }
    }
    else if (hand && !needed) { a = drop; c = -2; }
    else if (need2 && r2.L < EX_INF) { a = r2.L > 0 ? r2.act : ((cf & 15) == T_KEY ? A_PICKUP : A_TOGGLE); c = -3; }
    else { a = A_DONE; c = -4; }
    action = a;
    cost = c;
}

#ifndef MGX_HOST_SIM
struct ExpertArgs {
    const EnvState *state;
    const uint8_t *grid;           // [n][GS]
    void *actions;                 // i32 or i64 [n]
    int32_t *cost;                 // i32 [n] or null
    int64_t n;
    int S, GS, action_bytes;
};

__global__ __launch_bounds__(EX_THREADS) void mgx_expert_kernel(ExpertArgs a) {
    __shared__ uint4 s_grid[EX_THREADS * EX_GRID_SLOTS];
    __shared__ __align__(16) uint32_t s_brd[EX_THREADS * EX_BOARD_WORDS];
    const int lane = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * EX_THREADS, e = e0 + lane;
    const int nv = (int)((a.n - e0) < (int64_t)EX_THREADS ? (a.n - e0) : (int64_t)EX_THREADS);
    const int gslots = a.GS >> 4, stride = gslots | 1;               // gslots <= 16 (the host checks)
    const uint4 *src = reinterpret_cast<const uint4 *>(a.grid + e0 * a.GS);
    const int total = nv * gslots;                                   // the wave's grids are contiguous in HBM
    for (int q = lane; q < total; q += EX_THREADS) {
        const int env = q / gslots;
        s_grid[env * stride + (q - env * gslots)] = src[q];
    }
    __syncthreads();
    const bool live = e < a.n;
    EnvState st = {};
    st.mission_done = 1;
    if (live) st = a.state[e];
    int action, cost;
    ex_lane(st, live, reinterpret_cast<const uint8_t *>(s_grid + lane * stride), s_brd + lane * EX_BOARD_WORDS, a.S,
            action, cost);
    if (live) {
        if (a.action_bytes == 8) reinterpret_cast<int64_t *>(a.actions)[e] = action;
        else reinterpret_cast<int32_t *>(a.actions)[e] = action;
        if (a.cost) a.cost[e] = cost;
    }
}
#endif
