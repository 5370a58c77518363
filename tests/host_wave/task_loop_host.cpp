// task_loop_host.cpp -- TEST INFRASTRUCTURE: the engine's episode generator on the host, one reset ATTEMPT at a time
// (host_lane.h), with the live-lock word cap `llw` as an argument.  Beside every episode's state (what
// placement_host.cpp records) it reports, per episode, what its ABANDONED attempts had placed when they were
// abandoned: tests/test_task_loop_host.py checks every episode against the C oracle and, from these counts, that the
// key / object task loop was left while placements of the same attempt were done and others still pending.
#include "host_lane.h"

using namespace hostlane;

namespace {
template <int NW, bool EXT>
int run(const Config &c, int n, int64_t seed, int episodes, const std::vector<uint64_t> &tab, uint8_t *grids,
        uint8_t *agent, uint8_t *target, int64_t *cursor, uint64_t *pcg, int32_t *livelock, int32_t *left) {
    const int S = c.S;
    uint32_t err = 0;
    for (int i = 0; i < n; i++) {
        Lane<NW, EXT> L;
        L.init(c, tab, (uint64_t)(seed + i));
        Gen<NW> &G = L.G;
        for (int k = 0; k < episodes; k++) {
            const size_t o = (size_t)i * episodes + k;
            ResetOut R;
            int32_t *lf = left + o * 4;
            lf[0] = lf[1] = lf[2] = lf[3] = 0;
            while (!L.attempt(R)) {
                if (L.livelocks > 100000) return -1;
                // the abandoned attempt's objs list: keys (OBJ_KEYFLAG) and objects placed before it was abandoned
                // (doors and the goal come before the task loop)
                int keys = 0, objs = 0;
                for (int j = 0; j < G.nobjs; j++) {
                    const uint32_t e = G.objs[j];
                    const int t = (int)(e & 15u);
                    if (e & OBJ_KEYFLAG) keys++;
                    else if (t != T_DOOR && t != T_GOAL) objs++;
                }
                lf[0] += keys > 0;                     // ... with a key placed
                lf[1] += objs > 0;                     // ... with an object placed
                lf[2] += keys + objs == 0;             // ... with nothing placed yet
                lf[3] += keys > 1;                     // ... with both keys of a room placed
            }
            std::memcpy(grids + o * S * S, G.g, (size_t)S * S);
            agent[o * 3] = (uint8_t)G.ax; agent[o * 3 + 1] = (uint8_t)G.ay; agent[o * 3 + 2] = (uint8_t)G.adir;
            target[o * 4] = R.tx; target[o * 4 + 1] = R.ty; target[o * 4 + 2] = R.ta; target[o * 4 + 3] = R.mission_id;
            cursor[o] = (int64_t)G.cur;
            pcg[o * 4] = G.pcg.sh; pcg[o * 4 + 1] = G.pcg.sl; pcg[o * 4 + 2] = G.pcg.has; pcg[o * 4 + 3] = G.pcg.uinteger;
            livelock[o] = R.livelocks;
        }
        err |= G.err;
    }
    return (int)err;
}
}  // namespace

extern "C" int tl_run(int problem, int mission, int S, int nobj, int ado, int llw, int n, int64_t seed, int episodes,
                      uint8_t *grids, uint8_t *agent, uint8_t *target, int64_t *cursor, uint64_t *pcg,
                      int32_t *livelock, int32_t *left) {
    const std::vector<uint64_t> tab = mt_table(seed, 1 << 18);
    const Config c{problem, mission, S, nobj, ado, 0, (uint32_t)llw};
    const int nw = S * S <= 64 ? 1 : (S * S <= 128 ? 2 : 4);
#define TL(NW_) return run<NW_, false>(c, n, seed, episodes, tab, grids, agent, target, cursor, pcg, livelock, left)
    if (nw == 1) TL(1);
    if (nw == 2) TL(2);
    TL(4);
#undef TL
}
