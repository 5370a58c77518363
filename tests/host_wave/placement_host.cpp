// placement_host.cpp -- TEST INFRASTRUCTURE: the engine's episode generator on the host (reset_env, one env
// after the other) with the live-lock word cap `llw` as an argument, so that small caps make the cap fire inside
// the placement draws (tests/test_placement_draws_host.py checks every episode against the C oracle).
#include "host_lane.h"

using namespace hostlane;

namespace {
template <int NW, bool EXT>
int run(const Config &c, int n, int64_t seed, int episodes, const std::vector<uint64_t> &tab, uint8_t *grids,
        uint8_t *agent, uint8_t *target, int64_t *cursor, uint64_t *pcg, int32_t *livelock) {
    const int S = c.S;
    uint32_t err = 0;
    for (int i = 0; i < n; i++) {
        Lane<NW, EXT> L;
        L.init(c, tab, (uint64_t)(seed + i));
        Gen<NW> &G = L.G;
        for (int k = 0; k < episodes; k++) {
            ResetOut R;
            reset_env<NW, EXT>(G, R);
            const size_t o = (size_t)i * episodes + k;
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

extern "C" int pd_run(int problem, int mission, int S, int nobj, int ado, int llw, int n, int64_t seed, int episodes,
                      uint8_t *grids, uint8_t *agent, uint8_t *target, int64_t *cursor, uint64_t *pcg,
                      int32_t *livelock) {
    const std::vector<uint64_t> tab = mt_table(seed, 1 << 18);
    const Config c{problem, mission, S, nobj, ado, 0, (uint32_t)llw};
    const int nw = S * S <= 64 ? 1 : (S * S <= 128 ? 2 : 4);
#define PD(NW_) return run<NW_, false>(c, n, seed, episodes, tab, grids, agent, target, cursor, pcg, livelock)
    if (nw == 1) PD(1);
    if (nw == 2) PD(2);
    PD(4);
#undef PD
}
