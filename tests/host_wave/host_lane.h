// host_lane.h -- TEST INFRASTRUCTURE: one env ("lane") of the engine's episode generator
// (minigrid-rl_amd/csrc/mgx_device.h) on the host with the live-lock word cap as a parameter, one reset ATTEMPT
// at a time, the way a refill wave runs it (one attempt per lane per round).  Shared by the placement-draw
// check against the C oracle (placement_host.cpp, tests/test_placement_draws_host.py) and the refill wave-cost
// model (tools/refill_wave_model.cpp).  Built with -DMGX_HOST_SIM, tests/host_gen/host_sim.h on the include path.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "mgx_device.h"

namespace hostlane {
using namespace mgx;

struct MT {                                         // CPython random.seed(n) + genrand_uint32
    uint32_t mt[624];
    int mti;
    void init(uint32_t s) {
        mt[0] = s;
        for (int i = 1; i < 624; i++) mt[i] = 1812433253U * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
        mti = 624;
    }
    void seed(uint64_t n) {
        uint32_t key[2];
        int klen = 0;
        if (n == 0) key[klen++] = 0;
        while (n) { key[klen++] = (uint32_t)n; n >>= 32; }
        init(19650218U);
        int i = 1, j = 0, k = 624 > klen ? 624 : klen;
        for (; k; k--) {
            mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525U)) + key[j] + (uint32_t)j;
            i++; j++;
            if (i >= 624) { mt[0] = mt[623]; i = 1; }
            if (j >= klen) j = 0;
        }
        for (k = 623; k; k--) {
            mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941U)) - (uint32_t)i;
            i++;
            if (i >= 624) { mt[0] = mt[623]; i = 1; }
        }
        mt[0] = 0x80000000U;
    }
    uint32_t next() {
        static const uint32_t mag01[2] = {0U, 0x9908b0dfU};
        uint32_t y;
        if (mti >= 624) {
            int kk;
            for (kk = 0; kk < 624 - 397; kk++) {
                y = (mt[kk] & 0x80000000U) | (mt[kk + 1] & 0x7fffffffU);
                mt[kk] = mt[kk + 397] ^ (y >> 1) ^ mag01[y & 1U];
            }
            for (; kk < 623; kk++) {
                y = (mt[kk] & 0x80000000U) | (mt[kk + 1] & 0x7fffffffU);
                mt[kk] = mt[kk + (397 - 624)] ^ (y >> 1) ^ mag01[y & 1U];
            }
            y = (mt[623] & 0x80000000U) | (mt[0] & 0x7fffffffU);
            mt[623] = mt[396] ^ (y >> 1) ^ mag01[y & 1U];
            mti = 0;
        }
        y = mt[mti++];
        y ^= (y >> 11);
        y ^= (y << 7) & 0x9d2c5680U;
        y ^= (y << 15) & 0xefc60000U;
        y ^= (y >> 18);
        return y;
    }
};

// the packed MT19937(seed) stream (ten top-5-bit fields per group) as one unwrapped ring + the mirror pad
inline std::vector<uint64_t> mt_table(int64_t seed, int64_t groups) {
    std::vector<uint64_t> tab((size_t)groups + MT_PAD, 0ull);
    MT m;
    m.seed((uint64_t)seed);
    for (int64_t w = 0; w < groups * MT_FIELDS; w++) {
        const uint64_t f = m.next() >> 27;
        tab[(size_t)(w / MT_FIELDS)] |= f << (6 * (w % MT_FIELDS));
    }
    for (int k = 0; k < MT_PAD; k++) tab[(size_t)groups + k] = tab[(size_t)k];
    return tab;
}

struct Config {
    int problem, mission, S, nobj, ado, n_obst;
    uint32_t llw;
};

template <int NW, bool EXT>
struct Lane {
    Gen<NW> G;
    std::vector<uint32_t> win, objs;
    std::vector<uint8_t> g;
    int livelocks = 0;                                  // abandoned attempts of the episode in the making

    void init(const Config &c, const std::vector<uint64_t> &tab, uint64_t pcg_seed_) {
        win.assign(win_stride<NW>() + 2, 0u);
        objs.assign(MAX_OBJS + 1, 0u);
        g.assign((size_t)c.S * c.S + 16, 0);
        G.g = g.data();
        G.S = c.S;
        G.table = tab.data();
        G.rmask = (uint64_t)tab.size() - MT_PAD - 1;
        G.tlo = 0;
        G.thi = G.rmask + 1;
        G.win = reinterpret_cast<uint64_t *>(win.data());
        G.objs = objs.data();
        G.llw = c.llw;
        G.err = 0;
        G.problem = c.problem; G.cfg_mission = c.mission; G.num_objects = c.nobj; G.all_doors_open = c.ado;
        G.n_obstacles = c.n_obst;
        G.abort = false; G.nobjs = 0; G.ax = G.ay = -1; G.adir = 0;
        G.phave = false; G.prec = 0;                    // no prefix records on the host: every prefix drawn
        gen_init(G);
        pcg_seed(G.pcg, pcg_seed_);
        G.cur = 0;
        G.gbase = ~0ull >> 1;
    }
    // one attempt, as a refill round runs it; true: an episode was generated (R.livelocks = attempts abandoned for it)
    bool attempt(ResetOut &R) {
        G.astart = G.cur;
        G.abort = false;
        mt_sync(G);
        gen_attempt<NW, EXT>(G, R);
        if (G.abort) { livelocks++; return false; }
        R.livelocks = livelocks;
        livelocks = 0;
        return true;
    }
};
}  // namespace hostlane
