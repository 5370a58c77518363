// expert_host.cpp -- TEST INFRASTRUCTURE: the expert kernel's per-lane routine (minigrid-rl_amd/csrc/mgx_expert.h:
// ex_lane -- the board scan, the layered search, the rules) compiled for the host, one lane at a time, as a CPU
// check against mgx.expert.expert_reference (tests/test_expert_cpu.py).  The wave's staging of the grids through
// LDS is the one part of the kernel that does not run here.
#define MGX_HOST_SIM
#include "mgx_device.h"
using namespace mgx;
#include "mgx_expert.h"

// grid: u8 [n][GS] cell codes (y * S + x); state: [n][16] EnvState bytes; act / cost: i32 [n]
extern "C" void expert_host(const uint8_t *grid, const uint8_t *state, int n, int S, int GS, int32_t *act,
                            int32_t *cost) {
    alignas(16) uint8_t g[272];
    alignas(16) uint32_t brd[EX_BOARD_WORDS];
    for (int e = 0; e < n; ++e) {
        std::memset(g, 0, sizeof g);
        std::memcpy(g, grid + (size_t)e * GS, (size_t)GS);
        EnvState st;
        std::memcpy(&st, state + (size_t)e * 16, 16);
        int a, c;
        ex_lane(st, true, g, brd, S, a, c);
        act[e] = a;
        cost[e] = c;
    }
}
