// refill_wave_model.cpp -- the refill kernel's wave cost, modelled on the host.  A refill wave executes every path
// any of its lanes takes, so a loop costs the wave its UNION trip count: the maximum over the lanes, taken per
// enclosing iteration (task by task, pass by pass).  This program runs the generator of mgx_device.h
// (-DMGX_HOST_SIM, a counting hook behind its GCOUNT sites) for N envs x E episodes, grouped as the kernel groups
// them -- W consecutive envs per wave, one reset ATTEMPT per lane per round, an abandoned attempt retried in the
// next round -- and prints, per attempt round, the lane-mean and the wave-union trip count of every generator loop.
// tools/refill_wave_model.py builds it, runs it and prices the counts with the static instruction counts.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -DMGX_HOST_SIM -Itests/host_gen -Itests/host_wave \
//       -Iminigrid-rl_amd/csrc -o refill_wave_model tools/refill_wave_model.cpp
//   ./refill_wave_model --mission 5 --size 8 --envs 4096 --episodes 11 [--wave 64] [--llw 4096] [--cursors FILE]
//
// Sites (mgx_device.h): 20 key/object task, 27 placement pass (cell_pass), 25 its candidate iteration, 26 word-by-word
// tail entered (builds that still have one), 21 randbelow pass, 24 randbelow call, 22 goal/agent PCG64 iteration,
// 23 MT window reload.
// Round 18 runs all tasks of an attempt through ONE loop over passes: a lane's p-th pass of the attempt, whatever
// task it serves, runs beside every other lane's p-th pass.  "flat_passes" / "flat_cand_iters" are the union counts
// of that loop (the most passes any lane takes; per pass the most candidates), "tasks" / "draw_passes" /
// "cand_iters" those of the task loop around a pass loop that the builds before it have.  The host draws every MT-only prefix (the kernel looks most of them up in its prefix
// records): those passes are reported apart ("prefix_passes") and are no part of the round's model.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace wm {
struct Attempt {
    int ga = 0, pre = 0, post = 0, reload = 0, tasks = 0;
    bool skip21 = false, after_rb = false;
    std::vector<int> passes;                         // [task]
    std::vector<std::vector<int>> cand, tail, tailrb;   // [task][pass]
    void hook(int k) {
        switch (k) {
        case 20: tasks++; passes.push_back(0); cand.emplace_back(); tail.emplace_back(); tailrb.emplace_back(); after_rb = false; break;
        case 27:
            if (tasks) { passes.back()++; cand.back().push_back(0); tail.back().push_back(0); tailrb.back().push_back(0); }
            skip21 = true;
            break;
        case 25: if (tasks && !cand.back().empty()) cand.back().back()++; break;
        case 26: if (tasks && !tail.back().empty()) tail.back().back()++; break;
        case 24: after_rb = true; break;
        case 21:
            if (skip21) { skip21 = false; break; }
            if (!tasks) pre++;
            else if (after_rb || tailrb.back().empty()) post++;
            else tailrb.back().back()++;
            break;
        case 22: ga++; break;
        case 23: reload++; break;
        default: break;
        }
    }
};
Attempt *cur = nullptr;
inline void hook(int k) { if (cur) cur->hook(k); }
}  // namespace wm
#define MGX_GCOUNT_HOOK(k) ::wm::hook(k)

#include "host_lane.h"

using namespace hostlane;

namespace {
const char *NAMES[] = {"tasks", "draw_passes", "cand_iters", "tail_entries", "tail_rb_passes", "goal_agent_iters",
                       "post_rb_passes", "prefix_passes", "window_reloads", "flat_passes", "flat_cand_iters"};
constexpr int NC = 11;

template <int NW>
int run(const Config &c, int n, int W, int64_t seed, int episodes, const char *cursors) {
    const std::vector<uint64_t> tab = mt_table(seed, 1 << 18);
    double lane[NC] = {0}, wave[NC] = {0};
    long long lane_attempts = 0, wave_rounds = 0, abandoned = 0;
    std::vector<long long> final_cur((size_t)n, 0);
    uint32_t err = 0;
    for (int w0 = 0; w0 < n; w0 += W) {
        const int nl = n - w0 < W ? n - w0 : W;
        std::vector<Lane<NW, false>> L((size_t)nl);
        std::vector<int> done((size_t)nl, 0);
        for (int l = 0; l < nl; l++) L[(size_t)l].init(c, tab, (uint64_t)(seed + w0 + l));
        for (;;) {
            std::vector<wm::Attempt> A;
            A.reserve((size_t)nl);
            for (int l = 0; l < nl; l++) {
                if (done[(size_t)l] >= episodes) continue;
                A.emplace_back();
                wm::cur = &A.back();
                ResetOut R;
                if (L[(size_t)l].attempt(R)) done[(size_t)l]++; else abandoned++;
                wm::cur = nullptr;
            }
            if (A.empty()) break;
            wave_rounds++;
            lane_attempts += (long long)A.size();
            // lane sums
            size_t mt = 0;
            for (const auto &a : A) {
                lane[0] += a.tasks;
                for (int t = 0; t < a.tasks; t++) {
                    lane[1] += a.passes[(size_t)t];
                    for (int v : a.cand[(size_t)t]) lane[2] += v;
                    for (int v : a.tail[(size_t)t]) lane[3] += v;
                    for (int v : a.tailrb[(size_t)t]) lane[4] += v;
                }
                lane[5] += a.ga; lane[6] += a.post; lane[7] += a.pre; lane[8] += a.reload;
                for (int t = 0; t < a.tasks; t++) {              // (a lane's own counts do not depend on the loop's shape)
                    lane[9] += a.passes[(size_t)t];
                    for (int v : a.cand[(size_t)t]) lane[10] += v;
                }
                if ((size_t)a.tasks > mt) mt = (size_t)a.tasks;
            }
            // wave unions: the maximum over the lanes per enclosing iteration
            int u5 = 0, u6 = 0, u7 = 0, u8 = 0;
            for (const auto &a : A) {
                if (a.ga > u5) u5 = a.ga;
                if (a.post > u6) u6 = a.post;
                if (a.pre > u7) u7 = a.pre;
                if (a.reload > u8) u8 = a.reload;
            }
            wave[0] += (double)mt; wave[5] += u5; wave[6] += u6; wave[7] += u7; wave[8] += u8;
            {   // one loop over passes: the lane's passes of all its tasks in a row
                std::vector<std::vector<int>> flat;
                size_t fp = 0;
                for (const auto &a : A) {
                    flat.emplace_back();
                    for (int t = 0; t < a.tasks; t++)
                        for (int v : a.cand[(size_t)t]) flat.back().push_back(v);
                    if (flat.back().size() > fp) fp = flat.back().size();
                }
                wave[9] += (double)fp;
                for (size_t p = 0; p < fp; p++) {
                    int uc = 0;
                    for (const auto &f : flat)
                        if (f.size() > p && f[p] > uc) uc = f[p];
                    wave[10] += uc;
                }
            }
            for (size_t t = 0; t < mt; t++) {
                size_t mp = 0;
                for (const auto &a : A)
                    if ((size_t)a.tasks > t && (size_t)a.passes[t] > mp) mp = (size_t)a.passes[t];
                wave[1] += (double)mp;
                for (size_t p = 0; p < mp; p++) {
                    int uc = 0, ut = 0, ur = 0;
                    for (const auto &a : A) {
                        if ((size_t)a.tasks <= t || a.cand[t].size() <= p) continue;
                        if (a.cand[t][p] > uc) uc = a.cand[t][p];
                        if (a.tail[t][p] > ut) ut = a.tail[t][p];
                        if (a.tailrb[t][p] > ur) ur = a.tailrb[t][p];
                    }
                    wave[2] += uc; wave[3] += ut; wave[4] += ur;
                }
            }
        }
        for (int l = 0; l < nl; l++) {
            final_cur[(size_t)(w0 + l)] = (long long)L[(size_t)l].G.cur;
            err |= L[(size_t)l].G.err;
        }
    }
    std::printf("{\"mission\": %d, \"size\": %d, \"all_doors_open\": %d, \"llw\": %u, \"envs\": %d, \"episodes\": %d, "
                "\"wave\": %d, \"err\": %u, \"lane_attempts\": %lld, \"wave_rounds\": %lld, \"abandoned\": %lld, "
                "\"lane_mean\": {", c.mission, c.S, c.ado, c.llw, n, episodes, W, err, lane_attempts, wave_rounds, abandoned);
    for (int i = 0; i < NC; i++) std::printf("%s\"%s\": %.4f", i ? ", " : "", NAMES[i], lane[i] / (double)lane_attempts);
    std::printf("}, \"wave_union\": {");
    for (int i = 0; i < NC; i++) std::printf("%s\"%s\": %.4f", i ? ", " : "", NAMES[i], wave[i] / (double)wave_rounds);
    std::printf("}}\n");
    if (cursors) {
        FILE *f = std::fopen(cursors, "w");
        if (!f) return 2;
        for (int i = 0; i < n; i++) std::fprintf(f, "%lld\n", final_cur[(size_t)i]);
        std::fclose(f);
    }
    return err ? 1 : 0;
}
}  // namespace

int main(int argc, char **argv) {
    int mission = 5, S = 8, n = 4096, episodes = 11, W = 64, ado = 0, llw = 4096;
    long long seed = 42;
    const char *cursors = nullptr;
    for (int i = 1; i + 1 < argc; i += 2) {
        const std::string k = argv[i];
        const char *v = argv[i + 1];
        if (k == "--mission") mission = std::atoi(v);
        else if (k == "--size") S = std::atoi(v);
        else if (k == "--envs") n = std::atoi(v);
        else if (k == "--episodes") episodes = std::atoi(v);
        else if (k == "--wave") W = std::atoi(v);
        else if (k == "--ado") ado = std::atoi(v);
        else if (k == "--llw") llw = std::atoi(v);
        else if (k == "--seed") seed = std::atoll(v);
        else if (k == "--cursors") cursors = v;
        else { std::fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    if (W < 1 || n < 1 || episodes < 1) return 2;
    const Config c{0, mission, S, 4, ado, 0, (uint32_t)llw};
    const int nw = S * S <= 64 ? 1 : (S * S <= 128 ? 2 : 4);
    if (nw == 1) return run<1>(c, n, W, (int64_t)seed, episodes, cursors);
    if (nw == 2) return run<2>(c, n, W, (int64_t)seed, episodes, cursors);
    return run<4>(c, n, W, (int64_t)seed, episodes, cursors);
}
