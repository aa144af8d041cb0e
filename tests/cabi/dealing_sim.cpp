// Host-side play of the pipelined render kernel's ray dealing (g-nerf_amd/csrc/pipe_dealing.h), for tests/test_render_dealing_cpu.py:
//   dealing_sim <total_seq> <workgroups per XCD> <unit> <seed> <schedule 0|1|2> <on demand 0|1>
// Every workgroup walks its local rays r = 0, 1, 2, ... exactly as the scalar wave's propose_issue does (advance on the first ray of a
// unit with what the fetch-add returned, fetch while the unit's last ray is proposed); a seeded scheduler picks which workgroup
// makes its next move: 0 uniformly, 1 one workgroup of each XCD a hundred times as often, 2 one workgroup moves only when no other can.
// Prints "ok <rays>" when every position of the sequence was produced exactly once, inside its XCD's range, and no counter went
// past the number of units plus one overshoot per workgroup.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "pipe_dealing.h"

struct Wg { PipeDeal deal; int r = 0; unsigned next = 0; bool open = true; };

int main(int argc, char** argv) {
    if (argc != 7) return 2;
    const long long total = atoll(argv[1]);
    const int W = atoi(argv[2]), unit = atoi(argv[3]), schedule = atoi(argv[5]);
    const bool dyn = atoi(argv[6]) != 0;
    unsigned long long rng = 0x9E3779B97F4A7C15ull ^ (unsigned long long)atoll(argv[4]);
    auto draw = [&]() { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return unsigned(rng >> 33); };
    const int n_xcd = 8;
    std::vector<int> hits(total, 0);
    long long produced = 0;
    for (int xcd = 0; xcd < n_xcd; xcd++) {
        std::vector<Wg> wgs(W);
        unsigned counter = 0;
        for (int w = 0; w < W; w++) { wgs[w].deal.init(total, n_xcd, xcd, W, w, unit); wgs[w].open = dyn ? wgs[w].deal.has_unit() : wgs[w].deal.static_units() > 0; }
        const int special = int(draw() % unsigned(W));
        for (;;) {
            std::vector<int> open;
            for (int w = 0; w < W; w++) if (wgs[w].open) open.push_back(w);
            if (open.empty()) break;
            int pick = open[draw() % open.size()];
            if (schedule == 1 && wgs[special].open && draw() % 101 != 0) pick = special;
            if (schedule == 2 && pick == special && open.size() > 1) continue;
            Wg& g = wgs[pick];
            const int pos = g.r % unit;
            if (pos == 0 && g.r > 0) {
                const bool more = dyn ? g.deal.advance_to(g.deal.fetched_unit(g.next)) : g.deal.advance_static();
                if (!more) { g.open = false; continue; }
            }
            if (dyn && pos == unit - 1) g.next = counter++;
            const long long s = g.deal.seq(pos);
            if (s >= 0) {
                if (s < g.deal.x0 || s >= g.deal.x1 || s >= total) { printf("FAIL position %lld outside [%lld, %lld)\n", s, (long long)g.deal.x0, (long long)g.deal.x1); return 1; }
                hits[s]++; produced++;
            }
            g.r++;
        }
        if (dyn && counter > unsigned(wgs[0].deal.n_units) + unsigned(W)) { printf("FAIL counter %u of XCD %d past %d units + %d\n", counter, xcd, wgs[0].deal.n_units, W); return 1; }
    }
    for (long long s = 0; s < total; s++) if (hits[s] != 1) { printf("FAIL position %lld produced %d times\n", s, hits[s]); return 1; }
    printf("ok %lld\n", produced);
    return 0;
}
