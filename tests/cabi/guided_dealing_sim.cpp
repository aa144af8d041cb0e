// Host-side play of the pipelined render kernel's GUIDED ray dealing (g-nerf_amd/csrc/pipe_dealing.h), for
// tests/test_render_guided_dealing_cpu.py:
//   guided_dealing_sim one   <total_seq> <n_xcd> <W> <unit> <c> <smallest> <schedule> <seed>
//   guided_dealing_sim sweep <max range length> <W> <unit> <c> <smallest> <schedule> <seed>      (every range length 0 .. max, one XCD)
// First the schedule of every XCD's range is checked on its own: unit_start(0) = 0, unit_start(k + 1) = unit_start(k) + unit_len(k),
// lengths never increase along the index, the units cover the range, seq() answers -1 exactly for positions at or past x1, and
//   eligible (c > 0, unit = 8, range >= 8 W)  every unit is full, the first W units have 8 rays, every later length is 4, 2 or 1 (not 1
//                                             before the last unit when smallest = 2), no shrinking level has more than c W + 1 units
//   otherwise                                 unit k starts at k * unit and has `unit` rays: the uniform schedule.
// Then every workgroup walks its local rays exactly as the scalar wave's propose_issue does (a running position inside the unit;
// on reaching the unit's length, advance with what the fetch-add returned; fetch while the unit's last ray is proposed), in the
// order a scheduler picks: 0 uniformly at random, 1 one workgroup takes everything it can, 2 strict round robin, 3 one workgroup
// stalls on its first unit until no other can move.  Prints "ok <rays>" when every position was produced exactly once.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "pipe_dealing.h"

struct Wg { PipeDeal deal; int upos = 0; unsigned next = 0; bool open = true; };

static unsigned long long rng_state;
static unsigned draw() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return unsigned(rng_state >> 33); }

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL " __VA_ARGS__); printf("  [total %lld xcd %d/%d W %d unit %d c %d smallest %d]\n", total, xcd, n_xcd, W, unit, c, smallest); return false; } } while (0)

static bool check_schedule(long long total, int n_xcd, int xcd, int W, int unit, int c, int smallest) {
    PipeDeal d;
    d.init(total, n_xcd, xcd, W, 0, unit, c, smallest);
    const long long L = d.x1 - d.x0;
    const bool eligible = c > 0 && unit == 8 && L >= 8ll * W;
    CHECK(d.unit_start(0) == 0, "unit_start(0) = %lld\n", (long long)d.unit_start(0));
    int per_level[9] = {};
    for (int k = 0; k < d.n_units; k++) {
        const long long s = d.unit_start(k);
        const int len = d.unit_len(k);
        CHECK(len >= 1 && len <= unit, "unit %d has %d rays\n", k, len);
        CHECK(d.unit_start(k + 1) == s + len, "unit_start(%d) = %lld, not %lld + %d\n", k + 1, (long long)d.unit_start(k + 1), s, len);
        if (k > 0) CHECK(len <= d.unit_len(k - 1), "unit %d is longer (%d) than unit %d (%d)\n", k, len, k - 1, d.unit_len(k - 1));
        CHECK(s < L, "unit %d starts at %lld, past the range of %lld\n", k, s, L);
        PipeDeal w = d;
        w.set_unit(k);
        for (int i = 0; i < len; i++) {
            const long long q = w.seq(i), want = d.x0 + s + i;
            CHECK(q == (want < d.x1 ? want : -1), "seq(%d) of unit %d is %lld (position %lld, x1 %lld)\n", i, k, q, want, (long long)d.x1);
        }
        if (eligible) {
            CHECK(s + len <= L, "guided unit %d is short\n", k);
            CHECK(k >= W || len == 8, "guided: own unit %d has %d rays\n", k, len);
            CHECK(len == 8 || len == 4 || len == 2 || len == 1, "guided unit %d has %d rays\n", k, len);
            CHECK(smallest <= 1 || len >= 2 || k == d.n_units - 1, "a one-ray unit %d before the last with smallest = 2\n", k);
            per_level[len]++;
        } else {
            CHECK(s == (long long)k * unit && len == unit, "uniform unit %d: start %lld length %d\n", k, s, len);
        }
    }
    CHECK(d.unit_start(d.n_units) >= L, "the units end at %lld, the range at %lld\n", (long long)d.unit_start(d.n_units), L);
    if (eligible) {
        CHECK(d.unit_start(d.n_units) == L, "guided units end at %lld, the range at %lld\n", (long long)d.unit_start(d.n_units), L);
        for (int len = 1; len <= 4; len *= 2) CHECK(per_level[len] <= c * W + 1, "%d units of %d rays\n", per_level[len], len);
    } else {
        CHECK(d.n_units == int((L + unit - 1) / unit), "uniform: %d units\n", d.n_units);
    }
    return true;
}

static bool play(long long total, int n_xcd, int W, int unit, int c, int smallest, int schedule) {
    std::vector<int> hits(total, 0);
    long long produced = 0;
    for (int xcd = 0; xcd < n_xcd; xcd++) {
        if (!check_schedule(total, n_xcd, xcd, W, unit, c, smallest)) return false;
        std::vector<Wg> wgs(W);
        unsigned counter = 0;
        for (int w = 0; w < W; w++) { wgs[w].deal.init(total, n_xcd, xcd, W, w, unit, c, smallest); wgs[w].open = wgs[w].deal.has_unit(); }
        const int special = int(draw() % unsigned(W));
        int turn = 0;
        for (;;) {
            std::vector<int> open;
            for (int w = 0; w < W; w++) if (wgs[w].open) open.push_back(w);
            if (open.empty()) break;
            int pick = open[draw() % open.size()];
            if (schedule == 1 && wgs[special].open) pick = special;
            if (schedule == 2) pick = open[turn++ % open.size()];
            if (schedule == 3 && pick == special && open.size() > 1) continue;
            Wg& g = wgs[pick];
            if (g.upos == g.deal.len) {
                g.upos = 0;
                if (!g.deal.advance_to(g.deal.fetched_unit(g.next))) { g.open = false; continue; }
            }
            const int pos = g.upos++;
            if (pos == g.deal.len - 1) g.next = counter++;
            const long long s = g.deal.seq(pos);
            if (s >= 0) {
                CHECK(s >= g.deal.x0 && s < g.deal.x1 && s < total, "position %lld outside [%lld, %lld)\n", s, (long long)g.deal.x0, (long long)g.deal.x1);
                hits[s]++; produced++;
            }
        }
        CHECK(counter <= unsigned(wgs[0].deal.n_units) + unsigned(W), "counter %u past %d units + %d\n", counter, wgs[0].deal.n_units, W);
    }
    const int xcd = -1;
    for (long long s = 0; s < total; s++) CHECK(hits[s] == 1, "position %lld produced %d times\n", s, hits[s]);
    CHECK(produced == total, "%lld rays of %lld\n", produced, total);
    return true;
}

int main(int argc, char** argv) {
    if (argc != 10 && !(argc == 9 && !strcmp(argv[1], "sweep"))) return 2;
    const bool sweep = !strcmp(argv[1], "sweep");
    int a = 2;
    const long long total = atoll(argv[a++]);
    const int n_xcd = sweep ? 1 : atoi(argv[a++]);
    const int W = atoi(argv[a++]), unit = atoi(argv[a++]), c = atoi(argv[a++]), smallest = atoi(argv[a++]), schedule = atoi(argv[a++]);
    rng_state = 0x9E3779B97F4A7C15ull ^ (unsigned long long)atoll(argv[a++]);
    long long rays = 0;
    for (long long t = sweep ? 0 : total; t <= total; t++) {
        if (!play(t, n_xcd, W, unit, c, smallest, schedule)) return 1;
        rays += t;
    }
    printf("ok %lld\n", rays);
    return 0;
}
