// How the pipelined render kernel hands the locality-ordered ray sequence to its workgroups (render_pipe.inl).  Plain C++ on
// purpose: the kernel's scalar wave runs it, and tests/test_render_dealing_cpu.py / test_render_guided_dealing_cpu.py compile it
// for the host and play arbitrary interleavings of workgroups against it.
//
// Workgroups b, b+8, ... share an XCD (round-robin dispatch), and each XCD owns a contiguous eighth [x0, x1) of the sequence,
// cut into UNITS of consecutive rays.  Inside an XCD the units are taken in order by its W workgroups, so at any moment
// those are within a few units of each other, i.e. on neighbouring rays, and the XCD's 4 MB L2 holds the texels they share.
//   static     workgroup wg renders units wg, wg + W, wg + 2 W, ...: equal ray counts, and the launch lasts as long as its slowest
//              workgroup (profiles/r08_wg_lifetimes.json: 16 % of the workgroup slot-time of config 2 idle behind it).
//   on demand  workgroup wg starts on unit wg and takes every further one from the XCD's counter: unit W + (value fetched).  A
//              fetched unit >= n_units means the XCD's range is dealt out and the workgroup drains its pipeline and ends.  The
//              fetch-add is the only operation between workgroups; nobody waits for anybody.
// The UNIFORM schedule cuts the range into units of `unit` rays (the last one may be short: seq() answers -1 past x1).  The GUIDED
// schedule (on demand only, unit = 8, ranges of at least W full units) shrinks the units as the range runs out, so that the
// workgroups of an XCD end within about one ray of each other instead of one 8-ray unit: counted from the END of the range, the last
// c W units hold 1 ray, the c W before them 2, the c W before those 4, everything in front `unit` (guided_c = c; guided_min = 2 leaves
// the 1-ray level out).  A range too short for all of that fills the levels from the smallest up, and what is left over of a
// whole number of 8-ray units (0..7 rays) goes out as at most one extra unit of 4, 2 and 1 rays at the end of those levels: every
// guided unit is full, lengths never increase along the index, and the first W units (the workgroups' own) are `unit` rays long.
// unit_start / unit_len are O(1) in the unit index: three level boundaries k2 <= k4 <= k8 (pure functions of x1 - x0, W and unit).
// Speed only -- every assignment renders each ray once, with the same arithmetic.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GNERF_DEAL_HD __host__ __device__ __forceinline__
#else
#define GNERF_DEAL_HD inline
#endif

struct PipeDeal {
    int64_t x0, x1;         // this XCD's range of the sequence
    int unit, n_units, W, wg;
    int k2, k4, k8;         // first unit index of the levels unit/2, unit/4, unit/8 (kNoLevel: the uniform schedule)
    static constexpr int kNoLevel = 0x7fffffff;
    int u;                  // the unit this workgroup is on (index inside the XCD's range)
    int taken;              // units it has started so far (uniform schedule: its local ray index r lies in unit number r / unit)
    int64_t start;          // unit_start(u)
    int len;                // unit_len(u)

    GNERF_DEAL_HD void init(int64_t total_seq, int n_xcd, int xcd, int workgroups_per_xcd, int wg_in_xcd, int unit_rays, int guided_c = 0, int guided_min = 1) {
        x0 = total_seq * xcd / n_xcd; x1 = total_seq * (xcd + 1) / n_xcd;
        unit = unit_rays; W = workgroups_per_xcd; wg = wg_in_xcd;
        const int64_t L = x1 - x0;
        n_units = int((L + unit - 1) / unit);
        k2 = k4 = k8 = kNoLevel;
        if (guided_c > 0 && unit == 8 && L >= int64_t(8) * W) {
            int64_t R = L - int64_t(8) * W;                     // what the workgroups' own first units leave
            const int64_t cap = int64_t(guided_c) * W;
            int64_t n1 = guided_min <= 1 ? (R < cap ? R : cap) : 0; R -= n1;
            int64_t n2 = R / 2 < cap ? R / 2 : cap; R -= 2 * n2;
            int64_t n4 = R / 4 < cap ? R / 4 : cap; R -= 4 * n4;
            const int64_t n8 = W + R / 8;
            const int rem = int(R % 8);
            n4 += (rem >> 2) & 1; n2 += (rem >> 1) & 1; n1 += rem & 1;
            k2 = int(n8); k4 = int(n8 + n4); k8 = int(n8 + n4 + n2); n_units = int(n8 + n4 + n2 + n1);
        }
        taken = 0; set_unit(wg);
    }
    // first position (relative to x0) and nominal length of unit k, 0 <= k <= n_units
    GNERF_DEAL_HD int64_t unit_start(int k) const {
        const int h = unit >> 1, q = unit >> 2, e = unit >> 3;
        return int64_t(k) * unit - int64_t(k > k2 ? k - k2 : 0) * (unit - h) - int64_t(k > k4 ? k - k4 : 0) * (h - q) - int64_t(k > k8 ? k - k8 : 0) * (q - e);
    }
    GNERF_DEAL_HD int unit_len(int k) const { return unit >> (int(k >= k2) + int(k >= k4) + int(k >= k8)); }
    GNERF_DEAL_HD void set_unit(int k) { u = k; start = unit_start(k); len = unit_len(k); }
    // static dealing: how many units this workgroup renders in all
    GNERF_DEAL_HD int static_units() const { return n_units > wg ? (n_units - wg + W - 1) / W : 0; }
    // the unit a workgroup on demand moves to, from what its fetch-add on the XCD's counter returned (counters start at zero)
    GNERF_DEAL_HD int fetched_unit(unsigned counter_value) const { return counter_value < unsigned(n_units) ? W + int(counter_value) : n_units; }
    // move to the next unit (static: the round-robin successor; on demand: `next` = fetched_unit(...)); false = no unit left
    GNERF_DEAL_HD bool advance_static() { taken++; set_unit(wg + taken * W); return u < n_units; }
    GNERF_DEAL_HD bool advance_to(int next) { taken++; set_unit(next); return u < n_units; }
    GNERF_DEAL_HD bool has_unit() const { return u < n_units; }
    // position i (0 <= i < len) of the current unit -> position of the sequence, or -1 (past the XCD's range: the uniform schedule's
    // short last unit)
    GNERF_DEAL_HD int64_t seq(int i) const {
        const int64_t s = x0 + start + i;
        return (u < n_units && s < x1) ? s : -1;
    }
};
