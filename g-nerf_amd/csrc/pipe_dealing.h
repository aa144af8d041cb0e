// How the pipelined render kernel hands the locality-ordered ray sequence to its workgroups (render_pipe.inl).  Plain C++ on
// purpose: the kernel's scalar wave runs it, and tests/test_render_dealing_cpu.py compiles it for the host and plays arbitrary
// interleavings of workgroups against it.
//
// Workgroups b, b+8, ... share an XCD (round-robin dispatch), and each XCD owns a contiguous eighth [x0, x1) of the sequence,
// cut into UNITS of `unit` consecutive rays.  Inside an XCD the units are taken in order by its W workgroups, so at any moment
// those are within a few units of each other, i.e. on neighbouring rays, and the XCD's 4 MB L2 holds the texels they share.
//   static     workgroup wg renders units wg, wg + W, wg + 2 W, ...: equal ray counts, and the launch lasts as long as its slowest
//              workgroup (profiles/r08_wg_lifetimes.json: 16 % of the workgroup slot-time of config 2 idle behind it).
//   on demand  workgroup wg starts on unit wg and takes every further one from the XCD's counter: unit W + (value fetched).  A
//              fetched unit >= n_units means the XCD's range is dealt out and the workgroup drains its pipeline and ends.  The
//              fetch-add is the only operation between workgroups; nobody waits for anybody.
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
    int u;                  // the unit this workgroup is on (index inside the XCD's range)
    int taken;              // units it has started so far: its local ray index r lies in unit number r / unit

    GNERF_DEAL_HD void init(int64_t total_seq, int n_xcd, int xcd, int workgroups_per_xcd, int wg_in_xcd, int unit_rays) {
        x0 = total_seq * xcd / n_xcd; x1 = total_seq * (xcd + 1) / n_xcd;
        unit = unit_rays; W = workgroups_per_xcd; wg = wg_in_xcd;
        n_units = int((x1 - x0 + unit - 1) / unit);
        u = wg; taken = 0;
    }
    // static dealing: how many units this workgroup renders in all
    GNERF_DEAL_HD int static_units() const { return n_units > wg ? (n_units - wg + W - 1) / W : 0; }
    // the unit a workgroup on demand moves to, from what its fetch-add on the XCD's counter returned (counters start at zero)
    GNERF_DEAL_HD int fetched_unit(unsigned counter_value) const { return counter_value < unsigned(n_units) ? W + int(counter_value) : n_units; }
    // move to the next unit (static: the round-robin successor; on demand: `next` = fetched_unit(...)); false = no unit left
    GNERF_DEAL_HD bool advance_static() { taken++; u = wg + taken * W; return u < n_units; }
    GNERF_DEAL_HD bool advance_to(int next) { taken++; u = next; return u < n_units; }
    GNERF_DEAL_HD bool has_unit() const { return u < n_units; }
    // position i (0 <= i < unit) of the current unit -> position of the sequence, or -1 (past the XCD's range: a short last unit)
    GNERF_DEAL_HD int64_t seq(int i) const {
        const int64_t s = x0 + int64_t(u) * unit + i;
        return (u < n_units && s < x1) ? s : -1;
    }
};
