// What the point-query entry points open with (csrc/render_query.hip, csrc/query_lattice.hip): the cap on the number of points and fill_query.
#pragma once
#include "render_params.h"

// The three point-query kernels index pts[idx * 3 + k] and 16 * t + j in int.  The largest n_points for which neither overflows
// (include/gnerf_hip.h states it); checked before anything else of the call, the pointers included.
constexpr int kMaxQueryPoints = (INT32_MAX - 15) / 3;

// What the three point-query entry points open with: the n_points cap, the planes and decoder as render params (check_common), the
// derived fields the kernels read and the tile counts.  `tiles` may still exceed int: the entries refuse that after their own checks.
static int fill_query(const char* name, const float* planes_nhwc, int n_items, int plane_h, int plane_w, int n_points, float box_warp,
                      const float* w1, const float* b1, const float* w2, const float* b2, int planes_interleaved,
                      Params& P, int& tiles_per_item, int64_t& tiles) {
    if (n_points > kMaxQueryPoints) return gnerf::fail(GNERF_E_ARG, "%s: too many points (n_points %d > %d)", name, n_points, kMaxQueryPoints);
    P = Params{};
    gnerf_render_params& p = P.p;
    p.planes_interleaved = planes_interleaved;
    p.planes_nhwc = planes_nhwc; p.n_items = n_items; p.plane_h = plane_h; p.plane_w = plane_w;
    p.w1 = w1; p.b1 = b1; p.w2 = w2; p.b2 = b2; p.box_warp = box_warp;
    if (int e = check_common(&p)) return e;
    P.box_scale = float(2.0 / double(box_warp));
    fill_pitches(P);
    tiles_per_item = (n_points + 15) / 16;
    tiles = int64_t(n_items) * tiles_per_item;
    return GNERF_OK;
}
