// The derivative side of a plane lookup: the taps with their derivative weights (plane_taps_grad: the point queries' tile stages in
// query_grad.inl, and the ray gradient, render_ray_grad.inl) and one plane's share of dL/dposition (plane_position_grad: the zero-padding
// rule lives in the former, the plane routing in the latter; the tile stages call it, the ray kernel holds a timed copy).  No kernel is defined here.
#pragma once
#include "render_core.inl"

namespace {

// plane_taps (render_shade.inl) with the derivative of the blend: a tap outside the image is a zero texel, so with the taps
// (t00 t10 / t01 t11) and fractions (fx, fy)   df/dix = (t10 - t00)(1 - fy) + (t11 - t01) fy,   df/diy = (t01 - t00)(1 - fx) + (t11 - t10) fx
// and dix/du = W / 2, diy/dv = H / 2 (u, v in [-1, 1], align_corners=False).  floor's derivative is the one-sided one, as grid_sample's.
__device__ __forceinline__ void plane_taps_grad(int H, int W, float u, float v, unsigned tex_pitch, unsigned row_pitch, unsigned plane_bytes_off,
                                                uint4& off, v4f& wgt, v4f& du, v4f& dv) {
    float ix = ((u + 1.f) * float(W) - 1.f) * 0.5f;
    float iy = ((v + 1.f) * float(H) - 1.f) * 0.5f;
    ix = clamp_nn(ix, -1.5f, float(W) + 0.5f);           // beyond the clamp every tap is outside: weights and derivatives are all zero
    iy = clamp_nn(iy, -1.5f, float(H) + 0.5f);
    const float x0f = floorf(ix), y0f = floorf(iy);
    const float fx = ix - x0f, fy = iy - y0f;
    const int x0 = int(x0f), y0 = int(y0f), x1 = x0 + 1, y1 = y0 + 1;
    auto inside = [](int i, int n) { return unsigned(i) < unsigned(n); };
    auto clamp0 = [](int i, int last) { return min(max(i, 0), last); };
    const bool in_x0 = inside(x0, W), in_x1 = inside(x1, W), in_y0 = inside(y0, H), in_y1 = inside(y1, H);
    const float wx0 = in_x0 ? 1.f - fx : 0.f, wx1 = in_x1 ? fx : 0.f;
    const float wy0 = in_y0 ? (1.f - fy) * (1.f / 3.f) : 0.f, wy1 = in_y1 ? fy * (1.f / 3.f) : 0.f;
    const float sx = 0.5f * float(W), sy = 0.5f * float(H) * (1.f / 3.f);
    const float dx0 = in_x0 ? -sx : 0.f, dx1 = in_x1 ? sx : 0.f;
    const float dy0 = in_y0 ? -sy : 0.f, dy1 = in_y1 ? sy : 0.f;
    const unsigned cx0 = __umul24(unsigned(clamp0(x0, W - 1)), tex_pitch), cx1 = __umul24(unsigned(clamp0(x1, W - 1)), tex_pitch);
    const unsigned cy0 = __umul24(unsigned(clamp0(y0, H - 1)), row_pitch) + plane_bytes_off;
    const unsigned cy1 = __umul24(unsigned(clamp0(y1, H - 1)), row_pitch) + plane_bytes_off;
    off = make_uint4(cy0 + cx0, cy0 + cx1, cy1 + cx0, cy1 + cx1);
    wgt = (v4f){wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1};
    du = (v4f){dx0 * wy0, dx1 * wy0, dx0 * wy1, dx1 * wy1};
    dv = (v4f){wx0 * dy0, wx1 * dy0, wx0 * dy1, wx1 * dy1};
}

// One plane's share of dL/dposition over this lane's four channels (cq16 = the lane's byte offset inside a texel, dxv = its four channels
// of dL/d(mean feature)): the four texels against the derivative weights, summed pairwise, and routed by what plane pl reads --
// (x,y), (x,z), (z,x).  The callers sum the result over the 8 lanes of a texel.
__device__ __forceinline__ void plane_position_grad(const char* planes, int pl, const uint4& off, const v4f& du, const v4f& dv, const v4f& dxv, int cq16,
                                                    float& gx, float& gy, float& gz) {
    const v4f t00 = *reinterpret_cast<const v4f*>(planes + off.x + cq16);
    const v4f t10 = *reinterpret_cast<const v4f*>(planes + off.y + cq16);
    const v4f t01 = *reinterpret_cast<const v4f*>(planes + off.z + cq16);
    const v4f t11 = *reinterpret_cast<const v4f*>(planes + off.w + cq16);
    const v4f fu = (t00 * du[0] + t10 * du[1] + t01 * du[2] + t11 * du[3]) * dxv;
    const v4f fv = (t00 * dv[0] + t10 * dv[1] + t01 * dv[2] + t11 * dv[3]) * dxv;
    const float su = (fu[0] + fu[1]) + (fu[2] + fu[3]), sv = (fv[0] + fv[1]) + (fv[2] + fv[3]);
    if (pl == 0) { gx += su; gy += sv; }
    else if (pl == 1) { gx += su; gz += sv; }
    else { gz += su; gx += sv; }
}

}  // namespace
