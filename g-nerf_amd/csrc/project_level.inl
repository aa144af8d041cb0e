// Newton projection of points onto the level set sigma = level (gnerf_project_points_to_level; include/gnerf_hip.h states the rules per
// point).  Included by render_query.hip alone (it holds a kernel).  It calls the tile stages of query_grad.inl -- grad_tap_records, grad_lookup,
// bwd_mlp_forward, grad_dx_from_dh (the sigma-only decoder backward on the exact fp32 MFMA), grad_point_gradient -- inside a wave-uniform loop
// over the steps, and owns what is not a stage: the affine, the seed dL/dsigma = 1, the Newton state, the ballots and every lds_wave_sync:
//   every lane keeps the state of point j = lane & 15 of its tile in registers (start, position, status, residuals; the four lanes of a point
//   hold the same values, computed from the same operands), so the record lanes (lane < 48) read their point's position without a hand-off;
//   sigma comes out of bwd_mlp_forward in every lane of its point; the gradient comes out of the derivative lookup in the 8-lane group of point
//   8 a + b and crosses to the state lanes through 64 floats of the tile's stage rows (free between the decoder forward and the next lookup);
//   a ballot over "some point of my tile still iterates" ends the loop, once after the residual test (the last step never pays for a
//   gradient) and once after the move, so every lds_wave_sync is reached by the whole wave.  A point that has stopped keeps its state: it
//   rides along with frozen operands.  The pad points of a partial last tile repeat the last point (they stop when it does) and are never stored.
// Plain stores, no atomics: the same bits on every run, in every tile and batch position.
#pragma once
#include "query_grad.inl"

namespace {

struct ProjectArgs {
    const float* points;
    float *points_out, *residual_in, *residual_out;
    unsigned char* status;
    float a[12];                // world = A p + b, row-major [A | b]
    int has_affine;
    float level, radius, tol;
    int max_steps;
    int n_points, tiles_per_item, n_tiles;
};

constexpr int kProjectActive = 255;     // status of a point that still iterates (never stored)

__global__ __launch_bounds__(kBwdThreads, 3) void project_level_kernel(Params P, ProjectArgs Q) {
    extern __shared__ __align__(16) float smem[];
    const gnerf_render_params& p = P.p;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    BwdLds L = {};
    bwd_stage_decoder_f32<kBwdThreads>(L, smem, p, tid);
    L.stage = smem + kBwdWeightFloats + size_t(wv) * query_grad_wave_floats();
    L.tbuf = L.stage + 16 * kStagePitch;
    float* recs = L.tbuf + 16 * kTPitch;
    const int j = lane & 15, g = lane >> 4, b = lane >> 3, cq = lane & 7;
    const int64_t plane_floats = int64_t(3) * p.plane_h * p.plane_w * 32;
    const float* A = Q.a;
    for (int tile = blockIdx.x * kBwdWaves + wv; tile < Q.n_tiles; tile += gridDim.x * kBwdWaves) {
        const int item = tile / Q.tiles_per_item, t = tile % Q.tiles_per_item;
        const char* planes = reinterpret_cast<const char*>(p.planes_nhwc + int64_t(item) * plane_floats);
        const float* pts = Q.points + int64_t(item) * Q.n_points * 3;
        const int64_t pt0 = int64_t(item) * Q.n_points + 16 * t;
        const int64_t idx = min(16 * t + j, Q.n_points - 1);
        const float sx = pts[idx * 3 + 0], sy = pts[idx * 3 + 1], sz = pts[idx * 3 + 2];        // the start
        float px = sx, py = sy, pz = sz;
        float e = 0.f, e_in = 0.f;
        int st = kProjectActive;
        for (int k = 0;; k++) {
            float wx = px, wy = py, wz = pz;
            if (Q.has_affine) {
                wx = ((A[0] * px + A[1] * py) + A[2] * pz) + A[3];
                wy = ((A[4] * px + A[5] * py) + A[6] * pz) + A[7];
                wz = ((A[8] * px + A[9] * py) + A[10] * pz) + A[11];
            }
            const bool finite_pos = isfinite(wx) && isfinite(wy) && isfinite(wz);
            // ---- 1. tap records
            grad_tap_records(P, recs, lane, wx * P.box_scale, wy * P.box_scale, wz * P.box_scale);
            lds_wave_sync();
            // ---- 2. lookup and decoder forward
            grad_lookup(L, recs, planes, b, cq);
            lds_wave_sync();
            v4f h[4], o[2];
            float sig;
            bwd_mlp_forward(L, lane, h, o, sig);          // (the colour rows o are not used: the compiler drops their products)
            // ---- the residual test
            if (st == kProjectActive) {
                e = finite_pos ? sig - Q.level : __builtin_nanf("");       // a point with a non-finite coordinate has no density
                if (k == 0) e_in = e;
                if (!isfinite(e)) st = 2;
                else if (fabsf(e) <= Q.tol) st = 0;
                else if (k >= Q.max_steps) st = 1;
            }
            if (!__any(st == kProjectActive)) break;       // wave-uniform; always taken at k == max_steps
            // ---- 3. decoder backward with dL/dsigma = 1
            v4f dh[4];
#pragma unroll
            for (int m = 0; m < 4; m++) dh[m] = *reinterpret_cast<const v4f*>(L.w2 + 16 * m + 4 * g);
            v4f dx[2];
            grad_dx_from_dh(L, h, dh, j, g, dx);
            *reinterpret_cast<v4f*>(L.tbuf + j * kTPitch + 4 * g) = dx[0];           // dX[point][channel]
            *reinterpret_cast<v4f*>(L.tbuf + j * kTPitch + 16 + 4 * g) = dx[1];
            lds_wave_sync();
            // ---- 4. the same texels against the derivative weights; the gradient crosses to the state lanes through the stage rows
#pragma unroll
            for (int a = 0; a < 2; a++) {
                const int js = 8 * a + b;
                float gx, gy, gz;
                grad_point_gradient(L, recs, planes, js, cq, gx, gy, gz);
                if (cq < 3) L.stage[js * 4 + cq] = (cq == 0 ? gx : (cq == 1 ? gy : gz)) * P.box_scale;
            }
            lds_wave_sync();                               // also: the records and dX are the next step's to overwrite
            // ---- the move
            const float gwx = L.stage[j * 4 + 0], gwy = L.stage[j * 4 + 1], gwz = L.stage[j * 4 + 2];
            if (st == kProjectActive) {
                float gx = gwx, gy = gwy, gz = gwz;
                if (Q.has_affine) {                        // a covector: A^T g_world
                    gx = (A[0] * gwx + A[4] * gwy) + A[8] * gwz;
                    gy = (A[1] * gwx + A[5] * gwy) + A[9] * gwz;
                    gz = (A[2] * gwx + A[6] * gwy) + A[10] * gwz;
                }
                const float gg = (gx * gx + gy * gy) + gz * gz;
                if (!(gg > 0.f) || !isfinite(gg)) {
                    st = 2;
                } else {
                    const float s = e / gg;
                    px = fminf(fmaxf(px - s * gx, sx - Q.radius), sx + Q.radius);      // fmaxf drops a NaN operand: the box's lower face
                    py = fminf(fmaxf(py - s * gy, sy - Q.radius), sy + Q.radius);
                    pz = fminf(fmaxf(pz - s * gz, sz - Q.radius), sz + Q.radius);
                }
            }
            if (!__any(st == kProjectActive)) break;
        }
        lds_wave_sync();                                   // the stage rows and the records are the next tile's to overwrite
        if (g == 0 && 16 * t + j < Q.n_points) {
            const bool done = st == 0;
            float* out = Q.points_out + (pt0 + j) * 3;
            out[0] = done ? px : sx;
            out[1] = done ? py : sy;
            out[2] = done ? pz : sz;
            Q.residual_in[pt0 + j] = e_in;
            Q.residual_out[pt0 + j] = done ? e : e_in;
            Q.status[pt0 + j] = (unsigned char)st;
        }
    }
}

}  // namespace
