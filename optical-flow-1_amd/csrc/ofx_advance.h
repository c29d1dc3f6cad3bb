// ofx_advance.h -- one step of a point through a step payload, in double: the rule that the sparse tracks of ofx_compose.hip and the
// dense point trajectories of ofx_tracks.hip share (include/ofx.h, "Flows composed along a sequence").  Device code, one copy.
//     inside(x, y)     = 0 <= x <= nx - 1 and 0 <= y <= ny - 1                        (NaN and Inf fail it, before any int cast)
//     sample(S, x, y)  = bicubic_interpolation_at_color(S, x, y, nx, ny, 2, 0 / 1, false): flow_check's sample (ofx_flow.hip), both
//                        channels of a tap in one 8-byte load
//     flagged(M, x, y) = a non-zero byte among the up to four map pixels around an inside position; false without a map
//     advance(p, S, M) = flagged(M, p) -> lost;  q = p + sample(S, p);  !inside(q) -> lost;  else the point moves to q
#pragma once

#include "ofx_device.h"

OFX_DEV bool cp_inside(double x, double y, int nx, int ny)
{
    return x >= 0.0 && x <= (double) (nx - 1) && y >= 0.0 && y <= (double) (ny - 1);
}

// (x, y) inside: x0 <= nx - 1, and x > x0 only where x0 <= nx - 2 -- no index leaves the map
OFX_DEV bool cp_flagged(const unsigned char *__restrict__ M, double x, double y, int nx)
{
    if (!M) return false;
    const int x0 = (int) x, y0 = (int) y;
    const int x1 = x0 + (x > (double) x0 ? 1 : 0), y1 = y0 + (y > (double) y0 ? 1 : 0);
    const size_t r0 = (size_t) y0 * nx, r1 = (size_t) y1 * nx;
    return (M[r0 + x0] | M[r0 + x1] | M[r1 + x0] | M[r1 + x1]) != 0;
}

OFX_DEV double2 cp_sample(const float2 *__restrict__ S, double x, double y, int nx, int ny)
{
    const BicubicTaps t = bicubic_taps(x, y, nx, ny);
    double c1[4], c2[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double2 v0 = ldw2(S + (size_t) t.row[0] * nx + t.col[k]);
        const double2 v1 = ldw2(S + (size_t) t.row[1] * nx + t.col[k]);
        const double2 v2 = ldw2(S + (size_t) t.row[2] * nx + t.col[k]);
        const double2 v3 = ldw2(S + (size_t) t.row[3] * nx + t.col[k]);
        c1[k] = cubic_cell(v0.x, v1.x, v2.x, v3.x, t.fy);
        c2[k] = cubic_cell(v0.y, v1.y, v2.y, v3.y, t.fy);
    }
    return make_double2(cubic_cell(c1[0], c1[1], c1[2], c1[3], t.fx), cubic_cell(c2[0], c2[1], c2[2], c2[3], t.fx));
}

// the point at the inside position (x, y): false = lost, (x, y) unchanged; true = moved
OFX_DEV bool cp_advance(const float2 *__restrict__ S, const unsigned char *__restrict__ M, double &x, double &y, int nx, int ny)
{
    if (cp_flagged(M, x, y, nx)) return false;
    const double2 b = cp_sample(S, x, y, nx, ny);
    const double qx = x + b.x, qy = y + b.y;
    if (!cp_inside(qx, qy, nx, ny)) return false;
    x = qx;
    y = qy;
    return true;
}
