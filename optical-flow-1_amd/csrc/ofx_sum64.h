// ofx_sum64.h -- the fixed-order double sum of a wave (include/ofx.h, "sum64"), shared by ofx_tracks.hip and ofx_motion.hip:
//     p[l] = v[l] + v[l + 64] + v[l + 128] + ...   left to right, l = 0 .. 63; a lane without an element holds +0.0
//     for s = 32, 16, 8, 4, 2, 1:  p[l] = p[l] + p[l + s] for l < s;  the value is p[0]
// A wave is the 64 lanes: the order is fixed, so is the result.  Lanes at and above s add what no lower lane reads again.
#pragma once

#include "ofx_device.h"

// the second half: the 64 lane values p -> the sum, valid in lane 0
OFX_DEV double tk_sum64_lanes(double p)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) p = p + __shfl_down(p, s, 64);
    return p;
}
OFX_DEV double tk_sum64(const double *__restrict__ v, int n)
{
    const int l = (int) threadIdx.x & 63;
    double p = 0.0;
    if (l < n) {
        p = v[l];
        for (int j = l + 64; j < n; j += 64) p = p + v[j];
    }
    return tk_sum64_lanes(p);
}
