// chunk_sums.hpp -- the fixed-order fp64 sums that f5 and f11 (both in icp.hip) and
// f13 (rgbd_odometry.hip) share (device only):
// per 256-item chunk by xor shuffles and an LDS stage, then over the chunks in
// order by one wave.  No float atomics: two calls are bitwise equal.
#pragma once
#include "pdsc_common.hpp"

namespace pdsc {

// The fixed-order sum of a chunk's NS per-point values v (thread t of 256, all
// of them calling together: it holds workgroup barriers): xor shuffles inside
// each wave, the four waves' rows through red ([4][NS] of LDS) in wave order,
// to part[NS chunk ..] (chunk < nchunks).
template <int NS>
PDSC_DEV void icp_reduce_chunk(const double (&v)[NS], int t, int chunk, int nchunks, double *red, double *part) {
    const int w = t >> 6;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const double s = wave_sum(v[j]);
        if ((t & 63) == 0) red[w * NS + j] = s;
    }
    __syncthreads();
    if (t < NS && chunk < nchunks)
        part[(size_t)chunk * NS + t] = ((red[t] + red[NS + t]) + red[2 * NS + t]) + red[3 * NS + t];
    __syncthreads();  // red is free for the next chunk
}

// f11's sums of G^T G over the correspondences' points t: the count, sum t, the
// six entries of sum t t^T; and the 36 entries they make (+0 without a point).
constexpr int INFO_NSUM = 10;  // count, x, y, z, xx, xy, xz, yy, yz, zz
PDSC_DEV void info_from_sums(const double (&S)[INFO_NSUM], double *info) {
    const double n = S[0], x = S[1], y = S[2], z = S[3], xx = S[4], xy = S[5], xz = S[6], yy = S[7], yz = S[8],
                 zz = S[9];
    const double M[36] = {yy + zz, -xy, -xz, 0.0, -z,  y,    //
                          -xy, xx + zz, -yz, z,   0.0, -x,   //
                          -xz, -yz, xx + yy, -y,  x,   0.0,  //
                          0.0, z,   -y,  n,   0.0, 0.0,      //
                          -z,  0.0, x,   0.0, n,   0.0,      //
                          y,   -x,  0.0, 0.0, 0.0, n};
    for (int i = 0; i < 36; ++i) info[i] = n > 0.0 ? M[i] : 0.0;  // no correspondence: +0 everywhere
}

}  // namespace pdsc
