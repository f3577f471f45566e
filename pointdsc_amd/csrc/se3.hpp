// se3.hpp -- rigid transforms as their 3x4 part, row-major [12], in fp64 (device
// only).  Every product is in the order ((a0 b0 + a1 b1) + a2 b2) (+ a3), which
// the tests' restatements repeat.  Shared by f12 (posegraph.hip), f13
// (rgbd_odometry.hip) and f14 (tsdf.hip).
#pragma once
#include "pdsc_common.hpp"

namespace pdsc {

PDSC_DEV void aff_load(const double *T, double (&A)[12]) {
#pragma unroll
    for (int i = 0; i < 12; ++i) A[i] = T[i];
}
PDSC_DEV void aff_inv(const double (&T)[12], double (&I)[12]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) I[4 * r + c] = T[4 * c + r];
        I[4 * r + 3] = -((I[4 * r] * T[3] + I[4 * r + 1] * T[7]) + I[4 * r + 2] * T[11]);
    }
}
PDSC_DEV void aff_mul(const double (&A)[12], const double (&B)[12], double (&C)[12]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double s = (A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c];
            C[4 * r + c] = c == 3 ? s + A[4 * r + 3] : s;
        }
    }
}
// A x for a point: ((a0 x + a1 y) + a2 z) + a3 per row
PDSC_DEV void aff_apply(const double (&A)[12], double x, double y, double z, double &ox, double &oy, double &oz) {
    ox = ((A[0] * x + A[1] * y) + A[2] * z) + A[3];
    oy = ((A[4] * x + A[5] * y) + A[6] * z) + A[7];
    oz = ((A[8] * x + A[9] * y) + A[10] * z) + A[11];
}
// open3d's TransformVector6dToMatrix4d: Exp(d) = Rz(d2) Ry(d1) Rx(d0) with translation d3..5
PDSC_DEV void se3_exp(const double *d, double (&Ex)[12]) {
    const double cx = cos(d[0]), sx = sin(d[0]), cy = cos(d[1]), sy = sin(d[1]), cz = cos(d[2]), sz = sin(d[2]);
    Ex[0] = cz * cy;
    Ex[1] = cz * sy * sx - sz * cx;
    Ex[2] = cz * sy * cx + sz * sx;
    Ex[3] = d[3];
    Ex[4] = sz * cy;
    Ex[5] = sz * sy * sx + cz * cx;
    Ex[6] = sz * sy * cx - cz * sx;
    Ex[7] = d[4];
    Ex[8] = -sy;
    Ex[9] = cy * sx;
    Ex[10] = cy * cx;
    Ex[11] = d[5];
}

}  // namespace pdsc
