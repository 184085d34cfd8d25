// pg_pose_align.h -- the 3 x 3 part of a Procrustes alignment: the orthogonal factor T = V U^T of the singular value
// decomposition A = U diag(s) V^T of a cross-covariance, with the two reflection rules of the reference
// (core/utils/evaluation_helpers.py:437-449 reflection='best'; run_gan.py:1408-1414 det(R) = +1), and the sum of the singular values
// that goes with T.  Plain C++ in double, no HIP calls: pg_posescore.hip runs it uniformly in every lane of a wave, the host tests
// and tools/sanitize/pose_align_asan.cpp compile it with a host compiler.
//
// One-sided (Hestenes) Jacobi: plane rotations from the right make the columns of A orthogonal, A V = U diag(s); V is their product.
// SWEEPS is fixed and nothing loops on a value of the matrix: a NaN falls through every comparison and comes out as NaN, a zero
// matrix as s = 0.  A 3 x 3 matrix converges quadratically and is at rounding level after 5 or 6 sweeps; 12 leaves a margin.
//
// U is not read off the columns alone: u1 = a1 / s1, u2 is a2 made orthogonal to u1 once more, and u3 = +-(u1 x u2) with the sign
// of a3 . (u1 x u2).  For a matrix of full rank this changes rounding errors only; for rank 2 and rank 1 (a planar or collinear
// pose) it completes U to an orthogonal matrix, so T is orthogonal whatever the rank and trace(A T) = sum s holds.  V is a product
// of rotations and of the column exchanges that sort the singular values, det V = +-1 is read off V, and det T = det V det U:
// the rotation mode takes the u3 that makes det T = +1 and counts s3 with the sign of the unconstrained determinant.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PG_ALIGN_HD __host__ __device__ __forceinline__
#else
#define PG_ALIGN_HD inline
#endif

namespace pgalign {

constexpr int SWEEPS = 12;

struct Result {
    double T[9];       // row-major [b][a]: Z0 = Y0 T maps the centred prediction onto the centred target
    double s[3];       // singular values, descending, s[2] without the sign below
    double sum_s;      // s0 + s1 + s2, in rotation mode s0 + s1 + det * s2
    double det;        // +1 or -1: the determinant of the unconstrained T = V U^T
};

// columns p, q of the 3 x 3 row-major m and v rotated so that m's columns p and q become orthogonal
PG_ALIGN_HD void rotate_pair(double* m, double* v, int p, int q) {
    const double alpha = m[p] * m[p] + m[3 + p] * m[3 + p] + m[6 + p] * m[6 + p];
    const double beta = m[q] * m[q] + m[3 + q] * m[3 + q] + m[6 + q] * m[6 + q];
    const double gamma = m[p] * m[q] + m[3 + p] * m[3 + q] + m[6 + p] * m[6 + q];
    double c = 1.0, s = 0.0;
    if (gamma != 0.0) {                                          // (true for a NaN: it propagates)
        const double zeta = (beta - alpha) / (2.0 * gamma);      // +-inf for a tiny gamma: t = 0
        const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        c = 1.0 / sqrt(1.0 + t * t);
        s = c * t;
    }
    for (int r = 0; r < 3; ++r) {
        const double mp = m[3 * r + p], mq = m[3 * r + q];
        m[3 * r + p] = c * mp - s * mq;
        m[3 * r + q] = s * mp + c * mq;
        const double vp = v[3 * r + p], vq = v[3 * r + q];
        v[3 * r + p] = c * vp - s * vq;
        v[3 * r + q] = s * vp + c * vq;
    }
}

// columns p < q of m and v and their norms exchanged where n[p] < n[q]
PG_ALIGN_HD void order_pair(double* m, double* v, double* n, int p, int q) {
    const bool sw = n[p] < n[q];
    for (int r = 0; r < 3; ++r) {
        const double mp = m[3 * r + p], mq = m[3 * r + q], vp = v[3 * r + p], vq = v[3 * r + q];
        m[3 * r + p] = sw ? mq : mp; m[3 * r + q] = sw ? mp : mq;
        v[3 * r + p] = sw ? vq : vp; v[3 * r + q] = sw ? vp : vq;
    }
    const double np_ = n[p], nq = n[q];
    n[p] = sw ? nq : np_; n[q] = sw ? np_ : nq;
}

// A row-major [a][b] = sum_j X0[j][a] Y0[j][b] (X the target, Y the set that is moved).  rotation_only: det T = +1.
PG_ALIGN_HD Result align(const double* A, bool rotation_only) {
    double m[9], v[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    for (int i = 0; i < 9; ++i) m[i] = A[i];
    for (int sweep = 0; sweep < SWEEPS; ++sweep) {
        rotate_pair(m, v, 0, 1);
        rotate_pair(m, v, 0, 2);
        rotate_pair(m, v, 1, 2);
    }
    double n[3];
    for (int c = 0; c < 3; ++c) n[c] = sqrt(m[c] * m[c] + m[3 + c] * m[3 + c] + m[6 + c] * m[6 + c]);
    order_pair(m, v, n, 0, 1);
    order_pair(m, v, n, 1, 2);
    order_pair(m, v, n, 0, 1);

    // u1: the first column's direction (any unit vector for a zero matrix)
    double u1[3], u2[3], u3[3];
    const bool has1 = n[0] > 0.0;
    u1[0] = has1 ? m[0] / n[0] : 1.0;
    u1[1] = has1 ? m[3] / n[0] : 0.0;
    u1[2] = has1 ? m[6] / n[0] : 0.0;
    // u2: the second column without its part along u1; for rank <= 1 the coordinate axis farthest from u1 instead
    const double a0 = fabs(u1[0]), a1 = fabs(u1[1]), a2 = fabs(u1[2]);
    const int far = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);
    const bool has2 = n[1] > 1e-200;
    double w[3];
    w[0] = has2 ? m[1] : (far == 0 ? 1.0 : 0.0);
    w[1] = has2 ? m[4] : (far == 1 ? 1.0 : 0.0);
    w[2] = has2 ? m[7] : (far == 2 ? 1.0 : 0.0);
    const double along = w[0] * u1[0] + w[1] * u1[1] + w[2] * u1[2];
    for (int r = 0; r < 3; ++r) w[r] -= along * u1[r];
    const double wn = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    for (int r = 0; r < 3; ++r) u2[r] = w[r] / wn;
    // u3 = +-(u1 x u2)
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
    u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
    u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    const double side = m[2] * u3[0] + m[5] * u3[1] + m[8] * u3[2];
    const double uside = side < 0.0 ? -1.0 : 1.0;                // the true u3 = uside (u1 x u2): det U = uside
    // det V: +1 for the product of rotations, -1 after an odd number of column exchanges
    const double vdet = v[0] * (v[4] * v[8] - v[5] * v[7]) - v[1] * (v[3] * v[8] - v[5] * v[6]) + v[2] * (v[3] * v[7] - v[4] * v[6]);
    const double vside = vdet < 0.0 ? -1.0 : 1.0;
    const double det = uside * vside;                            // of the unconstrained T = V U^T
    const double flip = rotation_only ? vside : uside;          // rotation mode: det U = det V

    Result out;
    for (int b = 0; b < 3; ++b)
        for (int a = 0; a < 3; ++a) out.T[3 * b + a] = v[3 * b] * u1[a] + v[3 * b + 1] * u2[a] + flip * v[3 * b + 2] * u3[a];
    out.s[0] = n[0]; out.s[1] = n[1]; out.s[2] = n[2];
    out.sum_s = n[0] + n[1] + (rotation_only ? det * n[2] : n[2]);
    out.det = det;
    return out;
}

}  // namespace pgalign
