// pose_core.h -- the one copy of the device pose solver: pvnet_pnp_solve (pvnet_amd/csrc/pvnet_pnp.cpp) restated for gfx950, one
// item per wavefront, float64 throughout.  Two translation units compile it, each with a kernel and a C entry point of its own:
//   pose_solve.hip    (libpvnet_vote.so)   pvnet_pose_solve: one item per image, one point set shared by the images
//   pose_classes.hip  (libpvnet_poses.so)  pvnet_pose_solve_classes: one item per (image, class), a point set per class, gated
// Either kernel is PVNET_POSE_KERNEL (at the end of this file) over an argument struct of its own, which says where an item's
// inputs are; everything an item computes is here, so the two give the same bits for the same item.
//
// Same algorithm and constants as the host library, which is the solver's oracle (tests/test_pose_device.py):
//   linear start   dlt_pose: conditioned object points, the 12x12 A^T A of the DLT on normalised image points, cyclic Jacobi
//                  (60 sweeps at most, off <= 1e-30 diag), the eigenvector of the smallest eigenvalue with its sign fixed by
//                  det, the 3x3 block projected onto SO(3) through the eigen-decomposition of P3^T P3, the conditioning undone;
//   refinement     pvnet_pnp_refine: angle-axis + translation, analytic Jacobian, Marquardt damping on diag(J^T J), Nielsen's
//                  update, the same stopping rules; unweighted first, then (with weights) weighted from the unweighted optimum.
// Every sum runs in the host's order (serially, over LDS), so the DLT matrix, the Jacobi rotations and the normal equations
// round as the host's do; only sin / cos / atan2 of the device's math library may differ from the host's in the last place.
//
// Work split inside the wave: lane i owns key-point i (pn <= 64): its normalised point, its residuals and its two Jacobian rows;
// the 78 + 66 entries of the DLT matrix, the 12 rows of a Jacobi rotation and the 27 normal-equation sums are spread over lanes;
// the small scalar chain (rotation angles, the 6x6 Cholesky, accept / reject) runs redundantly in every lane on wave-uniform
// values.  A batch of 32 is 32 waves: the solver is latency-bound, the dependent chain is what costs.
#ifndef PVNET_POSE_CORE_H_
#define PVNET_POSE_CORE_H_

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pvnet_vote.h"

// no contraction anywhere in a translation unit that includes this header, from here to its end: the host library is compiled
// without FMA, and the device must round every product and sum as it does.  The rule is stated here, at file scope, and not in
// the including file, so that it covers the helper functions below and whatever kernel is built on them: a translation unit
// cannot have the solver without it.
#pragma clang fp contract(off)

namespace {

// one unused VGPR granule beyond what a kernel uses: see PVNET_SPARE_VGPRS in vote_common.h
#define PVNET_SPARE_VGPRS_(r) asm volatile("" ::: "v" #r)
#define PVNET_SPARE_VGPRS(r) PVNET_SPARE_VGPRS_(r)

constexpr int PS_LANES = PVNET_POSE_MAX_PN;  // a lane per key-point

struct Shared {
    double x2[PS_LANES][2];   // image points as the host reads them (widened)
    double x3[PS_LANES][3];   // object points
    double nx[PS_LANES][6];   // DLT: xn, yn, Xh[0..2] of every point
    double M[144], V[144];    // DLT normal matrix / its eigenvectors
    double r[2 * PS_LANES];   // residuals of the last evaluation
    double J[2 * PS_LANES][6];
    double H[36], g[6];
};

__device__ inline void cross_matrix(const double* v, double* M) {
    M[0] = 0; M[1] = -v[2]; M[2] = v[1];
    M[3] = v[2]; M[4] = 0; M[5] = -v[0];
    M[6] = -v[1]; M[7] = v[0]; M[8] = 0;
}
__device__ inline void matmul3(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
__device__ inline double det3(const double* M) {
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}
__device__ inline bool inverse3(const double* M, double* I) {
    const double d = det3(M);
    if (!(fabs(d) > 1e-300)) return false;
    I[0] = (M[4] * M[8] - M[5] * M[7]) / d; I[1] = (M[2] * M[7] - M[1] * M[8]) / d; I[2] = (M[1] * M[5] - M[2] * M[4]) / d;
    I[3] = (M[5] * M[6] - M[3] * M[8]) / d; I[4] = (M[0] * M[8] - M[2] * M[6]) / d; I[5] = (M[2] * M[3] - M[0] * M[5]) / d;
    I[6] = (M[3] * M[7] - M[4] * M[6]) / d; I[7] = (M[1] * M[6] - M[0] * M[7]) / d; I[8] = (M[0] * M[4] - M[1] * M[3]) / d;
    return true;
}

// R = exp([w]x) and the right Jacobian Jr(w) of SO(3) (pvnet_pnp.cpp: rotation_and_right_jacobian)
__device__ void rotation_and_right_jacobian(const double* w, double* R, double* Jr) {
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(th2);
    double a, b, c;
    if (th < 1e-5) {
        a = 1.0 - th2 / 6.0;
        b = 0.5 - th2 / 24.0;
        c = 1.0 / 6.0 - th2 / 120.0;
    } else {
        const double s = sin(th);
        a = s / th;
        b = (1.0 - cos(th)) / th2;
        c = (th - s) / (th2 * th);
    }
    double Wx[9], W2[9];
    cross_matrix(w, Wx);
    matmul3(Wx, Wx, W2);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const double I = (i % 4 == 0) ? 1.0 : 0.0;
        R[i] = I + a * Wx[i] + b * W2[i];
        if (Jr) Jr[i] = I - b * Wx[i] + c * W2[i];
    }
}

// pvnet_matrix_to_angle_axis: quaternion first (largest-component branch), then angle-axis
__device__ void matrix_to_angle_axis(const double* R, double* aa) {
    double q[4];
    const double tr = R[0] + R[4] + R[8];
    if (tr > 0) {
        const double s = sqrt(tr + 1.0) * 2;
        q[0] = 0.25 * s; q[1] = (R[7] - R[5]) / s; q[2] = (R[2] - R[6]) / s; q[3] = (R[3] - R[1]) / s;
    } else if (R[0] > R[4] && R[0] > R[8]) {
        const double s = sqrt(1.0 + R[0] - R[4] - R[8]) * 2;
        q[0] = (R[7] - R[5]) / s; q[1] = 0.25 * s; q[2] = (R[1] + R[3]) / s; q[3] = (R[2] + R[6]) / s;
    } else if (R[4] > R[8]) {
        const double s = sqrt(1.0 + R[4] - R[0] - R[8]) * 2;
        q[0] = (R[2] - R[6]) / s; q[1] = (R[1] + R[3]) / s; q[2] = 0.25 * s; q[3] = (R[5] + R[7]) / s;
    } else {
        const double s = sqrt(1.0 + R[8] - R[0] - R[4]) * 2;
        q[0] = (R[3] - R[1]) / s; q[1] = (R[2] + R[6]) / s; q[2] = (R[5] + R[7]) / s; q[3] = 0.25 * s;
    }
    if (q[0] < 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = -q[k];
    const double sn = sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double k = sn < 1e-12 ? 2.0 : 2.0 * atan2(sn, q[0]) / sn;
    aa[0] = k * q[1]; aa[1] = k * q[2]; aa[2] = k * q[3];
}

// the host's jacobi_eigen for the 3x3 block, in registers of every lane (all loops unrolled: static indices)
__device__ void jacobi3(double* A, double* V, double* w) {
#pragma unroll
    for (int i = 0; i < 9; ++i) V[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0, diag = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (i == j) diag += A[i * 3 + j] * A[i * 3 + j];
                else off += A[i * 3 + j] * A[i * 3 + j];
            }
        if (off <= 1e-30 * diag || off == 0.0) break;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                const double apq = A[p * 3 + q];
                if (apq == 0.0) continue;
                const double theta = (A[q * 3 + q] - A[p * 3 + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double akp = A[k * 3 + p], akq = A[k * 3 + q];
                    A[k * 3 + p] = c * akp - sn * akq;
                    A[k * 3 + q] = sn * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double apk = A[p * 3 + k], aqk = A[q * 3 + k];
                    A[p * 3 + k] = c * apk - sn * aqk;
                    A[q * 3 + k] = sn * apk + c * aqk;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double vkp = V[k * 3 + p], vkq = V[k * 3 + q];
                    V[k * 3 + p] = c * vkp - sn * vkq;
                    V[k * 3 + q] = sn * vkp + c * vkq;
                }
            }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = A[i * 3 + i];
}

// the host's jacobi_eigen for the 12x12 DLT matrix, A and V in LDS: the rotation angles are computed in every lane (broadcast
// reads), lane k < 12 rotates row / column k.  Same rotation order and arithmetic as the host, so the same bits.
__device__ void jacobi12(double* A, double* V, int lane) {
    constexpr int n = 12;
    for (int e = lane; e < n * n; e += PS_LANES) V[e] = (e / n == e % n) ? 1.0 : 0.0;
    __syncthreads();
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0, diag = 0;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                const double a = A[i * n + j];
                if (i == j) diag += a * a;
                else off += a * a;
            }
        if (off <= 1e-30 * diag || off == 0.0) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[p * n + q];
                if (apq == 0.0) continue;
                const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                __syncthreads();  // every lane has read the pivot before it changes
                const int k = lane;
                if (k < n) {  // A <- J^T A J: column rotation ...
                    const double akp = A[k * n + p], akq = A[k * n + q];
                    A[k * n + p] = c * akp - sn * akq;
                    A[k * n + q] = sn * akp + c * akq;
                    const double vkp = V[k * n + p], vkq = V[k * n + q];
                    V[k * n + p] = c * vkp - sn * vkq;
                    V[k * n + q] = sn * vkp + c * vkq;
                }
                __syncthreads();
                if (k < n) {  // ... then row rotation, reading what the column rotation wrote
                    const double apk = A[p * n + k], aqk = A[q * n + k];
                    A[p * n + k] = c * apk - sn * aqk;
                    A[q * n + k] = sn * apk + c * aqk;
                }
                __syncthreads();
            }
    }
}

// dlt_pose on the wave.  x3 / x2 of every point are in LDS; false on degenerate input (uniform)
__device__ bool dlt_pose(Shared& S, const double* K, int pn, int lane, double* R, double* t) {
    double Ki[9];
    if (!inverse3(K, Ki)) return false;
    double c[3] = {0, 0, 0};
    for (int i = 0; i < pn; ++i)
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] += S.x3[i][a] / pn;
    double s = 0;
    for (int i = 0; i < pn; ++i)
#pragma unroll
        for (int a = 0; a < 3; ++a) s += (S.x3[i][a] - c[a]) * (S.x3[i][a] - c[a]);
    s = sqrt(s / pn) + 1e-12;
    if (lane < pn) {
        const double u = S.x2[lane][0], v = S.x2[lane][1];
        const double zn = Ki[6] * u + Ki[7] * v + Ki[8];
        S.nx[lane][0] = (Ki[0] * u + Ki[1] * v + Ki[2]) / zn;
        S.nx[lane][1] = (Ki[3] * u + Ki[4] * v + Ki[5]) / zn;
#pragma unroll
        for (int a = 0; a < 3; ++a) S.nx[lane][2 + a] = (S.x3[lane][a] - c[a]) / s;
    }
    __syncthreads();
    // M = A^T A, entry (a, b) by one lane, summed over the points in the host's order
    for (int e = lane; e < 144; e += PS_LANES) {
        const int a = e / 12, b = e % 12;
        double m = 0;
        for (int i = 0; i < pn; ++i) {
            const double xn = S.nx[i][0], yn = S.nx[i][1];
            const double Xa = (a & 3) == 3 ? 1.0 : S.nx[i][2 + (a & 3)], Xb = (b & 3) == 3 ? 1.0 : S.nx[i][2 + (b & 3)];
            const double r0a = a < 4 ? Xa : a < 8 ? 0.0 : -xn * Xa, r0b = b < 4 ? Xb : b < 8 ? 0.0 : -xn * Xb;
            const double r1a = a < 4 ? 0.0 : a < 8 ? Xa : -yn * Xa, r1b = b < 4 ? 0.0 : b < 8 ? Xb : -yn * Xb;
            m += r0a * r0b + r1a * r1b;
        }
        S.M[e] = m;
    }
    __syncthreads();
    jacobi12(S.M, S.V, lane);
    int kmin = 0;
    for (int i = 1; i < 12; ++i)
        if (S.M[i * 13] < S.M[kmin * 13]) kmin = i;
    double P[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) P[i] = S.V[i * 12 + kmin];
    double P3[9] = {P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10]};
    if (det3(P3) < 0) {
#pragma unroll
        for (int i = 0; i < 12; ++i) P[i] = -P[i];
#pragma unroll
        for (int i = 0; i < 9; ++i) P3[i] = -P3[i];
    }
    double G[9], W3[9], e[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) G[a * 3 + b] = P3[a] * P3[b] + P3[3 + a] * P3[3 + b] + P3[6 + a] * P3[6 + b];
    jacobi3(G, W3, e);
    double sv[3], smean = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(e[a] > 1e-300)) return false;
        sv[a] = sqrt(e[a]);
        smean += sv[a] / 3.0;
    }
    double T[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
            T[a * 3 + b] = W3[a * 3] * W3[b * 3] / sv[0] + W3[a * 3 + 1] * W3[b * 3 + 1] / sv[1] + W3[a * 3 + 2] * W3[b * 3 + 2] / sv[2];
    matmul3(P3, T, R);
    if (det3(R) < 0)
#pragma unroll
        for (int a = 0; a < 9; ++a) R[a] = -R[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double tp = P[4 * a + 3] / smean - (R[a * 3] * c[0] + R[a * 3 + 1] * c[1] + R[a * 3 + 2] * c[2]) / s;
        t[a] = tp * s;
    }
    return isfinite(t[0]) && isfinite(t[1]) && isfinite(t[2]);
}

// the host's evaluate on the wave: lane i writes residuals 2i, 2i+1 (and Jacobian rows) to LDS; false (uniform) if a point
// falls on / behind the camera plane.  w = this lane's (wxx, wxy, wyy).
__device__ bool evaluate(Shared& S, const double* K, int pn, int lane, const double* w, const double* p, bool want_J) {
    double R[9], Jr[9];
    rotation_and_right_jacobian(p, R, want_J ? Jr : nullptr);
    bool bad = false;
    if (lane < pn) {
        const double fx = K[0], fy = K[4], px = K[2], py = K[5];
        const double X[3] = {S.x3[lane][0], S.x3[lane][1], S.x3[lane][2]};
        const double RX[3] = {R[0] * X[0] + R[1] * X[1] + R[2] * X[2], R[3] * X[0] + R[4] * X[1] + R[5] * X[2],
                              R[6] * X[0] + R[7] * X[1] + R[8] * X[2]};
        const double Y[3] = {RX[0] + p[3], RX[1] + p[4], RX[2] + p[5]};
        bad = !(fabs(Y[2]) > 1e-12);
        const double iz = 1.0 / Y[2];
        const double dx = fx * Y[0] * iz + px - S.x2[lane][0], dy = fy * Y[1] * iz + py - S.x2[lane][1];
        S.r[2 * lane] = w[0] * dx + w[1] * dy;
        S.r[2 * lane + 1] = w[1] * dx + w[2] * dy;
        if (want_J) {
            const double A[6] = {fx * iz, 0.0, -fx * Y[0] * iz * iz, 0.0, fy * iz, -fy * Y[1] * iz * iz};
            double Xx[9], RXx[9], D[9];
            cross_matrix(X, Xx);
            matmul3(R, Xx, RXx);
            matmul3(RXx, Jr, D);
            double Jp[12];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                Jp[c] = -(A[0] * D[c] + A[1] * D[3 + c] + A[2] * D[6 + c]);
                Jp[6 + c] = -(A[3] * D[c] + A[4] * D[3 + c] + A[5] * D[6 + c]);
                Jp[3 + c] = A[c];
                Jp[9 + c] = A[3 + c];
            }
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                S.J[2 * lane][c] = w[0] * Jp[c] + w[1] * Jp[6 + c];
                S.J[2 * lane + 1][c] = w[1] * Jp[c] + w[2] * Jp[6 + c];
            }
        }
    }
    const bool any_bad = __any(bad);
    __syncthreads();
    return !any_bad;
}

__device__ inline double cost_of(const Shared& S, int pn) {
    double c = 0;
    for (int i = 0; i < 2 * pn; ++i) c += S.r[i] * S.r[i];
    return 0.5 * c;
}

// solve6: Cholesky of the SPD 6x6 system, every lane redundantly
__device__ bool solve6(const double* A, const double* b, double* x) {
    double L[36];
#pragma unroll
    for (int i = 0; i < 36; ++i) L[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double s = A[i * 6 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= L[i * 6 + k] * L[j * 6 + k];
            if (i == j) {
                if (!(s > 0.0) || !isfinite(s)) return false;
                L[i * 6 + i] = sqrt(s);
            } else {
                L[i * 6 + j] = s / L[j * 6 + j];
            }
        }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[i * 6 + k] * y[k];
        y[i] = s / L[i * 6 + i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) s -= L[k * 6 + i] * x[k];
        x[i] = s / L[i * 6 + i];
    }
    return true;
}

// pvnet_pnp_refine on the wave: p (in/out, uniform), returns the iteration count
__device__ int refine(Shared& S, const double* K, int pn, int lane, const double* w, double* p, int max_iterations) {
    int it = 0;
    if (!evaluate(S, K, pn, lane, w, p, true)) return 0;
    double cost = cost_of(S, pn);
    double lambda = 1e-4, nu = 2.0;
    for (; it < max_iterations; ++it) {
        // normal equations: entry e < 21 of the lower triangle, or g[e - 21], summed by one lane in the host's order
        if (lane < 27) {
            int a, b = -1;
            if (lane < 21) {
                a = 0;
                while ((a + 1) * (a + 2) / 2 <= lane) ++a;
                b = lane - a * (a + 1) / 2;
            } else {
                a = lane - 21;
            }
            double s = 0;
            if (b >= 0) {
                for (int i = 0; i < 2 * pn; ++i) s += S.J[i][a] * S.J[i][b];
                S.H[a * 6 + b] = s;
                S.H[b * 6 + a] = s;
            } else {
                for (int i = 0; i < 2 * pn; ++i) s -= S.J[i][a] * S.r[i];
                S.g[a] = s;
            }
        }
        __syncthreads();
        double H[36], g[6];
#pragma unroll
        for (int e = 0; e < 36; ++e) H[e] = S.H[e];
#pragma unroll
        for (int a = 0; a < 6; ++a) g[a] = S.g[a];
        __syncthreads();
        double gmax = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a) gmax = fmax(gmax, fabs(g[a]));
        if (gmax < 1e-14) break;
        bool stepped = false, tiny = false;
        for (int tries = 0; tries < 40 && !stepped; ++tries) {
            double A[36], d[6], pnw[6];
#pragma unroll
            for (int e = 0; e < 36; ++e) A[e] = H[e];
#pragma unroll
            for (int a = 0; a < 6; ++a) A[a * 6 + a] += lambda * (H[a * 6 + a] > 1e-300 ? H[a * 6 + a] : 1.0);
            if (solve6(A, g, d)) {
                double dn = 0, xn = 0;
#pragma unroll
                for (int a = 0; a < 6; ++a) { pnw[a] = p[a] + d[a]; dn += d[a] * d[a]; xn += p[a] * p[a]; }
                if (sqrt(dn) <= 1e-15 * (sqrt(xn) + 1e-15)) { tiny = true; break; }
                if (evaluate(S, K, pn, lane, w, pnw, false)) {
                    const double cn = cost_of(S, pn);
                    double pred = 0;
#pragma unroll
                    for (int a = 0; a < 6; ++a)
                        pred += 0.5 * d[a] * (lambda * (H[a * 6 + a] > 1e-300 ? H[a * 6 + a] : 1.0) * d[a] + g[a]);
                    const double rho = pred > 0 ? (cost - cn) / pred : -1.0;
                    if (cn < cost && rho > 0) {
#pragma unroll
                        for (int a = 0; a < 6; ++a) p[a] = pnw[a];
                        const double rel = (cost - cn) / (cost > 1e-300 ? cost : 1e-300);
                        cost = cn;
                        const double t = 2.0 * rho - 1.0;
                        lambda *= fmax(1.0 / 3.0, 1.0 - t * t * t);
                        nu = 2.0;
                        stepped = true;
                        if (rel < 1e-16) tiny = true;
                        continue;
                    }
                }
            }
            lambda *= nu;
            nu *= 2.0;
        }
        if (!stepped || tiny) break;
        if (!evaluate(S, K, pn, lane, w, p, true)) break;
    }
    return it;
}

// Evaluator.evaluate_uncertainty's weight of one key-point (pvnet_amd/evaluation.py): zero when cov[0,0] < 1e-6 or an entry is
// NaN, else the inverse matrix square root V diag(1 / sqrt(max(w, 1e-30))) V^T of the (lower-triangle) symmetric 2x2 matrix
__device__ void covariance_weight(const float* cv, double* w) {
    const double a = cv[0], b = cv[2], c = cv[3];
    if (a < 1e-6 || isnan(cv[0]) || isnan(cv[1]) || isnan(cv[2]) || isnan(cv[3])) {
        w[0] = w[1] = w[2] = 0.0;
        return;
    }
    if (b == 0.0) {  // already diagonal: the eigenvalues are the diagonal, exactly as an eigen-solver returns them
        w[0] = 1.0 / sqrt(fmax(a, 1e-30));
        w[1] = 0.0;
        w[2] = 1.0 / sqrt(fmax(c, 1e-30));
        return;
    }
    const double m = 0.5 * (a + c), h = 0.5 * (a - c), r = sqrt(h * h + b * b);
    const double l1 = m + r;                  // >= a > 0
    const double l2 = (a * c - b * b) / l1;   // the small one through the determinant: no cancellation
    double vx, vy;                            // eigenvector of l1
    if (h >= 0) { vx = h + r; vy = b; } else { vx = b; vy = r - h; }
    const double nn = sqrt(vx * vx + vy * vy);
    vx /= nn;
    vy /= nn;
    const double s1 = 1.0 / sqrt(fmax(l1, 1e-30)), s2 = 1.0 / sqrt(fmax(l2, 1e-30));
    w[0] = s1 * vx * vx + s2 * vy * vy;
    w[1] = (s1 - s2) * vx * vy;
    w[2] = s1 * vy * vy + s2 * vx * vx;
}

// PVNET_POSE_KERNEL(name, Args, spare, gate) defines the kernel `name(Args A)`: one item on the wave, from its key-points in global
// memory to its rows of rt / poses / status.  The body is stated here once and expanded in the kernel itself, not called: a
// function that the kernel inlines is optimised on its own first, and pose_solve_kernel would no longer be, instruction for
// instruction, the kernel that tests/test_pose_device*.py and the pose sweeps were run on.
//   Args    the kernel's own argument struct: the fields pose_solve.hip's PoseArgs has under these names (pts2d, s1, s2, f64,
//           weights, weight_kind, pn, max_iterations, rt, poses, status; weights, rt, poses and status have one row per item) and
//           three answers about where item `img` (the block index) is:
//             const double* camera(int img)       its [3,3]
//             int64_t point_offset(int img)       the element offset of its first key-point in pts2d
//             const double* points(int img)       its object points [pn,3]
//   spare   the VGPR that PVNET_SPARE_VGPRS names: one granule beyond what the kernel uses
//   gate    a statement that runs before the item reads anything, with A, img and lane in scope; it may return
#define PVNET_POSE_KERNEL(name, Args, spare, gate)                                                                              \
    __global__ __launch_bounds__(PS_LANES) void name(Args A) {                                                                  \
        PVNET_SPARE_VGPRS(spare);                                                                                               \
        __shared__ Shared S;                                                                                                    \
        const int img = blockIdx.x, lane = threadIdx.x, pn = A.pn;                                                              \
        gate;                                                                                                                   \
        const double* Kp = A.camera(img);                                                                                       \
        double K[9];                                                                                                            \
        _Pragma("unroll")                                                                                                       \
        for (int e = 0; e < 9; ++e) K[e] = Kp[e];                                                                               \
        double w[3] = {0.0, 0.0, 0.0};                                                                                          \
        if (lane < pn) {                                                                                                        \
            const int64_t o = A.point_offset(img) + lane * A.s1;                                                                \
            if (A.f64) {                                                                                                        \
                const double* x = static_cast<const double*>(A.pts2d);                                                          \
                S.x2[lane][0] = x[o];                                                                                           \
                S.x2[lane][1] = x[o + A.s2];                                                                                    \
            } else {                                                                                                            \
                const float* x = static_cast<const float*>(A.pts2d);                                                            \
                S.x2[lane][0] = x[o];                                                                                           \
                S.x2[lane][1] = x[o + A.s2];                                                                                    \
            }                                                                                                                   \
            _Pragma("unroll")                                                                                                   \
            for (int a = 0; a < 3; ++a) S.x3[lane][a] = A.points(img)[lane * 3 + a];                                            \
            if (A.weight_kind == PVNET_POSE_W_EXPLICIT) {                                                                       \
                const double* W = static_cast<const double*>(A.weights) + ((size_t)img * pn + lane) * 3;                        \
                w[0] = W[0]; w[1] = W[1]; w[2] = W[2];                                                                          \
            } else if (A.weight_kind == PVNET_POSE_W_COV_F32) {                                                                 \
                covariance_weight(static_cast<const float*>(A.weights) + ((size_t)img * pn + lane) * 4, w);                     \
            }                                                                                                                   \
        }                                                                                                                       \
        __syncthreads();                                                                                                        \
        double R[9], t[3], p[6];                                                                                                \
        int it = -2;                                                                                                            \
        if (dlt_pose(S, K, pn, lane, R, t)) {                                                                                   \
            matrix_to_angle_axis(R, p);                                                                                         \
            p[3] = t[0]; p[4] = t[1]; p[5] = t[2];                                                                              \
            const double unit[3] = {1.0, 0.0, 1.0};                                                                             \
            it = refine(S, K, pn, lane, unit, p, A.max_iterations);                                                             \
            if (A.weight_kind != PVNET_POSE_W_NONE) it += refine(S, K, pn, lane, w, p, A.max_iterations);                       \
        } else {                                                                                                                \
            _Pragma("unroll")                                                                                                   \
            for (int a = 0; a < 6; ++a) p[a] = 0.0;                                                                             \
        }                                                                                                                       \
        if (A.rt && lane < 6) A.rt[(size_t)img * 6 + lane] = p[lane];                                                           \
        if (A.poses && lane < 12) {                                                                                             \
            bool any = false;                                                                                                   \
            _Pragma("unroll")                                                                                                   \
            for (int a = 0; a < 6; ++a) any = any || p[a] != 0.0;                                                               \
            double v = 0.0;                                                                                                     \
            if (any) {                                                                                                          \
                rotation_and_right_jacobian(p, R, nullptr);                                                                     \
                const int r = lane / 4, c = lane % 4;                                                                           \
                v = c < 3 ? R[r * 3 + c] : p[3 + r];                                                                            \
            }                                                                                                                   \
            A.poses[(size_t)img * 12 + lane] = v;                                                                               \
        }                                                                                                                       \
        if (A.status && lane == 0) A.status[img] = it;                                                                          \
    }

}  // namespace

#endif  // PVNET_POSE_CORE_H_
