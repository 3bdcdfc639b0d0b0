// plba_posegn.hpp — what the pose-only Gauss–Newton kernels share: k_lcpose (csrc/plba_lcpose.hpp,
// the loop-closure relative pose) and k_trackpose (csrc/plba_trackpose.hpp, the frame-to-frame pose).
// The reprojection of a 3-D point and its Jacobian row, x = H⁻¹g as Eigen's ColPivHouseholderQR
// solves it (with logAbsDeterminant from the same R), the eigenvalues of a symmetric 6x6 by cyclic
// Jacobi rotations, the inverse of a 6x6, and the fixed-order reduction of a workgroup's partial
// sums. Plain C++ apart from the reduction, with no HIP type, so that host/track_pose.cpp
// (plslam_track_pose_cpu) evaluates the same expressions; every function switches contraction off.
#pragma once

#include <float.h>
#include <math.h>

#if defined(__HIPCC__)
#define PLBA_PGN_FN __host__ __device__ inline
#else
#define PLBA_PGN_FN inline
#endif
#if defined(__clang__)
#define PLBA_PGN_EXACT _Pragma("clang fp contract(off)")
#define PLBA_PGN_UNROLL _Pragma("unroll")
#else
#define PLBA_PGN_EXACT
#define PLBA_PGN_UNROLL
#endif

namespace plba {
namespace pgn {

// T.block(0,0,3,3)·P + T.col(3).head(3) of a row-major 4x4 (or 3x4)
PLBA_PGN_FN void xform(const double *T, const double *P, double *G) {
    PLBA_PGN_EXACT
    for (int i = 0; i < 3; ++i) G[i] = ((T[4 * i] * P[0] + T[4 * i + 1] * P[1]) + T[4 * i + 2] * P[2]) + T[4 * i + 3];
}

// the six entries the reference writes for one projected point G and the image direction (a, b)
// (src/mapHandler.cpp:4724-4729, :4769-4774; src2/stereoFrameHandler.cpp:1118-1123, :1214-1219):
// fx scales both image directions
template <typename CamT>
PLBA_PGN_FN void jrow(const CamT &c, double hth, const double *G, double a, double b, double *J) {
    PLBA_PGN_EXACT
    const double gx = G[0], gy = G[1], gz = G[2];
    const double gz2 = gz * gz;
    const double fgz2 = c.fx / fmax(hth, gz2);
    J[0] = +fgz2 * a * gz;
    J[1] = +fgz2 * b * gz;
    J[2] = -fgz2 * (gx * a + gy * b);
    J[3] = -fgz2 * (gx * gy * a + gy * gy * b + gz * gz * b);
    J[4] = +fgz2 * (gx * gx * a + gz * gz * a + gx * gy * b);
    J[5] = +fgz2 * (gx * gz * b - gy * gz * a);
}

template <typename CamT>
PLBA_PGN_FN void project(const CamT &c, const double *G, double &u, double &v) {
    PLBA_PGN_EXACT
    u = c.cx + c.fx * G[0] / G[2];
    v = c.cy + c.fy * G[1] / G[2];
}

// The serial part's workspace (in LDS on the device: the small dense routines index it dynamically)
struct Work {
    double A[36], W[36], c[6], y[6];
    int perm[6];
};

// x = H⁻¹g as Eigen's ColPivHouseholderQR solves it: Householder reflections with the largest
// remaining column first, rank = the pivots above Eigen's threshold, the rest of x zero. logdet (if
// asked for) receives logAbsDeterminant(): the sum of log|R_kk| over all six pivots.
PLBA_PGN_FN void qr_solve(const double *H, const double *g, double *x, Work &w, double *logdet = nullptr) {
    PLBA_PGN_EXACT
    double *A = w.A, *c = w.c, *y = w.y;
    int *perm = w.perm;
    double maxn2 = 0.0;
    bool finite = true;
    for (int j = 0; j < 6; ++j) {
        double s = 0.0;
        for (int i = 0; i < 6; ++i) {
            A[6 * i + j] = H[6 * i + j];
            s += H[6 * i + j] * H[6 * i + j];
            finite = finite && __builtin_isfinite(H[6 * i + j]);
        }
        finite = finite && __builtin_isfinite(g[j]);
        maxn2 = fmax(maxn2, s);
        perm[j] = j;
        c[j] = g[j];
    }
    // A non-finite system (a match with z = 0) has no pivot to compare: Eigen drops no rank on a NaN
    // norm and its reflections spread the NaN, so x is NaN. (fmax and the pivot search below would
    // skip the NaN, find rank 0 and return x = 0, a step that looks converged.)
    if (!finite) {
        for (int i = 0; i < 6; ++i) x[i] = NAN;
        if (logdet) *logdet = NAN;
        return;
    }
    const double th = sqrt(maxn2) * DBL_EPSILON / 6.0, thr = th * th;
    int nz = 6;
    for (int k = 0; k < 6; ++k) {
        int best = k;
        double bn = -1.0;
        for (int j = k; j < 6; ++j) {
            double s = 0.0;
            for (int i = k; i < 6; ++i) s += A[6 * i + j] * A[6 * i + j];
            if (s > bn) {
                bn = s;
                best = j;
            }
        }
        if (nz == 6 && bn < thr * (double)(6 - k)) nz = k;
        if (best != k) {
            for (int i = 0; i < 6; ++i) {
                const double t = A[6 * i + k];
                A[6 * i + k] = A[6 * i + best];
                A[6 * i + best] = t;
            }
            const int t = perm[k];
            perm[k] = perm[best];
            perm[best] = t;
        }
        // makeHouseholderInPlace: v = [1; essential], H_k = I − τ·v·vᵀ
        const double c0 = A[6 * k + k];
        double tail = 0.0;
        for (int i = k + 1; i < 6; ++i) tail += A[6 * i + k] * A[6 * i + k];
        double tau = 0.0, beta = c0;
        if (tail > DBL_MIN) {
            beta = sqrt(c0 * c0 + tail);
            if (c0 >= 0.0) beta = -beta;
            for (int i = k + 1; i < 6; ++i) A[6 * i + k] /= (c0 - beta);
            tau = (beta - c0) / beta;
        } else {
            for (int i = k + 1; i < 6; ++i) A[6 * i + k] = 0.0;
        }
        A[6 * k + k] = beta;
        for (int j = k + 1; j <= 6; ++j) {  // the trailing columns, then Qᵀg (j == 6)
            double s = (j < 6) ? A[6 * k + j] : c[k];
            for (int i = k + 1; i < 6; ++i) s += A[6 * i + k] * ((j < 6) ? A[6 * i + j] : c[i]);
            s *= tau;
            if (j < 6) {
                A[6 * k + j] -= s;
                for (int i = k + 1; i < 6; ++i) A[6 * i + j] -= s * A[6 * i + k];
            } else {
                c[k] -= s;
                for (int i = k + 1; i < 6; ++i) c[i] -= s * A[6 * i + k];
            }
        }
    }
    if (logdet) {
        double s = 0.0;
        for (int k = 0; k < 6; ++k) s += log(fabs(A[7 * k]));
        *logdet = s;
    }
    for (int i = 0; i < 6; ++i) x[i] = 0.0;
    for (int i = nz - 1; i >= 0; --i) {
        double s = c[i];
        for (int j = i + 1; j < nz; ++j) s -= A[6 * i + j] * y[j];
        y[i] = s / A[6 * i + i];
    }
    for (int i = 0; i < nz; ++i) x[perm[i]] = y[i];
}

// The eigenvalues of the symmetric 6x6 H by cyclic Jacobi rotations on its upper triangle: they are
// left on the diagonal of w.W (entries 7 i), in no particular order.
PLBA_PGN_FN void sym_eig6(const double *H, Work &w) {
    PLBA_PGN_EXACT
    double *a = w.W;
    for (int k = 0; k < 36; ++k) a[k] = H[k];
    for (int sweep = 0; sweep < 50; ++sweep) {
        double sm = 0.0;
        for (int p = 0; p < 5; ++p)
            for (int q = p + 1; q < 6; ++q) sm += fabs(a[6 * p + q]);
        if (sm == 0.0) break;
        for (int p = 0; p < 5; ++p)
            for (int q = p + 1; q < 6; ++q) {
                const double apq = a[6 * p + q], gg = 100.0 * fabs(apq);
                const double app = a[6 * p + p], aqq = a[6 * q + q];
                if (sweep > 3 && fabs(app) + gg == fabs(app) && fabs(aqq) + gg == fabs(aqq)) {
                    a[6 * p + q] = 0.0;
                    continue;
                }
                if (apq == 0.0) continue;
                double h = aqq - app, t;
                if (fabs(h) + gg == fabs(h)) {
                    t = apq / h;
                } else {
                    const double theta = 0.5 * h / apq;
                    t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
                    if (theta < 0.0) t = -t;
                }
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = t * cs, tau = sn / (1.0 + cs);
                h = t * apq;
                a[6 * p + p] = app - h;
                a[6 * q + q] = aqq + h;
                a[6 * p + q] = 0.0;
                for (int j = 0; j < 6; ++j) {
                    if (j == p || j == q) continue;
                    double *u = j < p ? &a[6 * j + p] : &a[6 * p + j];
                    double *v = j < q ? &a[6 * j + q] : &a[6 * q + j];
                    const double gu = *u, hv = *v;
                    *u = gu - sn * (hv + gu * tau);
                    *v = hv + sn * (gu - hv * tau);
                }
            }
    }
}

// smallest eigenvalue of the symmetric 6x6 H
PLBA_PGN_FN double min_eig(const double *H, Work &w) {
    sym_eig6(H, w);
    double m = w.W[0];
    for (int i = 1; i < 6; ++i) m = fmin(m, w.W[7 * i]);
    return m;
}

// all six eigenvalues of the symmetric 6x6 H, ascending (a NaN anywhere gives six NaN)
PLBA_PGN_FN void eig6_sorted(const double *H, double *ev, Work &w) {
    sym_eig6(H, w);
    bool nan = false;
    for (int i = 0; i < 6; ++i) {
        ev[i] = w.W[7 * i];
        nan = nan || ev[i] != ev[i];
    }
    for (int i = 1; i < 6; ++i) {  // insertion sort
        const double v = ev[i];
        int j = i - 1;
        for (; j >= 0 && ev[j] > v; --j) ev[j + 1] = ev[j];
        ev[j + 1] = v;
    }
    if (nan)
        for (int i = 0; i < 6; ++i) ev[i] = NAN;
}

// C = H⁻¹ of a 6x6 by Gauss–Jordan elimination with partial pivoting (w.A is the workspace). false,
// with C all NaN, for a zero or non-finite pivot or a non-finite result.
PLBA_PGN_FN bool inverse6(const double *H, double *C, Work &w) {
    PLBA_PGN_EXACT
    double *A = w.A;
    bool ok = true;
    for (int k = 0; k < 36; ++k) {
        A[k] = H[k];
        C[k] = (k % 7 == 0) ? 1.0 : 0.0;
    }
    for (int k = 0; k < 6 && ok; ++k) {
        int piv = k;
        double best = fabs(A[6 * k + k]);
        for (int i = k + 1; i < 6; ++i)
            if (fabs(A[6 * i + k]) > best) {
                best = fabs(A[6 * i + k]);
                piv = i;
            }
        if (!(best > 0.0) || !__builtin_isfinite(best)) {
            ok = false;
            break;
        }
        if (piv != k)
            for (int j = 0; j < 6; ++j) {
                double t = A[6 * k + j];
                A[6 * k + j] = A[6 * piv + j];
                A[6 * piv + j] = t;
                t = C[6 * k + j];
                C[6 * k + j] = C[6 * piv + j];
                C[6 * piv + j] = t;
            }
        const double d = A[6 * k + k];
        for (int j = 0; j < 6; ++j) {
            A[6 * k + j] = A[6 * k + j] / d;
            C[6 * k + j] = C[6 * k + j] / d;
        }
        for (int i = 0; i < 6; ++i) {
            if (i == k) continue;
            const double f = A[6 * i + k];
            for (int j = 0; j < 6; ++j) {
                A[6 * i + j] -= f * A[6 * k + j];
                C[6 * i + j] -= f * C[6 * k + j];
            }
        }
    }
    for (int k = 0; k < 36 && ok; ++k) ok = __builtin_isfinite(C[k]);
    if (!ok)
        for (int k = 0; k < 36; ++k) C[k] = NAN;
    return ok;
}

#if defined(__HIPCC__)
// The fixed-order reduction of NA per-thread sums over a workgroup of WAVES waves: an xor butterfly
// inside each wave, whose lane 0 leaves the wave's sums in part[wave]. After a barrier, block_sum
// adds the waves in index order. The same input gives bitwise the same output.
template <int NA, int WAVES>
__device__ __forceinline__ void wave_reduce(const double *acc, double (*part)[NA], int lane, int wave) {
    PLBA_PGN_EXACT
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        double v = acc[k];
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
        if (lane == 0) part[wave][k] = v;
    }
}

template <int NA, int WAVES>
__device__ __forceinline__ void block_sum(const double (*part)[NA], double *S) {
    PLBA_PGN_EXACT
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        double v = part[0][k];
#pragma unroll
        for (int wv = 1; wv < WAVES; ++wv) v += part[wv][k];
        S[k] = v;
    }
}
#endif

}  // namespace pgn
}  // namespace plba
