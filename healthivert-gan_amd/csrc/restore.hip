// Restore of a (synthesized) straightened vertebra crop to patient CT space: the inverse of the straightening stage, for every voxel of a
// patient-space box (reference straighten/straighten/curve.py:104-150,223-239 Interpolator.global_to_local / _to_local / interpolate_coords,
// which the reference runs one point at a time in Python).
//
//   restore_kernel<LDS>     one lane per patient voxel p of the box: the local coordinate of p along the curve exactly as _to_local +
//                           interpolate_coords compute it (two scans over the knots: the nearest knot, then the sign change of the distance
//                           to the plane nearest to it; linear interpolation to distance 0 over up to four planes), from there the
//                           coordinate in the crop, the coverage test, a trilinear sample of the crop's CT (map_coordinates order 1), a
//                           nearest sample of its label (order 0), and the write rule.  Knots, frames and cumulative lengths sit in LDS
//                           (13 doubles per knot); LDS = false reads them from global memory when they do not fit.
//                           ORDER = 3 (hv_restore_volume_spline): the CT sample is cubic (map_coordinates order 3), 4 x 4 x 4 taps of the
//                           B-spline coefficients of the crop's filled sub-box; everything else is shared.
//                           With anisotropic voxels (hv_restore_volume_sp) p enters the scans as p * spacing; the rest is unchanged.
//   curve_points_kernel<LDS> one lane per point of a list: global_to_local or local_to_global (curve.py:110-114,131-138) through the same
//                           device function (rs_curve_map) as the restore, no crop involved.
//   restore_uncrop_kernel   the single-centroid branch (the crop was cut from the raw volume): the plain un-crop of the box.
// Everything in doubles in the reference's operation order (-ffp-contract=off); element offsets are 64-bit.
#include <cmath>
#include "volume_access.h"                                 // hv_ld_dt
#include "spline_tap.h"                                    // hv_spline_sample

#define RS_THREADS 512
#define RS_KNOT_DOUBLES 13                                    // knot 3, frame 9, cumulative length 1
#define RS_LDS_BYTES 65536                                    // what a launch gets without asking for more: 630 knots

struct RsCurve { const double* knots; const double* basis; const double* cumlen; int N; double c1, c2, sp0, sp1, sp2; };
struct RsArgs {
    const void* crop_ct; int crop_dt; long long cs0, cs1, cs2;
    const uint8_t* crop_lab; long long ls0, ls1, ls2;
    int lo0, lo1, lo2, n0, n1, n2, st0, st1, st2;             // the crop_box row of the vertebra
    const void* plab; int pdt; long long ps0, ps1, ps2;       // the patient's own label (vertebra rule), may be null for the crop rule
    int r0, r1, r2, rn0, rn1, rn2;                            // the patient-space box: origin and size
    int where, vert_id;
    double* out_ct; long long os0, os1, os2;
    uint8_t* out_lab; long long qs0, qs1, qs2;
    uint8_t* cov; long long vs0, vs1, vs2;
    double* local;
};

__device__ __forceinline__ double rs_ld_ct(const void* p, int dt, long long o) {
    return dt == HV_DT_F32 ? (double)((const float*)p)[o] : ((const double*)p)[o];
}

__device__ __forceinline__ int rs_sign(double v) { return (v > 0.0) - (v < 0.0); }   // np.sign: sign(0) = 0

// the write rule and the three stores of one voxel
__device__ __forceinline__ void rs_write(const RsArgs& A, long long px, long long py, long long pz, double v, int l) {
    if (A.where == HV_RESTORE_VERTEBRA) {
        bool own = l == A.vert_id;
        if (!own) own = hv_ld_dt(A.plab, A.pdt, px * A.ps0 + py * A.ps1 + pz * A.ps2) == (double)A.vert_id;
        if (!own) return;
    }
    A.out_ct[px * A.os0 + py * A.os1 + pz * A.os2] = v;
    A.out_lab[px * A.qs0 + py * A.qs1 + pz * A.qs2] = (uint8_t)l;
    if (A.cov) A.cov[px * A.vs0 + py * A.vs1 + pz * A.vs2] = 1;
}

extern __shared__ double rs_lds[];

// knots, frames and cumulative lengths of the curve into LDS (all lanes of the block; ends in a barrier)
__device__ __forceinline__ void rs_stage(const RsCurve& cv) {
    const int N = cv.N;
    for (int i = threadIdx.x; i < 3 * N; i += RS_THREADS) rs_lds[i] = cv.knots[i];
    for (int i = threadIdx.x; i < 9 * N; i += RS_THREADS) rs_lds[3 * N + i] = cv.basis[i];
    for (int i = threadIdx.x; i < N; i += RS_THREADS) rs_lds[12 * N + i] = cv.cumlen[i];
    __syncthreads();
}

// One point through Interpolator._to_local (TO_GLOBAL = false: P in millimetres -> local) or ._to_global (true: P local -> millimetres)
// and interpolate_coords (curve.py:122-138,223-239).  Per knot n, with centre[n] = (cumlen[n], c1, c2):
//   _to_local   d = P - knots[n],  to_origin = |d|,  q = basis[n]^T d ('nji,nj->ni'),  to_plane = q[0],  coords = q + centre[n]
//   _to_global  d = P - centre[n], to_plane = d[0],  q = basis[n] d   ('nij,nj->ni'),  to_origin = |q|,  coords = q + knots[n]
// then two scans over the knots (the nearest knot, the sign change of to_plane nearest to it) and the interpolation to to_plane = 0 over
// up to four planes.  The result may be non-finite (a duplicate to_plane in the window).
template <bool LDS, bool TO_GLOBAL>
__device__ __forceinline__ void rs_curve_map(const RsCurve& cv, const double P0, const double P1, const double P2, double& l0, double& l1,
                                             double& l2) {
    const int N = cv.N;
#define RS_K(n, i) (LDS ? rs_lds[3 * (n) + (i)] : cv.knots[3 * (long long)(n) + (i)])
#define RS_B(n, j, i) (LDS ? rs_lds[3 * N + 9 * (n) + 3 * (j) + (i)] : cv.basis[9 * (long long)(n) + 3 * (j) + (i)])
#define RS_C(n) (LDS ? rs_lds[12 * N + (n)] : cv.cumlen[n])
    // scan 1: idx = to_origin.argmin(), the first minimum
    double best = __builtin_inf();
    int idx = 0;
    for (int n = 0; n < N; ++n) {
        double r;
        if (TO_GLOBAL) {
            const double d0 = P0 - RS_C(n), d1 = P1 - cv.c1, d2 = P2 - cv.c2;
            const double g0 = (RS_B(n, 0, 0) * d0 + RS_B(n, 0, 1) * d1) + RS_B(n, 0, 2) * d2;
            const double g1 = (RS_B(n, 1, 0) * d0 + RS_B(n, 1, 1) * d1) + RS_B(n, 1, 2) * d2;
            const double g2 = (RS_B(n, 2, 0) * d0 + RS_B(n, 2, 1) * d1) + RS_B(n, 2, 2) * d2;
            r = sqrt((g0 * g0 + g1 * g1) + g2 * g2);
        } else {
            const double d0 = P0 - RS_K(n, 0), d1 = P1 - RS_K(n, 1), d2 = P2 - RS_K(n, 2);
            r = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
        }
        if (r < best) { best = r; idx = n; }
    }
    // scan 2: the candidates n with sign(to_plane[n + 1]) - sign(to_plane[n]) != 0; the one nearest idx, the lowest on ties
    {
        int cand = -1, cand_d = 0x7fffffff;
        int s_prev;
        if (TO_GLOBAL) {
            s_prev = rs_sign(P0 - RS_C(0));
        } else {
            const double d0 = P0 - RS_K(0, 0), d1 = P1 - RS_K(0, 1), d2 = P2 - RS_K(0, 2);
            s_prev = rs_sign((RS_B(0, 0, 0) * d0 + RS_B(0, 1, 0) * d1) + RS_B(0, 2, 0) * d2);
        }
        for (int n = 0; n + 1 < N; ++n) {
            int s_next;
            if (TO_GLOBAL) {
                s_next = rs_sign(P0 - RS_C(n + 1));
            } else {
                const double d0 = P0 - RS_K(n + 1, 0), d1 = P1 - RS_K(n + 1, 1), d2 = P2 - RS_K(n + 1, 2);
                s_next = rs_sign((RS_B(n + 1, 0, 0) * d0 + RS_B(n + 1, 1, 0) * d1) + RS_B(n + 1, 2, 0) * d2);
            }
            if (s_next != s_prev) {
                const int dd = n > idx ? n - idx : idx - n;
                if (dd < cand_d) { cand_d = dd; cand = n; }
            }
            s_prev = s_next;
        }
        if (cand >= 0) idx = cand;
    }
    // the window [max(0, idx - 2), idx + 2) clipped to N: up to four planes; the slots past its end sort last (+inf)
    const int w0 = idx - 2 > 0 ? idx - 2 : 0, w1 = idx + 2 < N ? idx + 2 : N, L = w1 - w0;
    double x[4], y0[4], y1[4], y2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool valid = k < L;
        const int n = valid ? w0 + k : w0;
        if (TO_GLOBAL) {
            const double d0 = P0 - RS_C(n), d1 = P1 - cv.c1, d2 = P2 - cv.c2;
            const double g0 = (RS_B(n, 0, 0) * d0 + RS_B(n, 0, 1) * d1) + RS_B(n, 0, 2) * d2;
            const double g1 = (RS_B(n, 1, 0) * d0 + RS_B(n, 1, 1) * d1) + RS_B(n, 1, 2) * d2;
            const double g2 = (RS_B(n, 2, 0) * d0 + RS_B(n, 2, 1) * d1) + RS_B(n, 2, 2) * d2;
            x[k] = valid ? d0 : __builtin_inf();
            y0[k] = g0 + RS_K(n, 0);
            y1[k] = g1 + RS_K(n, 1);
            y2[k] = g2 + RS_K(n, 2);
        } else {
            const double d0 = P0 - RS_K(n, 0), d1 = P1 - RS_K(n, 1), d2 = P2 - RS_K(n, 2);
            const double q0 = (RS_B(n, 0, 0) * d0 + RS_B(n, 1, 0) * d1) + RS_B(n, 2, 0) * d2;
            const double q1 = (RS_B(n, 0, 1) * d0 + RS_B(n, 1, 1) * d1) + RS_B(n, 2, 1) * d2;
            const double q2 = (RS_B(n, 0, 2) * d0 + RS_B(n, 1, 2) * d1) + RS_B(n, 2, 2) * d2;
            x[k] = valid ? q0 : __builtin_inf();
            y0[k] = q0 + RS_C(n);
            y1[k] = q1 + cv.c1;
            y2[k] = q2 + cv.c2;
        }
    }
    // interp1d to 0 as straighten.interp_linear restates it: stable sort by to_plane (adjacent exchanges on a strict >), searchsorted left,
    // the segment clipped to [1, L - 1], slope * (0 - x_lo) + y_lo
#define RS_CX(a, b)                                                                      \
    if (x[a] > x[b]) {                                                                   \
        double t;                                                                        \
        t = x[a]; x[a] = x[b]; x[b] = t;       t = y0[a]; y0[a] = y0[b]; y0[b] = t;      \
        t = y1[a]; y1[a] = y1[b]; y1[b] = t;   t = y2[a]; y2[a] = y2[b]; y2[b] = t;      \
    }
    RS_CX(0, 1) RS_CX(1, 2) RS_CX(2, 3) RS_CX(0, 1) RS_CX(1, 2) RS_CX(0, 1)
#undef RS_CX
    int hi = (x[0] < 0.0) + (x[1] < 0.0) + (x[2] < 0.0) + (x[3] < 0.0);
    hi = hi < 1 ? 1 : hi;
    hi = hi > L - 1 ? L - 1 : hi;
#define RS_SEL(a, k) ((k) == 1 ? a[1] : (k) == 2 ? a[2] : (k) == 3 ? a[3] : a[0])
    const double x_lo = RS_SEL(x, hi - 1), x_hi = RS_SEL(x, hi);
    const double dx = x_hi - x_lo, xn = 0.0 - x_lo;
    const double a0 = RS_SEL(y0, hi - 1), a1 = RS_SEL(y1, hi - 1), a2 = RS_SEL(y2, hi - 1);
    l0 = ((RS_SEL(y0, hi) - a0) / dx) * xn + a0;
    l1 = ((RS_SEL(y1, hi) - a1) / dx) * xn + a1;
    l2 = ((RS_SEL(y2, hi) - a2) / dx) * xn + a2;
#undef RS_SEL
#undef RS_K
#undef RS_B
#undef RS_C
}

template <bool LDS, int ORDER>
__global__ __launch_bounds__(RS_THREADS) void restore_kernel(RsCurve cv, RsArgs A) {
    if (LDS) rs_stage(cv);
    const long long total = (long long)A.rn0 * A.rn1 * A.rn2;
    const long long e = (long long)blockIdx.x * RS_THREADS + threadIdx.x;
    if (e >= total) return;
    const int iz = (int)(e % A.rn2), iy = (int)((e / A.rn2) % A.rn1), ix = (int)(e / ((long long)A.rn1 * A.rn2));
    const long long px = A.r0 + ix, py = A.r1 + iy, pz = A.r2 + iz;
    // the voxel in millimetres (pixel_to_spatial, curve.py:160-176): the knots are in millimetres
    double l0, l1, l2;
    rs_curve_map<LDS, false>(cv, (double)px * cv.sp0, (double)py * cv.sp1, (double)pz * cv.sp2, l0, l1, l2);
    const bool finite = isfinite(l0) && isfinite(l1) && isfinite(l2);
    if (A.local) {
        const double nan = __builtin_nan("");
        A.local[3 * e] = finite ? l0 : nan;
        A.local[3 * e + 1] = finite ? l1 : nan;
        A.local[3 * e + 2] = finite ? l2 : nan;
    }
    if (!finite) return;      // duplicate to_plane in the window: not covered
    // Local coordinates are (cumulative length, offset along frame vector 1, along frame vector 2); the straight volume [N][PA][PB] the crop
    // was cut from is indexed (n, a, b) with a along frame vector 2 and b along frame vector 1 (interpolate_along's meshgrid), so the
    // in-plane pair swaps on the way to the crop.
    const double c0 = (l0 - (double)A.lo0) + (double)A.st0, c1 = (l2 - (double)A.lo1) + (double)A.st1, c2 = (l1 - (double)A.lo2) + (double)A.st2;
    const int e0 = A.st0 + A.n0 - 1, e1 = A.st1 + A.n1 - 1, e2 = A.st2 + A.n2 - 1;     // last filled index per axis
    if (!(c0 >= (double)A.st0 && c0 <= (double)e0 && c1 >= (double)A.st1 && c1 <= (double)e1 && c2 >= (double)A.st2 && c2 <= (double)e2)) return;
    double v = 0.0;
    if constexpr (ORDER == 3) {
        // crop_ct holds the coefficients of the filled sub-box alone ([n0][n1][n2] contiguous, mirrored at its own edges): the sample lies at
        // c - start, inside [0, n - 1] by the coverage test (the difference is monotonic in c)
        v = hv_spline_sample((const double*)A.crop_ct, A.n0, A.n1, A.n2, c0 - (double)A.st0, c1 - (double)A.st1, c2 - (double)A.st2);
    } else {
        const double f0 = floor(c0), f1 = floor(c1), f2 = floor(c2);
        const double t0 = c0 - f0, t1 = c1 - f1, t2 = c2 - f2;
        const long long i0 = (long long)f0, i1 = (long long)f1, i2 = (long long)f2;
        // at c = the last filled index the upper weight is 0 and the upper neighbour (the crop's zero padding) is not read
        const long long ox[2] = {i0 * A.cs0, (i0 + 1 <= e0 ? i0 + 1 : i0) * A.cs0}, oy[2] = {i1 * A.cs1, (i1 + 1 <= e1 ? i1 + 1 : i1) * A.cs1},
                        oz[2] = {i2 * A.cs2, (i2 + 1 <= e2 ? i2 + 1 : i2) * A.cs2};
        const double wx[2] = {1.0 - t0, t0}, wy[2] = {1.0 - t1, t1}, wz[2] = {1.0 - t2, t2};
        // map_coordinates order 1: sum over the 8 corners, last axis fastest, coefficient = value * w_x * w_y * w_z
#pragma unroll
        for (int hx = 0; hx < 2; ++hx)
#pragma unroll
            for (int hy = 0; hy < 2; ++hy)
#pragma unroll
                for (int hz = 0; hz < 2; ++hz) v += ((rs_ld_ct(A.crop_ct, A.crop_dt, ox[hx] + oy[hy] + oz[hz]) * wx[hx]) * wy[hy]) * wz[hz];
    }
    const long long m0 = (long long)floor(c0 + 0.5), m1 = (long long)floor(c1 + 0.5), m2 = (long long)floor(c2 + 0.5);   // order 0
    const int l = (int)A.crop_lab[m0 * A.ls0 + m1 * A.ls1 + m2 * A.ls2];
    rs_write(A, px, py, pz, v, l);
}

// knots == NULL: the crop was cut from the raw volume at box.lo, so crop voxel (p - lo + start) goes back to p
__global__ __launch_bounds__(256) void restore_uncrop_kernel(RsArgs A) {
    const long long total = (long long)A.rn0 * A.rn1 * A.rn2;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int iz = (int)(e % A.rn2), iy = (int)((e / A.rn2) % A.rn1), ix = (int)(e / ((long long)A.rn1 * A.rn2));
    const long long px = A.r0 + ix, py = A.r1 + iy, pz = A.r2 + iz;
    const long long s0 = px - A.lo0, s1 = py - A.lo1, s2 = pz - A.lo2;
    if (A.local) {
        A.local[3 * e] = (double)px; A.local[3 * e + 1] = (double)py; A.local[3 * e + 2] = (double)pz;
    }
    if (!(s0 >= 0 && s0 < A.n0 && s1 >= 0 && s1 < A.n1 && s2 >= 0 && s2 < A.n2)) return;
    const long long c0 = s0 + A.st0, c1 = s1 + A.st1, c2 = s2 + A.st2;
    const double v = rs_ld_ct(A.crop_ct, A.crop_dt, c0 * A.cs0 + c1 * A.cs1 + c2 * A.cs2);
    const int l = (int)A.crop_lab[c0 * A.ls0 + c1 * A.ls1 + c2 * A.ls2];
    rs_write(A, px, py, pz, v, l);
}

// hv_curve_points: one lane per point.  direction 0: the point (voxel indices) times the spacing through _to_local, the local coordinate
// in the reference's order (no in-plane swap); direction 1: the local point through _to_global, the result divided by the spacing.
template <bool LDS>
__global__ __launch_bounds__(RS_THREADS) void curve_points_kernel(RsCurve cv, const double* __restrict__ points, long long M, int direction,
                                                                  double* __restrict__ out) {
    if (LDS) rs_stage(cv);
    const long long m = (long long)blockIdx.x * RS_THREADS + threadIdx.x;
    if (m >= M) return;
    const double p0 = points[3 * m], p1 = points[3 * m + 1], p2 = points[3 * m + 2];
    double r0, r1, r2;
    if (direction == HV_CURVE_TO_LOCAL) {
        rs_curve_map<LDS, false>(cv, p0 * cv.sp0, p1 * cv.sp1, p2 * cv.sp2, r0, r1, r2);
    } else {
        rs_curve_map<LDS, true>(cv, p0, p1, p2, r0, r1, r2);
        r0 = r0 / cv.sp0; r1 = r1 / cv.sp1; r2 = r2 / cv.sp2;        // spatial_to_pixel (curve.py:179-195)
    }
    const bool finite = isfinite(r0) && isfinite(r1) && isfinite(r2);
    const double nan = __builtin_nan("");
    out[3 * m] = finite ? r0 : nan;
    out[3 * m + 1] = finite ? r1 : nan;
    out[3 * m + 2] = finite ? r2 : nan;
}

static bool rs_spacing_ok(const double* sp) {
    if (!sp) return false;
    for (int i = 0; i < 3; ++i)
        if (!(sp[i] > 0.0) || !std::isfinite(sp[i])) return false;
    return true;
}

// both restore entries: order 1 reads the crop's CT (crop_dtype, strides), order 3 the contiguous float64 coefficients of its filled sub-box
static int rs_restore(int order, const void* crop_ct, int crop_dtype, long long cs0, long long cs1, long long cs2, const uint8_t* crop_label,
                      long long ls0, long long ls1, long long ls2, int O0, int O1, int O2, const int* box, const double* knots,
                      const double* basis, const double* cumlen, int N, double centre1, double centre2, const void* patient_label,
                      int label_dtype, long long ps0, long long ps1, long long ps2, int D0, int D1, int D2, const int* region, int where,
                      int vert_id, double* ct_out, long long os0, long long os1, long long os2, uint8_t* label_out, long long qs0,
                      long long qs1, long long qs2, uint8_t* covered, long long vs0, long long vs1, long long vs2, double* local_out,
                      const double* spacing, void* stream) {
    if (!rs_spacing_ok(spacing)) return HV_ERR_ARG;
    if (order == 3 && !knots) return HV_ERR_ARG;         // the un-crop branch copies voxels: it has no cubic form
    if (!crop_ct || !crop_label || !box || !region || !ct_out || !label_out || O0 <= 0 || O1 <= 0 || O2 <= 0 || D0 <= 0 || D1 <= 0 || D2 <= 0 ||
        (crop_dtype != HV_DT_F32 && crop_dtype != HV_DT_F64) || (where != HV_RESTORE_CROP && where != HV_RESTORE_VERTEBRA) || vert_id < 0 ||
        vert_id > 255)
        return HV_ERR_ARG;
    if (where == HV_RESTORE_VERTEBRA && (!patient_label || label_dtype < HV_DT_U8 || label_dtype > HV_DT_F64)) return HV_ERR_ARG;
    if (knots && (!basis || !cumlen || N < 2)) return HV_ERR_ARG;
    const int O[3] = {O0, O1, O2}, D[3] = {D0, D1, D2};
    for (int i = 0; i < 3; ++i) {
        // the filled part of the crop lies inside the crop, the patient-space box inside the patient: every index the kernels form is in range
        if (box[i] < 0 || box[3 + i] < 0 || box[6 + i] < 0 || (long long)box[6 + i] + box[3 + i] > O[i]) return HV_ERR_ARG;
        if (region[i] < 0 || region[3 + i] < 0 || (long long)region[i] + region[3 + i] > D[i]) return HV_ERR_ARG;
    }
    const long long total = (long long)region[3] * region[4] * region[5];
    if (total == 0 || box[3] == 0 || box[4] == 0 || box[5] == 0) return HV_OK;      // nothing is covered
    if (total > 0x7fffffffLL * 64) return HV_ERR_UNSUPPORTED;
    RsArgs A;
    A.crop_ct = crop_ct; A.crop_dt = crop_dtype; A.cs0 = cs0; A.cs1 = cs1; A.cs2 = cs2;
    A.crop_lab = crop_label; A.ls0 = ls0; A.ls1 = ls1; A.ls2 = ls2;
    A.lo0 = box[0]; A.lo1 = box[1]; A.lo2 = box[2]; A.n0 = box[3]; A.n1 = box[4]; A.n2 = box[5]; A.st0 = box[6]; A.st1 = box[7]; A.st2 = box[8];
    A.plab = where == HV_RESTORE_VERTEBRA ? patient_label : nullptr; A.pdt = label_dtype; A.ps0 = ps0; A.ps1 = ps1; A.ps2 = ps2;
    A.r0 = region[0]; A.r1 = region[1]; A.r2 = region[2]; A.rn0 = region[3]; A.rn1 = region[4]; A.rn2 = region[5];
    A.where = where; A.vert_id = vert_id;
    A.out_ct = ct_out; A.os0 = os0; A.os1 = os1; A.os2 = os2;
    A.out_lab = label_out; A.qs0 = qs0; A.qs1 = qs1; A.qs2 = qs2;
    A.cov = covered; A.vs0 = vs0; A.vs1 = vs1; A.vs2 = vs2;
    A.local = local_out;
    hipStream_t s = (hipStream_t)stream;
    if (!knots) {
        hipLaunchKernelGGL(restore_uncrop_kernel, dim3(hv_cdiv(total, 256)), dim3(256), 0, s, A);
        HV_LAUNCH_CHECK();
        return HV_OK;
    }
    RsCurve cv;
    cv.knots = knots; cv.basis = basis; cv.cumlen = cumlen; cv.N = N; cv.c1 = centre1; cv.c2 = centre2;
    cv.sp0 = spacing[0]; cv.sp1 = spacing[1]; cv.sp2 = spacing[2];
    const size_t lds = (size_t)N * RS_KNOT_DOUBLES * sizeof(double);
    const int grid = hv_cdiv(total, RS_THREADS);
    if (order == 3) {
        if (lds <= RS_LDS_BYTES) hipLaunchKernelGGL((restore_kernel<true, 3>), dim3(grid), dim3(RS_THREADS), lds, s, cv, A);
        else hipLaunchKernelGGL((restore_kernel<false, 3>), dim3(grid), dim3(RS_THREADS), 0, s, cv, A);
    } else {
        if (lds <= RS_LDS_BYTES) hipLaunchKernelGGL((restore_kernel<true, 1>), dim3(grid), dim3(RS_THREADS), lds, s, cv, A);
        else hipLaunchKernelGGL((restore_kernel<false, 1>), dim3(grid), dim3(RS_THREADS), 0, s, cv, A);
    }
    HV_LAUNCH_CHECK();
    return HV_OK;
}

extern "C" int hv_restore_volume_sp(const void* crop_ct, int crop_dtype, long long cs0, long long cs1, long long cs2,
                                    const uint8_t* crop_label, long long ls0, long long ls1, long long ls2, int O0, int O1, int O2, const int* box, const double* knots,
                                 const double* basis, const double* cumlen, int N, double centre1, double centre2, const void* patient_label,
                                 int label_dtype, long long ps0, long long ps1, long long ps2, int D0, int D1, int D2, const int* region,
                                 int where, int vert_id, double* ct_out, long long os0, long long os1, long long os2, uint8_t* label_out,
                                 long long qs0, long long qs1, long long qs2, uint8_t* covered, long long vs0, long long vs1, long long vs2,
                                 double* local_out, const double* spacing, void* stream) {
    return rs_restore(1, crop_ct, crop_dtype, cs0, cs1, cs2, crop_label, ls0, ls1, ls2, O0, O1, O2, box, knots, basis, cumlen, N, centre1, centre2,
                      patient_label, label_dtype, ps0, ps1, ps2, D0, D1, D2, region, where, vert_id, ct_out, os0, os1, os2, label_out, qs0, qs1,
                      qs2, covered, vs0, vs1, vs2, local_out, spacing, stream);
}

// order 3: the CT sample is cubic, taken from `crop_coef`, hv_spline_prefilter's output for the filled sub-box of the crop alone
// ([len0][len1][len2] of the box row, contiguous); the label crop, the coverage test and the write rules are hv_restore_volume_sp's
extern "C" int hv_restore_volume_spline(const double* crop_coef, const uint8_t* crop_label, long long ls0, long long ls1, long long ls2, int O0,
                                        int O1, int O2, const int* box, const double* knots, const double* basis, const double* cumlen, int N,
                                        double centre1, double centre2, const void* patient_label, int label_dtype, long long ps0,
                                        long long ps1, long long ps2, int D0, int D1, int D2, const int* region, int where, int vert_id,
                                        double* ct_out, long long os0, long long os1, long long os2, uint8_t* label_out, long long qs0,
                                        long long qs1, long long qs2, uint8_t* covered, long long vs0, long long vs1, long long vs2,
                                        double* local_out, const double* spacing, void* stream) {
    return rs_restore(3, crop_coef, HV_DT_F64, 0, 0, 0, crop_label, ls0, ls1, ls2, O0, O1, O2, box, knots, basis, cumlen, N, centre1, centre2,
                      patient_label, label_dtype, ps0, ps1, ps2, D0, D1, D2, region, where, vert_id, ct_out, os0, os1, os2, label_out, qs0, qs1,
                      qs2, covered, vs0, vs1, vs2, local_out, spacing, stream);
}

// the entry from before the spacing: voxel indices are millimetres (x * 1.0 is exact: the same bits)
extern "C" int hv_restore_volume(const void* crop_ct, int crop_dtype, long long cs0, long long cs1, long long cs2, const uint8_t* crop_label,
                                 long long ls0, long long ls1, long long ls2, int O0, int O1, int O2, const int* box, const double* knots,
                                 const double* basis, const double* cumlen, int N, double centre1, double centre2, const void* patient_label,
                                 int label_dtype, long long ps0, long long ps1, long long ps2, int D0, int D1, int D2, const int* region,
                                 int where, int vert_id, double* ct_out, long long os0, long long os1, long long os2, uint8_t* label_out,
                                 long long qs0, long long qs1, long long qs2, uint8_t* covered, long long vs0, long long vs1, long long vs2,
                                 double* local_out, void* stream) {
    const double ones[3] = {1.0, 1.0, 1.0};
    return hv_restore_volume_sp(crop_ct, crop_dtype, cs0, cs1, cs2, crop_label, ls0, ls1, ls2, O0, O1, O2, box, knots, basis, cumlen, N, centre1,
                                centre2, patient_label, label_dtype, ps0, ps1, ps2, D0, D1, D2, region, where, vert_id, ct_out, os0, os1, os2,
                                label_out, qs0, qs1, qs2, covered, vs0, vs1, vs2, local_out, ones, stream);
}

extern "C" int hv_curve_points(const double* points, long long M, const double* knots, const double* basis, const double* cumlen, int N,
                               double centre1, double centre2, const double* spacing, int direction, double* out, void* stream) {
    if (!points || !knots || !basis || !cumlen || !out || M <= 0 || N < 2 || !rs_spacing_ok(spacing) ||
        (direction != HV_CURVE_TO_LOCAL && direction != HV_CURVE_TO_GLOBAL))
        return HV_ERR_ARG;
    if (M > 0x7fffffffLL * 64) return HV_ERR_UNSUPPORTED;
    RsCurve cv;
    cv.knots = knots; cv.basis = basis; cv.cumlen = cumlen; cv.N = N; cv.c1 = centre1; cv.c2 = centre2;
    cv.sp0 = spacing[0]; cv.sp1 = spacing[1]; cv.sp2 = spacing[2];
    const size_t lds = (size_t)N * RS_KNOT_DOUBLES * sizeof(double);
    const int grid = hv_cdiv(M, RS_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (lds <= RS_LDS_BYTES) hipLaunchKernelGGL(curve_points_kernel<true>, dim3(grid), dim3(RS_THREADS), lds, s, cv, points, M, direction, out);
    else hipLaunchKernelGGL(curve_points_kernel<false>, dim3(grid), dim3(RS_THREADS), 0, s, cv, points, M, direction, out);
    HV_LAUNCH_CHECK();
    return HV_OK;
}
