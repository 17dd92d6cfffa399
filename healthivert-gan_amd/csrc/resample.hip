// 3-D affine resampling on the device: hv_resample -- scipy.ndimage.affine_transform, zoom and shift of a volume
// onto a lattice given by a matrix and an offset (HV_RESAMPLE_MATRIX) or by a per-axis zoom and shift (HV_RESAMPLE_ZOOMSHIFT, scipy's
// zoom_shift), at spline order 0, 1 or 3.  The definitions are NI_GeometricTransform's / NI_ZoomShift's, in float64 and in scipy's order of
// operations (-ffp-contract=off: no fused multiply-add), so that the bytes are scipy's:
//   coordinates  matrix form      u_h = ((o0 m[h][0] + o1 m[h][1]) + o2 m[h][2]) + offset[h]   (products summed from 0.0, the offset last)
//                zoom-shift form  u_h = (o_h + shift[h]) * zoom[h]
//   outside      mode constant: u_h < 0 or u_h > A_h - 1 on any axis gives cval; mode nearest (order 0 only): u_h clamped to [0, A_h - 1]
//   taps         order 0: floor(u + 0.5), no weight; order 1: floor(u), floor(u) + 1 with w0 = 1 - y, w1 = 1 - w0 (scipy forms the last
//                weight as one minus the others); order 3: hv_spline_taps (spline_tap.h) on the float64 coefficients hv_spline_prefilter
//                leaves.  Tap indices beyond the ends are mirrored about the end points (hv_spline_mirror).
//   sum          over the taps, last axis fastest, each term ((c w0) w1) w2, added from 0.0: hv_spline_sample's loop on strided sources
//   output       float64 as it is; float32 rounded once; int16 t > 0 ? t + 0.5 : t - 0.5, clamped, truncated; uint8 t > 0 ? t + 0.5 : 0
//
// One kernel template over source dtype x order, one launch.  A workgroup of 256 lanes owns a tile of RS_T^3 outputs whatever the strides
// (hv_resample_tile reports RS_T for every axis): the lanes run along the output axis whose image in the source has the smallest stride
// (role L), eight of them, then along the next (M); each lane computes two outputs RS_T / 2 apart along the third (O), one after the other.
// Every lane computes its own coordinates and weights in both forms: next to the 4 x 4 x 4 gathers and their 192 multiplies that is a small
// part, and the one code path keeps the two forms' arithmetic identical.  The descriptor travels in the kernel arguments.  No atomics, no
// workspace, no LDS, no scratch, no workgroup waits for another; every index is formed from a coordinate already tested (or clamped) to lie
// in [0, A - 1] -- a NaN coordinate fails the test and counts as outside -- so nothing outside the source box is read.
#include <cmath>
#include "hv_common.h"
#include "spline_tap.h"

#define RS_THREADS 256
#define RS_T 8                          // outputs per workgroup along each axis

struct RsP {
    const void* src; void* dst;
    long long s0, s1, s2, d0, d1, d2;   // element strides by HOST axis
    int A0, A1, A2, O0, O1, O2;
    int r0, r1, r2;                     // the role (0 = L, 1 = M, 2 = O) of host output axis 0 / 1 / 2
    int nL, nM, nO;                     // the output extents by role
    int dst_dt;
    hv_resample_desc D;
};

template <typename T>
__device__ __forceinline__ double rs_ld(const T* p, long long o) { return (double)p[o]; }

// the coordinate along one axis against the outside rule: false = outside (constant mode); nearest clamps
__device__ __forceinline__ bool rs_inside(double& u, int n, int mode) {
    const double hi = (double)(n - 1);
    if (mode == HV_FILT_NEAREST) {
        u = u >= 0.0 ? (u <= hi ? u : hi) : 0.0;
        return true;
    }
    return u >= 0.0 && u <= hi;         // false for a NaN
}

template <int ORDER>
__device__ __forceinline__ void rs_taps(double u, int n, long long s, long long (&o)[ORDER + 1], double (&w)[ORDER + 1]) {
    if constexpr (ORDER == 0) {
        o[0] = (long long)floor(u + 0.5) * s;
        w[0] = 1.0;
    } else if constexpr (ORDER == 1) {
        const double f = floor(u);
        w[0] = 1.0 - (u - f);
        w[1] = 1.0 - w[0];
        const long long i = (long long)f;
        o[0] = i * s;                   // 0 <= i <= n - 1
        o[1] = hv_spline_mirror(i + 1, n) * s;
    } else {
        hv_spline_taps(u, n, s, o, w);
    }
}

__device__ __forceinline__ void rs_store(void* dst, int dt, long long off, double t) {
    switch (dt) {
        case HV_DT_F64: ((double*)dst)[off] = t; break;
        case HV_DT_F32: ((float*)dst)[off] = (float)t; break;
        case HV_DT_I16: {
            t = t > 0.0 ? t + 0.5 : t - 0.5;
            t = t > 32767.0 ? 32767.0 : t;
            t = t < -32768.0 ? -32768.0 : t;
            ((int16_t*)dst)[off] = (int16_t)(int)t;
            break;
        }
        default: {
            t = t > 0.0 ? t + 0.5 : 0.0;
            t = t > 255.0 ? 255.0 : t;
            ((uint8_t*)dst)[off] = (uint8_t)(int)t;
            break;
        }
    }
}

__device__ __forceinline__ int rs_pick(int role, int gL, int gM, int gO) { return role == 0 ? gL : role == 1 ? gM : gO; }

// grid: the tiles, the one along L fastest
template <typename T, int ORDER>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(RsP P) {
    constexpr int NT = ORDER + 1;
    const int ntL = (P.nL + RS_T - 1) / RS_T, ntM = (P.nM + RS_T - 1) / RS_T;
    const int tL = (int)(blockIdx.x % ntL), tM = (int)((blockIdx.x / ntL) % ntM), tO = (int)(blockIdx.x / ((unsigned)ntL * ntM));
    const int gL = tL * RS_T + (int)(threadIdx.x % RS_T), gM = tM * RS_T + (int)((threadIdx.x / RS_T) % RS_T);
    if (gL >= P.nL || gM >= P.nM) return;
    const T* src = reinterpret_cast<const T*>(P.src);
    const hv_resample_desc& D = P.D;
#pragma unroll 1
    for (int rep = 0; rep < 2; ++rep) {
        const int gO = tO * RS_T + (int)(threadIdx.x / (RS_T * RS_T)) + rep * (RS_T / 2);
        if (gO >= P.nO) return;
        const int i0 = rs_pick(P.r0, gL, gM, gO), i1 = rs_pick(P.r1, gL, gM, gO), i2 = rs_pick(P.r2, gL, gM, gO);
        const double c0 = (double)i0, c1 = (double)i1, c2 = (double)i2;
        double u0, u1, u2;
        if (D.form == HV_RESAMPLE_MATRIX) {
            u0 = (((0.0 + c0 * D.matrix[0]) + c1 * D.matrix[1]) + c2 * D.matrix[2]) + D.offset[0];
            u1 = (((0.0 + c0 * D.matrix[3]) + c1 * D.matrix[4]) + c2 * D.matrix[5]) + D.offset[1];
            u2 = (((0.0 + c0 * D.matrix[6]) + c1 * D.matrix[7]) + c2 * D.matrix[8]) + D.offset[2];
        } else {
            u0 = (c0 + D.shift[0]) * D.zoom[0];
            u1 = (c1 + D.shift[1]) * D.zoom[1];
            u2 = (c2 + D.shift[2]) * D.zoom[2];
        }
        const bool in0 = rs_inside(u0, P.A0, D.mode), in1 = rs_inside(u1, P.A1, D.mode), in2 = rs_inside(u2, P.A2, D.mode);
        double t = D.cval;
        if (in0 && in1 && in2) {
            long long o0[NT], o1[NT], o2[NT];
            double w0[NT], w1[NT], w2[NT];
            rs_taps<ORDER>(u0, P.A0, P.s0, o0, w0);
            rs_taps<ORDER>(u1, P.A1, P.s1, o1, w1);
            rs_taps<ORDER>(u2, P.A2, P.s2, o2, w2);
            t = 0.0;
#pragma unroll
            for (int a = 0; a < NT; ++a)
#pragma unroll
                for (int b = 0; b < NT; ++b) {
                    const long long ob = o0[a] + o1[b];
#pragma unroll
                    for (int c = 0; c < NT; ++c) {
                        const double v = rs_ld(src, ob + o2[c]);
                        if constexpr (ORDER == 0) t += v;
                        else t += ((v * w0[a]) * w1[b]) * w2[c];
                    }
                }
        }
        rs_store(P.dst, P.dst_dt, i0 * P.d0 + i1 * P.d1 + i2 * P.d2, t);
    }
}

// ------------------------------------------------------------------------------------------------ host side
static inline long long rs_abs(long long v) { return v < 0 ? -v : v; }
static inline bool rs_dtype_ok(int dt) { return dt == HV_DT_U8 || dt == HV_DT_I16 || dt == HV_DT_F32 || dt == HV_DT_F64; }
static inline size_t rs_elem(int dt) { return dt == HV_DT_U8 ? 1 : dt == HV_DT_I16 ? 2 : dt == HV_DT_F32 ? 4 : 8; }
// the bytes [lo, hi) a strided box touches, relative to its base pointer
static void rs_span(const int* A, const long long* s, size_t elem, long long* lo, long long* hi) {
    long long mn = 0, mx = 0;
    for (int a = 0; a < 3; ++a) {
        const long long e = (long long)(A[a] - 1) * s[a];
        if (e < 0) mn += e; else mx += e;
    }
    *lo = mn * (long long)elem;
    *hi = (mx + 1) * (long long)elem;
}

template <typename T>
static void rs_launch(int order, dim3 grid, hipStream_t st, const RsP& P) {
    if (order == 0) hipLaunchKernelGGL((resample_kernel<T, 0>), grid, dim3(RS_THREADS), 0, st, P);
    else if (order == 1) hipLaunchKernelGGL((resample_kernel<T, 1>), grid, dim3(RS_THREADS), 0, st, P);
}
static void rs_launch_coef(dim3 grid, hipStream_t st, const RsP& P) {
    hipLaunchKernelGGL((resample_kernel<double, 3>), grid, dim3(RS_THREADS), 0, st, P);
}

extern "C" int hv_resample_tile(int* dims) {
    if (!dims) return HV_ERR_ARG;
    dims[0] = dims[1] = dims[2] = RS_T;
    return HV_OK;
}

extern "C" int hv_resample(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, void* out,
                           int out_dtype, long long os0, long long os1, long long os2, int O0, int O1, int O2, const hv_resample_desc* desc,
                           void* stream) {
    if (!vol || !out || !desc || A0 <= 0 || A1 <= 0 || A2 <= 0 || O0 <= 0 || O1 <= 0 || O2 <= 0 || !rs_dtype_ok(dtype) ||
        !rs_dtype_ok(out_dtype))
        return HV_ERR_ARG;
    const hv_resample_desc& D = *desc;
    if ((D.form != HV_RESAMPLE_MATRIX && D.form != HV_RESAMPLE_ZOOMSHIFT) || (D.order != 0 && D.order != 1 && D.order != 3) ||
        D.mode < HV_FILT_REFLECT || D.mode > HV_FILT_WRAP)
        return HV_ERR_ARG;
    bool finite = std::isfinite(D.cval);
    for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(D.matrix[i]);
    for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(D.offset[i]) && std::isfinite(D.zoom[i]) && std::isfinite(D.shift[i]);
    if (!finite) return HV_ERR_ARG;
    if (out_dtype == HV_DT_U8 || out_dtype == HV_DT_I16) {
        const double lo = out_dtype == HV_DT_U8 ? 0.0 : -32768.0, hi = out_dtype == HV_DT_U8 ? 255.0 : 32767.0;
        if (D.cval < lo || D.cval > hi || D.cval != std::floor(D.cval)) return HV_ERR_ARG;
    }
    if (D.order == 3 && dtype != HV_DT_F64) return HV_ERR_ARG;             // order 3 samples coefficients, and those are doubles
    if (((uintptr_t)vol & (rs_elem(dtype) - 1)) || ((uintptr_t)out & (rs_elem(out_dtype) - 1))) return HV_ERR_ARG;
    // the modes not built: mirror / reflect / wrap; nearest above order 0 (order 1: scipy's edge rule is not a clamp; order 3: its 12-voxel
    // pre-padding)
    if (D.mode != HV_FILT_CONSTANT && !(D.mode == HV_FILT_NEAREST && D.order == 0)) return HV_ERR_UNSUPPORTED;
    if ((long long)A0 * A1 * A2 > (1LL << 30) || (long long)O0 * O1 * O2 > (1LL << 30)) return HV_ERR_UNSUPPORTED;
    const int A[3] = {A0, A1, A2}, O[3] = {O0, O1, O2};
    const long long ss[3] = {s0, s1, s2}, os[3] = {os0, os1, os2};
    long long vlo, vhi, olo, ohi;
    rs_span(A, ss, rs_elem(dtype), &vlo, &vhi);
    rs_span(O, os, rs_elem(out_dtype), &olo, &ohi);
    if ((intptr_t)vol + vlo < (intptr_t)out + ohi && (intptr_t)out + olo < (intptr_t)vol + vhi) return HV_ERR_ARG;
    // the roles: L the output axis whose unit step moves least far in the source (an axis of extent 1 comes last), then M, then O
    double img[3];
    for (int j = 0; j < 3; ++j) {
        if (D.form == HV_RESAMPLE_MATRIX) {
            img[j] = 0.0;
            for (int h = 0; h < 3; ++h) img[j] += std::fabs(D.matrix[3 * h + j]) * (double)rs_abs(ss[h]);
        } else {
            img[j] = std::fabs(D.zoom[j]) * (double)rs_abs(ss[j]);
        }
    }
    int ord[3] = {0, 1, 2};
    auto before = [&](int a, int b) {
        if ((O[a] > 1) != (O[b] > 1)) return O[a] > 1;
        if (img[a] != img[b]) return img[a] < img[b];
        return a > b;
    };
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2 - i; ++j)
            if (before(ord[j + 1], ord[j])) { const int t = ord[j]; ord[j] = ord[j + 1]; ord[j + 1] = t; }
    RsP P;
    P.src = vol; P.dst = out;
    P.s0 = s0; P.s1 = s1; P.s2 = s2; P.d0 = os0; P.d1 = os1; P.d2 = os2;
    P.A0 = A0; P.A1 = A1; P.A2 = A2; P.O0 = O0; P.O1 = O1; P.O2 = O2;
    int role[3];
    for (int r = 0; r < 3; ++r) role[ord[r]] = r;
    P.r0 = role[0]; P.r1 = role[1]; P.r2 = role[2];
    P.nL = O[ord[0]]; P.nM = O[ord[1]]; P.nO = O[ord[2]];
    P.dst_dt = out_dtype;
    P.D = D;
    const long long blocks = (long long)hv_cdiv(O0, RS_T) * hv_cdiv(O1, RS_T) * hv_cdiv(O2, RS_T);
    const dim3 grid((unsigned)blocks);
    hipStream_t st = (hipStream_t)stream;
    if (D.order == 3) rs_launch_coef(grid, st, P);
    else switch (dtype) {
        case HV_DT_U8: rs_launch<uint8_t>(D.order, grid, st, P); break;
        case HV_DT_I16: rs_launch<int16_t>(D.order, grid, st, P); break;
        case HV_DT_F32: rs_launch<float>(D.order, grid, st, P); break;
        default: rs_launch<double>(D.order, grid, st, P); break;
    }
    HV_LAUNCH_CHECK();
    return HV_OK;
}
