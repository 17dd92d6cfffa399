// What the samplers of resample.hip (hv_resample) and warp.hip (hv_map_coordinates, hv_warp_grid) share, so that "from the coordinate u on"
// is one piece of code: the outside rule, the taps and weights at orders 0 / 1 / 3, the four output conversions, the tile roles,
// and the host's dtype and byte-span helpers.  The definitions are in resample.hip's header comment; -ffp-contract=off throughout.
#pragma once
#include <cmath>
#include "hv_common.h"
#include "spline_tap.h"

#define RS_THREADS 256
#define RS_T 8                          // outputs per workgroup along each axis

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

// ------------------------------------------------------------------------------------------------ host side
static inline long long rs_abs(long long v) { return v < 0 ? -v : v; }
static inline bool rs_dtype_ok(int dt) { return dt == HV_DT_U8 || dt == HV_DT_I16 || dt == HV_DT_F32 || dt == HV_DT_F64; }
static inline size_t rs_elem(int dt) { return dt == HV_DT_U8 ? 1 : dt == HV_DT_I16 ? 2 : dt == HV_DT_F32 ? 4 : 8; }
// the bytes [lo, hi) a strided box of n axes touches, relative to its base pointer
static inline void rs_span(const int* A, const long long* s, size_t elem, long long* lo, long long* hi, int n = 3) {
    long long mn = 0, mx = 0;
    for (int a = 0; a < n; ++a) {
        const long long e = (long long)(A[a] - 1) * s[a];
        if (e < 0) mn += e; else mx += e;
    }
    *lo = mn * (long long)elem;
    *hi = (mx + 1) * (long long)elem;
}
// do the bytes of two boxes intersect?
static inline bool rs_meet(const void* a, long long alo, long long ahi, const void* b, long long blo, long long bhi) {
    return (intptr_t)a + alo < (intptr_t)b + bhi && (intptr_t)b + blo < (intptr_t)a + ahi;
}

// The refusals every sampler shares, in two steps so that an entry can put its own HV_ERR_ARG checks between them.  First HV_ERR_ARG: a NULL
// pointer, a non-positive extent, an unknown dtype, order or mode, a cval that is not finite or not a value of an integer out_dtype, order 3
// on anything but float64, a pointer not aligned to its element.
static inline int rs_check_args(const void* vol, int dtype, const int* A, const void* out, int out_dtype, const int* O, int order, int mode,
                                double cval) {
    if (!vol || !out || A[0] <= 0 || A[1] <= 0 || A[2] <= 0 || O[0] <= 0 || O[1] <= 0 || O[2] <= 0 || !rs_dtype_ok(dtype) ||
        !rs_dtype_ok(out_dtype))
        return HV_ERR_ARG;
    if ((order != 0 && order != 1 && order != 3) || mode < HV_FILT_REFLECT || mode > HV_FILT_WRAP || !std::isfinite(cval)) return HV_ERR_ARG;
    if (out_dtype == HV_DT_U8 || out_dtype == HV_DT_I16) {
        const double lo = out_dtype == HV_DT_U8 ? 0.0 : -32768.0, hi = out_dtype == HV_DT_U8 ? 255.0 : 32767.0;
        if (cval < lo || cval > hi || cval != std::floor(cval)) return HV_ERR_ARG;
    }
    if (order == 3 && dtype != HV_DT_F64) return HV_ERR_ARG;               // order 3 samples coefficients, and those are doubles
    if (((uintptr_t)vol & (rs_elem(dtype) - 1)) || ((uintptr_t)out & (rs_elem(out_dtype) - 1))) return HV_ERR_ARG;
    return HV_OK;
}
// Then HV_ERR_UNSUPPORTED: the modes not built -- mirror / reflect / wrap; nearest above order 0 (order 1: scipy's edge rule is not a clamp;
// order 3: its 12-voxel pre-padding) -- and more than 2^30 voxels on either side; and HV_ERR_ARG for out intersecting vol.
static inline int rs_check_support(const void* vol, int dtype, const int* A, const long long* ss, const void* out, int out_dtype, const int* O,
                                   const long long* os, int order, int mode) {
    if (mode != HV_FILT_CONSTANT && !(mode == HV_FILT_NEAREST && order == 0)) return HV_ERR_UNSUPPORTED;
    if ((long long)A[0] * A[1] * A[2] > (1LL << 30) || (long long)O[0] * O[1] * O[2] > (1LL << 30)) return HV_ERR_UNSUPPORTED;
    long long vlo, vhi, olo, ohi;
    rs_span(A, ss, rs_elem(dtype), &vlo, &vhi);
    rs_span(O, os, rs_elem(out_dtype), &olo, &ohi);
    return rs_meet(vol, vlo, vhi, out, olo, ohi) ? HV_ERR_ARG : HV_OK;
}
// the lattice of a descriptor: a known form, and every field finite whatever the form
static inline bool rs_desc_ok(const hv_resample_desc& D) {
    bool ok = D.form == HV_RESAMPLE_MATRIX || D.form == HV_RESAMPLE_ZOOMSHIFT;
    for (int i = 0; i < 9; ++i) ok = ok && std::isfinite(D.matrix[i]);
    for (int i = 0; i < 3; ++i) ok = ok && std::isfinite(D.offset[i]) && std::isfinite(D.zoom[i]) && std::isfinite(D.shift[i]);
    return ok;
}
// img[j]: how far a unit step along output axis j moves in the source, in elements
static inline void rs_image(const hv_resample_desc& D, const long long* ss, double* img) {
    for (int j = 0; j < 3; ++j) {
        if (D.form == HV_RESAMPLE_MATRIX) {
            img[j] = 0.0;
            for (int h = 0; h < 3; ++h) img[j] += std::fabs(D.matrix[3 * h + j]) * (double)rs_abs(ss[h]);
        } else {
            img[j] = std::fabs(D.zoom[j]) * (double)rs_abs(ss[j]);
        }
    }
}

// the roles of the three output axes: L the axis with the smallest key (an axis of extent 1 comes last; ties: the later axis), then M, then O.
// ord[r] = the axis with role r.
static inline void rs_roles(const int* O, const double* key, int* ord) {
    ord[0] = 0; ord[1] = 1; ord[2] = 2;
    auto before = [&](int a, int b) {
        if ((O[a] > 1) != (O[b] > 1)) return O[a] > 1;
        if (key[a] != key[b]) return key[a] < key[b];
        return a > b;
    };
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2 - i; ++j)
            if (before(ord[j + 1], ord[j])) { const int t = ord[j]; ord[j] = ord[j + 1]; ord[j + 1] = t; }
}
