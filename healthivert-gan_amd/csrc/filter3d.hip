// Separable linear filtering of a volume on the device: hv_separable_filter -- scipy.ndimage.correlate1d along up to
// three axes, which with Gaussian weights is gaussian_filter1d / gaussian_filter, derivative orders included -- and hv_blend_lerp, the weighted
// composite of two volumes.  The weights come from the host inside the kernel arguments (hv_filter_axis, one struct per launch); the arithmetic
// is float64 and is NI_Correlate1D's, operation for operation, so the doubles equal scipy's on the float64 copy of the input bit for bit:
//     symmetric      t = x[c] w[r];  for ii = -r .. -1:  t += (x[c + ii] + x[c - ii]) w[ii + r]
//     antisymmetric  the same with    (x[c + ii] - x[c - ii])
//     general        t = x[c + r] w[2r];  for ii = 0 .. 2r - 1:  t += x[c - r + ii] w[ii]       (scipy starts with the LAST tap)
// x is the line extended through the boundary map (reflect / constant / nearest / mirror / wrap, defined for any offset), c the output's place
// in it.  The file is compiled with -ffp-contract=off and states it again below: no fma, no reassociation.
//
// One launch per filtered axis, in the order 0, 1, 2; each pass reads the doubles the pass before wrote.  The first pass reads the caller's
// volume through its strides and converts (HV_FILT_IN_VALUE) or forms the indicator vol == value (HV_FILT_IN_EQ); the last pass writes through
// out's strides, either the double or, for a uint8 out, the byte t >= threshold, so that the doubles of the last pass are never stored.  The
// passes between use C-ordered double volumes: for a float64 out they alternate between out and the workspace (ending in out), for a uint8 out
// between two volumes of the workspace.
//
// Two kernels, told apart by whether the filtered axis is the one the lanes run along (the axis of the smallest stride of what the pass reads):
//   filt_cross_kernel   the filtered axis is NOT the lane axis.  A workgroup stages [FI_T + 2r rows along the filtered axis][32 columns along
//                       the lane axis] doubles in LDS -- consecutive lanes read consecutive unit-stride elements, the halo rows come through
//                       the boundary map -- and each lane sums FI_T / 8 outputs of its column.
//   filt_along_kernel   the filtered axis IS the lane axis.  A workgroup stages FI_T + 2r elements of FI_LN line segments; a wave sums the 64
//                       outputs of one segment from consecutive LDS addresses.
// A line is tiled by FI_T outputs, so its length is not limited by LDS.  No workgroup waits for another, no atomics, no host synchronisation, no
// scratch; every double of the workspace that is read was written by an earlier launch of the same call.
#include <cmath>
#include "volume_access.h"                  // hv_up16
#include "boundary_map.h"

#pragma clang fp contract(off)

#define FI_THREADS 256
#define FI_T 64                        // outputs per tile along the filtered axis (both kernels)
#define FI_COLS 32                     // columns per tile of the cross pass
#define FI_ROWG (FI_THREADS / FI_COLS)
#define FI_LN 16                       // line segments per workgroup of the along pass
#define FI_OUT_F64 0
#define FI_OUT_THR 1

// one pass as the kernels see it: the roles F (filtered), L (lanes) and O (the third axis) are the host's permutation of the axes
struct FiPass {
    const void* src; int dt, in_eq; double value;          // dt: HV_DT_*; in_eq: the indicator src == value instead of the value
    long long sF, sL, sO;
    void* dst; int out_kind; double threshold;
    long long dF, dL, dO;
    int nF, nL, nO;
    int mode; double cval;
};

__device__ __forceinline__ double fi_load(const FiPass& P, long long o) {
    double v;
    switch (P.dt) {
        case HV_DT_U8: v = (double)((const uint8_t*)P.src)[o]; break;
        case HV_DT_I16: v = (double)((const short*)P.src)[o]; break;
        case HV_DT_F32: v = (double)((const float*)P.src)[o]; break;
        default: v = ((const double*)P.src)[o]; break;
    }
    return P.in_eq ? (v == P.value ? 1.0 : 0.0) : v;
}
__device__ __forceinline__ void fi_store(const FiPass& P, long long o, double t) {
    if (P.out_kind == FI_OUT_THR) ((uint8_t*)P.dst)[o] = (uint8_t)(t >= P.threshold ? 1 : 0);
    else ((double*)P.dst)[o] = t;
}
// (fi_map, the index in [0, n) that position p of the extended line reads, -1 for cval: boundary_map.h)
// the sum of one output: x points at the output's own element of the staged line, consecutive elements of the line `st` doubles apart
__device__ __forceinline__ double fi_sum(const double* x, int st, const hv_filter_axis& W) {
    const int r = W.radius;
    double t;
    if (W.form > 0) {
        t = x[0] * W.w[r];
        for (int ii = -r; ii < 0; ++ii) t = t + (x[ii * st] + x[-ii * st]) * W.w[ii + r];
    } else if (W.form < 0) {
        t = x[0] * W.w[r];
        for (int ii = -r; ii < 0; ++ii) t = t + (x[ii * st] - x[-ii * st]) * W.w[ii + r];
    } else {
        t = x[r * st] * W.w[2 * r];
        for (int ii = 0; ii < 2 * r; ++ii) t = t + x[(ii - r) * st] * W.w[ii];
    }
    return t;
}

// grid: nO x (tiles along F) x (column tiles along L), the column tile fastest
__global__ __launch_bounds__(FI_THREADS) void filt_cross_kernel(FiPass P, hv_filter_axis W) {
    extern __shared__ double fi_lds[];
    const int r = W.radius;
    const int nct = (P.nL + FI_COLS - 1) / FI_COLS, nft = (P.nF + FI_T - 1) / FI_T;
    const int ct = (int)(blockIdx.x % nct), ft = (int)((blockIdx.x / nct) % nft), o = (int)(blockIdx.x / ((unsigned)nct * nft));
    if (o >= P.nO) return;
    const int f0 = ft * FI_T, tl = min(FI_T, P.nF - f0);
    const int col = threadIdx.x % FI_COLS, rg = threadIdx.x / FI_COLS, l = ct * FI_COLS + col;
    const bool live = l < P.nL;
    const long long sb = o * P.sO + l * P.sL;
    for (int row = rg; row < tl + 2 * r; row += FI_ROWG) {
        const int idx = fi_map(f0 - r + row, P.nF, P.mode);
        fi_lds[row * FI_COLS + col] = !live ? 0.0 : (idx < 0 ? P.cval : fi_load(P, sb + idx * P.sF));
    }
    __syncthreads();
    if (!live) return;
    const long long db = o * P.dO + l * P.dL;
    for (int j = rg; j < tl; j += FI_ROWG) fi_store(P, db + (f0 + j) * P.dF, fi_sum(fi_lds + (j + r) * FI_COLS + col, FI_COLS, W));
}

// lines are numbered o * nL + q (q along the role L: here the faster of the two axes that are not filtered); grid: line groups x tiles along F
__global__ __launch_bounds__(FI_THREADS) void filt_along_kernel(FiPass P, hv_filter_axis W) {
    extern __shared__ double fi_lds[];
    const int r = W.radius;
    const int nft = (P.nF + FI_T - 1) / FI_T;
    const int ft = (int)(blockIdx.x % nft);
    const long long line0 = (long long)(blockIdx.x / nft) * FI_LN, nlines = (long long)P.nO * P.nL;
    if (line0 >= nlines) return;
    const int cnt = (int)min((long long)FI_LN, nlines - line0);
    const int f0 = ft * FI_T, tl = min(FI_T, P.nF - f0), wd = tl + 2 * r;
    for (int e = threadIdx.x; e < cnt * wd; e += FI_THREADS) {
        const int ln = e / wd, row = e % wd;
        const long long L = line0 + ln;
        const int idx = fi_map(f0 - r + row, P.nF, P.mode);
        fi_lds[e] = idx < 0 ? P.cval : fi_load(P, (L / P.nL) * P.sO + (L % P.nL) * P.sL + idx * P.sF);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < cnt * tl; e += FI_THREADS) {
        const int ln = e / tl, j = e % tl;
        const long long L = line0 + ln;
        fi_store(P, (L / P.nL) * P.dO + (L % P.nL) * P.dL + (f0 + j) * P.dF, fi_sum(fi_lds + ln * wd + j + r, 1, W));
    }
}

// ------------------------------------------------------------------------------------------------ the composite
struct FiBlend {
    const void* a; const void* b; const void* w; double* out;
    int a_dt, b_dt, w_dt;
    long long a_s[3], b_s[3], w_s[3], o_s[3];      // in the order of n[]: n[2] runs along the lanes
    int n[3];
};
__device__ __forceinline__ double fi_value(const void* p, int dt, long long o) {
    switch (dt) {
        case HV_DT_U8: return ((const uint8_t*)p)[o] != 0 ? 1.0 : 0.0;          // a mask (w only)
        case HV_DT_I16: return (double)((const short*)p)[o];
        case HV_DT_F32: return (double)((const float*)p)[o];
        default: return ((const double*)p)[o];
    }
}
__global__ __launch_bounds__(FI_THREADS) void blend_lerp_kernel(FiBlend B, long long N) {
    const long long p = (long long)blockIdx.x * FI_THREADS + threadIdx.x;
    if (p >= N) return;
    const int k = (int)(p % B.n[2]), j = (int)((p / B.n[2]) % B.n[1]), i = (int)(p / ((long long)B.n[2] * B.n[1]));
    const double w = fi_value(B.w, B.w_dt, i * B.w_s[0] + j * B.w_s[1] + k * B.w_s[2]);
    const double a = fi_value(B.a, B.a_dt, i * B.a_s[0] + j * B.a_s[1] + k * B.a_s[2]);
    const double b = fi_value(B.b, B.b_dt, i * B.b_s[0] + j * B.b_s[1] + k * B.b_s[2]);
    B.out[i * B.o_s[0] + j * B.o_s[1] + k * B.o_s[2]] = ((1.0 - w) * a) + (w * b);
}

// ------------------------------------------------------------------------------------------------ host side
static inline bool fi_dims_ok(int A0, int A1, int A2) { return A0 > 0 && A1 > 0 && A2 > 0; }
static inline bool fi_in_dtype_ok(int dt) { return dt == HV_DT_U8 || dt == HV_DT_I16 || dt == HV_DT_F32 || dt == HV_DT_F64; }
static inline size_t fi_elem(int dt) { return dt == HV_DT_U8 ? 1 : dt == HV_DT_I16 ? 2 : dt == HV_DT_F32 ? 4 : 8; }
static inline long long fi_abs(long long v) { return v < 0 ? -v : v; }
// HV_OK, or why the three descriptors are refused; *passes = the axes that are filtered
static int fi_axes_check(const hv_filter_axis* axes, int* passes) {
    if (!axes) return HV_ERR_ARG;
    int n = 0;
    for (int a = 0; a < 3; ++a) {
        const hv_filter_axis& X = axes[a];
        if (X.radius < 0) continue;
        if (X.radius > HV_FILT_MAX_RADIUS) return HV_ERR_UNSUPPORTED;
        if (X.form < -1 || X.form > 1) return HV_ERR_ARG;
        for (int t = 0; t <= 2 * X.radius; ++t)
            if (!std::isfinite(X.w[t])) return HV_ERR_ARG;
        ++n;
    }
    *passes = n;
    return HV_OK;
}
// the bytes [lo, hi) a strided box touches, relative to its base pointer
static void fi_span(const int* A, const long long* s, size_t elem, long long* lo, long long* hi) {
    long long mn = 0, mx = 0;
    for (int a = 0; a < 3; ++a) {
        const long long e = (long long)(A[a] - 1) * s[a];
        if (e < 0) mn += e; else mx += e;
    }
    *lo = mn * (long long)elem;
    *hi = (mx + 1) * (long long)elem;
}
static bool fi_overlap(const void* p, const int* A, const long long* ps, size_t pe, const void* q, const long long* qs, size_t qe) {
    long long plo, phi, qlo, qhi;
    fi_span(A, ps, pe, &plo, &phi);
    fi_span(A, qs, qe, &qlo, &qhi);
    const intptr_t P = (intptr_t)p, Q = (intptr_t)q;
    return P + plo < Q + qhi && Q + qlo < P + phi;
}

extern "C" int hv_filter_tile(int* dims) {
    if (!dims) return HV_ERR_ARG;
    dims[0] = dims[1] = dims[2] = FI_T;
    return HV_OK;
}

extern "C" size_t hv_filter_workspace_bytes(int A0, int A1, int A2, const hv_filter_axis* axes) {
    int passes = 0;
    if (!fi_dims_ok(A0, A1, A2) || (long long)A0 * A1 * A2 > (1LL << 30) || fi_axes_check(axes, &passes) != HV_OK) return 0;
    const size_t vol = hv_up16((size_t)A0 * A1 * A2 * sizeof(double));
    return passes <= 1 ? 16 : (size_t)(passes - 1) * vol;       // a uint8 out keeps both volumes between three passes; a float64 out needs one
}

// queue one pass along axis f: the lanes run along the axis of the smallest source stride
static int fi_launch(const void* src, int dt, int in_eq, double value, const long long* ss, void* dst, int out_kind, double threshold,
                     const long long* ds, const int* A, int f, const hv_filter_axis& W, int mode, double cval, hipStream_t st) {
    int l = -1;                                      // (an axis of extent 1 has no stride to speak of: it is taken only if all are such)
    for (int a = 0; a < 3; ++a)
        if (A[a] > 1 && (l < 0 || fi_abs(ss[a]) < fi_abs(ss[l]))) l = a;
    if (l < 0) l = 2;
    FiPass P;
    P.src = src; P.dt = dt; P.in_eq = in_eq; P.value = value; P.dst = dst; P.out_kind = out_kind; P.threshold = threshold;
    P.mode = mode; P.cval = cval;
    P.nF = A[f]; P.sF = ss[f]; P.dF = ds[f];
    const int nft = hv_cdiv(A[f], FI_T);
    if (l != f) {
        const int o = 3 - f - l;
        P.nL = A[l]; P.sL = ss[l]; P.dL = ds[l];
        P.nO = A[o]; P.sO = ss[o]; P.dO = ds[o];
        const long long blocks = (long long)A[o] * nft * hv_cdiv(A[l], FI_COLS);
        const size_t lds = (size_t)(FI_T + 2 * W.radius) * FI_COLS * sizeof(double);
        hipLaunchKernelGGL(filt_cross_kernel, dim3((unsigned)blocks), dim3(FI_THREADS), lds, st, P, W);
    } else {
        int q = f == 2 ? 1 : 2, o = f == 0 ? 1 : 0;              // the two other axes; q, the faster in the source, numbers the lines fastest
        if (fi_abs(ss[o]) < fi_abs(ss[q])) { const int t = q; q = o; o = t; }
        P.nL = A[q]; P.sL = ss[q]; P.dL = ds[q];
        P.nO = A[o]; P.sO = ss[o]; P.dO = ds[o];
        const long long blocks = (long long)hv_cdiv((long long)A[q] * A[o], FI_LN) * nft;
        const size_t lds = (size_t)(FI_T + 2 * W.radius) * FI_LN * sizeof(double);
        hipLaunchKernelGGL(filt_along_kernel, dim3((unsigned)blocks), dim3(FI_THREADS), lds, st, P, W);
    }
    HV_LAUNCH_CHECK();
    return HV_OK;
}

extern "C" int hv_separable_filter(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, int in_mode,
                                   double value, const hv_filter_axis* axes, int mode, double cval, void* out, int out_dtype, double threshold,
                                   long long os0, long long os1, long long os2, void* workspace, size_t workspace_bytes, void* stream) {
    if (!vol || !out || !workspace || !axes || !fi_dims_ok(A0, A1, A2) || !fi_in_dtype_ok(dtype) ||
        (in_mode != HV_FILT_IN_VALUE && in_mode != HV_FILT_IN_EQ) || mode < HV_FILT_REFLECT || mode > HV_FILT_WRAP || !std::isfinite(cval) ||
        (out_dtype != HV_DT_F64 && out_dtype != HV_DT_U8) || ((uintptr_t)workspace & 15) || (out_dtype == HV_DT_F64 && ((uintptr_t)out & 7)))
        return HV_ERR_ARG;
    int passes = 0;
    const int rc = fi_axes_check(axes, &passes);
    if (rc != HV_OK) return rc;
    if ((long long)A0 * A1 * A2 > (1LL << 30)) return HV_ERR_UNSUPPORTED;
    if (workspace_bytes < hv_filter_workspace_bytes(A0, A1, A2, axes)) return HV_ERR_ARG;
    const int A[3] = {A0, A1, A2};
    const long long ss[3] = {s0, s1, s2}, os[3] = {os0, os1, os2}, cs[3] = {(long long)A1 * A2, A2, 1};
    if (fi_overlap(vol, A, ss, fi_elem(dtype), out, os, fi_elem(out_dtype))) return HV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const bool thr = out_dtype == HV_DT_U8;
    const int kind = thr ? FI_OUT_THR : FI_OUT_F64;
    if (passes == 0) {                               // the converted (or thresholded) input: one tap of weight 1, x * 1.0 is x
        hv_filter_axis I;
        I.radius = 0; I.form = 1; I.w[0] = 1.0;
        return fi_launch(vol, dtype, in_mode == HV_FILT_IN_EQ, value, ss, out, kind, threshold, os, A, 2, I, mode, cval, st);
    }
    double* wsv[2] = {(double*)workspace, (double*)((char*)workspace + hv_up16((size_t)A0 * A1 * A2 * sizeof(double)))};
    const void* src = vol;
    const long long* sst = ss;
    int sdt = dtype, seq = in_mode == HV_FILT_IN_EQ, done = 0;
    for (int a = 0; a < 3; ++a) {
        if (axes[a].radius < 0) continue;
        const int left = passes - done - 1;           // passes after this one
        void* dst;
        const long long* dst_s = cs;
        if (left == 0) { dst = out; dst_s = os; }
        else if (thr) dst = wsv[done & 1];
        else if (left & 1) dst = wsv[0];               // float64 out: ... -> out -> workspace -> out
        else { dst = out; dst_s = os; }
        const int e = fi_launch(src, sdt, seq, value, sst, dst, left == 0 ? kind : FI_OUT_F64, threshold, dst_s, A, a, axes[a], mode, cval, st);
        if (e != HV_OK) return e;
        src = dst; sst = dst_s; sdt = HV_DT_F64; seq = 0;
        ++done;
    }
    return HV_OK;
}

extern "C" int hv_blend_lerp(const void* a, int a_dtype, long long as0, long long as1, long long as2, const void* b, int b_dtype, long long bs0,
                             long long bs1, long long bs2, const void* w, int w_dtype, long long ws0, long long ws1, long long ws2, int A0, int A1,
                             int A2, double* out, long long os0, long long os1, long long os2, void* stream) {
    auto vdt = [](int dt) { return dt == HV_DT_I16 || dt == HV_DT_F32 || dt == HV_DT_F64; };
    if (!a || !b || !w || !out || !fi_dims_ok(A0, A1, A2) || !vdt(a_dtype) || !vdt(b_dtype) || (w_dtype != HV_DT_F64 && w_dtype != HV_DT_U8) ||
        ((uintptr_t)out & 7))
        return HV_ERR_ARG;
    if ((long long)A0 * A1 * A2 > (1LL << 30)) return HV_ERR_UNSUPPORTED;
    const int A[3] = {A0, A1, A2};
    const long long sa[3] = {as0, as1, as2}, sb[3] = {bs0, bs1, bs2}, sw[3] = {ws0, ws1, ws2}, so[3] = {os0, os1, os2};
    // out may be a itself (every voxel is read and written by one lane); any other overlap with an input is refused
    if ((const void*)out == a) {
        if (a_dtype != HV_DT_F64 || as0 != os0 || as1 != os1 || as2 != os2) return HV_ERR_ARG;
    } else if (fi_overlap(a, A, sa, fi_elem(a_dtype), out, so, 8)) return HV_ERR_ARG;
    if (fi_overlap(b, A, sb, fi_elem(b_dtype), out, so, 8) || fi_overlap(w, A, sw, fi_elem(w_dtype), out, so, 8)) return HV_ERR_ARG;
    int ord[3] = {0, 1, 2};                           // the axes by falling stride of out: the last runs along the lanes
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2 - i; ++j)
            if (fi_abs(so[ord[j]]) < fi_abs(so[ord[j + 1]])) { const int t = ord[j]; ord[j] = ord[j + 1]; ord[j + 1] = t; }
    FiBlend B;
    B.a = a; B.b = b; B.w = w; B.out = out; B.a_dt = a_dtype; B.b_dt = b_dtype; B.w_dt = w_dtype;
    for (int i = 0; i < 3; ++i) {
        B.n[i] = A[ord[i]]; B.a_s[i] = sa[ord[i]]; B.b_s[i] = sb[ord[i]]; B.w_s[i] = sw[ord[i]]; B.o_s[i] = so[ord[i]];
    }
    const long long N = (long long)A0 * A1 * A2;
    hipLaunchKernelGGL(blend_lerp_kernel, dim3(hv_cdiv(N, FI_THREADS)), dim3(FI_THREADS), 0, (hipStream_t)stream, B, N);
    HV_LAUNCH_CHECK();
    return HV_OK;
}
