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
#include "resample_core.h"

struct RsP {
    const void* src; void* dst;
    long long s0, s1, s2, d0, d1, d2;   // element strides by HOST axis
    int A0, A1, A2, O0, O1, O2;
    int r0, r1, r2;                     // the role (0 = L, 1 = M, 2 = O) of host output axis 0 / 1 / 2
    int nL, nM, nO;                     // the output extents by role
    int dst_dt;
    hv_resample_desc D;
};

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
    if (!desc) return HV_ERR_ARG;
    const hv_resample_desc& D = *desc;
    const int A[3] = {A0, A1, A2}, O[3] = {O0, O1, O2};
    const long long ss[3] = {s0, s1, s2}, os[3] = {os0, os1, os2};
    int rc = rs_check_args(vol, dtype, A, out, out_dtype, O, D.order, D.mode, D.cval);
    if (rc != HV_OK) return rc;
    if (!rs_desc_ok(D)) return HV_ERR_ARG;
    rc = rs_check_support(vol, dtype, A, ss, out, out_dtype, O, os, D.order, D.mode);
    if (rc != HV_OK) return rc;
    // the roles: L the output axis whose unit step moves least far in the source (an axis of extent 1 comes last), then M, then O
    double img[3];
    rs_image(D, ss, img);
    int ord[3];
    rs_roles(O, img, ord);
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
