// Cubic B-spline prefilter of a whole volume (scipy.ndimage.spline_filter(v, 3, mode='mirror') in float64, which is step one of
// map_coordinates(order=3); reference straighten/straighten/curve.py:77-102 interpolate_along(..., order=3)).
//
// Along each axis in turn every line c[0..n-1] goes through the recursive filter with the pole z = sqrt(3) - 2 (ni_splines.c):
//   c[i] *= (1 - z)(1 - 1/z);   c[0] = the mirror sum below;   c[i] += z c[i-1];   c[n-1] = z / (z^2 - 1) (c[n-1] + z c[n-2]);
//   c[i] = z (c[i+1] - c[i]);   a line of length 1 is left as it is.
// A line is serial: one lane per line, no atomics, no cross-lane sums, so the same input gives the same bits on every run.
//   spline_axis_kernel<FIRST>  axes 0 and 1 of the contiguous [D0][D1][D2] output: consecutive lanes take lines that are unit-stride
//                              neighbours, every load and store of a wave is one run of consecutive doubles.  FIRST (axis 0) reads the
//                              source (int16 / float32 / float64, any strides), windows each voxel as it is first read and writes doubles.
//   spline_axis2_kernel        the unit-stride axis: a workgroup stages [128 lines][32] tiles through LDS (row pitch 33 doubles: lane l
//                              walks row l, 2 banks on from lane l - 1), each lane walks its own row and carries its recursion state from
//                              tile to tile, forwards for the causal pass and backwards for the anticausal one.
// Causal start: the sum is truncated at SP_HORIZON = 32 terms, c[0] = sum_{i < 32} z^i c[i] (|z|^32 = 5e-19 < 2^-53: what is dropped is below
// one rounding of the sum); a line of n <= 32 takes scipy's full mirror sum
//   (c[0] + z^(n-1) c[n-1] + sum_{i=1..n-2} (z^i + z^(2n-2-i)) c[i]) / (1 - z^(2n-2)),  where the two images overlap.
// Everything in doubles (-ffp-contract=off); element offsets are 64-bit.  No workspace beyond the output.
#include <climits>
#include <cmath>
#include "hv_common.h"
#include "spline_tap.h"

#define SP_HORIZON 32
#define SP_BATCH 8                    // loads in flight per lane in the strided passes
#define SP_LINES 128                  // lines (= lanes) per workgroup of the unit-stride pass
#define SP_CHUNK 32                   // tile width; the causal start reads the first tile only
#define SP_PITCH (SP_CHUNK + 1)
static_assert(SP_CHUNK >= SP_HORIZON, "the causal start of the unit-stride pass reads one tile");

struct SpSrc { const void* p; int dt; long long s0, s1, s2; int win; double wmin, wmax; };

__device__ __forceinline__ double sp_ld(const SpSrc& S, long long o) {
    double v;
    switch (S.dt) {
        case HV_DT_I16: v = (double)((const int16_t*)S.p)[o]; break;
        case HV_DT_F32: v = (double)((const float*)S.p)[o]; break;
        default: v = ((const double*)S.p)[o]; break;
    }
    return S.win ? ss_window(v, S.wmin, S.wmax) : v;
}

struct SpPole { double z, gain, last; };
__device__ __forceinline__ SpPole sp_pole() {
    SpPole P;
    P.z = sqrt(3.0) - 2.0;
    P.gain = (1.0 - P.z) * (1.0 - 1.0 / P.z);
    P.last = P.z / (P.z * P.z - 1.0);
    return P;
}

// The causal start of a line of n >= 2 scaled values v(0 .. n - 1); get(i) must be valid for i < min(n, SP_HORIZON).
template <typename F>
__device__ __forceinline__ double sp_causal_start(const double z, const int n, F get) {
    const int lim = n <= SP_HORIZON ? n - 1 : SP_HORIZON;
    const double v0 = get(0);
    double zi = z, s = 0.0, h = 0.0;            // s = sum z^i v(i); h = sum z^(n-1-i) v(i) in Horner form (the mirror image, n <= horizon only)
    for (int i = 1; i < lim; ++i) {
        const double v = get(i);
        s += zi * v;
        h = (h + v) * z;
        zi *= z;
    }
    if (n > SP_HORIZON) return v0 + s;
    const double zn1 = zi;                      // z^(n-1)
    return (((v0 + zn1 * get(n - 1)) + s) + zn1 * h) / (1.0 - zn1 * zn1);
}

// Lines along axis 0 (pstride = D2: line (j, k) starts at j * D2 + k, step D1 * D2) or axis 1 (pstride = D1 * D2: line (i, k) starts at
// i * D1 * D2 + k, step D2) of the contiguous output.  FIRST: the values come from the source, line (j, k) at j * s1 + k * s2, step s0.
template <bool FIRST>
__global__ __launch_bounds__(256) void spline_axis_kernel(SpSrc S, double* __restrict__ coef, long long nl, int inner, long long pstride,
                                                          long long step, int n) {
    const long long L = (long long)blockIdx.x * 256 + threadIdx.x;
    if (L >= nl) return;
    const long long p = L / inner, k = L - p * inner;
    double* out = coef + (p * pstride + k);
    const long long sbase = FIRST ? p * S.s1 + k * S.s2 : 0;
    auto raw = [&](int i) -> double { return FIRST ? sp_ld(S, sbase + (long long)i * S.s0) : out[(long long)i * step]; };
    if (n == 1) {
        if (FIRST) out[0] = raw(0);
        return;
    }
    const SpPole P = sp_pole();
    double c = sp_causal_start(P.z, n, [&](int i) { return P.gain * raw(i); });
    double cp = c;
    out[0] = c;
    for (int i = 1; i < n; i += SP_BATCH) {
        double v[SP_BATCH];
#pragma unroll
        for (int u = 0; u < SP_BATCH; ++u) v[u] = i + u < n ? raw(i + u) : 0.0;
#pragma unroll
        for (int u = 0; u < SP_BATCH; ++u)
            if (i + u < n) {
                cp = c;
                c = P.gain * v[u] + P.z * c;
                out[(long long)(i + u) * step] = c;
            }
    }
    c = P.last * (c + P.z * cp);
    out[(long long)(n - 1) * step] = c;
    for (int i = n - 2; i >= 0; i -= SP_BATCH) {
        double v[SP_BATCH];
#pragma unroll
        for (int u = 0; u < SP_BATCH; ++u) v[u] = i - u >= 0 ? out[(long long)(i - u) * step] : 0.0;
#pragma unroll
        for (int u = 0; u < SP_BATCH; ++u)
            if (i - u >= 0) {
                c = P.z * (c - v[u]);
                out[(long long)(i - u) * step] = c;
            }
    }
}

// tile t of the workgroup's lines between global memory and LDS: 32 consecutive lanes move 32 consecutive doubles of one line
template <bool STORE>
__device__ __forceinline__ void sp_tile_move(double* __restrict__ coef, double* tile, long long line0, long long nl, int n, int t) {
#pragma unroll 4
    for (int it = 0; it < SP_CHUNK; ++it) {
        const int idx = it * SP_LINES + threadIdx.x;
        const int l = idx / SP_CHUNK, col = idx % SP_CHUNK;
        const int g = t * SP_CHUNK + col;
        if (line0 + l < nl && g < n) {
            double* q = coef + ((line0 + l) * n + g);
            if (STORE) *q = tile[l * SP_PITCH + col];
            else tile[l * SP_PITCH + col] = *q;
        }
    }
}

// the unit-stride axis of the contiguous output, in place: nl lines of n >= 2 doubles, line L at L * n
__global__ __launch_bounds__(SP_LINES) void spline_axis2_kernel(double* __restrict__ coef, long long nl, int n) {
    __shared__ double tile[SP_LINES * SP_PITCH];
    const long long line0 = (long long)blockIdx.x * SP_LINES;
    const bool live = line0 + threadIdx.x < nl;
    double* row = tile + threadIdx.x * SP_PITCH;
    const int T = (n + SP_CHUNK - 1) / SP_CHUNK;
    const SpPole P = sp_pole();
    double c = 0.0, cp = 0.0;
    for (int t = 0; t < T; ++t) {                 // causal, forwards; the last tile turns round in LDS
        sp_tile_move<false>(coef, tile, line0, nl, n, t);
        __syncthreads();
        if (live) {
            const int cnt = min(SP_CHUNK, n - t * SP_CHUNK);
            int j = 0;
            if (t == 0) {
                c = sp_causal_start(P.z, n, [&](int i) { return P.gain * row[i]; });
                cp = c;
                row[0] = c;
                j = 1;
            }
            for (; j < cnt; ++j) {
                cp = c;
                c = P.gain * row[j] + P.z * c;
                row[j] = c;
            }
            if (t == T - 1) {
                c = P.last * (c + P.z * cp);
                row[cnt - 1] = c;
                for (j = cnt - 2; j >= 0; --j) {
                    c = P.z * (c - row[j]);
                    row[j] = c;
                }
            }
        }
        __syncthreads();
        sp_tile_move<true>(coef, tile, line0, nl, n, t);
        __syncthreads();
    }
    for (int t = T - 2; t >= 0; --t) {            // anticausal, backwards
        sp_tile_move<false>(coef, tile, line0, nl, n, t);
        __syncthreads();
        if (live)
            for (int j = SP_CHUNK - 1; j >= 0; --j) {
                c = P.z * (c - row[j]);
                row[j] = c;
            }
        __syncthreads();
        sp_tile_move<true>(coef, tile, line0, nl, n, t);
        __syncthreads();
    }
}

extern "C" int hv_spline_prefilter(const void* src, int dtype, long long s0, long long s1, long long s2, int D0, int D1, int D2, int window,
                                   double win_min, double win_max, double* coef, void* stream) {
    if (!src || !coef || D0 <= 0 || D1 <= 0 || D2 <= 0 || (dtype != HV_DT_I16 && dtype != HV_DT_F32 && dtype != HV_DT_F64) ||
        ((uintptr_t)coef & 7))
        return HV_ERR_ARG;
    const long long plane = (long long)D1 * D2, l0 = plane, l1 = (long long)D0 * D2, l2 = (long long)D0 * D1;
    const long long lmax = l0 > l1 ? (l0 > l2 ? l0 : l2) : (l1 > l2 ? l1 : l2);
    if (plane > LLONG_MAX / 8 / D0 || lmax > 0x7fffffffLL * SP_LINES) return HV_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    SpSrc S;
    S.p = src; S.dt = dtype; S.s0 = s0; S.s1 = s1; S.s2 = s2; S.win = window; S.wmin = win_min; S.wmax = win_max;
    // axis 0 always runs: it is the pass that reads the source (a line of length 1 is only converted)
    hipLaunchKernelGGL(spline_axis_kernel<true>, dim3(hv_cdiv(l0, 256)), dim3(256), 0, s, S, coef, l0, D2, (long long)D2, plane, D0);
    HV_LAUNCH_CHECK();
    if (D1 > 1) {
        hipLaunchKernelGGL(spline_axis_kernel<false>, dim3(hv_cdiv(l1, 256)), dim3(256), 0, s, S, coef, l1, D2, plane, (long long)D2, D1);
        HV_LAUNCH_CHECK();
    }
    if (D2 > 1) {
        hipLaunchKernelGGL(spline_axis2_kernel, dim3(hv_cdiv(l2, SP_LINES)), dim3(SP_LINES), 0, s, coef, l2, D2);
        HV_LAUNCH_CHECK();
    }
    return HV_OK;
}
