// Cubic B-spline sampling of a coefficient volume (scipy.ndimage.map_coordinates order 3, mode 'constant'): the one __device__ tap function
// the straightening sampler (straighten.hip) and the restore (restore.hip) call, and the bone window the prefilter (spline.hip) shares with
// the order-1 sampler.  The coefficients are what hv_spline_prefilter leaves: spline_filter(v, 3, mode='mirror') in float64.
#pragma once

// window(img, win_min, win_max) on one value (straighten_mask_3d.py:178-183): 255.0 * (v - min) / (max - min), clipped to [0, 255]
__device__ __forceinline__ double ss_window(double v, double wmin, double wmax) {
    double r = 255.0 * (v - wmin) / (wmax - wmin);
    if (r < 0.0) r = 0.0;
    if (r > 255.0) r = 255.0;
    return r;
}

// tap index i of a line of n coefficients, mirrored about its end points (-1 -> 1, n -> n - 2): in [0, n - 1] for every i
__device__ __forceinline__ long long hv_spline_mirror(long long i, int n) {
    if (n == 1) return 0;
    const long long p = 2LL * (n - 1);
    i = i < 0 ? -i : i;
    i %= p;
    return i >= n ? p - i : i;
}

// offsets (in elements, stride s) of the four taps floor(u) - 1 .. floor(u) + 2 and their weights (ni_splines.c, order 3) for 0 <= u <= n - 1
__device__ __forceinline__ void hv_spline_taps(double u, int n, long long s, long long (&o)[4], double (&w)[4]) {
    const double f = floor(u);
    const double y = u - f, z = 1.0 - y;
    w[1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
    w[2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0;
    w[0] = z * z * z / 6.0;
    w[3] = 1.0 - w[0] - w[1] - w[2];
    const long long i = (long long)f;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = hv_spline_mirror(i - 1 + k, n) * s;
}

// the sample at (u0, u1, u2), each inside [0, n - 1] (the caller has applied the outside rule), of the contiguous coefficients [n0][n1][n2]:
// the sum over the 4 x 4 x 4 taps, last axis fastest, coefficient * w0 * w1 * w2.  No clipping: the value may leave the data's range.
__device__ __forceinline__ double hv_spline_sample(const double* __restrict__ coef, int n0, int n1, int n2, double u0, double u1, double u2) {
    long long o0[4], o1[4], o2[4];
    double w0[4], w1[4], w2[4];
    hv_spline_taps(u0, n0, (long long)n1 * n2, o0, w0);
    hv_spline_taps(u1, n1, (long long)n2, o1, w1);
    hv_spline_taps(u2, n2, 1, o2, w2);
    double v = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const double* p = coef + (o0[a] + o1[b]);
#pragma unroll
            for (int c = 0; c < 4; ++c) v += ((p[o2[c]] * w0[a]) * w1[b]) * w2[c];
        }
    return v;
}
