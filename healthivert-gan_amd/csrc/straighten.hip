// Spine straightening and per-vertebra volume extraction on the device (reference straighten/location_json_local.py:14-16,33-45 and
// straighten/straighten_mask_3d.py:123-146,172-184,222-247,463-563 with straighten/curve.py:54-102).
//
//   straighten_stats_ct_kernel<T>     one read of the CT: its min and max (the global decision of window(), :172-184)
//   straighten_stats_label_kernel<T>  one read of the label volume: per label 1..255 the voxel count and the u64 sums of the three indices
//                                     (the centroids of location_json_local.py, exact), a flag for non-integer / out-of-range labels, and
//                                     the raw-geometry presence bits of the split cleanup (the single-centroid branch, :499-502)
//   straighten_sample_kernel<T>       one lane per (n, a, b) of the straight volumes [N][PA][PB]: the fp64 sample coordinate
//                                     (knots[n] + basis[n][:,1] (b - PB/2) + basis[n][:,2] (a - PA/2)) / spacing (curve.py:54-102; knots and
//                                     frame in millimetres, the quotient per axis in voxel indices of the scan), trilinear on the
//                                     windowed CT (map_coordinates order 1, mode 'constant'), nearest on the label (order 0), and the
//                                     presence bits of column b = PB/2, rows a >= PA/2 (remove_spine_labels_after_split, :123-146)
//   straighten_crop_kernel            every requested vertebra in one launch: extract_3d_volume (:222-247) from the straight volumes (or the
//                                     raw ones, windowed on the fly), the per-label row cutoff of the split cleanup applied on the way
// Everything in doubles in the reference's operation order (-ffp-contract=off); element offsets are 64-bit (a float64 CT passes 2^31 bytes).
#include <climits>
#include <cmath>
#include <cstdlib>
#include "volume_access.h"                 // hv_ld_dt
#include "spline_tap.h"                   // ss_window, hv_spline_sample

#define SS_HDR 4                      // [0] ~key(min) (atomic max), [1] key(max), [2] bad-label flag, [3] unused
#define SS_CNT SS_HDR                 // [4 + l] voxel count of label l
#define SS_SUM (SS_CNT + 256)         // [260 + 3 l + axis] index sums
#define SS_PRES (SS_SUM + 3 * 256)    // [1028 + l * Rw + w] presence words of the raw geometry

__host__ __device__ static inline int ss_rows_words(int rows) { return (rows - rows / 2 + 63) / 64; }

// double -> u64 key whose unsigned order is the numeric order
__device__ __forceinline__ u64 ss_key(double v) {
    const u64 u = (u64)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

template <typename T> __device__ __forceinline__ double ss_ld(const T* p, long long o) { return (double)p[o]; }

// memory-order walk of a [D0][D1][D2] volume with arbitrary strides: the host passes the axes sorted by stride (innermost first)
struct SsWalk { long long n_in, n_mid, n_out, s_in, s_mid, s_out; int ax_in, ax_mid, ax_out; };

template <typename T>
__global__ __launch_bounds__(256) void straighten_stats_ct_kernel(const T* __restrict__ ct, SsWalk w, u64* __restrict__ stats) {
    __shared__ double smin[4], smax[4];
    double mn = __builtin_inf(), mx = -__builtin_inf();
    const long long rows = w.n_mid * w.n_out;
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
        const long long im = r % w.n_mid, io = r / w.n_mid;
        const T* p = ct + im * w.s_mid + io * w.s_out;
        for (long long i = threadIdx.x; i < w.n_in; i += 256) {
            const double v = ss_ld(p, i * w.s_in);
            mn = fmin(mn, v);
            mx = fmax(mx, v);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, o));
        mx = fmax(mx, __shfl_xor(mx, o));
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { smin[wv] = mn; smax[wv] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        mn = fmin(fmin(smin[0], smin[1]), fmin(smin[2], smin[3]));
        mx = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
        atomicMax(&stats[0], ~ss_key(mn));
        atomicMax(&stats[1], ss_key(mx));
    }
}

template <typename T>
__device__ __forceinline__ int ss_label(T v, int& bad) {
    const double d = (double)v;
    if (!(d >= 0.0 && d <= 255.0 && d == floor(d))) { bad = 1; return 0; }   // NaN fails the first test
    return (int)d;
}

// per-thread runs of one label are summed in registers and flushed to LDS on a label change: label 0 (most voxels) costs no atomic at all
template <typename T>
__global__ __launch_bounds__(256) void straighten_stats_label_kernel(const T* __restrict__ label, SsWalk w, int D1, int D2, u64* __restrict__ stats) {
    __shared__ u64 s_cnt[256], s_sum[3 * 256];
    for (int i = threadIdx.x; i < 256; i += 256) s_cnt[i] = 0;
    for (int i = threadIdx.x; i < 3 * 256; i += 256) s_sum[i] = 0;
    __syncthreads();
    const int row0 = D1 / 2, zc = D2 / 2, Rw = ss_rows_words(D1);
    u64* pres = stats + SS_PRES;
    int bad = 0, cur = 0;
    u64 cnt = 0, sx = 0, sy = 0, sz = 0;
    const long long rows = w.n_mid * w.n_out;
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
        const long long im = r % w.n_mid, io = r / w.n_mid;
        const T* p = label + im * w.s_mid + io * w.s_out;
        // index of the row's first voxel per axis, and which axis the walk advances along (selects: no private arrays)
        const long long bx = w.ax_mid == 0 ? im : (w.ax_out == 0 ? io : 0), by = w.ax_mid == 1 ? im : (w.ax_out == 1 ? io : 0),
                        bz = w.ax_mid == 2 ? im : (w.ax_out == 2 ? io : 0);
        for (long long i = threadIdx.x; i < w.n_in; i += 256) {
            const int l = ss_label(p[i * w.s_in], bad);
            if (l != cur) {
                if (cur != 0 && cnt) {
                    atomicAdd(&s_cnt[cur], cnt);
                    atomicAdd(&s_sum[3 * cur], sx); atomicAdd(&s_sum[3 * cur + 1], sy); atomicAdd(&s_sum[3 * cur + 2], sz);
                }
                cur = l; cnt = sx = sy = sz = 0;
            }
            if (l == 0) continue;
            const long long x = w.ax_in == 0 ? bx + i : bx, y = w.ax_in == 1 ? by + i : by, z = w.ax_in == 2 ? bz + i : bz;
            ++cnt; sx += (u64)x; sy += (u64)y; sz += (u64)z;
            if (z == zc && y >= row0) {
                const int h = (int)y - row0;
                atomicOr(&pres[(long long)l * Rw + (h >> 6)], 1ull << (h & 63));
            }
        }
    }
    if (cur != 0 && cnt) {
        atomicAdd(&s_cnt[cur], cnt);
        atomicAdd(&s_sum[3 * cur], sx); atomicAdd(&s_sum[3 * cur + 1], sy); atomicAdd(&s_sum[3 * cur + 2], sz);
    }
    if (bad) atomicOr(&stats[2], 1ull);
    __syncthreads();
    const int l = threadIdx.x;
    if (s_cnt[l]) {
        atomicAdd(&stats[SS_CNT + l], s_cnt[l]);
        for (int a = 0; a < 3; ++a) atomicAdd(&stats[SS_SUM + 3 * l + a], s_sum[3 * l + a]);
    }
}

struct SsSpacing { double s0, s1, s2; };      // millimetres per voxel along axes 0, 1, 2: a kernel argument, no device allocation

// one lane per sample; workgroups are renumbered so that consecutive planes (which read the same voxels) run on one XCD
// (the hardware hands workgroup i to XCD i % 8).  ORDER = 3: `ct` is the contiguous float64 coefficient volume hv_spline_prefilter left (the
// window already applied), read as 4 x 4 x 4 cubic B-spline taps; coordinates, the outside rule, the label and the presence bits are shared.
template <typename T, int ORDER>
__global__ __launch_bounds__(256) void straighten_sample_kernel(const T* __restrict__ ct, long long cs0, long long cs1, long long cs2,
                                                                const void* __restrict__ label, int ldt, long long ls0, long long ls1, long long ls2,
                                                                int D0, int D1, int D2, const double* __restrict__ knots,
                                                                const double* __restrict__ basis, int N, int PA, int PB, int win, double wmin,
                                                                double wmax, double* __restrict__ sct, uint8_t* __restrict__ slab,
                                                                u64* __restrict__ pres, int nblk, SsSpacing sp) {
    const int per_xcd = gridDim.x / 8;
    const int blk = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (blk >= nblk) return;
    const long long e = (long long)blk * 256 + threadIdx.x;
    const long long plane = (long long)PA * PB;
    if (e >= (long long)N * plane) return;
    const int n = (int)(e / plane);
    const int rem = (int)(e - (long long)n * plane);
    const int a = rem / PB, b = rem - a * PB;
    const double gb = (double)b - (double)PB / 2.0, ga = (double)a - (double)PA / 2.0;
    const double* B = basis + (long long)n * 9;
    const double* K = knots + (long long)n * 3;
    double c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] = ((B[3 * i] * 0.0 + B[3 * i + 1] * gb) + B[3 * i + 2] * ga) + K[i];
    // knots and frame are in millimetres: back to voxel indices (spatial_to_pixel, curve.py:74,179-195)
    c[0] = c[0] / sp.s0; c[1] = c[1] / sp.s1; c[2] = c[2] / sp.s2;
    const int D[3] = {D0, D1, D2};
    bool in = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) in = in && c[i] >= 0.0 && c[i] <= (double)(D[i] - 1);
    double v = 0.0;
    int l = 0;
    if (in) {
        if constexpr (ORDER == 3) {
            v = hv_spline_sample((const double*)ct, D0, D1, D2, c[0], c[1], c[2]);
        } else {
            long long i0[3], i1[3];
            double w0[3], w1[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double f = floor(c[i]);
                const double t = c[i] - f;
                i0[i] = (long long)f;
                i1[i] = i0[i] + 1 < D[i] ? i0[i] + 1 : i0[i];     // at c = D - 1 the upper weight is 0: not read
                w0[i] = 1.0 - t;
                w1[i] = t;
            }
            const long long ox[2] = {i0[0] * cs0, i1[0] * cs0}, oy[2] = {i0[1] * cs1, i1[1] * cs1}, oz[2] = {i0[2] * cs2, i1[2] * cs2};
            // map_coordinates: sum over the 8 corners, last axis fastest, coefficient = value * w_x * w_y * w_z
#pragma unroll
            for (int hx = 0; hx < 2; ++hx)
#pragma unroll
                for (int hy = 0; hy < 2; ++hy)
#pragma unroll
                    for (int hz = 0; hz < 2; ++hz) {
                        double u = ss_ld(ct, ox[hx] + oy[hy] + oz[hz]);
                        if (win) u = ss_window(u, wmin, wmax);
                        v += ((u * (hx ? w1[0] : w0[0])) * (hy ? w1[1] : w0[1])) * (hz ? w1[2] : w0[2]);
                    }
        }
        const long long n0 = (long long)floor(c[0] + 0.5), n1 = (long long)floor(c[1] + 0.5), n2 = (long long)floor(c[2] + 0.5);
        const double d = hv_ld_dt(label, ldt, n0 * ls0 + n1 * ls1 + n2 * ls2);
        l = d >= 0.0 && d <= 255.0 ? (int)d : 0;         // validated by the stats pass; the guard keeps the presence index in range
    }
    sct[e] = v;
    slab[e] = (uint8_t)l;
    if (l != 0 && b == PB / 2 && a >= PA / 2) {
        const int h = a - PA / 2;
        atomicOr(&pres[(long long)l * ss_rows_words(PA) + (h >> 6)], 1ull << (h & 63));
    }
}

// boxes[v]: {lo0, lo1, lo2, len0, len1, len2, start0, start1, start2}: output voxel (i, j, k) of vertebra v reads source
// (lo0 + i - start0, lo1 + j - start1, lo2 + k - start2) when 0 <= i - start0 < len0 (and so on), else it is 0
__global__ __launch_bounds__(256) void straighten_crop_kernel(const void* __restrict__ ct, int cdt, long long cs0, long long cs1, long long cs2,
                                                              const void* __restrict__ label, int ldt, long long ls0, long long ls1, long long ls2,
                                                              int D1, int win, double wmin, double wmax, const u64* __restrict__ pres,
                                                              const int* __restrict__ boxes, int O0, int O1, int O2, double* __restrict__ out_ct,
                                                              uint8_t* __restrict__ out_lab) {
    __shared__ int cut[256];
    {   // row cutoff of label l: the first row h >= D1/2 whose centre column lacks l (remove_spine_labels_after_split), D1 if none
        const int l = threadIdx.x, row0 = D1 / 2, R = D1 - row0, Rw = ss_rows_words(D1);
        int h = R;
        for (int wi = 0; wi < Rw; ++wi) {
            const u64 m = ~pres[(long long)l * Rw + wi];
            if (m) { h = min(R, wi * 64 + __builtin_ctzll(m)); break; }
        }
        cut[l] = row0 + h;
    }
    __syncthreads();
    const int v = blockIdx.y;
    const long long vol = (long long)O0 * O1 * O2;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= vol) return;
    const int k = (int)(e % O2), j = (int)((e / O2) % O1), i = (int)(e / ((long long)O1 * O2));
    const int* bx = boxes + 9 * v;
    const int si = i - bx[6], sj = j - bx[7], sk = k - bx[8];
    double c = 0.0;
    int l = 0;
    if (si >= 0 && si < bx[3] && sj >= 0 && sj < bx[4] && sk >= 0 && sk < bx[5]) {
        const long long x = bx[0] + si, y = bx[1] + sj, z = bx[2] + sk;
        c = hv_ld_dt(ct, cdt, x * cs0 + y * cs1 + z * cs2);
        if (win) c = ss_window(c, wmin, wmax);
        const double d = hv_ld_dt(label, ldt, x * ls0 + y * ls1 + z * ls2);
        l = d >= 0.0 && d <= 255.0 ? (int)d : 0;
        if (y >= cut[l]) l = 0;
    }
    out_ct[(long long)v * vol + e] = c;
    out_lab[(long long)v * vol + e] = (uint8_t)l;
}

static SsWalk ss_walk(long long s0, long long s1, long long s2, int D0, int D1, int D2) {
    long long st[3] = {s0, s1, s2}, n[3] = {D0, D1, D2};
    int ax[3] = {0, 1, 2};
    for (int i = 0; i < 3; ++i)   // sort axes by |stride|, innermost first (a size-1 axis goes outermost)
        for (int j = i + 1; j < 3; ++j) {
            const long long ki = n[ax[i]] == 1 ? LLONG_MAX : llabs(st[ax[i]]), kj = n[ax[j]] == 1 ? LLONG_MAX : llabs(st[ax[j]]);
            if (kj < ki) { const int t = ax[i]; ax[i] = ax[j]; ax[j] = t; }
        }
    SsWalk w;
    w.n_in = n[ax[0]]; w.n_mid = n[ax[1]]; w.n_out = n[ax[2]];
    w.s_in = st[ax[0]]; w.s_mid = st[ax[1]]; w.s_out = st[ax[2]];
    w.ax_in = ax[0]; w.ax_mid = ax[1]; w.ax_out = ax[2];
    return w;
}

static bool ss_ct_dtype(int dt) { return dt == HV_DT_I16 || dt == HV_DT_F32 || dt == HV_DT_F64; }
static bool ss_label_dtype(int dt) { return dt >= HV_DT_U8 && dt <= HV_DT_F64; }

extern "C" size_t hv_straighten_presence_bytes(int rows) {
    if (rows <= 0) return 0;
    return (size_t)256 * ss_rows_words(rows) * sizeof(u64);
}

extern "C" size_t hv_straighten_stats_bytes(int D1) {
    if (D1 <= 0) return 0;
    return (size_t)SS_PRES * sizeof(u64) + hv_straighten_presence_bytes(D1);
}

extern "C" int hv_straighten_stats(const void* ct, int ct_dtype, long long cs0, long long cs1, long long cs2, const void* label, int label_dtype,
                                   long long ls0, long long ls1, long long ls2, int D0, int D1, int D2, uint64_t* stats, size_t stats_bytes,
                                   void* stream) {
    if (!label || !stats || D0 <= 0 || D1 <= 0 || D2 <= 0 || (ct && !ss_ct_dtype(ct_dtype)) || !ss_label_dtype(label_dtype)) return HV_ERR_ARG;
    if (stats_bytes < hv_straighten_stats_bytes(D1) || ((uintptr_t)stats & 7)) return HV_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(stats, 0, hv_straighten_stats_bytes(D1), s) != hipSuccess) return -1000 - (int)hipGetLastError();
    const SsWalk wc = ss_walk(cs0, cs1, cs2, D0, D1, D2), wl = ss_walk(ls0, ls1, ls2, D0, D1, D2);
    const int gc = (int)min(wc.n_mid * wc.n_out, 2048LL), gl = (int)min(wl.n_mid * wl.n_out, 2048LL);
    if (ct) switch (ct_dtype) {
        case HV_DT_I16: hipLaunchKernelGGL(straighten_stats_ct_kernel<int16_t>, dim3(gc), dim3(256), 0, s, (const int16_t*)ct, wc, (u64*)stats); break;
        case HV_DT_F32: hipLaunchKernelGGL(straighten_stats_ct_kernel<float>, dim3(gc), dim3(256), 0, s, (const float*)ct, wc, (u64*)stats); break;
        default: hipLaunchKernelGGL(straighten_stats_ct_kernel<double>, dim3(gc), dim3(256), 0, s, (const double*)ct, wc, (u64*)stats); break;
    }
    HV_LAUNCH_CHECK();
#define SS_LAB(T) hipLaunchKernelGGL(straighten_stats_label_kernel<T>, dim3(gl), dim3(256), 0, s, (const T*)label, wl, D1, D2, (u64*)stats)
    switch (label_dtype) {
        case HV_DT_U8: SS_LAB(uint8_t); break;
        case HV_DT_I16: SS_LAB(int16_t); break;
        case HV_DT_I32: SS_LAB(int32_t); break;
        case HV_DT_I64: SS_LAB(long long); break;
        case HV_DT_F32: SS_LAB(float); break;
        default: SS_LAB(double); break;
    }
#undef SS_LAB
    HV_LAUNCH_CHECK();
    return HV_OK;
}

// both sampling entries: order 1 reads the scan (ct_dtype, strides), order 3 the contiguous float64 coefficients of the whole scan
static int ss_sample(int order, const void* ct, int ct_dtype, long long cs0, long long cs1, long long cs2, const void* label, int label_dtype,
                     long long ls0, long long ls1, long long ls2, int D0, int D1, int D2, const double* knots, const double* basis, int N, int PA,
                     int PB, int window, double win_min, double win_max, double* straight_ct, uint8_t* straight_label, uint64_t* presence,
                     size_t presence_bytes, const double* spacing, void* stream) {
    if (!spacing) return HV_ERR_ARG;
    for (int i = 0; i < 3; ++i)
        if (!(spacing[i] > 0.0) || !std::isfinite(spacing[i])) return HV_ERR_ARG;
    const SsSpacing sp = {spacing[0], spacing[1], spacing[2]};
    if (!ct || !label || !knots || !basis || !straight_ct || !straight_label || !presence || D0 <= 0 || D1 <= 0 || D2 <= 0 || N <= 0 ||
        PA <= 0 || PB <= 0 || !ss_ct_dtype(ct_dtype) || !ss_label_dtype(label_dtype))
        return HV_ERR_ARG;
    if (presence_bytes < hv_straighten_presence_bytes(PA) || ((uintptr_t)presence & 7)) return HV_ERR_WORKSPACE;
    const long long total = (long long)N * PA * PB;
    if (total > 0x7fffffffLL * 64) return HV_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(presence, 0, hv_straighten_presence_bytes(PA), s) != hipSuccess) return -1000 - (int)hipGetLastError();
    const int nblk = hv_cdiv(total, 256);
    const int grid = hv_cdiv(nblk, 8) * 8;
#define SS_SMP(T, ORDER) hipLaunchKernelGGL((straighten_sample_kernel<T, ORDER>), dim3(grid), dim3(256), 0, s, (const T*)ct, cs0, cs1, cs2, label, \
                                            label_dtype, ls0, ls1, ls2, D0, D1, D2, knots, basis, N, PA, PB, window, win_min, win_max, straight_ct, \
                                            straight_label, (u64*)presence, nblk, sp)
    if (order == 3) SS_SMP(double, 3);
    else switch (ct_dtype) {
        case HV_DT_I16: SS_SMP(int16_t, 1); break;
        case HV_DT_F32: SS_SMP(float, 1); break;
        default: SS_SMP(double, 1); break;
    }
#undef SS_SMP
    HV_LAUNCH_CHECK();
    return HV_OK;
}

extern "C" int hv_straighten_sample_sp(const void* ct, int ct_dtype, long long cs0, long long cs1, long long cs2, const void* label,
                                       int label_dtype, long long ls0, long long ls1, long long ls2, int D0, int D1, int D2, const double* knots,
                                       const double* basis, int N, int PA, int PB, int window, double win_min, double win_max,
                                       double* straight_ct, uint8_t* straight_label, uint64_t* presence, size_t presence_bytes,
                                       const double* spacing, void* stream) {
    return ss_sample(1, ct, ct_dtype, cs0, cs1, cs2, label, label_dtype, ls0, ls1, ls2, D0, D1, D2, knots, basis, N, PA, PB, window, win_min,
                     win_max, straight_ct, straight_label, presence, presence_bytes, spacing, stream);
}

// order 3: the CT is sampled cubically from `coef`, hv_spline_prefilter's output for the whole scan ([D0][D1][D2] contiguous, the window fused
// in there); label, presence bits, coordinates and the outside rule are hv_straighten_sample_sp's
extern "C" int hv_straighten_sample_spline(const double* coef, const void* label, int label_dtype, long long ls0, long long ls1, long long ls2,
                                           int D0, int D1, int D2, const double* knots, const double* basis, int N, int PA, int PB,
                                           double* straight_ct, uint8_t* straight_label, uint64_t* presence, size_t presence_bytes,
                                           const double* spacing, void* stream) {
    return ss_sample(3, coef, HV_DT_F64, 0, 0, 0, label, label_dtype, ls0, ls1, ls2, D0, D1, D2, knots, basis, N, PA, PB, 0, 0.0, 1.0,
                     straight_ct, straight_label, presence, presence_bytes, spacing, stream);
}

// the entry from before the spacing: the scan is on a 1 mm grid (x / 1.0 is exact: the same bits)
extern "C" int hv_straighten_sample(const void* ct, int ct_dtype, long long cs0, long long cs1, long long cs2, const void* label, int label_dtype,
                                    long long ls0, long long ls1, long long ls2, int D0, int D1, int D2, const double* knots, const double* basis,
                                    int N, int PA, int PB, int window, double win_min, double win_max, double* straight_ct,
                                    uint8_t* straight_label, uint64_t* presence, size_t presence_bytes, void* stream) {
    const double ones[3] = {1.0, 1.0, 1.0};
    return hv_straighten_sample_sp(ct, ct_dtype, cs0, cs1, cs2, label, label_dtype, ls0, ls1, ls2, D0, D1, D2, knots, basis, N, PA, PB, window,
                                   win_min, win_max, straight_ct, straight_label, presence, presence_bytes, ones, stream);
}

extern "C" int hv_straighten_crop(const void* ct, int ct_dtype, long long cs0, long long cs1, long long cs2, const void* label, int label_dtype,
                                  long long ls0, long long ls1, long long ls2, int D1, int window, double win_min, double win_max,
                                  const uint64_t* presence, const int* boxes, int V, int O0, int O1, int O2, double* ct_out, uint8_t* label_out,
                                  void* stream) {
    if (!ct || !label || !presence || !boxes || !ct_out || !label_out || D1 <= 0 || V <= 0 || O0 <= 0 || O1 <= 0 || O2 <= 0 ||
        !ss_ct_dtype(ct_dtype) || !ss_label_dtype(label_dtype))
        return HV_ERR_ARG;
    const long long vol = (long long)O0 * O1 * O2;
    if (vol > 0x7fffffffLL * 64 || V > 65535) return HV_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(straighten_crop_kernel, dim3(hv_cdiv(vol, 256), V), dim3(256), 0, (hipStream_t)stream, ct, ct_dtype, cs0, cs1, cs2, label,
                       label_dtype, ls0, ls1, ls2, D1, window, win_min, win_max, (const u64*)presence, boxes, O0, O1, O2, ct_out, label_out);
    HV_LAUNCH_CHECK();
    return HV_OK;
}
