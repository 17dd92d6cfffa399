// Parallel-beam projections of a resident volume under a list of affine poses: hv_project, what a radiograph
// (line integral), a maximum / minimum intensity projection, a thickness map and an areal density are computed from.  A projection is
// hv_resample's HV_RESAMPLE_MATRIX lattice (p0, p1, t) reduced over t without ever being written.  Per pose k, pixel (p0, p1) and step
// t = 0 .. T - 1, in float64 without fma, in this order:
//   1  u_h = ((p0 m[3h] + p1 m[3h+1]) + t m[3h+2]) + off[h], summed from 0.0, the offset last
//   2  rs_inside(u_h, A_h, HV_FILT_CONSTANT) on every axis; outside on any (a NaN fails it): info[k][2].  Nothing is padded
//   3  label != NULL and (double)label(q) != label_value, q_h = floor(u_h + 0.5): info[k][3]
//   4  y = the sampler's float64 sum at order 0 / 1 / 3, hv_resample's (rs_taps, mirrored indices, last axis fastest, ((c w0) w1) w2 from 0.0),
//      no output conversion; y not finite: info[k][4]
//   5  otherwise the sample is counted: info[k][1]
// Per pixel over the counted samples: the sum in chunks of HV_PROJ_CHUNK consecutive t -- a chunk's sum sequentially from +0.0 in increasing
// t, the chunk sums added sequentially from +0.0 in increasing chunk order, every chunk, the empty ones too; min and max by value, stored
// as m + 0.0; count, first and last counted t.  That order is the definition: it is what lets R lanes share a ray and still give one set of
// bytes.
//
//   pj_init_kernel            info zeroed
//   project_kernel<T, ORDER>  One workgroup of 256 lanes takes PX pixels of one pose (blockIdx.y), R = 256 / PX lanes per ray.  In a pass the R
//                             lanes of a ray take R consecutive chunks, each lane its chunk sequentially; the chunk sums go through LDS and the
//                             ray's first lane adds them onto the running sum in chunk order: R dependent adds per 16 R samples.  A lane whose
//                             chunk starts at or after T hands over +0.0, which leaves the running sum's bits alone (the sum starts at +0.0 and
//                             so is never -0.0).  Which lattice axis runs along adjacent lanes is rs_roles' choice on the image strides summed
//                             over the poses: t (the ray runs along the volume's contiguous axis; PX = 16 pixels along the detector axis with
//                             the smaller image, R = 16, lane = pixel * R + r) or a detector axis (PX = 64 pixels along it, R = 4, lane =
//                             r * PX + pixel: a wave reads 64 neighbouring pixels at one t).  min, max, count, first and last are folded over
//                             the R lanes once, at the end, through LDS.  A ray of fewer chunks than that takes the power of two of lanes
//                             that covers them (R = 1 for T <= 16) and the workgroup 256 / R pixels, so that short rays idle no lanes.
//                             The four info words are counted per lane, summed over the wave with shuffles, added to LDS by one lane per
//                             wave and flushed once per workgroup as 64-bit integer atomicAdd.
//   pj_final_kernel           one lane per pose: HV_LS_NONFINITE and HV_LS_EMPTY into info[k][0]
// The tap loop is resample_kernel's restated (jh_sample, wp_sample): resample.o's device code is not touched.  Only integer atomics and no
// float atomics; every pixel's six words are written by exactly one lane; no host synchronisation, no workspace, no scratch.  Every volume
// index is formed from a coordinate already tested to lie in [0, A - 1], every label index from floor(u + 0.5) of such coordinates, every
// output index from a pixel index below the detector's extents.
#include "resample_core.h"
#include "volume_access.h"                    // hv_ld_dt, hv_finite

#define PJ_THREADS RS_THREADS
#define PJ_PX_RAY 16                          // pixels per workgroup at the most lanes per ray when t runs along adjacent lanes
#define PJ_PX_DET 64                          // ... when a detector axis does

struct PjP {
    const void* vol; const void* lab;
    long long s0, s1, s2, l0, l1, l2;        // element strides: volume, label
    int A0, A1, A2, P0, P1, T;
    int ldt;                                  // label dtype
    int K;
    int ray;                                  // 1: t along adjacent lanes, 0: detector axis `fast`
    int fast;                                 // the detector axis the pixels of a workgroup lie along
    int ntf;                                  // tiles along it
    int R;                                    // lanes per ray, a power of two
    int npass;                                // passes of R chunks
    double lval;
    double pose[HV_PROJ_MAX_POSES][12];       // matrix[9], offset[3]
};

// the sum over the taps at (u0, u1, u2), each already inside [0, A - 1]: resample_kernel's tap loop restated
template <typename T, int ORDER>
__device__ __forceinline__ double pj_sample(const T* src, double u0, double u1, double u2, int A0, int A1, int A2, long long s0, long long s1,
                                            long long s2) {
    constexpr int NT = ORDER + 1;
    long long o0[NT], o1[NT], o2[NT];
    double w0[NT], w1[NT], w2[NT];
    rs_taps<ORDER>(u0, A0, s0, o0, w0);
    rs_taps<ORDER>(u1, A1, s1, o1, w1);
    rs_taps<ORDER>(u2, A2, s2, o2, w2);
    double t = 0.0;
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
    return t;
}

__global__ __launch_bounds__(64) void pj_init_kernel(int n, u64* __restrict__ info) {
    for (int e = threadIdx.x; e < n; e += 64) info[e] = 0ull;
}

__device__ __forceinline__ unsigned pj_wave_sum(unsigned v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (unsigned)__shfl_down((int)v, off, 64);
    return v;                                                         // lane 0 holds the wave's sum
}

template <typename T, int ORDER>
__global__ __launch_bounds__(PJ_THREADS) void project_kernel(PjP P, double* __restrict__ acc, int* __restrict__ idx, u64* __restrict__ info) {
    __shared__ double s_a[PJ_THREADS], s_b[PJ_THREADS];
    __shared__ int s_c[PJ_THREADS], s_f[PJ_THREADS], s_l[PJ_THREADS];
    __shared__ unsigned s_info[4];
    const int tid = threadIdx.x, k = blockIdx.y;
    const int R = P.R, PX = PJ_THREADS / R;
    const int px = P.ray ? tid / R : tid % PX, r = P.ray ? tid % R : tid / PX;
    const int sr = P.ray ? 1 : PX, sb = P.ray ? px * R : px;        // the LDS slot of (px, j) is sb + j * sr; this lane's is tid
    if (tid < 4) s_info[tid] = 0u;
    const int tile = blockIdx.x, tf = tile % P.ntf, tother = tile / P.ntf;
    const int pf = tf * PX + px;
    const int p0 = P.fast == 0 ? pf : tother, p1 = P.fast == 0 ? tother : pf;
    const bool live = p0 < P.P0 && p1 < P.P1;
    const T* vol = reinterpret_cast<const T*>(P.vol);
    const double* m = P.pose[k];
    const double d0 = (double)p0, d1 = (double)p1;
    const double a0 = (0.0 + d0 * m[0]) + d1 * m[1], a1 = (0.0 + d0 * m[3]) + d1 * m[4], a2 = (0.0 + d0 * m[6]) + d1 * m[7];
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double run = 0.0, mn = inf, mx = -inf;
    int cnt = 0, first = P.T, last = -1;
    unsigned n_out = 0u, n_lab = 0u, n_nf = 0u;
    for (int pass = 0; pass < P.npass; ++pass) {
        const int t0 = (pass * R + r) * HV_PROJ_CHUNK;
        double cs = 0.0;
        if (live && t0 < P.T) {
            const int t1 = min(t0 + HV_PROJ_CHUNK, P.T);
#pragma unroll 1
            for (int t = t0; t < t1; ++t) {
                const double dt = (double)t;
                double u0 = (a0 + dt * m[2]) + m[9], u1 = (a1 + dt * m[5]) + m[10], u2 = (a2 + dt * m[8]) + m[11];
                if (!(rs_inside(u0, P.A0, HV_FILT_CONSTANT) && rs_inside(u1, P.A1, HV_FILT_CONSTANT) && rs_inside(u2, P.A2, HV_FILT_CONSTANT))) {
                    ++n_out;
                    continue;
                }
                if (P.lab) {
                    const long long q = (long long)floor(u0 + 0.5) * P.l0 + (long long)floor(u1 + 0.5) * P.l1 + (long long)floor(u2 + 0.5) * P.l2;
                    if (hv_ld_dt(P.lab, P.ldt, q) != P.lval) {
                        ++n_lab;
                        continue;
                    }
                }
                const double y = pj_sample<T, ORDER>(vol, u0, u1, u2, P.A0, P.A1, P.A2, P.s0, P.s1, P.s2);
                if (!hv_finite(y)) {
                    ++n_nf;
                    continue;
                }
                cs = cs + y;
                mn = y < mn ? y : mn;
                mx = y > mx ? y : mx;
                ++cnt;
                first = min(first, t);
                last = t;
            }
        }
        s_a[tid] = cs;
        __syncthreads();
        if (r == 0)
            for (int j = 0; j < R; ++j) run = run + s_a[sb + j * sr];  // chunk order: the definition
        __syncthreads();
    }
    s_a[tid] = mn; s_b[tid] = mx; s_c[tid] = cnt; s_f[tid] = first; s_l[tid] = last;
    __syncthreads();
    if (r == 0 && live) {
        for (int j = 1; j < R; ++j) {
            const int e = sb + j * sr;
            const double a = s_a[e], b = s_b[e];
            mn = a < mn ? a : mn;
            mx = b > mx ? b : mx;
            cnt += s_c[e];
            first = min(first, s_f[e]);
            last = max(last, s_l[e]);
        }
        const long long np = (long long)P.P0 * P.P1, o = (long long)k * 3 * np + (long long)p0 * P.P1 + p1;
        acc[o] = run;
        acc[o + np] = mn + 0.0;
        acc[o + 2 * np] = mx + 0.0;
        idx[o] = cnt;
        idx[o + np] = first;
        idx[o + 2 * np] = last;
    }
    const unsigned mine = (unsigned)s_c[tid];                        // this lane's own count, as it was before the fold
    const unsigned w_cnt = pj_wave_sum(mine), w_out = pj_wave_sum(n_out), w_lab = pj_wave_sum(n_lab), w_nf = pj_wave_sum(n_nf);
    if ((tid & 63) == 0) {
        if (w_cnt) atomicAdd(&s_info[0], w_cnt);
        if (w_out) atomicAdd(&s_info[1], w_out);
        if (w_lab) atomicAdd(&s_info[2], w_lab);
        if (w_nf) atomicAdd(&s_info[3], w_nf);
    }
    __syncthreads();
    if (tid < 4) {
        const unsigned w = s_info[tid];
        if (w != 0u) atomicAdd(&info[k * HV_PROJ_INFO + 1 + tid], (u64)w);
    }
}

__global__ __launch_bounds__(64) void pj_final_kernel(int K, u64* __restrict__ info) {
    const int k = threadIdx.x;
    if (k >= K) return;
    u64* w = info + k * HV_PROJ_INFO;
    w[0] = (u64)((w[4] ? HV_LS_NONFINITE : 0) | (w[1] ? 0 : HV_LS_EMPTY));
}

// ------------------------------------------------------------------------------------------------ host side
// dims[5]: HV_PROJ_CHUNK; the pixels per workgroup and the lanes per ray R when t runs along adjacent lanes; the same two when a detector
// axis does, each for a ray of at least R chunks (a shorter one: R the power of two that covers ceil(T / HV_PROJ_CHUNK), 256 / R pixels).
// A pass covers HV_PROJ_CHUNK * R steps of a ray.
extern "C" int hv_project_tile(int* dims) {
    if (!dims) return HV_ERR_ARG;
    dims[0] = HV_PROJ_CHUNK;
    dims[1] = PJ_PX_RAY; dims[2] = PJ_THREADS / PJ_PX_RAY;
    dims[3] = PJ_PX_DET; dims[4] = PJ_THREADS / PJ_PX_DET;
    return HV_OK;
}

// the running sums live in registers and LDS: 0 for every size
extern "C" size_t hv_project_workspace_bytes(int A0, int A1, int A2, int K, int P0, int P1, int T) {
    (void)A0; (void)A1; (void)A2; (void)K; (void)P0; (void)P1; (void)T;
    return 0;
}

template <typename T>
static void pj_launch(int order, dim3 grid, hipStream_t st, const PjP& P, double* acc, int* idx, u64* info) {
    if (order == 0) hipLaunchKernelGGL((project_kernel<T, 0>), grid, dim3(PJ_THREADS), 0, st, P, acc, idx, info);
    else hipLaunchKernelGGL((project_kernel<T, 1>), grid, dim3(PJ_THREADS), 0, st, P, acc, idx, info);
}

extern "C" int hv_project(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, const void* label,
                          int label_dtype, long long ls0, long long ls1, long long ls2, double label_value, const double* poses, int K,
                          int P0, int P1, int T, int order, double* acc, int* idx, long long* info, void* workspace, size_t workspace_bytes,
                          void* stream) {
    (void)workspace_bytes;                                           // nothing is queried, so nothing can be too small
    if (!vol || !poses || !acc || !idx || !info || A0 <= 0 || A1 <= 0 || A2 <= 0 || P0 <= 0 || P1 <= 0 || T <= 0 || K < 1 ||
        K > HV_PROJ_MAX_POSES || !rs_dtype_ok(dtype) || (order != 0 && order != 1 && order != 3) || (order == 3 && dtype != HV_DT_F64))
        return HV_ERR_ARG;
    if (!std::isfinite(label_value) || (label && (label_dtype < HV_DT_U8 || label_dtype > HV_DT_F64))) return HV_ERR_ARG;
    for (int i = 0; i < 12 * K; ++i)
        if (!std::isfinite(poses[i])) return HV_ERR_ARG;
    const size_t lelem = !label ? 1 : label_dtype == HV_DT_I32 ? 4 : label_dtype == HV_DT_I64 ? 8 : rs_elem(label_dtype);
    if (((uintptr_t)vol & (rs_elem(dtype) - 1)) || ((uintptr_t)label & (lelem - 1)) || ((uintptr_t)acc & 7) || ((uintptr_t)idx & 3) ||
        ((uintptr_t)info & 7) || ((uintptr_t)workspace & 15))
        return HV_ERR_ARG;
    if ((long long)A0 * A1 * A2 > (1LL << 30) || (long long)P0 * P1 > (1LL << 30) || (long long)P0 * P1 * T > (1LL << 30)) return HV_ERR_UNSUPPORTED;
    const int A[3] = {A0, A1, A2}, O[3] = {P0, P1, T};
    const long long ss[3] = {s0, s1, s2}, ls[3] = {ls0, ls1, ls2};
    const long long nacc = (long long)K * 3 * P0 * P1 * 8, nidx = (long long)K * 3 * P0 * P1 * 4, ninfo = (long long)K * HV_PROJ_INFO * 8;
    const void* outs[3] = {acc, idx, info};
    const long long nout[3] = {nacc, nidx, ninfo};
    long long vlo, vhi, llo = 0, lhi = 0;
    rs_span(A, ss, rs_elem(dtype), &vlo, &vhi);
    if (label) rs_span(A, ls, lelem, &llo, &lhi);
    for (int a = 0; a < 3; ++a) {
        if (rs_meet(vol, vlo, vhi, outs[a], 0, nout[a])) return HV_ERR_ARG;
        if (label && rs_meet(label, llo, lhi, outs[a], 0, nout[a])) return HV_ERR_ARG;
        for (int b = a + 1; b < 3; ++b)
            if (rs_meet(outs[a], 0, nout[a], outs[b], 0, nout[b])) return HV_ERR_ARG;
    }
    PjP P;
    P.vol = vol; P.lab = label;
    P.s0 = s0; P.s1 = s1; P.s2 = s2; P.l0 = ls0; P.l1 = ls1; P.l2 = ls2;
    P.A0 = A0; P.A1 = A1; P.A2 = A2; P.P0 = P0; P.P1 = P1; P.T = T;
    P.ldt = label_dtype; P.K = K; P.lval = label_value;
    for (int k = 0; k < HV_PROJ_MAX_POSES; ++k)
        for (int i = 0; i < 12; ++i) P.pose[k][i] = k < K ? poses[12 * k + i] : 0.0;
    // the roles: L the lattice axis whose unit step moves least far in the volume, summed over the poses (an axis of extent 1 comes last)
    double key[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < 3; ++j)
            for (int h = 0; h < 3; ++h) key[j] += std::fabs(P.pose[k][3 * h + j]) * (double)rs_abs(ss[h]);
    int ord[3];
    rs_roles(O, key, ord);
    P.ray = ord[0] == 2;
    P.fast = P.ray ? ord[1] : ord[0];
    // R: the power of two that covers the ray's chunks, at most 16 (t along the lanes) or 4 (a detector axis along them)
    const int nchunks = hv_cdiv(T, HV_PROJ_CHUNK), rmax = PJ_THREADS / (P.ray ? PJ_PX_RAY : PJ_PX_DET);
    P.R = 1;
    while (P.R < rmax && P.R < nchunks) P.R *= 2;
    const int PX = PJ_THREADS / P.R;
    P.ntf = hv_cdiv(O[P.fast], PX);
    P.npass = hv_cdiv(nchunks, P.R);
    const long long tiles = (long long)P.ntf * O[1 - P.fast];         // <= 2^30 pixels: fits an int
    hipStream_t st = (hipStream_t)stream;
    u64* inf = (u64*)info;
    hipLaunchKernelGGL(pj_init_kernel, dim3(1), dim3(64), 0, st, K * HV_PROJ_INFO, inf);
    HV_LAUNCH_CHECK();
    const dim3 grid((unsigned)tiles, (unsigned)K);
    if (order == 3) hipLaunchKernelGGL((project_kernel<double, 3>), grid, dim3(PJ_THREADS), 0, st, P, acc, idx, inf);
    else switch (dtype) {
        case HV_DT_U8: pj_launch<uint8_t>(order, grid, st, P, acc, idx, inf); break;
        case HV_DT_I16: pj_launch<int16_t>(order, grid, st, P, acc, idx, inf); break;
        case HV_DT_F32: pj_launch<float>(order, grid, st, P, acc, idx, inf); break;
        default: pj_launch<double>(order, grid, st, P, acc, idx, inf); break;
    }
    HV_LAUNCH_CHECK();
    hipLaunchKernelGGL(pj_final_kernel, dim3(1), dim3(64), 0, st, K, inf);
    HV_LAUNCH_CHECK();
    return HV_OK;
}
