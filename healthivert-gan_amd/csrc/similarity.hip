// Joint intensity histograms of a fixed and a moving volume under a list of affine poses: hv_joint_hist, what mutual
// information and its normalised forms are computed from (Collignon 1995; Viola and Wells 1997; Studholme 1999).  For every fixed voxel o and
// every pose k, in this order:
//   1  mask != NULL and mask(o) == 0: in no pair, counted in info[k][2]
//   2  x = (double)fixed(o) not finite: in no pair, info[k][3]
//   3  u_h = ((o0 m[3h] + o1 m[3h+1]) + o2 m[3h+2]) + off[h], hv_resample's HV_RESAMPLE_MATRIX expression (float64, no fma, summed from 0.0)
//   4  rs_inside(u_h, A_h, HV_FILT_CONSTANT) on every axis; outside on any (a NaN fails it): not counted, info[k][4].  No cval: only the overlap
//   5  y = the sampler's float64 sum at order 0 / 1 / 3, hv_resample's (rs_taps, mirrored indices, last axis fastest, ((c w0) w1) w2 from 0.0),
//      no output conversion; y not finite: not counted, info[k][3]
//   6  levels by hv_glcm's rule, t = (x - flo) / fwidth, 0 if t < 0, Gf - 1 if t >= Gf, else (int)t; the same for y: out[k][lf][lm] += 1
//
//   jh_init_kernel          out and info zeroed
//   joint_hist_kernel<T, ORDER>  T the moving dtype (the fixed dtype is a wave-uniform switch on one load per voxel).  A workgroup of 256 lanes
//                           walks tpb RS_T^3 tiles of the fixed lattice, lanes laid out as resample_kernel's (role L the fixed axis whose image in
//                           the moving volume has the smallest stride, summed over the poses; then M; two voxels RS_T / 2 apart along O).  A lane
//                           reads fixed(o) and mask(o) once per pass and loops over the pass's poses, which lie in the kernel arguments.  Counts go
//                           to the workgroup's LDS tables [pose][Gf][Gm] of 32-bit counters, as many poses per pass as fit 64 KiB (texture.hip's
//                           budget) beside the info words; a wave whose counting lanes all hit one bin (air, saturated bone, a constant pair) adds
//                           once for the wave.  The info words are counted per wave with ballots and added to LDS by one lane.  Tables are flushed
//                           once per workgroup and pass, non-zero bins only, as 64-bit global atomicAdd; the info words once per workgroup.
//   jh_final_kernel         one lane per pose: HV_LS_NONFINITE and HV_LS_EMPTY into info[k][0]
// The tap loop is resample_kernel's restated, as in warp.hip: sharing one function with resample_kernel changed its order-3 register
// allocation.  Only integer atomics, so the result does not depend on the order of anything; every word of out and info that is read was
// written by an earlier launch of the same call.  No host synchronisation, no workspace.  Every moving index is formed from a coordinate already
// tested to lie in [0, A - 1], every fixed and mask index from a voxel index below the extents, every table index from clamped levels.
#include "resample_core.h"
#include "volume_access.h"                    // hv_finite

#define JH_THREADS RS_THREADS
#define JH_MAX_PART 1024                      // workgroups at most
#define JH_LDS_BYTES 65536                    // dynamic LDS a launch may ask for without an attribute

struct JhP {
    const void* fix; const void* mov; const unsigned char* msk;
    long long f0, f1, f2, s0, s1, s2, k0, k1, k2;   // element strides by HOST axis: fixed, moving, mask
    int O0, O1, O2, A0, A1, A2;
    int fdt;
    int r0, r1, r2;                           // the role (0 = L, 1 = M, 2 = O) of fixed axis 0 / 1 / 2
    int nL, nM, nO;                           // the fixed extents by role
    int ntL, ntM, ntiles, tpb;                // tiles along L and M, tiles, tiles per workgroup
    int K, KC, Gf, Gm;                        // poses, poses per pass, levels
    double flo, fwidth, mlo, mwidth;
    double pose[HV_JH_MAX_POSES][12];         // matrix[9], offset[3]
};

__device__ __forceinline__ double jh_ld_dt(const void* p, int dt, long long o) {
    switch (dt) {
        case HV_DT_U8: return (double)((const uint8_t*)p)[o];
        case HV_DT_I16: return (double)((const int16_t*)p)[o];
        case HV_DT_F32: return (double)((const float*)p)[o];
        default: return ((const double*)p)[o];
    }
}

// the sum over the taps at (u0, u1, u2), each already inside [0, A - 1]: resample_kernel's tap loop restated (see warp.hip's wp_sample)
template <typename T, int ORDER>
__device__ __forceinline__ double jh_sample(const T* src, double u0, double u1, double u2, int A0, int A1, int A2, long long s0, long long s1,
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

__global__ __launch_bounds__(JH_THREADS) void jh_init_kernel(u64* __restrict__ out, int nout, u64* __restrict__ info, int ninfo) {
    const int g = blockIdx.x * JH_THREADS + threadIdx.x, step = gridDim.x * JH_THREADS;
    for (int e = g; e < nout; e += step) out[e] = 0ull;
    for (int e = g; e < ninfo; e += step) info[e] = 0ull;
}

__device__ __forceinline__ unsigned jh_votes(bool p) { return (unsigned)__popcll(__ballot(p)); }

// LDS: tbl [KC][Gf][Gm] u32 | s_info [K][HV_JH_INFO] u32
template <typename T, int ORDER>
__global__ __launch_bounds__(JH_THREADS) void joint_hist_kernel(JhP P, u64* __restrict__ out, u64* __restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) unsigned char jh_lds[];
    const int G2 = P.Gf * P.Gm;
    unsigned* tbl = (unsigned*)jh_lds;
    unsigned* s_info = tbl + P.KC * G2;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int e = tid; e < P.KC * G2; e += JH_THREADS) tbl[e] = 0u;
    for (int e = tid; e < P.K * HV_JH_INFO; e += JH_THREADS) s_info[e] = 0u;
    __syncthreads();
    const T* mov = reinterpret_cast<const T*>(P.mov);
    const int tile0 = (int)blockIdx.x * P.tpb, tile1 = min(tile0 + P.tpb, P.ntiles);
    const int lL = tid % RS_T, lM = (tid / RS_T) % RS_T, lO = tid / (RS_T * RS_T);
    unsigned n_mask = 0u, n_fnf = 0u;                                // this wave's voxels in no pair whatever the pose (first pass)
    for (int c0 = 0; c0 < P.K; c0 += P.KC) {
        const int nd = min(P.KC, P.K - c0);
        for (int tile = tile0; tile < tile1; ++tile) {
            const int tL = tile % P.ntL, tM = (tile / P.ntL) % P.ntM, tO = tile / (P.ntL * P.ntM);
            const int gL = tL * RS_T + lL, gM = tM * RS_T + lM;
#pragma unroll 1
            for (int rep = 0; rep < 2; ++rep) {
                const int gO = tO * RS_T + lO + rep * (RS_T / 2);
                const bool live = gL < P.nL && gM < P.nM && gO < P.nO;
                if (__ballot(live) == 0ull) continue;                // wave-uniform
                const int i0 = rs_pick(P.r0, gL, gM, gO), i1 = rs_pick(P.r1, gL, gM, gO), i2 = rs_pick(P.r2, gL, gM, gO);
                bool masked = false, fnf = false, flow = false, fhigh = false;
                int lf = 0;
                if (live) {
                    masked = P.msk && P.msk[i0 * P.k0 + i1 * P.k1 + i2 * P.k2] == 0;
                    if (!masked) {
                        const double x = jh_ld_dt(P.fix, P.fdt, i0 * P.f0 + i1 * P.f1 + i2 * P.f2);
                        if (hv_finite(x)) {
                            const double t = (x - P.flo) / P.fwidth;
                            flow = t < 0.0;
                            fhigh = t >= (double)P.Gf;
                            lf = flow ? 0 : (fhigh ? P.Gf - 1 : (int)t);
                        } else {
                            fnf = true;
                        }
                    }
                }
                const bool valid = live && !masked && !fnf;
                if (c0 == 0) {
                    n_mask += jh_votes(masked);
                    n_fnf += jh_votes(fnf);
                }
                if (__ballot(valid) == 0ull) continue;
                const double c0d = (double)i0, c1d = (double)i1, c2d = (double)i2;
#pragma unroll 1
                for (int dd = 0; dd < nd; ++dd) {
                    const double* m = P.pose[c0 + dd];
                    double u0 = (((0.0 + c0d * m[0]) + c1d * m[1]) + c2d * m[2]) + m[9];
                    double u1 = (((0.0 + c0d * m[3]) + c1d * m[4]) + c2d * m[5]) + m[10];
                    double u2 = (((0.0 + c0d * m[6]) + c1d * m[7]) + c2d * m[8]) + m[11];
                    const bool in0 = rs_inside(u0, P.A0, HV_FILT_CONSTANT), in1 = rs_inside(u1, P.A1, HV_FILT_CONSTANT),
                               in2 = rs_inside(u2, P.A2, HV_FILT_CONSTANT);
                    const bool in = in0 && in1 && in2;
                    bool cnt = false, ynf = false, mcl = false;
                    int bin = 0;
                    if (valid && in) {
                        const double y = jh_sample<T, ORDER>(mov, u0, u1, u2, P.A0, P.A1, P.A2, P.s0, P.s1, P.s2);
                        if (hv_finite(y)) {
                            const double t = (y - P.mlo) / P.mwidth;
                            const bool low = t < 0.0, high = t >= (double)P.Gm;
                            mcl = low || high;
                            bin = lf * P.Gm + (low ? 0 : (high ? P.Gm - 1 : (int)t));
                            cnt = true;
                        } else {
                            ynf = true;
                        }
                    }
                    const u64 act = __ballot(cnt);
                    if (act != 0ull) {                               // wave-uniform
                        unsigned* t = tbl + dd * G2;
                        const int first = __ffsll((long long)act) - 1;
                        const int b0 = __shfl(bin, first, 64);
                        if (__ballot(cnt && bin != b0) == 0ull) {    // one bin for the whole wave: one add
                            if (lane == first) atomicAdd(&t[b0], (unsigned)__popcll(act));
                        } else if (cnt) {
                            atomicAdd(&t[bin], 1u);
                        }
                    }
                    const unsigned n_out = jh_votes(valid && !in), n_ynf = jh_votes(ynf), n_lo = jh_votes(cnt && flow),
                                   n_hi = jh_votes(cnt && fhigh), n_mc = jh_votes(mcl);
                    if (lane == 0) {
                        unsigned* w = s_info + (c0 + dd) * HV_JH_INFO;
                        if (act != 0ull) atomicAdd(&w[1], (unsigned)__popcll(act));
                        if (n_ynf) atomicAdd(&w[3], n_ynf);
                        if (n_out) atomicAdd(&w[4], n_out);
                        if (n_lo) atomicAdd(&w[5], n_lo);
                        if (n_hi) atomicAdd(&w[6], n_hi);
                        if (n_mc) atomicAdd(&w[7], n_mc);
                    }
                }
            }
        }
        __syncthreads();                                             // every add of this pass has landed
        for (int e = tid; e < nd * G2; e += JH_THREADS) {
            const unsigned c = tbl[e];
            if (c == 0u) continue;
            tbl[e] = 0u;
            atomicAdd(&out[(long long)c0 * G2 + e], (u64)c);
        }
        __syncthreads();
    }
    if (lane == 0 && (n_mask | n_fnf))
        for (int k = 0; k < P.K; ++k) {
            if (n_mask) atomicAdd(&s_info[k * HV_JH_INFO + 2], n_mask);
            if (n_fnf) atomicAdd(&s_info[k * HV_JH_INFO + 3], n_fnf);
        }
    __syncthreads();
    for (int e = tid; e < P.K * HV_JH_INFO; e += JH_THREADS) {
        const unsigned w = s_info[e];
        if (w != 0u) atomicAdd(&info[e], (u64)w);
    }
}

__global__ __launch_bounds__(64) void jh_final_kernel(int K, u64* __restrict__ info) {
    const int k = threadIdx.x;
    if (k >= K) return;
    u64* w = info + k * HV_JH_INFO;
    w[0] = (u64)((w[3] ? HV_LS_NONFINITE : 0) | (w[1] ? 0 : HV_LS_EMPTY));
}

// ------------------------------------------------------------------------------------------------ host side
static inline bool jh_sizes_ok(int O0, int O1, int O2, int K, int Gf, int Gm) {
    return O0 > 0 && O1 > 0 && O2 > 0 && K >= 1 && K <= HV_JH_MAX_POSES && Gf >= 2 && Gf <= HV_JH_MAX_LEVELS && Gm >= 2 && Gm <= HV_JH_MAX_LEVELS;
}

// nothing is needed beside the LDS tables: 0 for every size
extern "C" size_t hv_joint_hist_workspace_bytes(int O0, int O1, int O2, int K, int Gf, int Gm) {
    (void)O0; (void)O1; (void)O2; (void)K; (void)Gf; (void)Gm;
    return 0;
}

template <typename T>
static void jh_launch(int order, dim3 grid, size_t lds, hipStream_t st, const JhP& P, u64* out, u64* info) {
    if (order == 0) hipLaunchKernelGGL((joint_hist_kernel<T, 0>), grid, dim3(JH_THREADS), lds, st, P, out, info);
    else hipLaunchKernelGGL((joint_hist_kernel<T, 1>), grid, dim3(JH_THREADS), lds, st, P, out, info);
}

extern "C" int hv_joint_hist(const void* fixed, int fixed_dtype, long long fs0, long long fs1, long long fs2, int O0, int O1, int O2,
                             const void* moving, int moving_dtype, long long ms0, long long ms1, long long ms2, int A0, int A1, int A2,
                             const void* mask, long long ks0, long long ks1, long long ks2, const double* poses, int K, int order, double flo,
                             double fwidth, int Gf, double mlo, double mwidth, int Gm, long long* out, long long* info, void* workspace,
                             size_t workspace_bytes, void* stream) {
    (void)workspace_bytes;                                           // nothing is queried, so nothing can be too small
    if (!fixed || !moving || !poses || !out || !info || A0 <= 0 || A1 <= 0 || A2 <= 0 || !jh_sizes_ok(O0, O1, O2, K, Gf, Gm) ||
        !rs_dtype_ok(fixed_dtype) || !rs_dtype_ok(moving_dtype) || (order != 0 && order != 1 && order != 3) ||
        (order == 3 && moving_dtype != HV_DT_F64) || !std::isfinite(flo) || !std::isfinite(mlo) || !std::isfinite(fwidth) || !(fwidth > 0.0) ||
        !std::isfinite(mwidth) || !(mwidth > 0.0))
        return HV_ERR_ARG;
    for (int i = 0; i < 12 * K; ++i)
        if (!std::isfinite(poses[i])) return HV_ERR_ARG;
    if (((uintptr_t)fixed & (rs_elem(fixed_dtype) - 1)) || ((uintptr_t)moving & (rs_elem(moving_dtype) - 1)) || ((uintptr_t)out & 7) ||
        ((uintptr_t)info & 7) || ((uintptr_t)workspace & 15))
        return HV_ERR_ARG;
    if ((long long)A0 * A1 * A2 > (1LL << 30) || (long long)O0 * O1 * O2 > (1LL << 30)) return HV_ERR_UNSUPPORTED;
    const int A[3] = {A0, A1, A2}, O[3] = {O0, O1, O2};
    const long long fs[3] = {fs0, fs1, fs2}, ms[3] = {ms0, ms1, ms2}, ks[3] = {ks0, ks1, ks2};
    const long long nout = (long long)K * Gf * Gm * 8, ninfo = (long long)K * HV_JH_INFO * 8;
    long long lo, hi;
    rs_span(O, fs, rs_elem(fixed_dtype), &lo, &hi);
    if (rs_meet(fixed, lo, hi, out, 0, nout) || rs_meet(fixed, lo, hi, info, 0, ninfo)) return HV_ERR_ARG;
    rs_span(A, ms, rs_elem(moving_dtype), &lo, &hi);
    if (rs_meet(moving, lo, hi, out, 0, nout) || rs_meet(moving, lo, hi, info, 0, ninfo)) return HV_ERR_ARG;
    if (mask) {
        rs_span(O, ks, 1, &lo, &hi);
        if (rs_meet(mask, lo, hi, out, 0, nout) || rs_meet(mask, lo, hi, info, 0, ninfo)) return HV_ERR_ARG;
    }
    if (rs_meet(out, 0, nout, info, 0, ninfo)) return HV_ERR_ARG;
    JhP P;
    P.fix = fixed; P.mov = moving; P.msk = (const unsigned char*)mask;
    P.f0 = fs0; P.f1 = fs1; P.f2 = fs2; P.s0 = ms0; P.s1 = ms1; P.s2 = ms2; P.k0 = ks0; P.k1 = ks1; P.k2 = ks2;
    P.O0 = O0; P.O1 = O1; P.O2 = O2; P.A0 = A0; P.A1 = A1; P.A2 = A2;
    P.fdt = fixed_dtype;
    P.K = K; P.Gf = Gf; P.Gm = Gm;
    P.flo = flo; P.fwidth = fwidth; P.mlo = mlo; P.mwidth = mwidth;
    // the roles: L the fixed axis whose unit step moves least far in the moving volume, summed over the poses (those of one search lie close
    // to each other; an axis of extent 1 comes last), then M, then O
    double key[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < HV_JH_MAX_POSES; ++k)
        for (int i = 0; i < 12; ++i) P.pose[k][i] = k < K ? poses[12 * k + i] : 0.0;
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < 3; ++j)
            for (int h = 0; h < 3; ++h) key[j] += std::fabs(P.pose[k][3 * h + j]) * (double)rs_abs(ms[h]);
    int ord[3], role[3];
    rs_roles(O, key, ord);
    for (int r = 0; r < 3; ++r) role[ord[r]] = r;
    P.r0 = role[0]; P.r1 = role[1]; P.r2 = role[2];
    P.nL = O[ord[0]]; P.nM = O[ord[1]]; P.nO = O[ord[2]];
    P.ntL = hv_cdiv(P.nL, RS_T); P.ntM = hv_cdiv(P.nM, RS_T);
    const long long nt = (long long)P.ntL * P.ntM * hv_cdiv(P.nO, RS_T);      // <= 2^30 voxels: fits an int
    P.ntiles = (int)nt;
    P.tpb = hv_cdiv(nt, JH_MAX_PART);
    const int blocks = hv_cdiv(nt, P.tpb);
    // as many poses per pass as fit beside the info words, the passes of equal length: 64 x 64 levels take 16 KiB a pose, so at least 3 fit
    const size_t table = (size_t)Gf * Gm * 4, words = (size_t)K * HV_JH_INFO * 4;
    const int fit = (int)((JH_LDS_BYTES - words) / table);
    const int passes = hv_cdiv(K, fit < K ? fit : K);
    P.KC = hv_cdiv(K, passes);
    const size_t lds = (size_t)P.KC * table + words;
    hipStream_t st = (hipStream_t)stream;
    u64* o = (u64*)out;
    u64* inf = (u64*)info;
    const int no = K * Gf * Gm, ni = K * HV_JH_INFO;
    hipLaunchKernelGGL(jh_init_kernel, dim3(hv_cdiv(no + ni, JH_THREADS * 4)), dim3(JH_THREADS), 0, st, o, no, inf, ni);
    HV_LAUNCH_CHECK();
    const dim3 grid((unsigned)blocks);
    if (order == 3) hipLaunchKernelGGL((joint_hist_kernel<double, 3>), grid, dim3(JH_THREADS), lds, st, P, o, inf);
    else switch (moving_dtype) {
        case HV_DT_U8: jh_launch<uint8_t>(order, grid, lds, st, P, o, inf); break;
        case HV_DT_I16: jh_launch<int16_t>(order, grid, lds, st, P, o, inf); break;
        case HV_DT_F32: jh_launch<float>(order, grid, lds, st, P, o, inf); break;
        default: jh_launch<double>(order, grid, lds, st, P, o, inf); break;
    }
    HV_LAUNCH_CHECK();
    hipLaunchKernelGGL(jh_final_kernel, dim3(1), dim3(64), 0, st, K, inf);
    HV_LAUNCH_CHECK();
    return HV_OK;
}
