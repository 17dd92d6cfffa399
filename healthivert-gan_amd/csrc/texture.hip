// Per-label 3-D grey-level co-occurrence matrices of V volumes on the device: hv_glcm.  For every listed label value
// of every volume and every offset d: out[v][s][d][a][b] = the number of voxel pairs (p, p + d), both inside the volume and both of slot s, with
// level(p) = a and level(p + d) = b (Haralick 1973; skimage.feature.graycomatrix in three dimensions, restricted to a label).  HV_GLCM_SYMMETRIC
// adds the transpose.  The slot of a voxel is hv_label_stats' (mask, label value -> slot table in the kernel arguments); its level is
// t = ((double)v - lo) / width clamped to [0, G - 1] and truncated; a NaN or infinity belongs to no pair and marks its slot.
//
//   glcm_init_kernel      out, info and the per-volume bad-label words zeroed
//   glcm_count_kernel<T>  a workgroup walks tpb 16 x 16 x 16 tiles.  Per tile: the tile and a halo of the offsets' reach per axis are staged in LDS
//                         as 16-bit (slot, level) codes (GLCM_NONE: outside the volume, no slot, not finite), the staging loop's fastest index on
//                         the logical axis with the smallest stride of vol.  A thread owns one row of 16 voxels along axis 2 and, per offset, folds
//                         runs of one bin in a register before it adds to the workgroup's LDS tables ([offset][G][G] 32-bit counters, as many
//                         offsets per pass as fit 64 KiB beside the staging).  The tables belong to one slot at a time and are flushed -- non-zero
//                         bins only, 64-bit global atomicAdd, the transposed bin as well when symmetric -- when the slot changes or the
//                         workgroup's tiles end: a workgroup inside one vertebra flushes once per pass.  The slot's voxel and clamp counts and its
//                         non-finite flag are gathered the same way (register runs, LDS, one global atomic per workgroup and word).
//   glcm_final_kernel     one lane per (volume, slot): HV_LS_BAD_LABEL and HV_LS_EMPTY into the status word
// Only integer atomics, so the result does not depend on the order of anything; every word of out, info and the workspace that is read was
// written by an earlier launch of the same call.  No host synchronisation: the grids come from the shape.
#include <cmath>
#include "texture_code.h"                     // GL_NONE, the staged code of a voxel that is in no pair; else (slot << 6) | level

#define GL_THREADS 256
#define GL_T 16                               // tile edge
#define GL_MAX_PART 1024                      // workgroups per volume at most
#define GL_LDS_BYTES 65536                    // dynamic LDS a launch may ask for without an attribute

struct GlArgs {
    HvVol vol, lab, msk;                      // msk.p == NULL: no mask
    int V, A0, A1, A2, S, D, G, symmetric;
    double lo, width;
    int ax_in, ax_mid, ax_out;                // logical axes by ascending stride of vol
    int n1, n2, ntiles, tpb;                  // tiles along axes 1 and 2, tiles, tiles per workgroup
    int r0, r1, r2;                           // the offsets' reach per axis: the halo
    int E0, E1, E2, P2;                       // staged extents (16 + 2 r) and the row pitch in codes: P2 / 2 odd, rows spread over the banks
    int DC;                                   // offsets per pass
    unsigned stage_bytes;                     // the staging's bytes, a multiple of 16
    signed char off[HV_GLCM_MAX_OFFSETS][3];
    unsigned char slot[256];
};

__global__ __launch_bounds__(GL_THREADS) void glcm_init_kernel(u64* __restrict__ out, long long nout, u64* __restrict__ info, long long ninfo,
                                                               u64* __restrict__ vbad, int V) {
    const long long g = (long long)blockIdx.x * GL_THREADS + threadIdx.x, step = (long long)gridDim.x * GL_THREADS;
    for (long long e = g; e < nout; e += step) out[e] = 0ull;
    for (long long e = g; e < ninfo; e += step) info[e] = 0ull;
    for (long long e = g; e < V; e += step) vbad[e] = 0ull;
}

// the tables of slot s and offsets [c0, c0 + nd) added to out, and zeroed
__device__ __forceinline__ void gl_flush(const GlArgs& a, unsigned* tbl, int v, int s, int c0, int nd, u64* __restrict__ out) {
    const int G = a.G, G2 = G * G;
    for (int e = threadIdx.x; e < nd * G2; e += GL_THREADS) {
        const unsigned c = tbl[e];
        if (c == 0u) continue;
        tbl[e] = 0u;
        const int dd = e / G2, bin = e - dd * G2, lp = bin / G, lq = bin - lp * G;
        u64* o = out + (((long long)v * a.S + s) * a.D + (c0 + dd)) * G2;
        atomicAdd(&o[bin], (u64)c);
        if (a.symmetric) atomicAdd(&o[lq * G + lp], (u64)c);         // the diagonal is doubled: P + P^T
    }
}

// LDS: tbl [DC][G][G] u32 | st [E0][E1][P2] u16 | s_info [S][HV_GLCM_INFO] u32 | s_present [2] u32
template <typename T>
__global__ __launch_bounds__(GL_THREADS) void glcm_count_kernel(GlArgs a, u64* __restrict__ out, u64* __restrict__ info, u64* __restrict__ vbad) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gl_lds[];
    const int G = a.G, G2 = G * G;
    unsigned* tbl = (unsigned*)gl_lds;
    unsigned short* st = (unsigned short*)(gl_lds + (size_t)a.DC * G2 * 4);
    unsigned* s_info = (unsigned*)((unsigned char*)st + a.stage_bytes);
    unsigned* s_present = s_info + a.S * HV_GLCM_INFO;
    const int tid = threadIdx.x, v = blockIdx.y, b = blockIdx.x;
    for (int e = tid; e < a.DC * G2; e += GL_THREADS) tbl[e] = 0u;
    for (int e = tid; e < a.S * HV_GLCM_INFO; e += GL_THREADS) s_info[e] = 0u;
    const int tile_end = min((b + 1) * a.tpb, a.ntiles);
    const int E[3] = {a.E0, a.E1, a.E2};
    const int e_in = E[a.ax_in], e_mid = E[a.ax_mid], nstage = a.E0 * a.E1 * a.E2;
    const int ri = tid >> 4, rj = tid & (GL_T - 1);                  // this thread's row of the tile: (ri, rj, 0 .. 15)
    const int prow = ((ri + a.r0) * a.E1 + (rj + a.r1)) * a.P2 + a.r2;
    int bad = 0;
    GlRun run;
    run.slot = 0xFF; run.n = run.low = run.high = run.flag = 0u;
    for (int c0 = 0; c0 < a.D; c0 += a.DC) {
        const int nd = min(a.DC, a.D - c0);
        int cur = -1;                                                // the slot the tables count for (workgroup-uniform)
        for (int tile = b * a.tpb; tile < tile_end; ++tile) {
            const int i0 = (tile / (a.n1 * a.n2)) * GL_T, j0 = ((tile / a.n2) % a.n1) * GL_T, k0 = (tile % a.n2) * GL_T;
            __syncthreads();                                         // the previous tile's rows are read, the tables' first zeroes stand
            if (tid < 2) s_present[tid] = 0u;
            __syncthreads();
            for (int e = tid; e < nstage; e += GL_THREADS) {
                const int u = e % e_in, m = (e / e_in) % e_mid, o = e / (e_in * e_mid);
                const int di = a.ax_in == 0 ? u : (a.ax_mid == 0 ? m : o), dj = a.ax_in == 1 ? u : (a.ax_mid == 1 ? m : o),
                          dk = a.ax_in == 2 ? u : (a.ax_mid == 2 ? m : o);
                const int i = i0 + di - a.r0, j = j0 + dj - a.r1, k = k0 + dk - a.r2;
                unsigned code = GL_NONE;
                if (i >= 0 && i < a.A0 && j >= 0 && j < a.A1 && k >= 0 && k < a.A2) {
                    // a voxel of the tile itself (not of its halo) is this workgroup's to account for, in the first pass
                    const bool centre = di >= a.r0 && di < a.r0 + GL_T && dj >= a.r1 && dj < a.r1 + GL_T && dk >= a.r2 && dk < a.r2 + GL_T;
                    const bool own = centre && c0 == 0;
                    int nobad = 0;
                    const int s = hv_slot(a, v, i, j, k, own ? bad : nobad);
                    if (own && s != run.slot) {
                        gl_run_flush(run, s_info);
                        run.slot = s; run.n = run.low = run.high = run.flag = 0u;
                    }
                    if (s != 0xFF) {
                        const double x = (double)((const T*)a.vol.p)[v * a.vol.sv + i * a.vol.s0 + j * a.vol.s1 + k * a.vol.s2];
                        if (hv_finite(x)) {
                            const double t = (x - a.lo) / a.width;
                            const int lev = t < 0.0 ? 0 : (t >= (double)G ? G - 1 : (int)t);
                            code = (unsigned)(s << 6 | lev);
                            if (own) { ++run.n; run.low += t < 0.0 ? 1u : 0u; run.high += t >= (double)G ? 1u : 0u; }
                            if (centre && !(s_present[s >> 5] >> (s & 31) & 1u)) atomicOr(&s_present[s >> 5], 1u << (s & 31));
                        } else if (own) {
                            run.flag |= (unsigned)HV_LS_NONFINITE;
                        }
                    }
                }
                st[(di * a.E1 + dj) * a.P2 + dk] = (unsigned short)code;
            }
            __syncthreads();
            u64 pm = (u64)s_present[0] | ((u64)s_present[1] << 32);
            if (pm == 0ull) continue;
            unsigned short pc[GL_T];
#pragma unroll
            for (int k = 0; k < GL_T; ++k) pc[k] = st[prow + k];
            while (pm) {
                const int s = __ffsll((long long)pm) - 1;
                pm &= pm - 1;
                if (s != cur) {
                    if (cur >= 0) {
                        __syncthreads();                             // every add for the old slot has landed
                        gl_flush(a, tbl, v, cur, c0, nd, out);
                        __syncthreads();
                    }
                    cur = s;
                }
                bool any = false;
#pragma unroll
                for (int k = 0; k < GL_T; ++k) any |= (pc[k] >> 6) == (unsigned)s;
                if (!any) continue;
                for (int dd = 0; dd < nd; ++dd) {
                    const int d0 = a.off[c0 + dd][0], d1 = a.off[c0 + dd][1], d2 = a.off[c0 + dd][2];
                    const unsigned short* q = st + prow + (d0 * a.E1 + d1) * a.P2 + d2;
                    unsigned* t = tbl + dd * G2;
                    int rbin = -1;
                    unsigned rcnt = 0u;
#pragma unroll
                    for (int k = 0; k < GL_T; ++k) {
                        const unsigned qc = q[k];
                        int bin = -1;
                        if ((pc[k] >> 6) == (unsigned)s && (qc >> 6) == (unsigned)s) bin = (int)(pc[k] & 63u) * G + (int)(qc & 63u);
                        if (bin != rbin) {
                            if (rbin >= 0) atomicAdd(&t[rbin], rcnt);
                            rbin = bin; rcnt = 0u;
                        }
                        ++rcnt;
                    }
                    if (rbin >= 0) atomicAdd(&t[rbin], rcnt);
                }
            }
        }
        __syncthreads();
        if (cur >= 0) gl_flush(a, tbl, v, cur, c0, nd, out);
    }
    gl_run_flush(run, s_info);
    if (bad) atomicOr(&vbad[v], 1ull);
    __syncthreads();
    for (int e = tid; e < a.S * HV_GLCM_INFO; e += GL_THREADS) {
        const unsigned w = s_info[e];
        if (w == 0u) continue;
        u64* g = info + (long long)v * a.S * HV_GLCM_INFO + e;
        if (e % HV_GLCM_INFO == 0) atomicOr(g, (u64)w);
        else atomicAdd(g, (u64)w);
    }
}

__global__ __launch_bounds__(64) void glcm_final_kernel(int V, int S, const u64* __restrict__ vbad, u64* __restrict__ info) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= V * S) return;
    u64* w = info + (long long)e * HV_GLCM_INFO;
    w[0] |= (u64)((vbad[e / S] ? HV_LS_BAD_LABEL : 0) | (w[1] ? 0 : HV_LS_EMPTY));
}

// ------------------------------------------------------------------------------------------------ host side
static inline bool gl_sizes_ok(int V, int A0, int A1, int A2, int S, int D, int G) {
    return V > 0 && A0 > 0 && A1 > 0 && A2 > 0 && S >= 1 && S <= HV_LS_MAX_LABELS && D >= 1 && D <= HV_GLCM_MAX_OFFSETS && G >= 2 &&
           G <= HV_GLCM_MAX_LEVELS;
}
static inline bool gl_vol_dtype_ok(int dt) { return dt == HV_DT_U8 || dt == HV_DT_I16 || dt == HV_DT_F32 || dt == HV_DT_F64; }
static inline bool gl_label_dtype_ok(int dt) { return dt >= HV_DT_U8 && dt <= HV_DT_F64; }

extern "C" size_t hv_glcm_workspace_bytes(int V, int A0, int A1, int A2, int S, int D, int G) {
    if (!gl_sizes_ok(V, A0, A1, A2, S, D, G) || hv_too_large(V, A0, A1, A2)) return 0;
    return hv_up16((size_t)V * 8);                                   // the per-volume bad-label words
}

template <typename T>
static int gl_run(const GlArgs& a, int P, size_t lds, u64* out, u64* info, u64* vbad, hipStream_t st) {
    const long long nout = (long long)a.V * a.S * a.D * a.G * a.G, ninfo = (long long)a.V * a.S * HV_GLCM_INFO;
    hipLaunchKernelGGL(glcm_init_kernel, dim3(min(hv_cdiv(nout, GL_THREADS * 4), 2048)), dim3(GL_THREADS), 0, st, out, nout, info, ninfo, vbad, a.V);
    HV_LAUNCH_CHECK();
    hipLaunchKernelGGL(glcm_count_kernel<T>, dim3(P, a.V), dim3(GL_THREADS), lds, st, a, out, info, vbad);
    HV_LAUNCH_CHECK();
    hipLaunchKernelGGL(glcm_final_kernel, dim3(hv_cdiv((long long)a.V * a.S, 64)), dim3(64), 0, st, a.V, a.S, (const u64*)vbad, info);
    HV_LAUNCH_CHECK();
    return HV_OK;
}

extern "C" int hv_glcm(const void* vol, int vol_dtype, long long sv, long long s0, long long s1, long long s2, const void* label, int label_dtype,
                       long long lsv, long long ls0, long long ls1, long long ls2, const void* mask, long long msv, long long ms0, long long ms1,
                       long long ms2, int V, int A0, int A1, int A2, const int* labels, int S, const int* offsets, int D, double lo, double width,
                       int G, int flags, long long* out, long long* info, void* workspace, size_t workspace_bytes, void* stream) {
    if (!vol || !label || !labels || !offsets || !out || !info || !workspace || !gl_sizes_ok(V, A0, A1, A2, S, D, G) ||
        !gl_vol_dtype_ok(vol_dtype) || !gl_label_dtype_ok(label_dtype) || !std::isfinite(lo) || !std::isfinite(width) || !(width > 0.0) ||
        (flags & ~HV_GLCM_SYMMETRIC) || ((uintptr_t)workspace & 15) || ((uintptr_t)out & 7) || ((uintptr_t)info & 7))
        return HV_ERR_ARG;
    GlArgs a;
    if (!hv_slot_table(a.slot, labels, S)) return HV_ERR_ARG;
    int reach[3] = {0, 0, 0};
    for (int d = 0; d < HV_GLCM_MAX_OFFSETS; ++d)
        for (int c = 0; c < 3; ++c) {
            a.off[d][c] = 0;
            if (d >= D) continue;
            const int o = offsets[3 * d + c];
            if (o < -HV_GLCM_MAX_REACH || o > HV_GLCM_MAX_REACH) return HV_ERR_ARG;
            a.off[d][c] = (signed char)o;
            reach[c] = (o < 0 ? -o : o) > reach[c] ? (o < 0 ? -o : o) : reach[c];
        }
    for (int d = 1; d < D; ++d)
        for (int e = 0; e < d; ++e)
            if (a.off[d][0] == a.off[e][0] && a.off[d][1] == a.off[e][1] && a.off[d][2] == a.off[e][2]) return HV_ERR_ARG;
    if (hv_too_large(V, A0, A1, A2)) return HV_ERR_UNSUPPORTED;
    if (workspace_bytes < hv_up16((size_t)V * 8)) return HV_ERR_ARG;
    a.vol = hv_vol(vol, vol_dtype, sv, s0, s1, s2);
    a.lab = hv_vol(label, label_dtype, lsv, ls0, ls1, ls2);
    a.msk = hv_vol(mask, HV_DT_U8, msv, ms0, ms1, ms2);
    a.V = V; a.A0 = A0; a.A1 = A1; a.A2 = A2; a.S = S; a.D = D; a.G = G; a.symmetric = (flags & HV_GLCM_SYMMETRIC) ? 1 : 0;
    a.lo = lo; a.width = width;
    hv_axis_order(a.vol, A0, A1, A2, a.ax_in, a.ax_mid, a.ax_out);
    const int n0 = hv_cdiv(A0, GL_T);
    a.n1 = hv_cdiv(A1, GL_T); a.n2 = hv_cdiv(A2, GL_T);
    const long long nt = (long long)n0 * a.n1 * a.n2;               // <= 2^30 voxels: fits an int
    a.ntiles = (int)nt;
    a.tpb = hv_cdiv(nt, GL_MAX_PART);
    const int P = hv_cdiv(nt, a.tpb);
    a.r0 = reach[0]; a.r1 = reach[1]; a.r2 = reach[2];
    a.E0 = GL_T + 2 * a.r0; a.E1 = GL_T + 2 * a.r1; a.E2 = GL_T + 2 * a.r2;
    a.P2 = (a.E2 / 2) % 2 ? a.E2 : a.E2 + 2;
    a.stage_bytes = (unsigned)hv_up16((size_t)a.E0 * a.E1 * a.P2 * 2);
    const size_t fixed = a.stage_bytes + (size_t)S * HV_GLCM_INFO * 4 + 16, table = (size_t)G * G * 4;
    const int fit = (int)((GL_LDS_BYTES - fixed) / table);           // >= 2: 24 * 24 * 26 codes and 64 slots leave 34 KiB, a table takes 16 at most
    a.DC = fit < D ? fit : D;
    const size_t lds = (size_t)a.DC * table + fixed;
    hipStream_t st = (hipStream_t)stream;
    u64* o = (u64*)out;
    u64* inf = (u64*)info;
    u64* vbad = (u64*)workspace;
    switch (vol_dtype) {
        case HV_DT_U8: return gl_run<uint8_t>(a, P, lds, o, inf, vbad, st);
        case HV_DT_I16: return gl_run<int16_t>(a, P, lds, o, inf, vbad, st);
        case HV_DT_F32: return gl_run<float>(a, P, lds, o, inf, vbad, st);
        default: return gl_run<double>(a, P, lds, o, inf, vbad, st);
    }
}
