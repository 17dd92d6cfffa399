// Per-label 3-D run-length and neighbourhood texture of V volumes on the device: hv_glrlm (Galloway 1975) and
// hv_gldm (Sun and Wee 1983, with the sums Amadasun and King's NGTDM needs).  Slot and level of a voxel are hv_glcm's (texture_code.h).
//
//   tr_init_kernel        the outputs, info and the per-volume bad-label words zeroed
//   tr_quant_kernel<T>    the 16-bit (slot << 6) | level code of every voxel (GL_NONE: no slot or not finite) into a C-contiguous code volume in
//                         the workspace, the loop's fastest index on the logical axis with the smallest stride of vol; the four info words are
//                         gathered as glcm_count_kernel gathers them.  Everything after it reads 2 bytes per voxel and no strides.
//   glrlm_count_kernel    grid (part, offset, volume).  A lane takes one voxel p: if p has a code and p - d is not alike it, p starts a run, and
//                         the lane walks p + d, p + 2d, ... while the code repeats (consecutive lanes read consecutive codes at every step).  Runs
//                         are counted in an LDS table [G][min(R, 64)] of 32-bit counters that belongs to one slot at a time (a workgroup covers
//                         fewer than 2^32 voxels: no counter wraps) and is flushed -- non-zero bins, 64-bit global atomicAdd -- when the slot
//                         changes or the workgroup's voxels end; a run that falls in a bin past the table goes to out directly.
//   gldm_count_kernel     grid (part, volume).  A lane takes one voxel and reads its 26 neighbours' codes through the cache; LDS tables [G][27]
//                         for dep and ngt's counts (32 bit) and ngt's sums (64 bit), one slot at a time, flushed the same way.
//   tr_final_kernel       one lane per (volume, slot): HV_LS_BAD_LABEL and HV_LS_EMPTY into the status word
// Only integer atomics, so the result does not depend on the order of anything; every word of the outputs and the workspace that is read was
// written by an earlier launch of the same call.  No host synchronisation: the grids come from the shape.
#include <climits>
#include <cmath>
#include "texture_code.h"

#define TR_THREADS 256
#define TR_MAX_PART 1024                      // workgroups per volume (and offset) at most, once a workgroup has TR_MIN_VPB voxels
#define TR_MIN_VPB 2048
#define TR_MAX_BINS 64                        // run-length bins of the LDS table
#define TR_NB HV_GLDM_NEIGHBOURS              // 0 .. 26 neighbours

struct TrArgs {
    HvVol vol, lab, msk;                      // msk.p == NULL: no mask
    int V, A0, A1, A2, N, S, D, G, R, RB, alpha;   // N voxels per volume; RB = min(R, TR_MAX_BINS)
    double lo, width;
    int ax_in, ax_mid;                        // logical axes by ascending stride of vol (the third is the outermost)
    int vpb;                                  // voxels per workgroup, a multiple of TR_THREADS
    signed char off[HV_GLRLM_MAX_OFFSETS][3];
    unsigned char slot[256];
};

__global__ __launch_bounds__(TR_THREADS) void tr_init_kernel(u64* __restrict__ a, long long na, u64* __restrict__ b, long long nb,
                                                             u64* __restrict__ c, long long nc, u64* __restrict__ vbad, int V) {
    const long long g = (long long)blockIdx.x * TR_THREADS + threadIdx.x, step = (long long)gridDim.x * TR_THREADS;
    for (long long e = g; e < na; e += step) a[e] = 0ull;
    for (long long e = g; e < nb; e += step) b[e] = 0ull;
    for (long long e = g; e < nc; e += step) c[e] = 0ull;
    for (long long e = g; e < V; e += step) vbad[e] = 0ull;
}

template <typename T>
__global__ __launch_bounds__(TR_THREADS) void tr_quant_kernel(TrArgs a, unsigned short* __restrict__ codes, u64* __restrict__ info, int info_words,
                                                              u64* __restrict__ vbad) {
    __shared__ unsigned s_info[HV_LS_MAX_LABELS * HV_GLCM_INFO];
    const int tid = threadIdx.x, v = blockIdx.y, G = a.G;
    for (int e = tid; e < a.S * HV_GLCM_INFO; e += TR_THREADS) s_info[e] = 0u;
    __syncthreads();
    const int dims[3] = {a.A0, a.A1, a.A2};
    const int e_in = dims[a.ax_in], e_mid = dims[a.ax_mid];
    const int end = min((blockIdx.x + 1) * a.vpb, a.N);              // N <= 2^30 and vpb <= 2^20 + 256: no overflow
    unsigned short* cv = codes + (long long)v * a.N;
    int bad = 0;
    GlRun run;
    run.slot = 0xFF; run.n = run.low = run.high = run.flag = 0u;
    for (int e = blockIdx.x * a.vpb + tid; e < end; e += TR_THREADS) {
        const int u = e % e_in, m = (e / e_in) % e_mid, o = e / (e_in * e_mid);
        const int i = a.ax_in == 0 ? u : (a.ax_mid == 0 ? m : o), j = a.ax_in == 1 ? u : (a.ax_mid == 1 ? m : o),
                  k = a.ax_in == 2 ? u : (a.ax_mid == 2 ? m : o);
        const int s = hv_slot(a, v, i, j, k, bad);
        if (s != run.slot) {
            gl_run_flush(run, s_info);
            run.slot = s; run.n = run.low = run.high = run.flag = 0u;
        }
        unsigned code = GL_NONE;
        if (s != 0xFF) {
            const double x = (double)((const T*)a.vol.p)[v * a.vol.sv + i * a.vol.s0 + j * a.vol.s1 + k * a.vol.s2];
            if (hv_finite(x)) {
                const double t = (x - a.lo) / a.width;
                const int lev = t < 0.0 ? 0 : (t >= (double)G ? G - 1 : (int)t);
                code = (unsigned)(s << 6 | lev);
                ++run.n; run.low += t < 0.0 ? 1u : 0u; run.high += t >= (double)G ? 1u : 0u;
            } else {
                run.flag |= (unsigned)HV_LS_NONFINITE;
            }
        }
        cv[(i * a.A1 + j) * a.A2 + k] = (unsigned short)code;
    }
    gl_run_flush(run, s_info);
    if (bad) atomicOr(&vbad[v], 1ull);
    __syncthreads();
    for (int e = tid; e < a.S * HV_GLCM_INFO; e += TR_THREADS) {
        const unsigned w = s_info[e];
        if (w == 0u) continue;
        u64* g = info + ((long long)v * a.S + e / HV_GLCM_INFO) * info_words + e % HV_GLCM_INFO;
        if (e % HV_GLCM_INFO == 0) atomicOr(g, (u64)w);
        else atomicAdd(g, (u64)w);
    }
}

// The workgroup-uniform walk over the slots its lanes hold (mine: this lane's slot, 0xFF for none): `count(s)` is run once per slot present, after
// `flush(old)` whenever the slot the LDS tables count for changes.  cur: that slot, -1 before the first.
template <typename Count, typename Flush>
__device__ __forceinline__ void tr_per_slot(unsigned* s_present, int mine, int& cur, Count count, Flush flush) {
    __syncthreads();                                                 // the previous round's mask is read, the tables' first zeroes stand
    if (threadIdx.x < 2) s_present[threadIdx.x] = 0u;
    __syncthreads();
    if (mine != 0xFF && !(s_present[mine >> 5] >> (mine & 31) & 1u)) atomicOr(&s_present[mine >> 5], 1u << (mine & 31));
    __syncthreads();
    u64 pm = (u64)s_present[0] | ((u64)s_present[1] << 32);
    while (pm) {
        const int s = __ffsll((long long)pm) - 1;
        pm &= pm - 1;
        if (s != cur) {
            if (cur >= 0) {
                __syncthreads();                                     // every add for the old slot has landed
                flush(cur);
                __syncthreads();
            }
            cur = s;
        }
        if (mine == s) count(s);
    }
}

// how many steps of d (one component: -1, 0, 1) stay inside [0, A) from x
__device__ __forceinline__ int tr_room(int x, int d, int A) { return d > 0 ? A - 1 - x : (d < 0 ? x : INT_MAX); }

// LDS: tbl [G][RB] u32 | capped [1] u32 | s_present [2] u32
__global__ __launch_bounds__(TR_THREADS) void glrlm_count_kernel(TrArgs a, const unsigned short* __restrict__ codes, u64* __restrict__ out,
                                                                 u64* __restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) unsigned tr_lds[];
    const int G = a.G, R = a.R, RB = a.RB, ntbl = G * RB;
    unsigned* tbl = tr_lds;
    unsigned* s_capped = tbl + ntbl;
    unsigned* s_present = s_capped + 1;
    const int tid = threadIdx.x, d = blockIdx.y, v = blockIdx.z;
    const int d0 = a.off[d][0], d1 = a.off[d][1], d2 = a.off[d][2], delta = (d0 * a.A1 + d1) * a.A2 + d2;
    const unsigned short* cv = codes + (long long)v * a.N;
    for (int e = tid; e <= ntbl; e += TR_THREADS) tbl[e] = 0u;       // the capped word as well
    const int first = blockIdx.x * a.vpb, end = min(first + a.vpb, a.N);
    auto flush = [&](int s) {
        u64* o = out + (((long long)v * a.S + s) * a.D + d) * G * (long long)R;
        for (int e = tid; e < ntbl; e += TR_THREADS) {
            const unsigned c = tbl[e];
            if (c == 0u) continue;
            tbl[e] = 0u;
            atomicAdd(&o[(long long)(e / RB) * R + e % RB], (u64)c);
        }
        if (tid == 0 && *s_capped) {
            atomicAdd(&info[((long long)v * a.S + s) * HV_GLRLM_INFO + HV_GLCM_INFO + d], (u64)*s_capped);
            *s_capped = 0u;
        }
    };
    int cur = -1;
    for (int base = first; base < end; base += TR_THREADS) {         // workgroup-uniform trip count
        const int e = base + tid;
        unsigned code = GL_NONE;
        int L = 0;                                                   // the length of the run that starts here, 0: none does
        if (e < end) {
            code = cv[e];
            if (code != GL_NONE) {
                const int k = e % a.A2, j = (e / a.A2) % a.A1, i = e / (a.A2 * a.A1);
                const bool before = tr_room(i, -d0, a.A0) > 0 && tr_room(j, -d1, a.A1) > 0 && tr_room(k, -d2, a.A2) > 0;   // p - d is inside
                if (!(before && cv[e - delta] == code)) {
                    const int room = min(tr_room(i, d0, a.A0), min(tr_room(j, d1, a.A1), tr_room(k, d2, a.A2)));         // finite: d != 0
                    L = 1;
                    while (L <= room && cv[e + L * delta] == code) ++L;
                }
            }
        }
        tr_per_slot(s_present, L ? (int)(code >> 6) : 0xFF, cur, [&](int s) {
            const int bin = min(L, R) - 1, lev = (int)(code & 63u);
            if (bin < RB) atomicAdd(&tbl[lev * RB + bin], 1u);
            else atomicAdd(&out[((((long long)v * a.S + s) * a.D + d) * G + lev) * R + bin], 1ull);
            if (L > R) atomicAdd(s_capped, 1u);
        }, flush);
    }
    __syncthreads();
    if (cur >= 0) flush(cur);
}

// LDS: sum [G][27] u64 | dep [G][27] u32 | cnt [G][27] u32 | s_present [2] u32
__global__ __launch_bounds__(TR_THREADS) void gldm_count_kernel(TrArgs a, const unsigned short* __restrict__ codes, u64* __restrict__ dep,
                                                                u64* __restrict__ ngt) {
    extern __shared__ __attribute__((aligned(16))) unsigned tr_lds[];
    const int G = a.G, ntbl = G * TR_NB;
    u64* t_sum = (u64*)tr_lds;
    unsigned* t_dep = tr_lds + 2 * ntbl;
    unsigned* t_cnt = t_dep + ntbl;
    unsigned* s_present = t_cnt + ntbl;
    const int tid = threadIdx.x, v = blockIdx.y;
    const unsigned short* cv = codes + (long long)v * a.N;
    for (int e = tid; e < ntbl; e += TR_THREADS) { t_sum[e] = 0ull; t_dep[e] = 0u; t_cnt[e] = 0u; }
    const int first = blockIdx.x * a.vpb, end = min(first + a.vpb, a.N);
    auto flush = [&](int s) {
        const long long o = ((long long)v * a.S + s) * ntbl;
        for (int e = tid; e < ntbl; e += TR_THREADS) {
            const unsigned c = t_dep[e], n = t_cnt[e];
            if (c) { t_dep[e] = 0u; atomicAdd(&dep[o + e], (u64)c); }
            if (n) {
                t_cnt[e] = 0u;
                atomicAdd(&ngt[(o + e) * 2], (u64)n);
                const u64 w = t_sum[e];
                if (w) { t_sum[e] = 0ull; atomicAdd(&ngt[(o + e) * 2 + 1], w); }
            }
        }
    };
    int cur = -1;
    for (int base = first; base < end; base += TR_THREADS) {         // workgroup-uniform trip count
        const int e = base + tid;
        const unsigned code = e < end ? cv[e] : GL_NONE;
        const int lev = (int)(code & 63u);
        int n = 0, sum = 0, close = 0;                               // neighbours of the slot, the sum of their levels, how many within alpha
        if (code != GL_NONE) {
            const int k = e % a.A2, j = (e / a.A2) % a.A1, i = e / (a.A2 * a.A1);
            for (int di = -1; di <= 1; ++di) {
                if ((unsigned)(i + di) >= (unsigned)a.A0) continue;
                for (int dj = -1; dj <= 1; ++dj) {
                    if ((unsigned)(j + dj) >= (unsigned)a.A1) continue;
                    const unsigned short* row = cv + e + (di * a.A1 + dj) * a.A2;
#pragma unroll
                    for (int dk = -1; dk <= 1; ++dk) {
                        if ((di | dj | dk) == 0 || (unsigned)(k + dk) >= (unsigned)a.A2) continue;
                        const unsigned q = row[dk];
                        if (q == GL_NONE || (q >> 6) != (code >> 6)) continue;
                        const int lq = (int)(q & 63u);
                        ++n; sum += lq; close += abs(lq - lev) <= a.alpha ? 1 : 0;
                    }
                }
            }
        }
        tr_per_slot(s_present, code != GL_NONE ? (int)(code >> 6) : 0xFF, cur, [&](int) {
            atomicAdd(&t_dep[lev * TR_NB + close], 1u);
            atomicAdd(&t_cnt[lev * TR_NB + n], 1u);
            if (lev * n != sum) atomicAdd(&t_sum[lev * TR_NB + n], (u64)abs(lev * n - sum));
        }, flush);
    }
    __syncthreads();
    if (cur >= 0) flush(cur);
}

__global__ __launch_bounds__(64) void tr_final_kernel(int V, int S, int info_words, const u64* __restrict__ vbad, u64* __restrict__ info) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= V * S) return;
    u64* w = info + (long long)e * info_words;
    w[0] |= (u64)((vbad[e / S] ? HV_LS_BAD_LABEL : 0) | (w[1] ? 0 : HV_LS_EMPTY));
}

// ------------------------------------------------------------------------------------------------ host side
static inline bool tr_sizes_ok(int V, int A0, int A1, int A2, int S, int G) {
    return V > 0 && A0 > 0 && A1 > 0 && A2 > 0 && S >= 1 && S <= HV_LS_MAX_LABELS && G >= 2 && G <= HV_GLCM_MAX_LEVELS;
}
// the per-volume bad-label words, then the code volumes
static inline size_t tr_workspace(int V, int A0, int A1, int A2) { return hv_up16((size_t)V * 8) + hv_up16((size_t)V * A0 * A1 * A2 * 2); }

extern "C" size_t hv_glrlm_workspace_bytes(int V, int A0, int A1, int A2, int S, int D, int G, int R) {
    if (!tr_sizes_ok(V, A0, A1, A2, S, G) || D < 1 || D > HV_GLRLM_MAX_OFFSETS || R < 1 || hv_too_large(V, A0, A1, A2)) return 0;
    return tr_workspace(V, A0, A1, A2);
}
extern "C" size_t hv_gldm_workspace_bytes(int V, int A0, int A1, int A2, int S, int G) {
    if (!tr_sizes_ok(V, A0, A1, A2, S, G) || hv_too_large(V, A0, A1, A2)) return 0;
    return tr_workspace(V, A0, A1, A2);
}

// what the two entries check alike (sizes apart), and the arguments they share; HV_OK or the refusal
static int tr_prepare(TrArgs& a, const void* vol, int vol_dtype, long long sv, long long s0, long long s1, long long s2, const void* label,
                      int label_dtype, long long lsv, long long ls0, long long ls1, long long ls2, const void* mask, long long msv, long long ms0,
                      long long ms1, long long ms2, int V, int A0, int A1, int A2, const int* labels, int S, double lo, double width, int G,
                      const void* info, const void* workspace) {
    const bool vol_dt = vol_dtype == HV_DT_U8 || vol_dtype == HV_DT_I16 || vol_dtype == HV_DT_F32 || vol_dtype == HV_DT_F64;
    if (!vol || !label || !labels || !info || !workspace || !tr_sizes_ok(V, A0, A1, A2, S, G) || !vol_dt || label_dtype < HV_DT_U8 ||
        label_dtype > HV_DT_F64 || !std::isfinite(lo) || !std::isfinite(width) || !(width > 0.0) || ((uintptr_t)workspace & 15) ||
        ((uintptr_t)info & 7))
        return HV_ERR_ARG;
    if (!hv_slot_table(a.slot, labels, S)) return HV_ERR_ARG;
    a.vol = hv_vol(vol, vol_dtype, sv, s0, s1, s2);
    a.lab = hv_vol(label, label_dtype, lsv, ls0, ls1, ls2);
    a.msk = hv_vol(mask, HV_DT_U8, msv, ms0, ms1, ms2);
    a.V = V; a.A0 = A0; a.A1 = A1; a.A2 = A2; a.S = S; a.G = G; a.D = 0; a.R = a.RB = 1; a.alpha = 0;
    a.lo = lo; a.width = width;
    for (int d = 0; d < HV_GLRLM_MAX_OFFSETS; ++d) a.off[d][0] = a.off[d][1] = a.off[d][2] = 0;
    return HV_OK;
}

// the sizes that need at most 2^30 voxels: N, the quantising loop's axes, the partition.  -> workgroups per volume
static int tr_partition(TrArgs& a) {
    a.N = a.A0 * a.A1 * a.A2;
    int ax_out;
    hv_axis_order(a.vol, a.A0, a.A1, a.A2, a.ax_in, a.ax_mid, ax_out);
    const int per = hv_cdiv(a.N, TR_MAX_PART);
    a.vpb = hv_cdiv(per > TR_MIN_VPB ? per : TR_MIN_VPB, TR_THREADS) * TR_THREADS;
    return hv_cdiv(a.N, a.vpb);
}

static int tr_quantise(const TrArgs& a, int P, unsigned short* codes, u64* info, int info_words, u64* vbad, hipStream_t st) {
    const dim3 grid(P, a.V), block(TR_THREADS);
    switch (a.vol.dt) {
        case HV_DT_U8: hipLaunchKernelGGL(tr_quant_kernel<uint8_t>, grid, block, 0, st, a, codes, info, info_words, vbad); break;
        case HV_DT_I16: hipLaunchKernelGGL(tr_quant_kernel<int16_t>, grid, block, 0, st, a, codes, info, info_words, vbad); break;
        case HV_DT_F32: hipLaunchKernelGGL(tr_quant_kernel<float>, grid, block, 0, st, a, codes, info, info_words, vbad); break;
        default: hipLaunchKernelGGL(tr_quant_kernel<double>, grid, block, 0, st, a, codes, info, info_words, vbad); break;
    }
    HV_LAUNCH_CHECK();
    return HV_OK;
}

extern "C" int hv_glrlm(const void* vol, int vol_dtype, long long sv, long long s0, long long s1, long long s2, const void* label, int label_dtype,
                        long long lsv, long long ls0, long long ls1, long long ls2, const void* mask, long long msv, long long ms0, long long ms1,
                        long long ms2, int V, int A0, int A1, int A2, const int* labels, int S, const int* offsets, int D, double lo, double width,
                        int G, int R, long long* out, long long* info, void* workspace, size_t workspace_bytes, void* stream) {
    TrArgs a;
    if (!offsets || !out || ((uintptr_t)out & 7) || D < 1 || D > HV_GLRLM_MAX_OFFSETS || R < 1) return HV_ERR_ARG;
    const int rc = tr_prepare(a, vol, vol_dtype, sv, s0, s1, s2, label, label_dtype, lsv, ls0, ls1, ls2, mask, msv, ms0, ms1, ms2, V, A0, A1, A2,
                              labels, S, lo, width, G, info, workspace);
    if (rc != HV_OK) return rc;
    for (int d = 0; d < D; ++d) {
        bool zero = true;
        for (int c = 0; c < 3; ++c) {
            const int o = offsets[3 * d + c];
            if (o < -1 || o > 1) return HV_ERR_ARG;
            a.off[d][c] = (signed char)o;
            zero = zero && o == 0;
        }
        if (zero) return HV_ERR_ARG;
        for (int e = 0; e < d; ++e) {                                // the same line twice: d again, or its negative
            const bool same = a.off[d][0] == a.off[e][0] && a.off[d][1] == a.off[e][1] && a.off[d][2] == a.off[e][2];
            const bool neg = a.off[d][0] == -a.off[e][0] && a.off[d][1] == -a.off[e][1] && a.off[d][2] == -a.off[e][2];
            if (same || neg) return HV_ERR_ARG;
        }
    }
    if (hv_too_large(V, A0, A1, A2)) return HV_ERR_UNSUPPORTED;
    if (workspace_bytes < tr_workspace(V, A0, A1, A2)) return HV_ERR_ARG;
    a.D = D; a.R = R; a.RB = R < TR_MAX_BINS ? R : TR_MAX_BINS;
    const int P = tr_partition(a);
    hipStream_t st = (hipStream_t)stream;
    u64* vbad = (u64*)workspace;
    unsigned short* codes = (unsigned short*)((char*)workspace + hv_up16((size_t)V * 8));
    const long long nout = (long long)V * S * D * G * R, ninfo = (long long)V * S * HV_GLRLM_INFO;
    hipLaunchKernelGGL(tr_init_kernel, dim3(min(hv_cdiv(nout, TR_THREADS * 4), 2048)), dim3(TR_THREADS), 0, st, (u64*)out, nout, (u64*)info, ninfo,
                       (u64*)nullptr, 0LL, vbad, V);
    HV_LAUNCH_CHECK();
    const int qrc = tr_quantise(a, P, codes, (u64*)info, HV_GLRLM_INFO, vbad, st);
    if (qrc != HV_OK) return qrc;
    hipLaunchKernelGGL(glrlm_count_kernel, dim3(P, D, V), dim3(TR_THREADS), (size_t)(G * a.RB + 3) * 4, st, a, (const unsigned short*)codes, (u64*)out,
                       (u64*)info);
    HV_LAUNCH_CHECK();
    hipLaunchKernelGGL(tr_final_kernel, dim3(hv_cdiv((long long)V * S, 64)), dim3(64), 0, st, V, S, (int)HV_GLRLM_INFO, (const u64*)vbad, (u64*)info);
    HV_LAUNCH_CHECK();
    return HV_OK;
}

extern "C" int hv_gldm(const void* vol, int vol_dtype, long long sv, long long s0, long long s1, long long s2, const void* label, int label_dtype,
                       long long lsv, long long ls0, long long ls1, long long ls2, const void* mask, long long msv, long long ms0, long long ms1,
                       long long ms2, int V, int A0, int A1, int A2, const int* labels, int S, double lo, double width, int G, int alpha,
                       long long* dep, long long* ngt, long long* info, void* workspace, size_t workspace_bytes, void* stream) {
    TrArgs a;
    if (!dep || !ngt || ((uintptr_t)dep & 7) || ((uintptr_t)ngt & 7)) return HV_ERR_ARG;
    const int rc = tr_prepare(a, vol, vol_dtype, sv, s0, s1, s2, label, label_dtype, lsv, ls0, ls1, ls2, mask, msv, ms0, ms1, ms2, V, A0, A1, A2,
                              labels, S, lo, width, G, info, workspace);
    if (rc != HV_OK) return rc;
    if (alpha < 0 || alpha > G - 1) return HV_ERR_ARG;
    if (hv_too_large(V, A0, A1, A2)) return HV_ERR_UNSUPPORTED;
    if (workspace_bytes < tr_workspace(V, A0, A1, A2)) return HV_ERR_ARG;
    a.alpha = alpha;
    const int P = tr_partition(a);
    hipStream_t st = (hipStream_t)stream;
    u64* vbad = (u64*)workspace;
    unsigned short* codes = (unsigned short*)((char*)workspace + hv_up16((size_t)V * 8));
    const long long ndep = (long long)V * S * G * TR_NB, ninfo = (long long)V * S * HV_GLCM_INFO;
    hipLaunchKernelGGL(tr_init_kernel, dim3(min(hv_cdiv(ndep * 2, TR_THREADS * 4), 2048)), dim3(TR_THREADS), 0, st, (u64*)dep, ndep, (u64*)ngt,
                       ndep * 2, (u64*)info, ninfo, vbad, V);
    HV_LAUNCH_CHECK();
    const int qrc = tr_quantise(a, P, codes, (u64*)info, HV_GLCM_INFO, vbad, st);
    if (qrc != HV_OK) return qrc;
    hipLaunchKernelGGL(gldm_count_kernel, dim3(P, V), dim3(TR_THREADS), (size_t)G * TR_NB * 16 + 8, st, a, (const unsigned short*)codes, (u64*)dep,
                       (u64*)ngt);
    HV_LAUNCH_CHECK();
    hipLaunchKernelGGL(tr_final_kernel, dim3(hv_cdiv((long long)V * S, 64)), dim3(64), 0, st, V, S, (int)HV_GLCM_INFO, (const u64*)vbad, (u64*)info);
    HV_LAUNCH_CHECK();
    return HV_OK;
}
