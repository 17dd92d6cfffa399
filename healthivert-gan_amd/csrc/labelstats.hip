// Per-label intensity statistics and order statistics of V volumes on the device: hv_label_stats.  For every listed
// label value of every volume: voxel count, sum v and sum v^2, minimum and maximum, the three coordinate sums, the bounding box and, per requested
// percentile q, the two order statistics x[lo], x[hi] that numpy's linear rule interpolates between (vi = (n - 1) * (q / 100) in float64, lo =
// floor(vi), hi = lo + 1, both n - 1 once vi >= n - 1).  The definitions are scipy.ndimage.sum_labels / minimum / maximum / center_of_mass /
// find_objects and np.percentile; the interpolation itself and the mean / variance are the wrapper's (label_statistics.py), in float64 on the host.
//
// A voxel is counted iff (mask == NULL or mask != 0) and its label is a listed value.  A label that is not an integer in [0, 255] sets the volume's
// status bit and is counted nowhere.  Listed values travel in the kernel arguments as a 256-entry value -> slot table, the percentiles beside them.
//
//   ls_init_kernel        the accumulator table's identities (0, ~0 for minima), the select's bins zeroed
//   ls_moments_kernel<T>  one read of vol, label and mask in 16 x 16 x 16 tiles, the tile's fastest thread index on the logical axis with the smallest
//                         stride.  A thread sums runs of one slot in registers and flushes on a slot change: integer atomics on a per-workgroup LDS
//                         table, then -- once per workgroup and slot -- on the global one.  Integer dtypes: sum v / sum v^2 are int64 the same way.
//                         Float dtypes: the tile is also staged in LDS at its LOGICAL position, so the order of every floating sum is a property of
//                         the shape alone, not of the strides: a wave owns a contiguous quarter of the tile's raster, folds (v, v*v) over the lanes of
//                         one slot with a fixed shuffle tree and adds to its own per-slot accumulator; the workgroup leaves ((w0 + w1) + w2) + w3
//                         per slot as one partial; no floating-point atomic anywhere.
//   ls_fold_kernel        one lane per (volume, slot): the partials in ascending workgroup order (float dtypes), and the select's ranks from the count
//   ls_hist_kernel<T>     one launch per 8-bit digit of the order-preserving key (2 / 4 / 8 passes for 16 / 32 / 64-bit keys): a voxel of slot s adds 1
//                         to hist[target][digit] for each of the slot's 2Q targets whose prefix equals the key's high bits; 32 (slot, target) pairs
//                         share 32 KiB of LDS bins, further groups are grid dimension y; non-empty bins are added to the global table at the end
//   ls_pick_kernel        one wave per (volume, slot, target): walks the 256 bins, fixes the digit, updates prefix and remaining rank, zeroes the bins
//   ls_final_kernel       one lane per (volume, slot): the record
// Only integer atomics; every workspace word that is read was written by an earlier launch of the same call.  No workgroup waits for another: the
// phases are kernel boundaries.  No host synchronisation: ranks come from the device counts, grids from the shape.
#include <cmath>
#include "volume_access.h"

#define LS_THREADS 256
#define LS_T 16                               // tile edge
#define LS_TILE (LS_T * LS_T * LS_T)
#define LS_P1 17                              // LDS pitch of a tile row (doubles) ...
#define LS_P0 (LS_T * LS_P1 + 1)              // ... and of a tile plane: a wave writing along any logical axis spreads over the banks
#define LS_CELLS (LS_T * LS_P0)
#define LS_ACC 16                             // u64 words per (volume, slot) accumulator
#define LS_MAX_PART 1024                      // workgroups (= partial sums) per volume at most
#define LS_PAIRS 32                           // (slot, target) pairs whose bins share one workgroup's LDS
#define LS_NONE HV_NO_SLOT

// accumulator words
enum { LA_CNT = 0, LA_SV = 1, LA_SVV = 2, LA_MIN = 3, LA_MAX = 4, LA_C0 = 5, LA_LO0 = 8, LA_HI0 = 11, LA_FLAG = 14 };

struct LsArgs {
    HvVol vol, lab, msk;                      // msk.p == NULL: no mask
    int V, A0, A1, A2, S, Q;
    int ax_in, ax_mid, ax_out;                // logical axes by ascending stride of vol
    int n0, n1, n2, ntiles, tpb, P;           // tiles per axis, tiles, tiles per workgroup, workgroups per volume
    unsigned char slot[256];
    double q[HV_LS_MAX_Q];
};

// the order-preserving unsigned key of a value, its width in bits, the way back, and what the sums add
template <typename T> struct LsKey;
template <> struct LsKey<uint8_t> {
    static constexpr int BITS = 16; static constexpr bool FLT = false;
    static __device__ __forceinline__ u64 key(uint8_t v) { return (u64)v; }
    static __device__ __forceinline__ double val(u64 k) { return (double)(int)k; }
    static __device__ __forceinline__ bool finite(uint8_t) { return true; }
};
template <> struct LsKey<int16_t> {
    static constexpr int BITS = 16; static constexpr bool FLT = false;
    static __device__ __forceinline__ u64 key(int16_t v) { return (u64)((int)v + 32768); }
    static __device__ __forceinline__ double val(u64 k) { return (double)((int)k - 32768); }
    static __device__ __forceinline__ bool finite(int16_t) { return true; }
};
template <> struct LsKey<float> {
    static constexpr int BITS = 32; static constexpr bool FLT = true;
    static __device__ __forceinline__ u64 key(float v) {
        const unsigned u = __float_as_uint(v);
        return (u64)((u >> 31) ? ~u : (u | 0x80000000u));
    }
    static __device__ __forceinline__ double val(u64 k) {
        const unsigned u = (unsigned)k;
        return (double)__uint_as_float((u >> 31) ? (u ^ 0x80000000u) : ~u);
    }
    static __device__ __forceinline__ bool finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
};
template <> struct LsKey<double> {
    static constexpr int BITS = 64; static constexpr bool FLT = true;
    static __device__ __forceinline__ u64 key(double v) {
        const u64 u = (u64)__double_as_longlong(v);
        return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    }
    static __device__ __forceinline__ double val(u64 k) { return __longlong_as_double((long long)((k >> 63) ? (k ^ 0x8000000000000000ull) : ~k)); }
    static __device__ __forceinline__ bool finite(double v) {
        return ((u64)__double_as_longlong(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
    }
};

// identity of accumulator word f: minima start at ~0, everything else at 0 (the box's upper corner is kept as hi + 1)
__device__ __forceinline__ u64 ls_identity(int f) { return (f == LA_MIN || (f >= LA_LO0 && f < LA_HI0)) ? ~0ull : 0ull; }

__global__ __launch_bounds__(LS_THREADS) void ls_init_kernel(u64* __restrict__ acc, long long nacc, u64* __restrict__ vbad, int V,
                                                             unsigned* __restrict__ hist, long long nhist) {
    const long long g = (long long)blockIdx.x * LS_THREADS + threadIdx.x, step = (long long)gridDim.x * LS_THREADS;
    for (long long e = g; e < nacc; e += step) acc[e] = ls_identity((int)(e % LS_ACC));
    for (long long e = g; e < V; e += step) vbad[e] = 0;
    for (long long e = g; e < nhist; e += step) hist[e] = 0u;
}

// a thread's run of one slot, kept in registers
struct LsRun { int slot; u64 cnt, c0, c1, c2, kmin, kmax, sv, svv, flag; int lo0, lo1, lo2, hi0, hi1, hi2; };

__device__ __forceinline__ void ls_run_reset(LsRun& r, int slot) {
    r.slot = slot; r.cnt = r.c0 = r.c1 = r.c2 = r.sv = r.svv = r.flag = 0; r.kmin = ~0ull; r.kmax = 0;
    r.lo0 = r.lo1 = r.lo2 = 0x7fffffff; r.hi0 = r.hi1 = r.hi2 = 0;
}
template <bool FLT>
__device__ __forceinline__ void ls_run_flush(const LsRun& r, u64* s_acc) {
    if (r.slot == LS_NONE || r.cnt == 0) return;
    u64* a = s_acc + r.slot * LS_ACC;
    atomicAdd(&a[LA_CNT], r.cnt);
    if (!FLT) { atomicAdd(&a[LA_SV], r.sv); atomicAdd(&a[LA_SVV], r.svv); }
    atomicMin(&a[LA_MIN], r.kmin); atomicMax(&a[LA_MAX], r.kmax);
    atomicAdd(&a[LA_C0], r.c0); atomicAdd(&a[LA_C0 + 1], r.c1); atomicAdd(&a[LA_C0 + 2], r.c2);
    atomicMin(&a[LA_LO0], (u64)r.lo0); atomicMin(&a[LA_LO0 + 1], (u64)r.lo1); atomicMin(&a[LA_LO0 + 2], (u64)r.lo2);
    atomicMax(&a[LA_HI0], (u64)r.hi0); atomicMax(&a[LA_HI0 + 1], (u64)r.hi1); atomicMax(&a[LA_HI0 + 2], (u64)r.hi2);
    if (r.flag) atomicOr(&a[LA_FLAG], r.flag);
}

// LDS: s_acc [S][LS_ACC] u64; float dtypes also: wacc [4][S][2] doubles, tile values [LS_CELLS] doubles, tile slots [LS_CELLS] bytes
template <typename T>
__global__ __launch_bounds__(LS_THREADS) void ls_moments_kernel(LsArgs a, u64* __restrict__ acc, u64* __restrict__ vbad, double* __restrict__ part) {
    typedef LsKey<T> K;
    extern __shared__ u64 ls_lds[];
    u64* s_acc = ls_lds;
    double* wacc = (double*)(s_acc + a.S * LS_ACC);
    double* t_val = wacc + 4 * a.S * 2;
    uint8_t* t_slot = (uint8_t*)(t_val + LS_CELLS);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, v = blockIdx.y, b = blockIdx.x;
    for (int e = tid; e < a.S * LS_ACC; e += LS_THREADS) s_acc[e] = ls_identity(e % LS_ACC);
    if (K::FLT)
        for (int e = tid; e < 4 * a.S * 2; e += LS_THREADS) wacc[e] = 0.0;
    __syncthreads();
    int bad = 0;
    LsRun r;
    ls_run_reset(r, LS_NONE);
    const int tile_end = min((b + 1) * a.tpb, a.ntiles);
    for (int tile = b * a.tpb; tile < tile_end; ++tile) {
        const int i0 = (tile / (a.n1 * a.n2)) * LS_T, j0 = ((tile / a.n2) % a.n1) * LS_T, k0 = (tile % a.n2) * LS_T;
        for (int e = tid; e < LS_TILE; e += LS_THREADS) {
            const int u = e & (LS_T - 1), m = (e >> 4) & (LS_T - 1), o = e >> 8;
            const int di = a.ax_in == 0 ? u : (a.ax_mid == 0 ? m : o), dj = a.ax_in == 1 ? u : (a.ax_mid == 1 ? m : o),
                      dk = a.ax_in == 2 ? u : (a.ax_mid == 2 ? m : o);
            const int i = i0 + di, j = j0 + dj, k = k0 + dk;
            int s = LS_NONE;
            T x = (T)0;
            if (i < a.A0 && j < a.A1 && k < a.A2) {
                s = hv_slot(a, v, i, j, k, bad);
                if (s != LS_NONE) x = ((const T*)a.vol.p)[v * a.vol.sv + i * a.vol.s0 + j * a.vol.s1 + k * a.vol.s2];
            }
            if (K::FLT) {
                const int cell = di * LS_P0 + dj * LS_P1 + dk;
                t_val[cell] = (double)x;
                t_slot[cell] = (uint8_t)s;
            }
            if (s != r.slot) {
                ls_run_flush<K::FLT>(r, s_acc);
                ls_run_reset(r, s);
            }
            if (s == LS_NONE) continue;
            const u64 key = K::key(x);
            ++r.cnt; r.c0 += (u64)i; r.c1 += (u64)j; r.c2 += (u64)k;
            r.kmin = key < r.kmin ? key : r.kmin; r.kmax = key > r.kmax ? key : r.kmax;
            r.lo0 = min(r.lo0, i); r.lo1 = min(r.lo1, j); r.lo2 = min(r.lo2, k);
            r.hi0 = max(r.hi0, i + 1); r.hi1 = max(r.hi1, j + 1); r.hi2 = max(r.hi2, k + 1);
            if (K::FLT) {
                if (!K::finite(x)) r.flag |= (u64)HV_LS_NONFINITE;
            } else {
                const long long xi = (long long)x;
                r.sv += (u64)xi; r.svv += (u64)(xi * xi);
            }
        }
        if (K::FLT) {
            __syncthreads();
            // wave wv owns cells [wv * 1024, (wv + 1) * 1024) of the tile's logical raster, 64 at a time in ascending order
            for (int st = 0; st < LS_TILE / LS_THREADS; ++st) {
                const int c = wv * (LS_TILE / 4) + st * 64 + lane;
                const int cell = (c >> 8) * LS_P0 + ((c >> 4) & (LS_T - 1)) * LS_P1 + (c & (LS_T - 1));
                const double x = t_val[cell];
                const int s = t_slot[cell];
                u64 pend = __ballot(s != LS_NONE);
                // one turn per distinct slot among the lanes: a turn retires every lane that holds the first pending lane's slot, that lane
                // included, so pend loses at least one bit per turn and the loop ends after at most 64 turns
                while (pend) {
                    const int cur = __shfl(s, __ffsll((long long)pend) - 1, 64);
                    const bool mine = s == cur;
                    double p = mine ? x : 0.0, pp = mine ? x * x : 0.0;
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) { p += __shfl_xor(p, o, 64); pp += __shfl_xor(pp, o, 64); }
                    if (lane == 0) { wacc[(wv * a.S + cur) * 2] += p; wacc[(wv * a.S + cur) * 2 + 1] += pp; }
                    pend &= ~__ballot(mine);
                }
            }
            __syncthreads();                      // the next tile overwrites the staging
        }
    }
    ls_run_flush<K::FLT>(r, s_acc);
    if (bad) atomicOr(&vbad[v], 1ull);
    __syncthreads();
    for (int e = tid; e < a.S * LS_ACC; e += LS_THREADS) {
        const int f = e % LS_ACC, s = e / LS_ACC;
        if (s_acc[s * LS_ACC + LA_CNT] == 0 || f > LA_FLAG) continue;
        if (K::FLT && (f == LA_SV || f == LA_SVV)) continue;
        const u64 w = s_acc[e];
        u64* g = acc + ((long long)v * a.S + s) * LS_ACC + f;
        if (f == LA_MIN || (f >= LA_LO0 && f < LA_HI0)) atomicMin(g, w);
        else if (f == LA_MAX || (f >= LA_HI0 && f < LA_FLAG)) atomicMax(g, w);
        else if (f == LA_FLAG) { if (w) atomicOr(g, w); }
        else atomicAdd(g, w);
    }
    if (K::FLT && tid < a.S) {
        double* o = part + (((long long)v * a.P + b) * a.S + tid) * 2;
#pragma unroll
        for (int c = 0; c < 2; ++c)
            o[c] = ((wacc[(0 * a.S + tid) * 2 + c] + wacc[(1 * a.S + tid) * 2 + c]) + wacc[(2 * a.S + tid) * 2 + c]) + wacc[(3 * a.S + tid) * 2 + c];
    }
}

// the select's state per (volume, slot, target): the key's bits fixed so far and the rank among the voxels that share them (~0: nothing to find)
struct LsSel { u64 prefix, rank; };

__global__ __launch_bounds__(64) void ls_fold_kernel(LsArgs a, int flt, u64* __restrict__ acc, const double* __restrict__ part,
                                                     LsSel* __restrict__ sel) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= a.V * a.S) return;
    const int v = e / a.S, s = e % a.S;
    u64* A = acc + (long long)e * LS_ACC;
    if (flt) {
        double sv = 0.0, svv = 0.0;
        for (int b = 0; b < a.P; ++b) {           // ascending workgroup order
            const double* p = part + (((long long)v * a.P + b) * a.S + s) * 2;
            sv += p[0]; svv += p[1];
        }
        A[LA_SV] = (u64)__double_as_longlong(sv);
        A[LA_SVV] = (u64)__double_as_longlong(svv);
    }
    const u64 n = A[LA_CNT];
    for (int t = 0; t < a.Q; ++t) {
        LsSel lo, hi;
        lo.prefix = hi.prefix = 0;
        if (n == 0) {
            lo.rank = hi.rank = ~0ull;
        } else {
            const double vi = (double)(n - 1) * (a.q[t] / 100.0);      // numpy: (n - 1) * quantile, the quantile q / 100
            if (vi >= (double)(n - 1)) {
                lo.rank = hi.rank = n - 1;
            } else {
                lo.rank = (u64)floor(vi);
                hi.rank = lo.rank + 1;
            }
        }
        sel[((long long)e * a.Q + t) * 2] = lo;
        sel[((long long)e * a.Q + t) * 2 + 1] = hi;
    }
}

template <typename T>
__global__ __launch_bounds__(LS_THREADS) void ls_hist_kernel(LsArgs a, int pass, const LsSel* __restrict__ sel, unsigned* __restrict__ hist) {
    typedef LsKey<T> K;
    __shared__ unsigned s_hist[LS_PAIRS * 256];
    __shared__ u64 s_prefix[LS_PAIRS];
    const int tid = threadIdx.x, v = blockIdx.z, T2 = 2 * a.Q;
    const int pair0 = blockIdx.y * LS_PAIRS, npair = min(LS_PAIRS, a.S * T2 - pair0);
    for (int e = tid; e < LS_PAIRS * 256; e += LS_THREADS) s_hist[e] = 0u;
    if (tid < npair) s_prefix[tid] = sel[(long long)v * a.S * T2 + pair0 + tid].prefix;
    __syncthreads();
    const int s_first = pair0 / T2, s_last = (pair0 + npair - 1) / T2;
    const int sh = K::BITS - 8 * pass;            // bits of the key below the prefix
    const unsigned N = (unsigned)a.A0 * a.A1 * a.A2;
    const unsigned n_in = a.ax_in == 0 ? a.A0 : (a.ax_in == 1 ? a.A1 : a.A2), n_mid = a.ax_mid == 0 ? a.A0 : (a.ax_mid == 1 ? a.A1 : a.A2);
    int bad = 0;
    for (unsigned e = blockIdx.x * LS_THREADS + tid; e < N; e += gridDim.x * LS_THREADS) {      // memory order of vol
        const int u = (int)(e % n_in), m = (int)((e / n_in) % n_mid), o = (int)(e / (n_in * n_mid));
        const int i = a.ax_in == 0 ? u : (a.ax_mid == 0 ? m : o), j = a.ax_in == 1 ? u : (a.ax_mid == 1 ? m : o),
                  k = a.ax_in == 2 ? u : (a.ax_mid == 2 ? m : o);
        const int s = hv_slot(a, v, i, j, k, bad);
        if (s == LS_NONE || s < s_first || s > s_last) continue;
        const u64 key = K::key(((const T*)a.vol.p)[v * a.vol.sv + i * a.vol.s0 + j * a.vol.s1 + k * a.vol.s2]);
        const u64 high = pass == 0 ? 0ull : key >> sh;
        const unsigned digit = (unsigned)(key >> (sh - 8)) & 255u;
        const int p_lo = max(s * T2 - pair0, 0), p_hi = min(s * T2 + T2 - pair0, npair);
        for (int p = p_lo; p < p_hi; ++p)
            if (s_prefix[p] == high) atomicAdd(&s_hist[p * 256 + digit], 1u);
    }
    __syncthreads();
    unsigned* g = hist + ((long long)v * a.S * T2 + pair0) * 256;
    for (int e = tid; e < npair * 256; e += LS_THREADS)
        if (s_hist[e]) atomicAdd(&g[e], s_hist[e]);
}

// one wave per (volume, slot, target): lane l holds bins 4l .. 4l + 3
__global__ __launch_bounds__(64) void ls_pick_kernel(LsSel* __restrict__ sel, unsigned* __restrict__ hist) {
    const long long pair = blockIdx.x;
    const int lane = threadIdx.x;
    unsigned* h = hist + pair * 256 + 4 * lane;
    const unsigned c0 = h[0], c1 = h[1], c2 = h[2], c3 = h[3];
    h[0] = h[1] = h[2] = h[3] = 0u;               // the next pass starts from empty bins
    const LsSel st = sel[pair];
    if (st.rank == ~0ull) return;                 // an empty slot: wave-uniform
    u64 incl = (u64)c0 + c1 + c2 + c3;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    const u64 before = incl - ((u64)c0 + c1 + c2 + c3);
    // the bins hold every voxel that shares the prefix, rank < their total: exactly one lane has before <= rank < incl
    if (before <= st.rank && st.rank < incl) {
        u64 r = st.rank - before;
        unsigned d = 4 * lane;
        if (r >= c0) { r -= c0; ++d; if (r >= c1) { r -= c1; ++d; if (r >= c2) { r -= c2; ++d; } } }
        LsSel nx;
        nx.prefix = (st.prefix << 8) | d;
        nx.rank = r;
        sel[pair] = nx;
    }
}

template <typename T>
__global__ __launch_bounds__(64) void ls_final_kernel(LsArgs a, const u64* __restrict__ acc, const u64* __restrict__ vbad,
                                                      const LsSel* __restrict__ sel, double* __restrict__ out) {
    typedef LsKey<T> K;
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= a.V * a.S) return;
    const int v = e / a.S;
    const u64* A = acc + (long long)e * LS_ACC;
    double* o = out + (long long)e * HV_LS_REC;
    const u64 n = A[LA_CNT];
    const int dims[3] = {a.A0, a.A1, a.A2};
    o[HV_LS_COUNT] = (double)n;
    o[HV_LS_SUM] = __longlong_as_double((long long)A[LA_SV]);          // int64 bits for the integer dtypes, a double for the float ones
    o[HV_LS_SUMSQ] = __longlong_as_double((long long)A[LA_SVV]);
    o[HV_LS_MIN] = n ? K::val(A[LA_MIN]) : (double)INFINITY;
    o[HV_LS_MAX] = n ? K::val(A[LA_MAX]) : -(double)INFINITY;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o[HV_LS_COORD + c] = (double)A[LA_C0 + c];
        o[HV_LS_LO + c] = n ? (double)A[LA_LO0 + c] : (double)dims[c];
        o[HV_LS_HI + c] = (double)((long long)A[LA_HI0 + c] - 1);
    }
    o[HV_LS_STATUS] = (double)((vbad[v] ? HV_LS_BAD_LABEL : 0) | (int)A[LA_FLAG] | (n ? 0 : HV_LS_EMPTY));
    o[HV_LS_STATUS + 1] = 0.0;
    for (int t = 0; t < 2 * a.Q; ++t)
        o[HV_LS_ORDER + t] = n ? K::val(sel[(long long)e * 2 * a.Q + t].prefix) : __longlong_as_double(0x7ff8000000000000ll);
}

// ------------------------------------------------------------------------------------------------ host side
struct LsWs { size_t acc, vbad, part, sel, hist, total; long long nacc, nhist; int P, tpb, ntiles, n0, n1, n2; };
static LsWs ls_layout(int V, int A0, int A1, int A2, int S, int Q) {
    LsWs W;
    W.n0 = hv_cdiv(A0, LS_T); W.n1 = hv_cdiv(A1, LS_T); W.n2 = hv_cdiv(A2, LS_T);
    const long long nt = (long long)W.n0 * W.n1 * W.n2;      // <= 2^30 voxels: fits an int
    W.ntiles = (int)nt;
    W.tpb = hv_cdiv(nt, LS_MAX_PART);
    W.P = hv_cdiv(nt, W.tpb);
    W.nacc = (long long)V * S * LS_ACC;
    W.nhist = (long long)V * S * 2 * Q * 256;
    W.acc = 0;
    W.vbad = W.acc + hv_up16((size_t)W.nacc * 8);
    W.part = W.vbad + hv_up16((size_t)V * 8);
    W.sel = W.part + hv_up16((size_t)V * W.P * S * 2 * 8);
    W.hist = W.sel + hv_up16((size_t)V * S * 2 * Q * sizeof(LsSel));
    W.total = W.hist + hv_up16((size_t)W.nhist * 4);
    return W;
}
static inline bool ls_sizes_ok(int V, int A0, int A1, int A2, int S, int Q) {
    return V > 0 && A0 > 0 && A1 > 0 && A2 > 0 && S >= 1 && S <= HV_LS_MAX_LABELS && Q >= 0 && Q <= HV_LS_MAX_Q;
}
static inline bool ls_vol_dtype_ok(int dt) { return dt == HV_DT_U8 || dt == HV_DT_I16 || dt == HV_DT_F32 || dt == HV_DT_F64; }
static inline bool ls_label_dtype_ok(int dt) { return dt >= HV_DT_U8 && dt <= HV_DT_F64; }

extern "C" size_t hv_label_stats_workspace_bytes(int V, int A0, int A1, int A2, int S, int Q) {
    if (!ls_sizes_ok(V, A0, A1, A2, S, Q) || hv_too_large(V, A0, A1, A2)) return 0;
    return ls_layout(V, A0, A1, A2, S, Q).total;
}

template <typename T>
static int ls_run(const LsArgs& a, const LsWs& W, char* ws, double* out, hipStream_t st) {
    typedef LsKey<T> K;
    u64* acc = (u64*)(ws + W.acc);
    u64* vbad = (u64*)(ws + W.vbad);
    double* part = (double*)(ws + W.part);
    LsSel* sel = (LsSel*)(ws + W.sel);
    unsigned* hist = (unsigned*)(ws + W.hist);
    const long long ninit = W.nacc > W.nhist ? W.nacc : W.nhist;
    hipLaunchKernelGGL(ls_init_kernel, dim3(min(hv_cdiv(ninit, LS_THREADS), 1024)), dim3(LS_THREADS), 0, st, acc, W.nacc, vbad, a.V, hist, W.nhist);
    HV_LAUNCH_CHECK();
    const size_t lds = (size_t)a.S * LS_ACC * 8 + (K::FLT ? (size_t)4 * a.S * 2 * 8 + (size_t)LS_CELLS * 8 + hv_up16(LS_CELLS) : 0);
    hipLaunchKernelGGL(ls_moments_kernel<T>, dim3(a.P, a.V), dim3(LS_THREADS), lds, st, a, acc, vbad, part);
    HV_LAUNCH_CHECK();
    const int nvs = a.V * a.S;
    hipLaunchKernelGGL(ls_fold_kernel, dim3(hv_cdiv(nvs, 64)), dim3(64), 0, st, a, K::FLT ? 1 : 0, acc, (const double*)part, sel);
    HV_LAUNCH_CHECK();
    if (a.Q > 0) {
        const long long N = (long long)a.A0 * a.A1 * a.A2;
        const int pairs = a.S * 2 * a.Q;
        const dim3 hg(min(hv_cdiv(N, LS_THREADS * 8), 1024), hv_cdiv(pairs, LS_PAIRS), a.V);
        for (int pass = 0; pass < K::BITS / 8; ++pass) {
            hipLaunchKernelGGL(ls_hist_kernel<T>, hg, dim3(LS_THREADS), 0, st, a, pass, (const LsSel*)sel, hist);
            HV_LAUNCH_CHECK();
            hipLaunchKernelGGL(ls_pick_kernel, dim3((unsigned)((long long)a.V * pairs)), dim3(64), 0, st, sel, hist);
            HV_LAUNCH_CHECK();
        }
    }
    hipLaunchKernelGGL(ls_final_kernel<T>, dim3(hv_cdiv(nvs, 64)), dim3(64), 0, st, a, (const u64*)acc, (const u64*)vbad, (const LsSel*)sel, out);
    HV_LAUNCH_CHECK();
    return HV_OK;
}

extern "C" int hv_label_stats(const void* vol, int vol_dtype, long long sv, long long s0, long long s1, long long s2, const void* label,
                              int label_dtype, long long lsv, long long ls0, long long ls1, long long ls2, const void* mask, long long msv,
                              long long ms0, long long ms1, long long ms2, int V, int A0, int A1, int A2, const int* labels, int S, const double* q,
                              int Q, double* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!vol || !label || !labels || !out || !workspace || !ls_sizes_ok(V, A0, A1, A2, S, Q) || (Q > 0 && !q) || !ls_vol_dtype_ok(vol_dtype) ||
        !ls_label_dtype_ok(label_dtype) || ((uintptr_t)workspace & 15) || ((uintptr_t)out & 7))
        return HV_ERR_ARG;
    LsArgs a;
    if (!hv_slot_table(a.slot, labels, S)) return HV_ERR_ARG;
    for (int t = 0; t < HV_LS_MAX_Q; ++t) {
        a.q[t] = 0.0;
        if (t < Q) {
            if (!(std::isfinite(q[t]) && q[t] >= 0.0 && q[t] <= 100.0)) return HV_ERR_ARG;
            a.q[t] = q[t];
        }
    }
    if (hv_too_large(V, A0, A1, A2)) return HV_ERR_UNSUPPORTED;
    const LsWs W = ls_layout(V, A0, A1, A2, S, Q);
    if (workspace_bytes < W.total) return HV_ERR_ARG;
    a.vol = hv_vol(vol, vol_dtype, sv, s0, s1, s2);
    a.lab = hv_vol(label, label_dtype, lsv, ls0, ls1, ls2);
    a.msk = hv_vol(mask, HV_DT_U8, msv, ms0, ms1, ms2);
    a.V = V; a.A0 = A0; a.A1 = A1; a.A2 = A2; a.S = S; a.Q = Q;
    hv_axis_order(a.vol, A0, A1, A2, a.ax_in, a.ax_mid, a.ax_out);
    a.n0 = W.n0; a.n1 = W.n1; a.n2 = W.n2; a.ntiles = W.ntiles; a.tpb = W.tpb; a.P = W.P;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    switch (vol_dtype) {
        case HV_DT_U8: return ls_run<uint8_t>(a, W, ws, out, st);
        case HV_DT_I16: return ls_run<int16_t>(a, W, ws, out, st);
        case HV_DT_F32: return ls_run<float>(a, W, ws, out, st);
        default: return ls_run<double>(a, W, ws, out, st);
    }
}
