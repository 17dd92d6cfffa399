// 3-D rank filters on the device: hv_rank_filter -- scipy.ndimage.rank_filter with a footprint of at most 9 x 9 x 9
// cells, the one kernel under median_filter, percentile_filter, minimum_filter / maximum_filter and the flat grey-scale morphology of
// rank_filters.py.  out[p] is the rank-th smallest of { ext(vol)[p + o] : o in the footprint }, ext the boundary extension of filter3d.hip
// (boundary_map.h).  Selection is exact in any arithmetic, so the result is scipy's without a tolerance; it is done on order-preserving integer
// keys of the element's own width (uint8: the byte; int16: the bits with the sign bit flipped; float32 / float64: all bits flipped for a
// negative number, the sign bit for a positive one -- -0.0 just below +0.0, NaNs at the two ends by their sign bit), and the voxel written is
// the key mapped back: one of the window's own voxels, or cval, bit for bit.
//
// One kernel, one launch.  A workgroup of 256 lanes owns a tile of RK_T^3 outputs whatever the strides (hv_rank_tile reports RK_T for every
// axis): the lanes run along the axis of the smallest source stride (role L), eight of them, then along the next (M); each lane computes two
// outputs RK_T / 2 apart along the third (O).  The tile plus a halo of the footprint's ACTUAL reach below and above along each axis (not 4) is
// staged as keys in LDS through the boundary map, so every later read is a plain LDS read and the tile's edge needs no test.  The footprint
// travels in the kernel arguments (hv_rank_footprint, 104 bytes); the tap loop walks its set bits with scalar instructions and is the same for
// every lane.  Rank 0 and rank n - 1 are one min / max sweep over the taps.  Any other rank is found by bisection of the key from its most
// significant bit: with `res` the bits known so far, the candidate res | bit is accepted when fewer than rank + 1 keys of the window lie below
// it.  That is (key bits) sweeps over the taps, whatever the data.  No atomics, no workspace, no scratch, no workgroup waits for another.
#include <cmath>
#include <cstring>
#include "hv_common.h"
#include "boundary_map.h"

#define RK_THREADS 256
#define RK_T 8                          // outputs per workgroup along each axis
#define RK_KEY_UNSIGNED 0
#define RK_KEY_SIGNED 1
#define RK_KEY_FLOAT 2

// the roles L (lanes), M and O are the host's permutation of the axes
struct RkP {
    const void* src; void* dst;
    long long sL, sM, sO, dL, dM, dO;
    int nL, nM, nO;
    int loL, loM, loO;                  // the halo below the tile (the footprint's reach towards negative offsets)
    int eL, eM, eO;                     // the staged extents: halo below + RK_T + halo above
    int f0, f1, f2;                     // what one step along the footprint's (= the host's) axis 0 / 1 / 2 is in staged elements
    int mode, rank, n;
    unsigned long long cval_key;
};

template <typename K, int KIND>
__device__ __forceinline__ K rk_to_key(K v) {
    constexpr K TOP = (K)((K)1 << (8 * sizeof(K) - 1));
    if (KIND == RK_KEY_UNSIGNED) return v;
    if (KIND == RK_KEY_SIGNED) return (K)(v ^ TOP);
    return (v & TOP) ? (K)~v : (K)(v ^ TOP);
}
template <typename K, int KIND>
__device__ __forceinline__ K rk_from_key(K k) {
    constexpr K TOP = (K)((K)1 << (8 * sizeof(K) - 1));
    if (KIND == RK_KEY_UNSIGNED) return k;
    if (KIND == RK_KEY_SIGNED) return (K)(k ^ TOP);
    return (k & TOP) ? (K)(k ^ TOP) : (K)~k;
}

// fn(the staged offset of a member from the window's centre) for every member of the footprint, in the order of the bits
template <typename Fn>
__device__ __forceinline__ void rk_taps(const hv_rank_footprint& F, const RkP& P, Fn fn) {
    for (int w = 0; w < HV_RANK_WORDS; ++w) {
        unsigned long long b = F.bits[w];
        while (b) {
            const int i = w * 64 + __builtin_ctzll(b);
            b &= b - 1;
            const int q = i / 9;
            fn((q / 9 - HV_RANK_REACH) * P.f0 + (q % 9 - HV_RANK_REACH) * P.f1 + (i % 9 - HV_RANK_REACH) * P.f2);
        }
    }
}

// grid: the tiles, the one along L fastest
template <typename K, int KIND>
__global__ __launch_bounds__(RK_THREADS) void rank_kernel(RkP P, hv_rank_footprint F) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rk_lds[];
    K* keys = reinterpret_cast<K*>(rk_lds);
    const int ntL = (P.nL + RK_T - 1) / RK_T, ntM = (P.nM + RK_T - 1) / RK_T;
    const int tL = (int)(blockIdx.x % ntL), tM = (int)((blockIdx.x / ntL) % ntM), tO = (int)(blockIdx.x / ((unsigned)ntL * ntM));
    const int bL = tL * RK_T - P.loL, bM = tM * RK_T - P.loM, bO = tO * RK_T - P.loO;      // where staged element 0 lies in the volume
    const K* src = reinterpret_cast<const K*>(P.src);
    const int ne = P.eL * P.eM * P.eO;
    for (int e = threadIdx.x; e < ne; e += RK_THREADS) {
        const int l = e % P.eL, m = (e / P.eL) % P.eM, o = e / (P.eL * P.eM);
        const int iL = fi_map(bL + l, P.nL, P.mode), iM = fi_map(bM + m, P.nM, P.mode), iO = fi_map(bO + o, P.nO, P.mode);
        K k = (K)P.cval_key;
        if ((iL | iM | iO) >= 0) k = rk_to_key<K, KIND>(src[iL * P.sL + iM * P.sM + iO * P.sO]);
        keys[e] = k;
    }
    __syncthreads();
    const int l = threadIdx.x % RK_T, m = (threadIdx.x / RK_T) % RK_T, o = threadIdx.x / (RK_T * RK_T);
    const K* w0 = keys + ((o + P.loO) * P.eM + m + P.loM) * P.eL + l + P.loL;              // the centre of the lane's first window
    const K* w1 = w0 + (RK_T / 2) * P.eM * P.eL;                                          // and of its second
    K r0, r1;
    if (P.rank == 0) {
        r0 = r1 = (K)~(K)0;
        rk_taps(F, P, [&](int off) {
            const K a = w0[off], b = w1[off];
            r0 = a < r0 ? a : r0;
            r1 = b < r1 ? b : r1;
        });
    } else if (P.rank == P.n - 1) {
        r0 = r1 = (K)0;
        rk_taps(F, P, [&](int off) {
            const K a = w0[off], b = w1[off];
            r0 = a > r0 ? a : r0;
            r1 = b > r1 ? b : r1;
        });
    } else {
        r0 = r1 = (K)0;
        for (int bit = 8 * (int)sizeof(K) - 1; bit >= 0; --bit) {
            const K c0 = (K)(r0 | (K)((K)1 << bit)), c1 = (K)(r1 | (K)((K)1 << bit));
            int below0 = 0, below1 = 0;
            rk_taps(F, P, [&](int off) {
                below0 += w0[off] < c0 ? 1 : 0;
                below1 += w1[off] < c1 ? 1 : 0;
            });
            r0 = below0 <= P.rank ? c0 : r0;          // at most `rank` keys below the candidate: the rank-th smallest is not below it
            r1 = below1 <= P.rank ? c1 : r1;
        }
    }
    const int gL = tL * RK_T + l, gM = tM * RK_T + m, gO = tO * RK_T + o;
    if (gL >= P.nL || gM >= P.nM) return;
    K* dst = reinterpret_cast<K*>(P.dst);
    const long long d = gL * P.dL + gM * P.dM;
    if (gO < P.nO) dst[d + gO * P.dO] = rk_from_key<K, KIND>(r0);
    if (gO + RK_T / 2 < P.nO) dst[d + (gO + RK_T / 2) * P.dO] = rk_from_key<K, KIND>(r1);
}

// ------------------------------------------------------------------------------------------------ host side
static inline long long rk_abs(long long v) { return v < 0 ? -v : v; }
static inline size_t rk_elem(int dt) { return dt == HV_DT_U8 ? 1 : dt == HV_DT_I16 ? 2 : dt == HV_DT_F32 ? 4 : 8; }
// the bytes [lo, hi) a strided box touches, relative to its base pointer
static void rk_span(const int* A, const long long* s, size_t elem, long long* lo, long long* hi) {
    long long mn = 0, mx = 0;
    for (int a = 0; a < 3; ++a) {
        const long long e = (long long)(A[a] - 1) * s[a];
        if (e < 0) mn += e; else mx += e;
    }
    *lo = mn * (long long)elem;
    *hi = (mx + 1) * (long long)elem;
}
// the key of cval; false: not finite or not a value of the dtype
static bool rk_cval_key(int dt, double cval, unsigned long long* key) {
    if (!std::isfinite(cval)) return false;
    if (dt == HV_DT_U8 || dt == HV_DT_I16) {
        const double lo = dt == HV_DT_U8 ? 0.0 : -32768.0, hi = dt == HV_DT_U8 ? 255.0 : 32767.0;
        if (cval < lo || cval > hi || cval != std::floor(cval)) return false;
        *key = dt == HV_DT_U8 ? (unsigned long long)(uint8_t)cval : (unsigned long long)(uint16_t)((uint16_t)(int16_t)cval ^ 0x8000u);
        return true;
    }
    if (dt == HV_DT_F32) {
        if (std::fabs(cval) > 3.4028234663852886e38) return false;          // beyond FLT_MAX: the conversion is not defined
        const float f = (float)cval;
        if ((double)f != cval) return false;
        uint32_t b;
        memcpy(&b, &f, 4);
        *key = (b & 0x80000000u) ? (uint32_t)~b : (b ^ 0x80000000u);
        return true;
    }
    uint64_t b;
    memcpy(&b, &cval, 8);
    *key = (b >> 63) ? ~b : (b ^ (1ULL << 63));
    return true;
}

extern "C" int hv_rank_tile(int* dims) {
    if (!dims) return HV_ERR_ARG;
    dims[0] = dims[1] = dims[2] = RK_T;
    return HV_OK;
}

extern "C" int hv_rank_filter(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2,
                              const hv_rank_footprint* fp, int rank, int mode, double cval, void* out, long long os0, long long os1,
                              long long os2, void* stream) {
    if (!vol || !out || !fp || A0 <= 0 || A1 <= 0 || A2 <= 0 || (dtype != HV_DT_U8 && dtype != HV_DT_I16 && dtype != HV_DT_F32 && dtype != HV_DT_F64) ||
        mode < HV_FILT_REFLECT || mode > HV_FILT_WRAP)
        return HV_ERR_ARG;
    // the footprint: its size, and its reach below and above along each axis
    if (fp->bits[HV_RANK_WORDS - 1] >> (729 - 64 * (HV_RANK_WORDS - 1))) return HV_ERR_ARG;
    int n = 0, mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    for (int w = 0; w < HV_RANK_WORDS; ++w)
        for (unsigned long long b = fp->bits[w]; b; b &= b - 1) {
            const int i = w * 64 + __builtin_ctzll(b);
            const int o[3] = {i / 81 - HV_RANK_REACH, (i / 9) % 9 - HV_RANK_REACH, i % 9 - HV_RANK_REACH};
            for (int a = 0; a < 3; ++a) {
                if (o[a] < mn[a]) mn[a] = o[a];
                if (o[a] > mx[a]) mx[a] = o[a];
            }
            ++n;
        }
    if (fp->n < 1 || fp->n != n || rank < 0 || rank >= n) return HV_ERR_ARG;
    RkP P;
    if (!rk_cval_key(dtype, cval, &P.cval_key)) return HV_ERR_ARG;
    if ((long long)A0 * A1 * A2 > (1LL << 30)) return HV_ERR_UNSUPPORTED;
    const int A[3] = {A0, A1, A2};
    const long long ss[3] = {s0, s1, s2}, os[3] = {os0, os1, os2};
    long long vlo, vhi, olo, ohi;
    rk_span(A, ss, rk_elem(dtype), &vlo, &vhi);
    rk_span(A, os, rk_elem(dtype), &olo, &ohi);
    if ((intptr_t)vol + vlo < (intptr_t)out + ohi && (intptr_t)out + olo < (intptr_t)vol + vhi) return HV_ERR_ARG;
    // the roles: L the axis of the smallest source stride (an axis of extent 1 has no stride to speak of: it comes last), then M, then O
    int ord[3] = {0, 1, 2};
    auto before = [&](int a, int b) {
        if ((A[a] > 1) != (A[b] > 1)) return A[a] > 1;
        if (rk_abs(ss[a]) != rk_abs(ss[b])) return rk_abs(ss[a]) < rk_abs(ss[b]);
        return a > b;
    };
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2 - i; ++j)
            if (before(ord[j + 1], ord[j])) { const int t = ord[j]; ord[j] = ord[j + 1]; ord[j + 1] = t; }
    const int L = ord[0], M = ord[1], O = ord[2];
    P.src = vol; P.dst = out;
    P.sL = ss[L]; P.sM = ss[M]; P.sO = ss[O]; P.dL = os[L]; P.dM = os[M]; P.dO = os[O];
    P.nL = A[L]; P.nM = A[M]; P.nO = A[O];
    P.loL = -mn[L]; P.loM = -mn[M]; P.loO = -mn[O];
    P.eL = RK_T + mx[L] - mn[L]; P.eM = RK_T + mx[M] - mn[M]; P.eO = RK_T + mx[O] - mn[O];
    int f[3];
    f[L] = 1; f[M] = P.eL; f[O] = P.eL * P.eM;
    P.f0 = f[0]; P.f1 = f[1]; P.f2 = f[2];
    P.mode = mode; P.rank = rank; P.n = n;
    const long long blocks = (long long)hv_cdiv(A0, RK_T) * hv_cdiv(A1, RK_T) * hv_cdiv(A2, RK_T);
    const size_t lds = ((size_t)P.eL * P.eM * P.eO * rk_elem(dtype) + 15) & ~(size_t)15;
    const dim3 grid((unsigned)blocks), block(RK_THREADS);
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
        case HV_DT_U8: hipLaunchKernelGGL((rank_kernel<uint8_t, RK_KEY_UNSIGNED>), grid, block, lds, st, P, *fp); break;
        case HV_DT_I16: hipLaunchKernelGGL((rank_kernel<uint16_t, RK_KEY_SIGNED>), grid, block, lds, st, P, *fp); break;
        case HV_DT_F32: hipLaunchKernelGGL((rank_kernel<uint32_t, RK_KEY_FLOAT>), grid, block, lds, st, P, *fp); break;
        default: hipLaunchKernelGGL((rank_kernel<uint64_t, RK_KEY_FLOAT>), grid, block, lds, st, P, *fp); break;
    }
    HV_LAUNCH_CHECK();
    return HV_OK;
}
