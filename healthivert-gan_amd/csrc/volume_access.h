// How a strided, typed, masked label volume is addressed, once for every kernel that does: the volume descriptor, the typed
// load, hv_label_stats' slot rule with the host's value -> slot table, the finiteness test, the axis order of a memory-order walk, and the two
// sizes every workspace layout and entry point repeats.  The Python side of the same contract is labelled.py.
#pragma once
#include "hv_common.h"

typedef unsigned long long u64;

// [V][A0][A1][A2] in elements: voxel (v; i, j, k) lies at p[v * sv + i * s0 + j * s1 + k * s2]
struct HvVol { const void* p; int dt; long long sv, s0, s1, s2; };

static inline HvVol hv_vol(const void* p, int dt, long long sv, long long s0, long long s1, long long s2) {
    HvVol x;
    x.p = p; x.dt = dt; x.sv = sv; x.s0 = s0; x.s1 = s1; x.s2 = s2;
    return x;
}

__device__ __forceinline__ double hv_ld_dt(const void* p, int dt, long long o) {
    switch (dt) {
        case HV_DT_U8: return (double)((const uint8_t*)p)[o];
        case HV_DT_I16: return (double)((const int16_t*)p)[o];
        case HV_DT_I32: return (double)((const int32_t*)p)[o];
        case HV_DT_I64: return (double)((const long long*)p)[o];
        case HV_DT_F32: return (double)((const float*)p)[o];
        default: return ((const double*)p)[o];
    }
}

__device__ __forceinline__ bool hv_finite(double x) { return ((u64)__double_as_longlong(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

#define HV_NO_SLOT 0xFF

// the slot of voxel (v; i, j, k) inside the volume: HV_NO_SLOT if masked out, not listed or not a label (then bad = 1).  A: kernel arguments with
// HvVol lab, msk (msk.p == NULL: no mask) and the table slot[256]
template <typename A>
__device__ __forceinline__ int hv_slot(const A& a, int v, int i, int j, int k, int& bad) {
    if (a.msk.p && ((const uint8_t*)a.msk.p)[v * a.msk.sv + i * a.msk.s0 + j * a.msk.s1 + k * a.msk.s2] == 0) return HV_NO_SLOT;
    const double d = hv_ld_dt(a.lab.p, a.lab.dt, v * a.lab.sv + i * a.lab.s0 + j * a.lab.s1 + k * a.lab.s2);
    if (!(d >= 0.0 && d <= 255.0 && d == floor(d))) { bad = 1; return HV_NO_SLOT; }   // NaN fails the first test
    return a.slot[(int)d];
}

// slot[value] = the value's index in labels[0 .. S), HV_NO_SLOT for a value not listed; false for a value outside [0, 255] or listed twice
static inline bool hv_slot_table(unsigned char slot[256], const int* labels, int S) {
    for (int i = 0; i < 256; ++i) slot[i] = HV_NO_SLOT;
    for (int s = 0; s < S; ++s) {
        if (labels[s] < 0 || labels[s] > 255 || slot[labels[s]] != HV_NO_SLOT) return false;
        slot[labels[s]] = (unsigned char)s;
    }
    return true;
}

// the logical axes by ascending |stride|, an extent-1 axis last; ties keep the higher axis inside (C order: 2, 1, 0)
static inline void hv_axis_order(const HvVol& x, int A0, int A1, int A2, int& ax_in, int& ax_mid, int& ax_out) {
    const long long str[3] = {x.s0, x.s1, x.s2};
    const int dims[3] = {A0, A1, A2};
    int ord[3] = {2, 1, 0};
    auto weight = [&](int ax) { return dims[ax] == 1 ? (long long)1 << 62 : (str[ax] < 0 ? -str[ax] : str[ax]); };
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2 - a; ++b)
            if (weight(ord[b + 1]) < weight(ord[b])) { const int t = ord[b]; ord[b] = ord[b + 1]; ord[b + 1] = t; }
    ax_in = ord[0]; ax_mid = ord[1]; ax_out = ord[2];
}

static inline size_t hv_up16(size_t b) { return (b + 15) & ~(size_t)15; }

// more than 2^30 voxels per volume or 65535 volumes per call (grid dimension y); positive extents: the product of two fits, checked before the third
static inline bool hv_too_large(int V, int A0, int A1, int A2) {
    return (long long)A0 * A1 > (1LL << 30) || (long long)A0 * A1 * A2 > (1LL << 30) || V > 65535;
}
