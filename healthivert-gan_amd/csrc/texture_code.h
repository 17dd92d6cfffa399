// The (slot, level) code of a voxel, shared by the texture kernels (texture.hip: hv_glcm; texture_runs.hip: hv_glrlm, hv_gldm): how a volume, a
// label volume and a mask are addressed, hv_label_stats' slot rule, and the finiteness test.  A voxel's code is (slot << 6) | level, GL_NONE for
// a voxel outside the volume, without a slot or not finite.
#pragma once
#include "hv_common.h"

#define GL_NONE 0xFFFFu

typedef unsigned long long u64;

struct GlVol { const void* p; int dt; long long sv, s0, s1, s2; };

__device__ __forceinline__ double gl_ld_dt(const void* p, int dt, long long o) {
    switch (dt) {
        case HV_DT_U8: return (double)((const uint8_t*)p)[o];
        case HV_DT_I16: return (double)((const int16_t*)p)[o];
        case HV_DT_I32: return (double)((const int32_t*)p)[o];
        case HV_DT_I64: return (double)((const long long*)p)[o];
        case HV_DT_F32: return (double)((const float*)p)[o];
        default: return ((const double*)p)[o];
    }
}

// the slot of voxel (v; i, j, k): 0xFF if masked out, not listed or not a label (then bad = 1); hv_label_stats' rule.  A: kernel arguments with
// GlVol lab, msk (msk.p == NULL: no mask) and the table slot[256]
template <typename A>
__device__ __forceinline__ int gl_slot(const A& a, int v, int i, int j, int k, int& bad) {
    if (a.msk.p && ((const uint8_t*)a.msk.p)[v * a.msk.sv + i * a.msk.s0 + j * a.msk.s1 + k * a.msk.s2] == 0) return 0xFF;
    const double d = gl_ld_dt(a.lab.p, a.lab.dt, v * a.lab.sv + i * a.lab.s0 + j * a.lab.s1 + k * a.lab.s2);
    if (!(d >= 0.0 && d <= 255.0 && d == floor(d))) { bad = 1; return 0xFF; }   // NaN fails the first test
    return a.slot[(int)d];
}

__device__ __forceinline__ bool gl_finite(double x) { return ((u64)__double_as_longlong(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

// a thread's run of one slot while it quantises: finite voxels, clamped from below, clamped from above, non-finite met; added to the workgroup's
// s_info [S][HV_GLCM_INFO] when the slot changes
struct GlRun { int slot; unsigned n, low, high, flag; };

__device__ __forceinline__ void gl_run_flush(const GlRun& r, unsigned* s_info) {
    if (r.slot == 0xFF) return;
    unsigned* w = s_info + r.slot * HV_GLCM_INFO;
    if (r.flag) atomicOr(&w[0], r.flag);
    if (r.n) atomicAdd(&w[1], r.n);
    if (r.low) atomicAdd(&w[2], r.low);
    if (r.high) atomicAdd(&w[3], r.high);
}

// the logical axes by ascending |stride|, an extent-1 axis last; ties keep the higher axis inside (C order: 2, 1, 0)
static inline void gl_axis_order(const long long str[3], const int dims[3], int ord[3]) {
    ord[0] = 2; ord[1] = 1; ord[2] = 0;
    auto weight = [&](int ax) { return dims[ax] == 1 ? (long long)1 << 62 : (str[ax] < 0 ? -str[ax] : str[ax]); };
    for (int x = 0; x < 2; ++x)
        for (int y = 0; y < 2 - x; ++y)
            if (weight(ord[y + 1]) < weight(ord[y])) { const int t = ord[y]; ord[y] = ord[y + 1]; ord[y + 1] = t; }
}
