// The boundary extension of the volume filters (filter3d.hip, rankfilt.hip): scipy.ndimage's modes for 1-D filters, defined for ANY offset.
#pragma once
#include "hv_common.h"

// the index in [0, n) that position p of the extended line reads; -1: cval
__device__ __forceinline__ int fi_map(int p, int n, int mode) {
    if (p >= 0 && p < n) return p;
    switch (mode) {
        case HV_FILT_CONSTANT: return -1;
        case HV_FILT_NEAREST: return p < 0 ? 0 : n - 1;
        case HV_FILT_WRAP: {
            const int m = p % n;
            return m < 0 ? m + n : m;
        }
        case HV_FILT_REFLECT: {
            const long long n2 = 2LL * n;
            long long m = p % n2;
            if (m < 0) m += n2;
            return (int)(m < n ? m : n2 - 1 - m);
        }
        default: {                                // HV_FILT_MIRROR
            if (n == 1) return 0;
            const long long n2 = 2LL * n - 2;
            long long m = p % n2;
            if (m < 0) m += n2;
            return (int)(m < n ? m : n2 - m);
        }
    }
}
