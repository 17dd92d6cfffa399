// The (slot, level) code of a voxel, shared by the texture kernels (texture.hip: hv_glcm; texture_runs.hip: hv_glrlm, hv_gldm): a voxel's code is
// (slot << 6) | level, GL_NONE for a voxel outside the volume, without a slot or not finite; and the run of one slot a thread keeps while it
// quantises.  How the volumes are addressed, the slot rule and the finiteness test are volume_access.h's.
#pragma once
#include "volume_access.h"

#define GL_NONE 0xFFFFu

// a thread's run of one slot while it quantises: finite voxels, clamped from below, clamped from above, non-finite met; added to the workgroup's
// s_info [S][HV_GLCM_INFO] when the slot changes
struct GlRun { int slot; unsigned n, low, high, flag; };

__device__ __forceinline__ void gl_run_flush(const GlRun& r, unsigned* s_info) {
    if (r.slot == HV_NO_SLOT) return;
    unsigned* w = s_info + r.slot * HV_GLCM_INFO;
    if (r.flag) atomicOr(&w[0], r.flag);
    if (r.n) atomicAdd(&w[1], r.n);
    if (r.low) atomicAdd(&w[2], r.low);
    if (r.high) atomicAdd(&w[3], r.high);
}

