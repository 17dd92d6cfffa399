// Slice preparation of the inference driver on the device (reference eval_3d_sagittal_twostage.py:15-30,46-98):
//   slice_components_kernel   8-connected components of (label == vertebra id) per slice, components below min_size dropped, then the
//                             statistics run_model derives from the remaining pixels: count, first / last row, sum of row indices
//   infer_prepare_kernel      bounding rows (40-row window around the mean row when the vertebra is taller than maxheight), the masked band,
//                             uint8 quantisation, row re-stacking, ToTensor / Normalize -> the four planes the generator consumes
//   select_slices_kernel      dst[s] = flag[s] ? src[s] : (keep dst[s] | 0): slices without the vertebra pass through a stage unchanged
// Integer / byte work, bit-exact against the reference (fixture G10).  One workgroup owns one slice.
#include "hv_common.h"

__device__ __forceinline__ int coherent_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Label equivalence (Hawick et al.): L[p] = index of a pixel of the same component with a smaller-or-equal index; "scan" lowers the root of
// a pixel's tree to the smallest neighbouring label (atomicMin), "analysis" points every pixel at its root; repeat until a scan changes
// nothing.  Labels live in global memory (64 K pixels x 4 B exceed the LDS) and are read with device-scope loads: the atomics resolve in L2.
// T = float (label maps of the inference driver) or unsigned char (the uint8 mask planes of the batch assembler).  keep != NULL: the filtered
// mask is written back (value where the pixel's component survived, 0 elsewhere; may be the input plane itself: it is read only by the
// first loop).
template <typename T>
__global__ __launch_bounds__(1024) void slice_components_kernel(const T* __restrict__ label, int H, int W, T value, int min_size,
                                                                int* __restrict__ Lall, int* __restrict__ Call, int* __restrict__ stats,
                                                                T* keep) {
    __shared__ int changed, s_cnt, s_min, s_max, s_sum;
    const int HW = H * W, tid = threadIdx.x;
    const T* lab = label + (long long)blockIdx.x * HW;
    int* L = Lall + (long long)blockIdx.x * HW;
    int* C = Call + (long long)blockIdx.x * HW;
    for (int p = tid; p < HW; p += 1024) {
        L[p] = lab[p] == value ? p : -1;
        C[p] = 0;
    }
    __threadfence();
    __syncthreads();
    for (int iter = 0; iter < 4096; ++iter) {      // bound: a pass that changes nothing ends the loop long before
        if (tid == 0) changed = 0;
        __syncthreads();
        for (int p = tid; p < HW; p += 1024) {
            const int l = coherent_load(L + p);
            if (l < 0) continue;
            const int r = p / W, c = p - r * W;
            int m = l;
#pragma unroll
            for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
                for (int dc = -1; dc <= 1; ++dc) {
                    if (!dr && !dc) continue;
                    const int rr = r + dr, cc = c + dc;
                    if ((unsigned)rr < (unsigned)H && (unsigned)cc < (unsigned)W) {
                        const int lq = coherent_load(L + rr * W + cc);
                        if (lq >= 0 && lq < m) m = lq;
                    }
                }
            if (m < l) {
                atomicMin(L + l, m);
                changed = 1;
            }
        }
        __threadfence();
        __syncthreads();
        for (int p = tid; p < HW; p += 1024) {
            int l = coherent_load(L + p);
            if (l < 0) continue;
            int r = coherent_load(L + l);
            while (r != l) { l = r; r = coherent_load(L + l); }
            L[p] = r;
        }
        __threadfence();
        __syncthreads();
        if (!changed) break;
        __syncthreads();
    }
    for (int p = tid; p < HW; p += 1024) {
        const int l = coherent_load(L + p);
        if (l >= 0) atomicAdd(C + l, 1);
    }
    if (tid == 0) { s_cnt = 0; s_min = 1 << 30; s_max = -1; s_sum = 0; }
    __threadfence();
    __syncthreads();
    int cnt = 0, rmin = 1 << 30, rmax = -1, rsum = 0;
    for (int p = tid; p < HW; p += 1024) {
        const int l = coherent_load(L + p);
        const bool kept = l >= 0 && coherent_load(C + l) >= min_size;
        if (kept) {
            const int r = p / W;
            ++cnt; rsum += r;
            rmin = min(rmin, r); rmax = max(rmax, r);
        }
        if (keep) keep[(long long)blockIdx.x * HW + p] = kept ? value : (T)0;
    }
    if (cnt) { atomicAdd(&s_cnt, cnt); atomicAdd(&s_sum, rsum); atomicMin(&s_min, rmin); atomicMax(&s_max, rmax); }
    __syncthreads();
    if (tid == 0) {
        int* o = stats + blockIdx.x * 4;
        o[0] = s_cnt; o[1] = s_cnt ? s_min : -1; o[2] = s_max; o[3] = s_sum;
    }
}

extern "C" size_t hv_slice_components_workspace_bytes(int S, int H, int W) {
    return (size_t)2 * S * H * W * sizeof(int);
}
// HV_OK, or the status to return before any launch.  Pixel indices are ints; the row sum (s_sum, the per-thread rsum and stats[3] are ints) of a full slice
// is W * (0 + 1 + ... + (H - 1)) = H * W * (H - 1) / 2, which must not pass INT_MAX: 65536 x 1 is the tallest column accepted.
static int components_shape(int H, int W) {
    if ((long long)H * W > (1 << 24)) return HV_ERR_UNSUPPORTED;
    if ((long long)H * W * (H - 1) / 2 > 2147483647ll) return HV_ERR_UNSUPPORTED;
    return HV_OK;
}
extern "C" int hv_slice_components(const float* label, int S, int H, int W, float value, int min_size, int* stats, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    if (!label || !stats || S <= 0 || H <= 0 || W <= 0) return HV_ERR_ARG;
    if (components_shape(H, W) != HV_OK) return HV_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < hv_slice_components_workspace_bytes(S, H, W)) return HV_ERR_WORKSPACE;
    int* L = reinterpret_cast<int*>(workspace);
    hipLaunchKernelGGL(slice_components_kernel<float>, dim3(S), dim3(1024), 0, (hipStream_t)stream, label, H, W, value, min_size, L,
                       L + (long long)S * H * W, stats, (float*)nullptr);
    HV_LAUNCH_CHECK();
    return HV_OK;
}
extern "C" int hv_slice_components_u8(const void* plane, int S, int H, int W, int value, int min_size, int* stats, void* filtered,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    if (!plane || !stats || S <= 0 || H <= 0 || W <= 0 || value <= 0 || value > 255) return HV_ERR_ARG;
    if (components_shape(H, W) != HV_OK) return HV_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < hv_slice_components_workspace_bytes(S, H, W)) return HV_ERR_WORKSPACE;
    int* L = reinterpret_cast<int*>(workspace);
    hipLaunchKernelGGL(slice_components_kernel<unsigned char>, dim3(S), dim3(1024), 0, (hipStream_t)stream, (const unsigned char*)plane, H, W,
                       (unsigned char)value, min_size, L, L + (long long)S * H * W, stats, (unsigned char*)filtered);
    HV_LAUNCH_CHECK();
    return HV_OK;
}

// count[s] = number of elements of slice s equal to `value` (the reference's `np.sum(label[:, :, z] == neighbour) > 200` gate on the ORIGINAL
// labels, eval_3d_sagittal_twostage.py:208,217): one workgroup per slice, integer sums in a fixed order
__global__ __launch_bounds__(1024) void slice_count_kernel(const float* __restrict__ label, long long per, float value, int* __restrict__ count) {
    __shared__ int red[16];
    const float* lab = label + (long long)blockIdx.x * per;
    int c = 0;
    for (long long i = threadIdx.x; i < per; i += 1024) c += lab[i] == value ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int k = 0; k < 16; ++k) t += red[k];
        count[blockIdx.x] = t;
    }
}
extern "C" int hv_slice_count(const float* label, int S, long long per_slice, float value, int* count, void* stream) {
    if (!label || !count || S <= 0 || per_slice <= 0 || per_slice > (1ll << 30)) return HV_ERR_ARG;
    hipLaunchKernelGGL(slice_count_kernel, dim3(S), dim3(1024), 0, (hipStream_t)stream, label, per_slice, value, count);
    HV_LAUNCH_CHECK();
    return HV_OK;
}

struct PrepK {
    const float* ct; const float* cam; const int* stats; const int* selected;
    float* ct_masked; float* ori_ct; float* mask; float* cam_out;
    long long* x1; long long* x2; long long* height; int* valid;
    int H, W, maxheight;
};

__device__ __forceinline__ unsigned quant_u8(float v) { return (unsigned)(int)v & 255u; }   // numpy astype(uint8) of an in-range float: truncation

__global__ __launch_bounds__(256) void infer_prepare_kernel(const PrepK k) {
    const int s = blockIdx.y, H = k.H, W = k.W;
    const int* st = k.stats + s * 4;
    const bool valid = st[0] > 0 && (!k.selected || k.selected[s]);
    int x1 = 0, x2 = 0, height = H, min_x = 0, max_x = 0;
    if (valid) {
        x1 = st[1]; x2 = st[2];
        height = x2 - x1;
        if (height > k.maxheight) {       // 40-row window around the mean row (:58-61); `height` keeps the full extent
            x1 = st[3] / st[0] - 20;
            x2 = x1 + 40;
        }
        const int mask_x = (x1 + x2) >> 1, h2 = k.maxheight;     // floor division like Python's // (x1 + x2 may be negative only when invalid)
        if (mask_x <= h2 / 2) min_x = 0;
        else if (2 * (H - mask_x) <= h2) min_x = H - h2;
        else min_x = mask_x - h2 / 2;
        max_x = min_x + h2;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // slices without the vertebra: rows that keep the re-compositing kernels inside the image (their result is discarded)
        k.x1[s] = x1; k.x2[s] = x2; k.height[s] = height; k.valid[s] = valid ? 1 : 0;
    }
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H * W) return;
    const int r = p / W;
    const long long o = (long long)s * H * W + p;
    const float* ct = k.ct + (long long)s * H * W;
    const float* cam = k.cam + (long long)s * H * W;
    k.ori_ct[o] = ((float)quant_u8(ct[p]) / 255.0f - 0.5f) / 0.5f;
    unsigned cq = 0, mq = 0;
    float band = 0.f;
    if (valid) {
        band = (r >= min_x && r <= max_x) ? 1.0f : 0.0f;                // one row more than the data band (:75)
        int src = -1;
        if (r < min_x) src = r + (x1 - min_x);
        else if (r >= max_x) src = x2 + (r - max_x);
        if ((unsigned)src < (unsigned)H) { cq = quant_u8(ct[src * W + (p - r * W)]); mq = quant_u8(cam[src * W + (p - r * W)]); }
    }
    k.ct_masked[o] = ((float)cq / 255.0f - 0.5f) / 0.5f;
    k.mask[o] = band;
    k.cam_out[o] = (float)mq / 255.0f;
}

extern "C" int hv_infer_prepare(const float* ct, const float* cam, const int* stats, const int* selected, int S, int H, int W, int maxheight,
                                float* ct_masked, float* ori_ct, float* mask, float* cam_out, long long* x1, long long* x2, long long* height,
                                int* valid, void* stream) {
    if (!ct || !cam || !stats || !ct_masked || !ori_ct || !mask || !cam_out || !x1 || !x2 || !height || !valid) return HV_ERR_ARG;
    if (S <= 0 || S > 65535 || H <= 0 || W <= 0 || maxheight <= 0 || maxheight > H || (maxheight & 1)) return HV_ERR_ARG;
    PrepK k{ct, cam, stats, selected, ct_masked, ori_ct, mask, cam_out, x1, x2, height, valid, H, W, maxheight};
    hipLaunchKernelGGL(infer_prepare_kernel, dim3(hv_cdiv((long long)H * W, 256), S), dim3(256), 0, (hipStream_t)stream, k);
    HV_LAUNCH_CHECK();
    return HV_OK;
}

__global__ void select_slices_kernel(const int* __restrict__ flag, const float* __restrict__ src, float* __restrict__ dst, long long per, int keep) {
    const int s = blockIdx.y;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= per) return;
    const long long o = (long long)s * per + i;
    if (flag[s]) dst[o] = src[o];
    else if (!keep) dst[o] = 0.f;
}
extern "C" int hv_select_slices(const int* flag, const float* src, float* dst, int S, long long per_slice, int keep_unflagged, void* stream) {
    if (!flag || !src || !dst || S <= 0 || S > 65535 || per_slice <= 0) return HV_ERR_ARG;
    hipLaunchKernelGGL(select_slices_kernel, dim3(hv_cdiv(per_slice, 256), S), dim3(256), 0, (hipStream_t)stream, flag, src, dst, per_slice, keep_unflagged);
    HV_LAUNCH_CHECK();
    return HV_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// Volume intake / output of the inference driver on the device (reference eval_3d_sagittal_twostage.py:186-197,:208,:217,:236-239 and the `[:, z, :]`
// slicing of evaluation/RHLV_quantification_coronal.py:51-54): the [A0][A1][A2] volumes (A2 fastest; float64 as nibabel hands them over, or the
// float32 / uint8 volumes a resident producer leaves) are read as they lie -- no scan and no float32 conversion on the host.
// Slice axis 2 (sagittal, planes [A0][A1], p = a0 * A1 + a1): neighbouring voxels belong to different slices
//   volume_scan_kernel     counts[j][z] = number of voxels of slice z equal to ids[j] (the vertebra's extent and the two neighbours' > 200-pixel
//                          gates in one pass over the label volume; integer sums: exact in any order)
//   volume_slices_kernel   out[s][p] = (float)vol[p][z0 + s]: cut the range, convert (C cast, numpy's astype) and transpose to slices
//   volume_merge_kernel    out[p][z] = (z in range and flag[z - z0]) ? src[z - z0][p] : 0: the output volume as the reference builds it
//                          (np.zeros + per-slice assignment), z fastest
// Slice axis 1 (coronal, planes [A0][A2]): a plane row is A2 contiguous elements in the volume and in the slice alike, so nothing is transposed
//   rows_scan_kernel       one wave per row (a0, a1): it counts its matches and adds once per row and id
//   rows_slices_kernel     out[s][a0][:] = (float)vol[a0][k0 + s][:]
//   rows_merge_kernel      out[a0][k][:] = (k in range and flag[k - k0]) ? src[k - k0][a0][:] : 0
//   each with a 4-elements-per-lane form (WIDE: A2 % 4 == 0 and row starts aligned to the vector) and a scalar form for odd A2 / unaligned rows
template <typename T>
__global__ __launch_bounds__(256) void volume_scan_kernel(const T* __restrict__ label, long long n, int Z, double id0, double id1, double id2,
                                                          int* __restrict__ counts) {
    extern __shared__ int hist[];      // [3][Z]
    for (int i = threadIdx.x; i < 3 * Z; i += 256) hist[i] = 0;
    __syncthreads();
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const double v = (double)label[i];
        if (v == 0.0) continue;          // background: no id is 0 (checked on the host side)
        const int z = (int)(i % Z);
        if (v == id0) atomicAdd(hist + z, 1);
        else if (v == id1) atomicAdd(hist + Z + z, 1);
        else if (v == id2) atomicAdd(hist + 2 * Z + z, 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * Z; i += 256)
        if (hist[i]) atomicAdd(counts + i, hist[i]);
}

// 64 pixels x 32 slices per workgroup through LDS: 256-byte runs of doubles in, 256-byte runs of floats out
template <typename T>
__global__ __launch_bounds__(256) void volume_slices_kernel(const T* __restrict__ vol, long long HW, int Z, int z0, int S, float* __restrict__ out) {
    __shared__ float t[64][33];
    const long long p0 = (long long)blockIdx.x * 64;
    const int s0 = blockIdx.y * 32, zz = threadIdx.x & 31, pr = threadIdx.x >> 5;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const long long p = p0 + pr + 8 * k;
        t[pr + 8 * k][zz] = (p < HW && s0 + zz < S) ? (float)vol[p * Z + z0 + s0 + zz] : 0.f;
    }
    __syncthreads();
    const int pl = threadIdx.x & 63, sr = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int s = s0 + sr + 4 * k;
        if (s < S && p0 + pl < HW) out[(long long)s * HW + p0 + pl] = t[pl][sr + 4 * k];
    }
}

template <typename TO>
__global__ __launch_bounds__(256) void volume_merge_kernel(const float* __restrict__ src, const int* __restrict__ flag, long long HW, int Z, int z0, int S,
                                                           TO* __restrict__ out) {
    __shared__ float t[64][33];
    const long long p0 = (long long)blockIdx.x * 64;
    const int zb = blockIdx.y * 32;                 // 32 output slices zb .. zb + 31 of the FULL z range
    const int pl = threadIdx.x & 63, sr = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int z = zb + sr + 4 * k, s = z - z0;
        const bool in = z < Z && s >= 0 && s < S && p0 + pl < HW && flag[s] != 0;
        t[pl][sr + 4 * k] = in ? src[(long long)s * HW + p0 + pl] : 0.f;
    }
    __syncthreads();
    const int zz = threadIdx.x & 31, pr = threadIdx.x >> 5;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const long long p = p0 + pr + 8 * k;
        if (p < HW && zb + zz < Z) out[p * Z + zb + zz] = (TO)t[pr + 8 * k][zz];
    }
}

template <typename T> using vec4_t = T __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void rows_count_add(int* dst, int c, int lane) {
    if (__ballot(c != 0) == 0) return;      // the same in every lane: all 64 lanes reach the shuffles
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) atomicAdd(dst, c);
}

// one wave per row of A2 contiguous voxels (all of one slice a1): per-lane match counts, one shuffle sum and one atomic per row and id that occurs
template <typename T, bool WIDE>
__global__ __launch_bounds__(256) void rows_scan_kernel(const T* __restrict__ label, long long rows, int A1, int A2, double id0, double id1, double id2,
                                                        int* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const long long nw = (long long)gridDim.x * 4;
    for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += nw) {
        const T* row = label + r * A2;
        int c0 = 0, c1 = 0, c2 = 0;
        if (WIDE) {
            for (int c = lane * 4; c < A2; c += 256) {
                const vec4_t<T> q = *reinterpret_cast<const vec4_t<T>*>(row + c);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double v = (double)q[j];
                    c0 += v == id0; c1 += v == id1; c2 += v == id2;
                }
            }
        } else {
            for (int c = lane; c < A2; c += 64) {
                const double v = (double)row[c];
                c0 += v == id0; c1 += v == id1; c2 += v == id2;
            }
        }
        const int k = (int)(r % A1);
        rows_count_add(counts + k, c0, lane);
        rows_count_add(counts + A1 + k, c1, lane);
        rows_count_add(counts + 2 * A1 + k, c2, lane);
    }
}

// grid (items of one slice / 256, S): item = 4 elements (WIDE) or 1 of row a0; rows are contiguous on both sides
template <typename T, bool WIDE>
__global__ __launch_bounds__(256) void rows_slices_kernel(const T* __restrict__ vol, int A0, int A1, int A2, int k0, float* __restrict__ out) {
    const unsigned per = WIDE ? (unsigned)A2 >> 2 : (unsigned)A2;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)A0 * per) return;
    const unsigned a0 = i / per, c = (i - a0 * per) * (WIDE ? 4u : 1u);
    const int s = blockIdx.y;
    const T* src = vol + ((long long)a0 * A1 + k0 + s) * A2 + c;
    float* dst = out + ((long long)s * A0 + a0) * A2 + c;
    if (WIDE) {
        const vec4_t<T> q = *reinterpret_cast<const vec4_t<T>*>(src);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (float)q[j];
        *reinterpret_cast<f32x4*>(dst) = o;
    } else {
        *dst = (float)*src;
    }
}

// grid (items of one slice / 256, A1): every element of out is written; the flag test is the same for the whole workgroup
template <typename TO, bool WIDE>
__global__ __launch_bounds__(256) void rows_merge_kernel(const float* __restrict__ src, const int* __restrict__ flag, int A0, int A1, int A2, int k0, int S,
                                                         TO* __restrict__ out) {
    const unsigned per = WIDE ? (unsigned)A2 >> 2 : (unsigned)A2;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)A0 * per) return;
    const unsigned a0 = i / per, c = (i - a0 * per) * (WIDE ? 4u : 1u);
    const int k = blockIdx.y, s = k - k0;
    const bool in = s >= 0 && s < S && flag[s] != 0;
    TO* dst = out + ((long long)a0 * A1 + k) * A2 + c;
    const float* from = src + ((long long)(in ? s : 0) * A0 + a0) * A2 + c;
    if (WIDE) {
        f32x4 q = {0.f, 0.f, 0.f, 0.f};
        if (in) q = *reinterpret_cast<const f32x4*>(from);
        vec4_t<TO> o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (TO)q[j];
        *reinterpret_cast<vec4_t<TO>*>(dst) = o;
    } else {
        *dst = in ? (TO)*from : (TO)0;
    }
}

static int scan_grid(long long n) { return (int)(n / (256 * 16) < 1 ? 1 : (n / (256 * 16) > 2048 ? 2048 : n / (256 * 16))); }
static size_t dt_bytes(int dtype) { return dtype == HV_DT_F64 ? 8 : dtype == HV_DT_F32 ? 4 : dtype == HV_DT_U8 ? 1 : 0; }
static bool aligned_to(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
// shared argument rules of the three view entries: HV_OK, or the status to return before any launch
static int view_args(const void* a, const void* b, int A0, int A1, int A2, int axis) {
    if (!a || !b || A0 <= 0 || A1 <= 0 || A2 <= 0 || (axis != 1 && axis != 2)) return HV_ERR_ARG;
    // 32-bit item indices inside a plane (axis 1) / the p index of the tiles (axis 2)
    if ((long long)A0 * A1 > (1ll << 31) || (long long)A0 * A2 > (1ll << 31)) return HV_ERR_UNSUPPORTED;
    return HV_OK;
}

template <typename T>
static void scan_launch(const void* label, int A0, int A1, int A2, int axis, double id0, double id1, double id2, int* counts, hipStream_t s) {
    const T* lab = (const T*)label;
    if (axis == 2) {
        const long long n = (long long)A0 * A1 * A2;
        hipLaunchKernelGGL(volume_scan_kernel<T>, dim3(scan_grid(n)), dim3(256), (size_t)3 * A2 * sizeof(int), s, lab, n, A2, id0, id1, id2, counts);
        return;
    }
    const long long rows = (long long)A0 * A1;
    const int grid = (int)(rows / 4 < 1 ? 1 : (rows / 4 > 2048 ? 2048 : rows / 4));
    if (A2 % 4 == 0 && aligned_to(label, 4 * sizeof(T)))
        hipLaunchKernelGGL((rows_scan_kernel<T, true>), dim3(grid), dim3(256), 0, s, lab, rows, A1, A2, id0, id1, id2, counts);
    else
        hipLaunchKernelGGL((rows_scan_kernel<T, false>), dim3(grid), dim3(256), 0, s, lab, rows, A1, A2, id0, id1, id2, counts);
}
extern "C" int hv_volume_scan_view(const void* label, int dtype, int A0, int A1, int A2, int axis, double id0, double id1, double id2, int* counts,
                                   void* stream) {
    const int rc = view_args(label, counts, A0, A1, A2, axis);
    if (rc != HV_OK) return rc;
    if (!dt_bytes(dtype)) return HV_ERR_ARG;
    if (id0 == 0.0 || id1 == 0.0 || id2 == 0.0) return HV_ERR_ARG;      // unused ids are passed as a negative number
    if (axis == 2 && A2 > 2048) return HV_ERR_UNSUPPORTED;              // the per-workgroup histogram in LDS
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)3 * (axis == 2 ? A2 : A1) * sizeof(int), (hipStream_t)stream);
    if (e != hipSuccess) return -1000 - (int)e;
    if (dtype == HV_DT_F64) scan_launch<double>(label, A0, A1, A2, axis, id0, id1, id2, counts, (hipStream_t)stream);
    else if (dtype == HV_DT_F32) scan_launch<float>(label, A0, A1, A2, axis, id0, id1, id2, counts, (hipStream_t)stream);
    else scan_launch<unsigned char>(label, A0, A1, A2, axis, id0, id1, id2, counts, (hipStream_t)stream);
    HV_LAUNCH_CHECK();
    return HV_OK;
}
extern "C" int hv_volume_scan(const double* label, long long HW, int Z, double id0, double id1, double id2, int* counts, void* stream) {
    if (!label || !counts || HW <= 0 || Z <= 0 || Z > 2048) return HV_ERR_ARG;
    if (id0 == 0.0 || id1 == 0.0 || id2 == 0.0) return HV_ERR_ARG;      // unused ids are passed as a negative number
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)3 * Z * sizeof(int), (hipStream_t)stream);
    if (e != hipSuccess) return -1000 - (int)e;
    const long long n = HW * Z;
    hipLaunchKernelGGL(volume_scan_kernel<double>, dim3(scan_grid(n)), dim3(256), (size_t)3 * Z * sizeof(int), (hipStream_t)stream, label, n, Z, id0, id1, id2, counts);
    HV_LAUNCH_CHECK();
    return HV_OK;
}

template <typename T>
static void slices_launch(const void* vol, int A0, int A1, int A2, int axis, int k0, int S, float* out, hipStream_t s) {
    const T* v = (const T*)vol;
    if (axis == 2) {
        const long long HW = (long long)A0 * A1;
        hipLaunchKernelGGL(volume_slices_kernel<T>, dim3((unsigned)hv_cdiv(HW, 64), hv_cdiv(S, 32)), dim3(256), 0, s, v, HW, A2, k0, S, out);
        return;
    }
    if (A2 % 4 == 0 && aligned_to(vol, 4 * sizeof(T)) && aligned_to(out, 16))
        hipLaunchKernelGGL((rows_slices_kernel<T, true>), dim3((unsigned)hv_cdiv((long long)A0 * (A2 / 4), 256), S), dim3(256), 0, s, v, A0, A1, A2, k0, out);
    else
        hipLaunchKernelGGL((rows_slices_kernel<T, false>), dim3((unsigned)hv_cdiv((long long)A0 * A2, 256), S), dim3(256), 0, s, v, A0, A1, A2, k0, out);
}
extern "C" int hv_volume_slices_view(const void* vol, int dtype, int A0, int A1, int A2, int axis, int k0, int S, float* out, void* stream) {
    const int rc = view_args(vol, out, A0, A1, A2, axis);
    if (rc != HV_OK) return rc;
    if (!dt_bytes(dtype) || k0 < 0 || S <= 0 || (long long)k0 + S > (axis == 2 ? A2 : A1)) return HV_ERR_ARG;
    if (S > (axis == 2 ? 32 * 65535 : 65535)) return HV_ERR_UNSUPPORTED;     // grid.y
    if (dtype == HV_DT_F64) slices_launch<double>(vol, A0, A1, A2, axis, k0, S, out, (hipStream_t)stream);
    else if (dtype == HV_DT_F32) slices_launch<float>(vol, A0, A1, A2, axis, k0, S, out, (hipStream_t)stream);
    else slices_launch<unsigned char>(vol, A0, A1, A2, axis, k0, S, out, (hipStream_t)stream);
    HV_LAUNCH_CHECK();
    return HV_OK;
}
extern "C" int hv_volume_slices(const double* vol, long long HW, int Z, int z0, int S, float* out, void* stream) {
    if (!vol || !out || HW <= 0 || Z <= 0 || z0 < 0 || S <= 0 || z0 + S > Z || HW > (1ll << 31) || S > 32 * 65535) return HV_ERR_ARG;
    hipLaunchKernelGGL(volume_slices_kernel<double>, dim3((unsigned)hv_cdiv(HW, 64), hv_cdiv(S, 32)), dim3(256), 0, (hipStream_t)stream, vol, HW, Z, z0, S, out);
    HV_LAUNCH_CHECK();
    return HV_OK;
}

template <typename TO>
static void merge_launch(const float* src, const int* flag, int A0, int A1, int A2, int axis, int k0, int S, void* out, hipStream_t s) {
    TO* o = (TO*)out;
    if (axis == 2) {
        const long long HW = (long long)A0 * A1;
        hipLaunchKernelGGL(volume_merge_kernel<TO>, dim3((unsigned)hv_cdiv(HW, 64), hv_cdiv(A2, 32)), dim3(256), 0, s, src, flag, HW, A2, k0, S, o);
        return;
    }
    if (A2 % 4 == 0 && aligned_to(src, 16) && aligned_to(out, 4 * sizeof(TO)))
        hipLaunchKernelGGL((rows_merge_kernel<TO, true>), dim3((unsigned)hv_cdiv((long long)A0 * (A2 / 4), 256), A1), dim3(256), 0, s, src, flag, A0, A1, A2, k0, S, o);
    else
        hipLaunchKernelGGL((rows_merge_kernel<TO, false>), dim3((unsigned)hv_cdiv((long long)A0 * A2, 256), A1), dim3(256), 0, s, src, flag, A0, A1, A2, k0, S, o);
}
extern "C" int hv_volume_merge_view(const float* src, const int* flag, int A0, int A1, int A2, int axis, int k0, int S, int out_dtype, void* out,
                                    void* stream) {
    const int rc = view_args(src, out, A0, A1, A2, axis);
    if (rc != HV_OK) return rc;
    if (!flag || (out_dtype != HV_DT_F64 && out_dtype != HV_DT_F32) || k0 < 0 || S <= 0 || (long long)k0 + S > (axis == 2 ? A2 : A1)) return HV_ERR_ARG;
    if ((axis == 2 ? A2 : A1) > (axis == 2 ? 32 * 65535 : 65535)) return HV_ERR_UNSUPPORTED;     // grid.y
    if (out_dtype == HV_DT_F64) merge_launch<double>(src, flag, A0, A1, A2, axis, k0, S, out, (hipStream_t)stream);
    else merge_launch<float>(src, flag, A0, A1, A2, axis, k0, S, out, (hipStream_t)stream);
    HV_LAUNCH_CHECK();
    return HV_OK;
}
extern "C" int hv_volume_merge(const float* src, const int* flag, long long HW, int Z, int z0, int S, double* out, void* stream) {
    if (!src || !flag || !out || HW <= 0 || Z <= 0 || z0 < 0 || S <= 0 || z0 + S > Z || HW > (1ll << 31)) return HV_ERR_ARG;
    hipLaunchKernelGGL(volume_merge_kernel<double>, dim3((unsigned)hv_cdiv(HW, 64), hv_cdiv(Z, 32)), dim3(256), 0, (hipStream_t)stream, src, flag, HW, Z, z0, S, out);
    HV_LAUNCH_CHECK();
    return HV_OK;
}
