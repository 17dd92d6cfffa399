// De-pedicling of vertebra label crops on the device (reference straighten/straighten_mask_3d.py:189-219 process_layer / process_3d_array and
// :249-280 find_single_component_layers).
//
//   depedicle_kernel<T>   one workgroup owns one slice [:, :, z] of one volume (grid = slices x volumes).  One labelling pass for all label
//                         values at once: two pixels are joined iff they are 4-neighbours holding the same non-zero value.  A component's
//                         identity is the smallest raster index p = i0 * A1 + i1 among its pixels (the order scipy numbers features in).  Per
//                         label value v the component with the smallest key (min i1 over the component, identity) is kept, every other pixel
//                         of value v becomes 0; the slice's component count per value goes to counts[256].
//
// Form: a union-find forest with one 16-bit parent per pixel, in LDS.  Run-based labelling would not be smaller in the worst case (a slice
// whose neighbouring pixels all differ has one run per pixel), so the per-pixel form with its simpler indexing was chosen.
// LDS bound: 65 536 pixels x 2 B = 128 KiB of parents + 256 x 4 B best keys + 256 x 4 B counts + one flag word = 133 124 B of the 160 KiB a
// workgroup may declare; that is why a slice is limited to A0 * A1 <= 65 536 (hv_depedicle refuses larger ones).
//   * parent[x] <= x always, and every value ever stored in parent[x] is an ancestor of x from then on (trees only merge), so a stale read is
//     still a valid step towards the root.  Every pixel starts as its own root (background too: it is never linked, so there is no
//     "background" sentinel and raster index 65 535 is an ordinary root).  The root of a finished tree is its smallest pixel.
//   * The label values cannot stay in LDS beside the parents (64 KiB more).  They are staged as bytes in the parents' storage first; each
//     thread takes its own 64 pixels (p = j * 1024 + tid) with their "same value as the left / upper neighbour" bits into registers (16 + 4
//     dwords), and only then are the parents initialised.  The slice is therefore read completely before a byte of it is written, and `out`
//     may be the input.
//   * Parents are 16-bit halves of 32-bit words and are changed only by a 32-bit LDS compare-and-swap on the containing word.
//   * The selection needs no per-component table: min over the pixels of value v of (i1, root) is the key of the component to keep, because
//     the pixel with the smallest i1 lies in the component with the smallest minimum, and equal i1 are ordered by the root.
// Termination: no barrier stands inside a data-dependent loop (the phases are separated by barriers every thread reaches), and every loop is
// bounded by the algorithm: a find walks strictly decreasing indices (< 65 536 steps); a union retries only when the larger root stopped
// being a root, after which the larger of the two new roots is strictly smaller (< 65 536 retries); a word's compare-and-swap fails only when
// one of its two halves decreased (< 2 x 65 536 failures).  Path halving keeps the walks short on spirals and combs.  A thread that exhausts
// a bound sets the slice's "not converged" flag and goes on to the next phase.
#include "hv_common.h"

#define DP_MAXPIX 65536
#define DP_THREADS 1024
#define DP_WORDS (DP_MAXPIX / DP_THREADS / 4)   // 16 dwords of 4 label bytes per thread
#define DP_BAD 1
#define DP_NOCONV 2

__device__ __forceinline__ unsigned dp_ld16(const unsigned* w32, unsigned x) {
    // the containing word, with the type the compare-and-swap uses, so that the compiler orders the two
    return (__hip_atomic_load(w32 + (x >> 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >> ((x & 1u) * 16u)) & 0xffffu;
}

// parent[idx]: expect -> val, retried while only the word's other half changed.  true: this call made the change
__device__ __forceinline__ bool dp_cas16(unsigned* w32, unsigned idx, unsigned expect, unsigned val, int tries, int& fail) {
    unsigned* w = w32 + (idx >> 1);
    const unsigned sh = (idx & 1u) * 16u;
    unsigned cur = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    for (int k = 0; k < tries; ++k) {
        if (((cur >> sh) & 0xffffu) != expect) return false;
        const unsigned prev = atomicCAS(w, cur, (cur & ~(0xffffu << sh)) | (val << sh));
        if (prev == cur) return true;
        cur = prev;
    }
    fail = 1;
    return false;
}

__device__ __forceinline__ unsigned dp_find(unsigned* w32, unsigned x, int& fail) {
    for (int k = 0; k < DP_MAXPIX; ++k) {
        const unsigned p = dp_ld16(w32, x);
        if (p == x) return x;
        const unsigned g = dp_ld16(w32, p);
        if (g != p) {   // path halving: one attempt, a lost race only leaves the path as it was
            int ignored = 0;
            dp_cas16(w32, x, p, g, 1, ignored);
        }
        x = g;
    }
    fail = 1;
    return x;
}

__device__ __forceinline__ void dp_union(unsigned* w32, unsigned a, unsigned b, int& fail) {
    for (int k = 0; k < DP_MAXPIX; ++k) {
        a = dp_find(w32, a, fail);
        b = dp_find(w32, b, fail);
        if (a == b) return;
        if (a < b) { const unsigned t = a; a = b; b = t; }
        if (dp_cas16(w32, a, a, b, 2 * DP_MAXPIX, fail)) return;   // the larger root hangs under the smaller one's tree
    }
    fail = 1;
}

template <typename T>
__device__ __forceinline__ unsigned dp_label(T v, int& bad) {
    const double d = (double)v;
    if (!(d >= 0.0 && d <= 255.0 && d == floor(d))) { bad = 1; return 0u; }   // NaN fails the first test
    return (unsigned)d;
}

template <typename T>
__global__ __launch_bounds__(DP_THREADS) void depedicle_kernel(const T* in,       long long s0, long long s1, long long s2, long long sv,
                                                               int A0, int A1, uint8_t* out, long long o0, long long o1, long long o2,
                                                               long long ov, int* __restrict__ counts, int* __restrict__ status) {
    __shared__ unsigned s_par[DP_MAXPIX / 2];
    __shared__ unsigned s_best[256];
    __shared__ int s_ncomp[256];
    __shared__ int s_flags;
    const int tid = threadIdx.x, z = blockIdx.x, v = blockIdx.y, HW = A0 * A1;
    uint8_t* stage = reinterpret_cast<uint8_t*>(s_par);
    if (tid < 256) { s_best[tid] = 0xffffffffu; s_ncomp[tid] = 0; }
    if (tid == 0) s_flags = 0;
    int bad = 0, fail = 0;
    {   // the whole slice, as bytes, into LDS
        const T* src = in + (long long)v * sv + (long long)z * s2;
        for (int p = tid; p < HW; p += DP_THREADS) {
            const int i0 = p / A1, i1 = p - i0 * A1;
            stage[p] = (uint8_t)dp_label(src[(long long)i0 * s0 + (long long)i1 * s1], bad);
        }
    }
    __syncthreads();
    unsigned val[DP_WORDS], eq[DP_WORDS / 4] = {0u, 0u, 0u, 0u};   // 4 values per dword; per pixel 2 bits: 1 = joins p - 1, 2 = joins p - A1
#pragma unroll
    for (int w = 0; w < DP_WORDS; ++w) {
        unsigned vw = 0u, ew = 0u;
        if (w * 4 * DP_THREADS < HW) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int p = (w * 4 + k) * DP_THREADS + tid;
                if (p < HW) {
                    const int i0 = p / A1, i1 = p - i0 * A1;
                    const unsigned c = stage[p];
                    unsigned e = 0u;
                    if (c) {
                        if (i1 > 0 && stage[p - 1] == c) e |= 1u;
                        if (i0 > 0 && stage[p - A1] == c) e |= 2u;
                    }
                    vw |= c << (8 * k);
                    ew |= e << (2 * k);
                }
            }
        }
        val[w] = vw;
        eq[w >> 2] |= ew << ((w & 3) * 8);
    }
    __syncthreads();   // every staged byte has been read: the storage becomes the parents
    for (int i = tid; i < (HW + 1) / 2; i += DP_THREADS) s_par[i] = (unsigned)(2 * i) | ((unsigned)(2 * i + 1) << 16);
    __syncthreads();
#pragma unroll
    for (int w = 0; w < DP_WORDS; ++w) {
        const unsigned ew = (eq[w >> 2] >> ((w & 3) * 8)) & 0xffu;
        if (ew) {
#pragma unroll 1
            for (int k = 0; k < 4; ++k) {
                const unsigned e = (ew >> (2 * k)) & 3u, p = (unsigned)((w * 4 + k) * DP_THREADS + tid);
                if (e & 1u) dp_union(s_par, p, p - 1u, fail);
                if (e & 2u) dp_union(s_par, p, p - (unsigned)A1, fail);
            }
        }
    }
    __syncthreads();   // the forest is final: a find now returns the component's smallest pixel
#pragma unroll
    for (int w = 0; w < DP_WORDS; ++w) {
        if (val[w]) {
#pragma unroll 1
            for (int k = 0; k < 4; ++k) {
                const unsigned c = (val[w] >> (8 * k)) & 0xffu;
                if (!c) continue;
                const unsigned p = (unsigned)((w * 4 + k) * DP_THREADS + tid);
                const unsigned i1 = p % (unsigned)A1;
                const unsigned r = dp_find(s_par, p, fail);
                const unsigned key = (i1 << 16) | r;
                if (key <= __hip_atomic_load(&s_best[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) atomicMin(&s_best[c], key);
                if (r == p) atomicAdd(&s_ncomp[c], 1);
            }
        }
    }
    if (bad | fail) atomicOr(&s_flags, (bad ? DP_BAD : 0) | (fail ? DP_NOCONV : 0));
    __syncthreads();
    const int flags = s_flags;
    if (out) {
        uint8_t* dst = out + (long long)v * ov + (long long)z * o2;
#pragma unroll
        for (int w = 0; w < DP_WORDS; ++w) {
            if (w * 4 * DP_THREADS < HW) {
#pragma unroll 1
                for (int k = 0; k < 4; ++k) {
                    const int p = (w * 4 + k) * DP_THREADS + tid;
                    if (p >= HW) break;
                    unsigned c = (val[w] >> (8 * k)) & 0xffu;
                    if (c && (s_best[c] & 0xffffu) != dp_find(s_par, (unsigned)p, fail)) c = 0u;
                    const int i0 = p / A1, i1 = p - i0 * A1;
                    dst[(long long)i0 * o0 + (long long)i1 * o1] = (uint8_t)c;
                }
            }
        }
    }
    if (counts && tid < 256) counts[((long long)v * gridDim.x + z) * 256 + tid] = (tid == 0 && (flags & DP_NOCONV)) ? -1 : s_ncomp[tid];
    if (tid == 0 && flags) atomicOr(status + v, flags);
}

extern "C" int hv_depedicle(const void* label, int label_dtype, long long ls0, long long ls1, long long ls2, long long lsv, int A0, int A1, int Z,
                            int V, uint8_t* out, long long os0, long long os1, long long os2, long long osv, int* counts, int* status,
                            void* stream) {
    if (!label || !status || (!out && !counts) || A0 <= 0 || A1 <= 0 || Z <= 0 || V <= 0 || label_dtype < HV_DT_U8 || label_dtype > HV_DT_F64)
        return HV_ERR_ARG;
    if ((long long)A0 * A1 > DP_MAXPIX || V > 65535) return HV_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, (size_t)V * sizeof(int), s) != hipSuccess) return -1000 - (int)hipGetLastError();
#define DP_RUN(T) hipLaunchKernelGGL(depedicle_kernel<T>, dim3(Z, V), dim3(DP_THREADS), 0, s, (const T*)label, ls0, ls1, ls2, lsv, A0, A1, out, os0, \
                                     os1, os2, osv, counts, status)
    switch (label_dtype) {
        case HV_DT_U8: DP_RUN(uint8_t); break;
        case HV_DT_I16: DP_RUN(int16_t); break;
        case HV_DT_I32: DP_RUN(int32_t); break;
        case HV_DT_I64: DP_RUN(long long); break;
        case HV_DT_F32: DP_RUN(float); break;
        default: DP_RUN(double); break;
    }
#undef DP_RUN
    HV_LAUNCH_CHECK();
    return HV_OK;
}
