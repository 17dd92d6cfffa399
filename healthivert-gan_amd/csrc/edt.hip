// Exact Euclidean distance transform of a 3-D volume (hv_edt) and the surface-distance metrics built on it (hv_surface_distance:
// Hausdorff distance, its 95th percentile, average symmetric surface distance).
//
// hv_edt: T = {vol == value}; out(p) = min over q in T of sqrt((s0 d0)^2 + (s1 d1)^2 + (s2 d2)^2), scipy.ndimage.distance_transform_edt(vol !=
// value, sampling=spacing).  The transform is separable over SQUARED distances, one pass per axis in the order 0, 1, 2, so that the sum is formed
// as ((s0 d0)^2 + (s1 d1)^2) + (s2 d2)^2:
//   edt_axis0_kernel   one lane per line along axis 0 (consecutive lanes = consecutive k): a forward and a backward scan find the nearest member
//                      of T along the line; the squared 1-D distance (or "none") is written.
//   edt_axis1_kernel   out(j) = min_j' g(j') + (s1 (j - j'))^2 along axis 1: a workgroup stages the tile [n1][KT <= ED_KT columns] in LDS (rows
//                      of consecutive k, loaded and stored as such), one lane per element; lanes of a wave are consecutive tile elements, so the
//                      reads of step d (element +- d * KT) are consecutive LDS words: no bank conflict.
//   edt_axis2_kernel   the same along the unit-stride axis: a workgroup stages up to ED_LINES whole lines, one lane per element (lanes consecutive
//                      along the line: the reads of step d are consecutive words again), then one square root per voxel.
// The line minimum is the plain min-plus scan outwards from the voxel, d = 1, 2, ...: it stops once (s d)^2 reaches the best value so far (no
// candidate further out can win), needs no stack and no loop whose length depends on another lane.  Rounding is monotonic, so the minimum over a
// line of fl(g + c) is fl(min g + c): the three passes give bit for bit the minimum over all of T of the sum formed in the order above.
// Squared distances are integers at unit spacing -- int32 in the workspace while A0^2 + A1^2 + A2^2 < 2^31, int64 in the output's own 8-byte slots
// beyond -- and doubles (in the output's slots) for any other spacing.  No floating-point atomics, no scratch, element offsets are 64-bit.
//
// hv_surface_distance: sd_stats_kernel (surface masks, per-slice counts and bounding box) -> sd_fold_kernel (one lane: totals, list offsets, the
// box) -> the three EDT passes for each surface mask inside the box -> sd_gather_kernel twice (the directed distances into compact lists, per-slice
// sums and maxima) -> sd_final_kernel (one lane folds the slices in ascending order; the workgroup finds the two order statistics of the 95th
// percentile by an 8 x 8-bit radix select on the doubles' bit patterns, integer LDS atomics only).  Every floating-point sum has a fixed order.
#include <climits>
#include <cmath>
#include "volume_access.h"                  // hv_up16

#define ED_KT 32                      // columns (unit-stride neighbours) per tile of the axis-1 pass
#define ED_LINES 32                   // lines per workgroup of the axis-2 pass
#define ED_THREADS 256
#define ED_LDS_BYTES 65536            // staging per workgroup
#define ED_BITS 100                   // EdSrc.dt: a uint8 volume of flag bits, T = {vol & bit}

struct EdSrc { const void* p; int dt; long long s0, s1, s2; double value; int bit; };
struct EdBox { int lo[3], n[3]; };
struct EdGeo { int A1, A2; EdBox box; const int* dbox; };      // dbox (device, {lo0, lo1, lo2, n0, n1, n2}) replaces box when given

__device__ __forceinline__ bool ed_in(const EdSrc& S, long long o) {
    switch (S.dt) {
        case ED_BITS: return (((const uint8_t*)S.p)[o] & S.bit) != 0;
        case HV_DT_U8: return (double)((const uint8_t*)S.p)[o] == S.value;
        case HV_DT_F32: return (double)((const float*)S.p)[o] == S.value;
        default: return ((const double*)S.p)[o] == S.value;
    }
}

__device__ __forceinline__ EdBox ed_box(const EdGeo& G) {
    if (!G.dbox) return G.box;
    EdBox B;
#pragma unroll
    for (int a = 0; a < 3; ++a) { B.lo[a] = G.dbox[a]; B.n[a] = G.dbox[3 + a]; }
    return B;
}

// how a squared distance is carried: NONE = no member of T seen yet
template <typename T> struct EdT;
template <> struct EdT<int> {
    static __device__ __forceinline__ int none() { return INT_MAX; }
    static __device__ __forceinline__ int sq(int d, double) { return d * d; }
    static __device__ __forceinline__ double root(int v) { return sqrt((double)v); }
};
template <> struct EdT<long long> {
    static __device__ __forceinline__ long long none() { return LLONG_MAX; }
    static __device__ __forceinline__ long long sq(int d, double) { return (long long)d * d; }
    static __device__ __forceinline__ double root(long long v) { return sqrt((double)v); }
};
template <> struct EdT<double> {
    static __device__ __forceinline__ double none() { return INFINITY; }
    static __device__ __forceinline__ double sq(int d, double s) { const double t = s * (double)d; return t * t; }
    static __device__ __forceinline__ double root(double v) { return sqrt(v); }
};

// min over j of g(j) + (s (i - j))^2 for a line of n values, get(j) = g(j)
template <typename T, typename F>
__device__ __forceinline__ T ed_line_min(F get, const int i, const int n, const double s) {
    T best = get(i);
    const int far = max(i, n - 1 - i);
    for (int d = 1; d <= far; ++d) {
        const T q = EdT<T>::sq(d, s);
        if (!(q < best)) break;                   // every candidate from here on is at least q
        if (i - d >= 0) {
            const T v = get(i - d);
            if (v < best) {                       // (v is finite here: the sum cannot overflow)
                const T c = v + q;
                if (c < best) best = c;
            }
        }
        if (i + d < n) {
            const T v = get(i + d);
            if (v < best) {
                const T c = v + q;
                if (c < best) best = c;
            }
        }
    }
    return best;
}

template <typename T>
__global__ __launch_bounds__(ED_THREADS) void edt_axis0_kernel(EdSrc S, EdGeo G, T* __restrict__ g, double s, int* __restrict__ status) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *status = 0;
    const EdBox B = ed_box(G);
    const long long nl = (long long)B.n[1] * B.n[2];
    const long long L = (long long)blockIdx.x * ED_THREADS + threadIdx.x;
    if (L >= nl) return;
    const int j = B.lo[1] + (int)(L / B.n[2]), k = B.lo[2] + (int)(L % B.n[2]);
    const long long step = (long long)G.A1 * G.A2;
    T* line = g + (((long long)B.lo[0] * G.A1 + j) * G.A2 + k);
    const long long sb = B.lo[0] * S.s0 + j * S.s1 + k * S.s2;
    const int n = B.n[0];
    int last = -1;
    for (int i = 0; i < n; ++i) {                 // forwards: the distance back to the last member, as a count
        if (ed_in(S, sb + i * S.s0)) last = i;
        line[i * step] = last < 0 ? EdT<T>::none() : (T)(i - last);
    }
    int next = -1;
    for (int i = n - 1; i >= 0; --i) {            // backwards: the nearer of the two, squared
        const T f = line[i * step];
        const bool nof = f == EdT<T>::none();
        int d = nof ? -1 : (int)f;
        if (d == 0) next = i;
        if (next >= 0 && (nof || next - i < d)) d = next - i;
        line[i * step] = d < 0 ? EdT<T>::none() : EdT<T>::sq(d, s);
    }
}

template <typename T>
__global__ __launch_bounds__(ED_THREADS) void edt_axis1_kernel(EdGeo G, T* g, double s, int KT) {
    extern __shared__ double ed_lds[];
    T* tile = (T*)ed_lds;
    const EdBox B = ed_box(G);
    const int tiles = (B.n[2] + KT - 1) / KT;
    if ((long long)blockIdx.x >= (long long)B.n[0] * tiles) return;
    const int i = B.lo[0] + (int)(blockIdx.x / tiles), k0 = (int)(blockIdx.x % tiles) * KT;
    const int kw = min(KT, B.n[2] - k0), n = B.n[1];
    T* base = g + (((long long)i * G.A1 + B.lo[1]) * G.A2 + B.lo[2] + k0);
    for (int e = threadIdx.x; e < n * KT; e += ED_THREADS) {
        const int j = e / KT, c = e % KT;
        if (c < kw) tile[e] = base[(long long)j * G.A2 + c];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n * KT; e += ED_THREADS) {
        const int j = e / KT, c = e % KT;
        if (c < kw) base[(long long)j * G.A2 + c] = ed_line_min<T>([&](int q) { return tile[q * KT + c]; }, j, n, s);
    }
}

template <typename T>
__global__ __launch_bounds__(ED_THREADS) void edt_axis2_kernel(EdGeo G, const T* g, double* out, double s, int LN, int* __restrict__ status) {
    extern __shared__ double ed_lds[];
    T* tile = (T*)ed_lds;
    const EdBox B = ed_box(G);
    const long long nl = (long long)B.n[0] * B.n[1], line0 = (long long)blockIdx.x * LN;
    if (line0 >= nl) return;
    const int cnt = (int)min((long long)LN, nl - line0), n = B.n[2];
    auto at = [&](int l) -> long long {
        const long long L = line0 + l;
        return (((long long)(B.lo[0] + (int)(L / B.n[1])) * G.A1 + B.lo[1] + (int)(L % B.n[1])) * G.A2 + B.lo[2]);
    };
    for (int e = threadIdx.x; e < cnt * n; e += ED_THREADS) {
        const int l = e / n, k = e % n;
        tile[e] = g[at(l) + k];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < cnt * n; e += ED_THREADS) {
        const int l = e / n, k = e % n;
        const T* row = tile + l * n;
        const T v = ed_line_min<T>([&](int q) { return row[q]; }, k, n, s);
        const bool nof = v == EdT<T>::none();
        out[at(l) + k] = nof ? (double)INFINITY : EdT<T>::root(v);
        if (nof) *status = 1;                     // T is empty (every voxel says so; the same value from every lane)
    }
}

static inline bool ed_dims_ok(int A0, int A1, int A2) { return A0 > 0 && A1 > 0 && A2 > 0; }
static inline bool ed_spacing_ok(const double* sp) {
    if (!sp) return false;
    for (int a = 0; a < 3; ++a)
        if (!(std::isfinite(sp[a]) && sp[a] > 0.0)) return false;
    return true;
}
enum { ED_I32 = 0, ED_I64 = 1, ED_F64 = 2 };
static inline int ed_carrier(int A0, int A1, int A2, const double* sp) {
    if (sp[0] != 1.0 || sp[1] != 1.0 || sp[2] != 1.0) return ED_F64;
    const long long q = (long long)A0 * A0 + (long long)A1 * A1 + (long long)A2 * A2;
    return q < (long long)INT_MAX ? ED_I32 : ED_I64;
}
// HV_OK, or HV_ERR_UNSUPPORTED where a line does not fit the staging or a grid does not fit an int
static int ed_supported(int A0, int A1, int A2, int carrier) {
    const long long esz = carrier == ED_I32 ? 4 : 8;
    if ((long long)A1 * esz > ED_LDS_BYTES || (long long)A2 * esz > ED_LDS_BYTES) return HV_ERR_UNSUPPORTED;
    if ((long long)A0 * A1 * A2 > (1LL << 30)) return HV_ERR_UNSUPPORTED;
    return HV_OK;
}

template <typename T>
static int ed_launch(const EdSrc& S, const EdGeo& G, const int* n /* host extents the grids are sized for */, const double* sp, T* g, double* out,
                     int* status, hipStream_t st) {
    const long long l0 = (long long)n[1] * n[2];
    hipLaunchKernelGGL(edt_axis0_kernel<T>, dim3(hv_cdiv(l0, ED_THREADS)), dim3(ED_THREADS), 0, st, S, G, g, sp[0], status);
    HV_LAUNCH_CHECK();
    int KT = ED_KT;
    while (KT > 1 && ((long long)n[1] * KT * (long long)sizeof(T) > ED_LDS_BYTES || KT / 2 >= n[2])) KT /= 2;
    hipLaunchKernelGGL(edt_axis1_kernel<T>, dim3((unsigned)((long long)n[0] * hv_cdiv(n[2], KT))), dim3(ED_THREADS), (size_t)n[1] * KT * sizeof(T), st,
                       G, g, sp[1], KT);
    HV_LAUNCH_CHECK();
    int LN = ED_LINES;
    while (LN > 1 && (long long)n[2] * LN * (long long)sizeof(T) > ED_LDS_BYTES) LN /= 2;
    hipLaunchKernelGGL(edt_axis2_kernel<T>, dim3(hv_cdiv((long long)n[0] * n[1], LN)), dim3(ED_THREADS), (size_t)n[2] * LN * sizeof(T), st, G,
                       (const T*)g, out, sp[2], LN, status);
    HV_LAUNCH_CHECK();
    return HV_OK;
}

// the three passes; `n`: the extents the grids cover (the box's, or the whole volume's when the box is only known on the device)
static int ed_run(const EdSrc& S, const EdGeo& G, const int* n, int carrier, const double* sp, double* out, int* status, void* ws32, hipStream_t st) {
    switch (carrier) {
        case ED_I32: return ed_launch<int>(S, G, n, sp, (int*)ws32, out, status, st);
        case ED_I64: return ed_launch<long long>(S, G, n, sp, (long long*)out, out, status, st);
        default: return ed_launch<double>(S, G, n, sp, out, out, status, st);
    }
}

extern "C" size_t hv_edt_workspace_bytes(int A0, int A1, int A2) {
    if (!ed_dims_ok(A0, A1, A2)) return 0;
    return hv_up16((size_t)A0 * A1 * A2 * 4);
}

extern "C" int hv_edt(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, double value,
                      const double* spacing, const int* box, double* out, int* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (!vol || !out || !status || !workspace || !ed_dims_ok(A0, A1, A2) || !ed_spacing_ok(spacing) ||
        (dtype != HV_DT_U8 && dtype != HV_DT_F32 && dtype != HV_DT_F64) || ((uintptr_t)out & 7) || ((uintptr_t)workspace & 15) ||
        ((uintptr_t)status & 3) || workspace_bytes < hv_edt_workspace_bytes(A0, A1, A2))
        return HV_ERR_ARG;
    EdGeo G;
    G.A1 = A1; G.A2 = A2; G.dbox = nullptr;
    const int dims[3] = {A0, A1, A2};
    for (int a = 0; a < 3; ++a) {
        G.box.lo[a] = box ? box[a] : 0;
        G.box.n[a] = box ? box[3 + a] : dims[a];
        if (G.box.lo[a] < 0 || G.box.n[a] < 1 || G.box.n[a] > dims[a] - G.box.lo[a]) return HV_ERR_ARG;
    }
    const int carrier = ed_carrier(A0, A1, A2, spacing);
    const int rc = ed_supported(A0, A1, A2, carrier);
    if (rc != HV_OK) return rc;
    EdSrc S;
    S.p = vol; S.dt = dtype; S.s0 = s0; S.s1 = s1; S.s2 = s2; S.value = value; S.bit = 0;
    return ed_run(S, G, G.box.n, carrier, spacing, out, status, workspace, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------ surface distances
#define SD_REC 8                      // ints per slice: { n_a, n_b, jmin, jmax, kmin, kmax, any, - }

struct SdWs {                         // byte offsets into the workspace, each a multiple of 16
    size_t da, db, list, ws32, mask, rec, off, psum, pmax, small, total;
};
static SdWs sd_layout(int A0, int A1, int A2) {
    const size_t N = (size_t)A0 * A1 * A2;
    SdWs W;
    size_t o = 0;
    W.da = o; o += hv_up16(N * 8);
    W.db = o; o += hv_up16(N * 8);
    W.list = o; o += hv_up16(N * 8);
    W.ws32 = o; o += hv_up16(N * 4);
    W.mask = o; o += hv_up16(N);
    W.rec = o; o += hv_up16((size_t)A0 * SD_REC * 4);
    W.off = o; o += hv_up16((size_t)A0 * 2 * 4);
    W.psum = o; o += hv_up16((size_t)A0 * 2 * 8);
    W.pmax = o; o += hv_up16((size_t)A0 * 2 * 8);
    W.small = o; o += 64;             // box[6], totals[2], EDT status[2]
    W.total = o;
    return W;
}

// One workgroup per slice i: the surface flags (bit 0: S_A, bit 1: S_B) of its voxels, the two surface counts and the slice's part of the
// bounding box of A | B.  A voxel of a set is a surface voxel if one of its six face neighbours is outside the set or outside the volume.
__global__ __launch_bounds__(ED_THREADS) void sd_stats_kernel(EdSrc SA, EdSrc SB, int A0, int A1, int A2, uint8_t* __restrict__ mask,
                                                              int* __restrict__ rec) {
    __shared__ int sh[SD_REC];
    const int i = blockIdx.x;
    if (threadIdx.x < SD_REC) sh[threadIdx.x] = threadIdx.x == 2 || threadIdx.x == 4 ? INT_MAX : (threadIdx.x == 3 || threadIdx.x == 5 ? -1 : 0);
    __syncthreads();
    auto surf = [&](const EdSrc& S, int j, int k) -> bool {
        auto in = [&](int a, int b, int c) -> bool {
            return a >= 0 && a < A0 && b >= 0 && b < A1 && c >= 0 && c < A2 && ed_in(S, a * S.s0 + b * S.s1 + c * S.s2);
        };
        return !(in(i - 1, j, k) && in(i + 1, j, k) && in(i, j - 1, k) && in(i, j + 1, k) && in(i, j, k - 1) && in(i, j, k + 1));
    };
    int na = 0, nb = 0, jmin = INT_MAX, jmax = -1, kmin = INT_MAX, kmax = -1;
    const int plane = A1 * A2;
    for (int e = threadIdx.x; e < plane; e += ED_THREADS) {
        const int j = e / A2, k = e % A2;
        const bool a = ed_in(SA, i * SA.s0 + j * SA.s1 + k * SA.s2), b = ed_in(SB, i * SB.s0 + j * SB.s1 + k * SB.s2);
        const int fa = a && surf(SA, j, k), fb = b && surf(SB, j, k);
        mask[(long long)i * plane + e] = (uint8_t)(fa | (fb << 1));
        na += fa; nb += fb;
        if (a || b) { jmin = min(jmin, j); jmax = max(jmax, j); kmin = min(kmin, k); kmax = max(kmax, k); }
    }
    if (na) atomicAdd(&sh[0], na);
    if (nb) atomicAdd(&sh[1], nb);
    if (jmax >= 0) { atomicMin(&sh[2], jmin); atomicMax(&sh[3], jmax); atomicMin(&sh[4], kmin); atomicMax(&sh[5], kmax); atomicOr(&sh[6], 1); }
    __syncthreads();
    if (threadIdx.x < SD_REC) rec[i * SD_REC + threadIdx.x] = sh[threadIdx.x];
}

// one lane: the totals, where each slice's part of the two lists starts, the box the transforms are restricted to
__global__ void sd_fold_kernel(const int* __restrict__ rec, int A0, int A1, int A2, int restricted, int* __restrict__ off, int* __restrict__ small) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int na = 0, nb = 0, imin = INT_MAX, imax = -1, jmin = INT_MAX, jmax = -1, kmin = INT_MAX, kmax = -1;
    for (int i = 0; i < A0; ++i) {
        const int* r = rec + i * SD_REC;
        off[2 * i] = na; off[2 * i + 1] = nb;
        na += r[0]; nb += r[1];
        if (r[6]) {
            imin = min(imin, i); imax = i;
            jmin = min(jmin, r[2]); jmax = max(jmax, r[3]); kmin = min(kmin, r[4]); kmax = max(kmax, r[5]);
        }
    }
    if (!restricted) { imin = jmin = kmin = 0; imax = A0 - 1; jmax = A1 - 1; kmax = A2 - 1; }
    const bool none = imax < 0;
    small[0] = none ? 0 : imin; small[1] = none ? 0 : jmin; small[2] = none ? 0 : kmin;
    small[3] = none ? 0 : imax - imin + 1; small[4] = none ? 0 : jmax - jmin + 1; small[5] = none ? 0 : kmax - kmin + 1;
    small[6] = na; small[7] = nb;
}

// One workgroup per slice: the distances D(p) of the slice's voxels with flag `bit` go to list[off + .] (any order inside the slice: only
// order-free quantities are taken from the list), their sum -- each lane its own voxels in ascending order, then a fixed tree -- and maximum
// to psum / pmax.  The whole plane is walked whatever the box is, so the sums do not depend on it.
__global__ __launch_bounds__(ED_THREADS) void sd_gather_kernel(const uint8_t* __restrict__ mask, int bit, const double* __restrict__ D, int plane,
                                                               const int* __restrict__ off, int dir, double* __restrict__ list,
                                                               double* __restrict__ psum, double* __restrict__ pmax) {
    __shared__ int cnt;
    __shared__ double ssum[ED_THREADS], smax[ED_THREADS];
    const int i = blockIdx.x;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    const long long base = (long long)i * plane;
    double* dst = list + off[2 * i + dir];
    double sum = 0.0, mx = 0.0;
    for (int e = threadIdx.x; e < plane; e += ED_THREADS)
        if (mask[base + e] & bit) {
            const double d = D[base + e];
            sum += d;
            mx = fmax(mx, d);
            dst[atomicAdd(&cnt, 1)] = d;
        }
    ssum[threadIdx.x] = sum; smax[threadIdx.x] = mx;
    __syncthreads();
    for (int h = ED_THREADS / 2; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) {
            ssum[threadIdx.x] += ssum[threadIdx.x + h];
            smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + h]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { psum[2 * i + dir] = ssum[0]; pmax[2 * i + dir] = smax[0]; }
}

#define SD_FINAL_THREADS 1024
// The 16 doubles.  Lane 0 folds the slices in ascending order; the workgroup then selects the order statistics klo = floor((n - 1) 0.95) and
// klo + 1 of the joined list: the distances are non-negative doubles, whose bit patterns order as unsigned integers.
__global__ __launch_bounds__(SD_FINAL_THREADS) void sd_final_kernel(const double* __restrict__ l_ab, const double* __restrict__ l_ba,
                                                                    const int* __restrict__ small, const double* __restrict__ psum,
                                                                    const double* __restrict__ pmax, int A0, double* __restrict__ out) {
    __shared__ unsigned hist[256];
    __shared__ unsigned long long s_prefix, s_min;
    __shared__ long long s_k;
    __shared__ unsigned s_eq;
    const int na = small[6], nb = small[7];
    const long long n = (long long)na + nb;
    const int tid = threadIdx.x;
    if (na == 0 || nb == 0) {
        if (tid == 0) {
            out[0] = (double)na; out[1] = (double)nb;
            for (int q = 2; q < 9; ++q) out[q] = NAN;
            out[9] = na == 0 ? 1.0 : 0.0; out[10] = nb == 0 ? 1.0 : 0.0;
            for (int q = 11; q < 16; ++q) out[q] = 0.0;
        }
        return;
    }
    if (tid == 0) {
        double sab = 0.0, sba = 0.0, mab = 0.0, mba = 0.0;
        for (int i = 0; i < A0; ++i) {
            sab += psum[2 * i]; sba += psum[2 * i + 1];
            mab = fmax(mab, pmax[2 * i]); mba = fmax(mba, pmax[2 * i + 1]);
        }
        const double aab = sab / (double)na, aba = sba / (double)nb;
        out[0] = (double)na; out[1] = (double)nb; out[2] = mab; out[3] = mba; out[4] = aab; out[5] = aba;
        out[6] = fmax(mab, mba);
        out[8] = (aab + aba) / 2.0;
        out[9] = 0.0; out[10] = 0.0;
        for (int q = 11; q < 16; ++q) out[q] = 0.0;
        s_prefix = 0ULL; s_min = ~0ULL;
    }
    const double vidx = (double)(n - 1) * 0.95;
    const long long klo = (long long)floor(vidx);
    const double t = vidx - (double)klo;
    auto key = [&](long long e) -> unsigned long long { return (unsigned long long)__double_as_longlong(e < na ? l_ab[e] : l_ba[e - na]); };
    unsigned long long prefix = 0ULL;
    long long k = klo;
    for (int pass = 7; pass >= 0; --pass) {
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        for (long long e = tid; e < n; e += SD_FINAL_THREADS) {
            const unsigned long long u = key(e);
            if (pass == 7 || (u >> (8 * (pass + 1))) == (prefix >> (8 * (pass + 1)))) atomicAdd(&hist[(unsigned)(u >> (8 * pass)) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            long long cum = 0;
            for (int d = 0; d < 256; ++d) {
                if (cum + (long long)hist[d] > k) {
                    s_prefix = prefix | ((unsigned long long)d << (8 * pass));
                    s_k = k - cum;
                    s_eq = hist[d];
                    break;
                }
                cum += hist[d];
            }
        }
        __syncthreads();
        prefix = s_prefix; k = s_k;
    }
    // prefix: the value of rank klo; k: its rank among the s_eq elements equal to it
    const bool same = klo + 1 > n - 1 || k + 1 < (long long)s_eq;
    if (!same) {
        for (long long e = tid; e < n; e += SD_FINAL_THREADS) {
            const unsigned long long u = key(e);
            if (u > prefix) atomicMin(&s_min, u);
        }
    }
    __syncthreads();
    if (tid == 0) {
        const double lo = __longlong_as_double((long long)prefix), hi = same ? lo : __longlong_as_double((long long)s_min);
        const double diff = hi - lo;
        out[7] = t < 0.5 ? lo + diff * t : hi - diff * (1.0 - t);
    }
}

extern "C" size_t hv_surface_distance_workspace_bytes(int A0, int A1, int A2) {
    if (!ed_dims_ok(A0, A1, A2)) return 0;
    return sd_layout(A0, A1, A2).total;
}

extern "C" int hv_surface_distance(const void* a, const void* b, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2,
                                   double value, const double* spacing, int restricted, double* out, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    if (!a || !b || !out || !workspace || !ed_dims_ok(A0, A1, A2) || !ed_spacing_ok(spacing) ||
        (dtype != HV_DT_U8 && dtype != HV_DT_F32 && dtype != HV_DT_F64) || ((uintptr_t)out & 7) || ((uintptr_t)workspace & 15) ||
        (restricted != 0 && restricted != 1) || workspace_bytes < hv_surface_distance_workspace_bytes(A0, A1, A2))
        return HV_ERR_ARG;
    const int carrier = ed_carrier(A0, A1, A2, spacing);
    const int rc = ed_supported(A0, A1, A2, carrier);
    if (rc != HV_OK) return rc;
    if ((long long)A1 * A2 > INT_MAX) return HV_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const SdWs W = sd_layout(A0, A1, A2);
    char* ws = (char*)workspace;
    double *DA = (double*)(ws + W.da), *DB = (double*)(ws + W.db), *list_ab = (double*)(ws + W.list), *list_ba = DB;
    uint8_t* mask = (uint8_t*)(ws + W.mask);
    int *rec = (int*)(ws + W.rec), *off = (int*)(ws + W.off), *small = (int*)(ws + W.small);
    double *psum = (double*)(ws + W.psum), *pmax = (double*)(ws + W.pmax);
    EdSrc SA, SB;
    SA.p = a; SA.dt = dtype; SA.s0 = s0; SA.s1 = s1; SA.s2 = s2; SA.value = value; SA.bit = 0;
    SB = SA; SB.p = b;
    hipLaunchKernelGGL(sd_stats_kernel, dim3(A0), dim3(ED_THREADS), 0, st, SA, SB, A0, A1, A2, mask, rec);
    HV_LAUNCH_CHECK();
    hipLaunchKernelGGL(sd_fold_kernel, dim3(1), dim3(64), 0, st, rec, A0, A1, A2, restricted, off, small);
    HV_LAUNCH_CHECK();
    EdGeo G;
    G.A1 = A1; G.A2 = A2; G.dbox = small;
    const int dims[3] = {A0, A1, A2};
    for (int q = 0; q < 3; ++q) { G.box.lo[q] = 0; G.box.n[q] = dims[q]; }
    EdSrc SM;
    SM.p = mask; SM.dt = ED_BITS; SM.s0 = (long long)A1 * A2; SM.s1 = A2; SM.s2 = 1; SM.value = 0.0;
    const int plane = A1 * A2;
    for (int dir = 0; dir < 2; ++dir) {           // dir 0: the transform of S_A, dir 1: of S_B
        SM.bit = 1 << dir;
        const int e = ed_run(SM, G, dims, carrier, spacing, dir ? DB : DA, small + 8 + dir, ws + W.ws32, st);
        if (e != HV_OK) return e;
    }
    // d(p, S_B) for p in S_A reads DB; the other list then overwrites DB, which nothing reads any more
    hipLaunchKernelGGL(sd_gather_kernel, dim3(A0), dim3(ED_THREADS), 0, st, mask, 1, DB, plane, off, 0, list_ab, psum, pmax);
    HV_LAUNCH_CHECK();
    hipLaunchKernelGGL(sd_gather_kernel, dim3(A0), dim3(ED_THREADS), 0, st, mask, 2, DA, plane, off, 1, list_ba, psum, pmax);
    HV_LAUNCH_CHECK();
    hipLaunchKernelGGL(sd_final_kernel, dim3(1), dim3(SD_FINAL_THREADS), 0, st, list_ab, list_ba, small, psum, pmax, A0, out);
    HV_LAUNCH_CHECK();
    return HV_OK;
}
