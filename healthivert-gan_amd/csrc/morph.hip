// 3-D binary morphology of a volume on the device: hv_morph_ball (dilation, erosion, opening, closing by a ball given
// in the spacing's units), hv_morph_struct (the same with generate_binary_structure(3, c), iterated) and hv_morph_merge (a mask written back into
// a label volume).  The definitions are scipy.ndimage.binary_dilation / binary_erosion / binary_opening / binary_closing; every result is a byte
// mask of 0 / 1, bit for bit scipy's.
//
// Foreground X = {vol == value} (HV_CCL_EQ) or {vol != value} (HV_CCL_NE).  The ball is the set of integer offsets o with
//     ((s0 o0)^2 + (s1 o1)^2) + (s2 o2)^2 <= radius * radius            (float64, in exactly this order: hv_edt's ordered sum)
// and a voxel p is in the dilation iff a member q of X has p - q in the ball; with border_value 1 the voxels outside the volume are members too.
// Erosion is the dual: erode(X, b) = 1 - dilate(1 - X, 1 - b) (the ball is symmetric), so ONE pipeline serves both, with the predicate and the
// output inverted.  The nearest outside voxel lies along one axis, min(i + 1, n - i) steps away: it enters each pass as a virtual member at index
// -1 and n of the line.  Opening = erosion then dilation, closing = dilation then erosion, both with the same border_value; the intermediate mask
// is a byte volume in the workspace that the second half reads with unit stride.
//
// A dilation needs no distances, only "is the ordered sum <= r^2", and the sum is non-decreasing in each |o_a| (rounding is monotonic).  So the
// three passes carry small integers, never a distance, and every scan is bounded by R_a = the largest step count d with (s_a d)^2 <= r^2:
//   morph_axis0_kernel   one lane per line along axis 0 (consecutive lanes = consecutive k).  c0(p) = steps to the nearest member along the
//                        line, saturated at R0 + 1 = "beyond the radius" (no member seen needs no other value): a forward and a backward scan.
//   morph_axis1_kernel   a workgroup stages the tile [A1][KT <= MO_KT columns] of counts in LDS.  v(j) = min over |j - j'| <= R1 of
//                        (s0 c0(j'))^2 + (s1 (j - j'))^2 in registers (float64; the scan also stops once (s1 d)^2 reaches the best so far);
//                        written back, in place, is the REACH e(p) = 1 + the largest d2 <= R2 with v + (s2 d2)^2 <= r^2, 0 if v > r^2.
//   morph_axis2_kernel   a workgroup stages up to MO_LINES whole lines of reaches in LDS; out(k) = 1 iff some k' has |k - k'| < e(k'),
//                        at most R2 steps outwards, stopping at the first hit; the byte (inverted for an erosion) goes out through out's strides.
// The carrier is the step count: uint8 while max(R0, R2) <= 254, uint16 up to 65 534 (wider is refused); at unit spacing the values compared are
// integers held exactly in the doubles, (double)d2 <= radius * radius.  No square root, no 8-byte volume, no atomics.
//
// hv_morph_struct: morph_stencil_kernel, one launch per iteration: a MO_T0 x MO_T1 x MO_T2 tile with a one-voxel halo is staged in LDS as bytes
// (border_value where the halo leaves the volume), each voxel takes the OR (dilation) or the AND (erosion) over the 7 / 19 / 27 cells of the
// structure.  The first launch reads the source through its strides and predicate, the last writes out through its strides, the launches between
// ping-pong between two byte volumes of the workspace.
// hv_morph_merge: morph_merge_kernel, one lane per voxel.
// No workgroup waits for another (phases are kernel boundaries), no host synchronisation, no scratch; every byte of the workspace that is read
// was written by an earlier launch of the same call: the result does not depend on what the workspace held.
#include <cmath>
#include "volume_access.h"                  // hv_up16

#define MO_THREADS 256
#define MO_KT 32                      // columns (unit-stride neighbours) per tile of the axis-1 pass
#define MO_LINES 32                   // lines per workgroup of the axis-2 pass
#define MO_LDS_BYTES 65536            // staging per workgroup, 2 bytes per staged count
#define MO_MAX_LINE (MO_LDS_BYTES / 2)
#define MO_MAX_REACH 65534            // R_a + 1 must fit the 16-bit carrier
#define MO_T0 4
#define MO_T1 8
#define MO_T2 64
#define MO_TILE (MO_T0 * MO_T1 * MO_T2)
#define MO_HALO ((MO_T0 + 2) * (MO_T1 + 2) * (MO_T2 + 2))
#define MO_MASK 101                   // MoSrc.dt: a byte mask, member = byte != 0

struct MoSrc { const void* p; int dt; long long s0, s1, s2; double value; int ne; };       // ne: the complement of the predicate
struct MoOut { uint8_t* p; long long s0, s1, s2; };
struct MoBall { int A0, A1, A2, R0, R1, R2; double s0, s1, s2, r2; int border, inv_out; };

__device__ __forceinline__ bool mo_eq(const void* p, int dt, long long o, double v) {
    switch (dt) {
        case HV_DT_U8: return (double)((const uint8_t*)p)[o] == v;
        case HV_DT_F32: return (double)((const float*)p)[o] == v;
        default: return ((const double*)p)[o] == v;
    }
}
__device__ __forceinline__ bool mo_in(const MoSrc& S, long long o) {
    const bool m = S.dt == MO_MASK ? ((const uint8_t*)S.p)[o] != 0 : mo_eq(S.p, S.dt, o, S.value);
    return m != (S.ne != 0);
}
__device__ __forceinline__ void mo_put(void* p, int dt, long long o, double v) {
    switch (dt) {
        case HV_DT_U8: ((uint8_t*)p)[o] = (uint8_t)v; break;
        case HV_DT_F32: ((float*)p)[o] = (float)v; break;
        default: ((double*)p)[o] = v; break;
    }
}
__device__ __forceinline__ void mo_copy(const void* s, long long so, void* d, long long dofs, int dt) {
    switch (dt) {
        case HV_DT_U8: ((uint8_t*)d)[dofs] = ((const uint8_t*)s)[so]; break;
        case HV_DT_F32: ((uint32_t*)d)[dofs] = ((const uint32_t*)s)[so]; break;          // bits, so that a NaN's payload survives
        default: ((unsigned long long*)d)[dofs] = ((const unsigned long long*)s)[so]; break;
    }
}
__device__ __forceinline__ double mo_sq(double s, int d) { const double t = s * (double)d; return t * t; }

// ------------------------------------------------------------------------------------------------ the ball: three bounded passes
template <typename C>
__global__ __launch_bounds__(MO_THREADS) void morph_axis0_kernel(MoSrc S, MoBall B, C* __restrict__ g) {
    const long long nl = (long long)B.A1 * B.A2;
    const long long L = (long long)blockIdx.x * MO_THREADS + threadIdx.x;
    if (L >= nl) return;
    const int j = (int)(L / B.A2), k = (int)(L % B.A2);
    const long long sb = j * S.s1 + k * S.s2;
    C* line = g + L;
    const int n = B.A0, none = B.R0 + 1;
    int c = B.border ? 1 : none;                  // the virtual member at index -1 is one step from index 0 (none >= 1)
    for (int i = 0; i < n; ++i) {                 // forwards: steps back to the last member, saturated
        if (mo_in(S, sb + i * S.s0)) c = 0;
        line[i * nl] = (C)c;
        c = min(c + 1, none);
    }
    c = B.border ? 1 : none;                      // the virtual member at index n
    for (int i = n - 1; i >= 0; --i) {            // backwards: the nearer of the two
        const int f = (int)line[i * nl];
        c = min(c, f);
        line[i * nl] = (C)c;
        c = min(c + 1, none);
    }
}

template <typename C>
__global__ __launch_bounds__(MO_THREADS) void morph_axis1_kernel(MoBall B, C* g, int KT) {
    extern __shared__ unsigned short mo_lds[];
    const int tiles = (B.A2 + KT - 1) / KT;
    const int i = (int)(blockIdx.x / tiles), k0 = (int)(blockIdx.x % tiles) * KT;
    if (i >= B.A0) return;
    const int kw = min(KT, B.A2 - k0), n = B.A1;
    C* base = g + ((long long)i * B.A1 * B.A2 + k0);
    for (int e = threadIdx.x; e < n * KT; e += MO_THREADS) {
        const int j = e / KT, c = e % KT;
        if (c < kw) mo_lds[e] = (unsigned short)base[(long long)j * B.A2 + c];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n * KT; e += MO_THREADS) {
        const int j = e / KT, c = e % KT;
        if (c >= kw) continue;
        auto a = [&](int q) -> double {           // (s0 c0)^2 of row q, +inf beyond the radius
            const int cnt = mo_lds[q * KT + c];
            return cnt > B.R0 ? (double)INFINITY : mo_sq(B.s0, cnt);
        };
        double best = a(j);
        const int far = min(B.R1, B.border ? max(j + 1, n - j) : max(j, n - 1 - j));
        for (int d = 1; d <= far; ++d) {
            const double q = mo_sq(B.s1, d);
            if (!(q < best)) break;               // every candidate from here on is at least q
            if (j - d >= 0) {
                const double v = a(j - d) + q;
                if (v < best) best = v;
            } else if (B.border && j - d == -1) {
                best = q;                         // the virtual member: 0 + q, and q < best
            }
            if (j + d < n) {
                const double v = a(j + d) + q;
                if (v < best) best = v;
            } else if (B.border && j + d == n) {
                if (q < best) best = q;
            }
        }
        int reach = 0;                            // 1 + the largest d2 <= R2 with best + (s2 d2)^2 <= r^2: the sum is non-decreasing in d2
        if (best <= B.r2) {
            int lo = 0, hi = B.R2;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (best + mo_sq(B.s2, mid) <= B.r2) lo = mid; else hi = mid - 1;
            }
            reach = lo + 1;
        }
        base[(long long)j * B.A2 + c] = (C)reach;
    }
}

template <typename C>
__global__ __launch_bounds__(MO_THREADS) void morph_axis2_kernel(MoBall B, const C* __restrict__ g, MoOut O, int LN) {
    extern __shared__ unsigned short mo_lds[];
    const long long nl = (long long)B.A0 * B.A1, line0 = (long long)blockIdx.x * LN;
    if (line0 >= nl) return;
    const int cnt = (int)min((long long)LN, nl - line0), n = B.A2;
    const C* src = g + line0 * n;                 // the staged lines are consecutive in the workspace
    for (int e = threadIdx.x; e < cnt * n; e += MO_THREADS) mo_lds[e] = (unsigned short)src[e];
    __syncthreads();
    for (int e = threadIdx.x; e < cnt * n; e += MO_THREADS) {
        const int l = e / n, k = e % n;
        const unsigned short* row = mo_lds + l * n;
        bool hit = B.border && min(k + 1, n - k) <= B.R2;
        const int far = min(B.R2, max(k, n - 1 - k));
        for (int d = 0; d <= far && !hit; ++d)
            hit = (k - d >= 0 && (int)row[k - d] > d) || (k + d < n && (int)row[k + d] > d);
        const long long Lg = line0 + l;
        O.p[(Lg / B.A1) * O.s0 + (Lg % B.A1) * O.s1 + k * O.s2] = (uint8_t)(hit != (B.inv_out != 0));
    }
}

// ------------------------------------------------------------------------------------------------ the 3 x 3 x 3 structures
__global__ __launch_bounds__(MO_THREADS) void morph_stencil_kernel(MoSrc S, MoOut O, int A0, int A1, int A2, int n1, int n2, int conn, int erode,
                                                                   int border) {
    __shared__ uint8_t t[MO_HALO];
    const int tile = blockIdx.x;
    const int i0 = (tile / (n2 * n1)) * MO_T0, j0 = ((tile / n2) % n1) * MO_T1, k0 = (tile % n2) * MO_T2;
    for (int l = threadIdx.x; l < MO_HALO; l += MO_THREADS) {
        const int i = i0 + l / ((MO_T1 + 2) * (MO_T2 + 2)) - 1, j = j0 + (l / (MO_T2 + 2)) % (MO_T1 + 2) - 1, k = k0 + l % (MO_T2 + 2) - 1;
        const bool inside = i >= 0 && i < A0 && j >= 0 && j < A1 && k >= 0 && k < A2;
        t[l] = (uint8_t)(inside ? (mo_in(S, i * S.s0 + j * S.s1 + k * S.s2) ? 1 : 0) : border);
    }
    __syncthreads();
    for (int l = threadIdx.x; l < MO_TILE; l += MO_THREADS) {
        const int a = l / (MO_T1 * MO_T2), b = (l / MO_T2) % MO_T1, c = l % MO_T2;
        const int i = i0 + a, j = j0 + b, k = k0 + c;
        if (i >= A0 || j >= A1 || k >= A2) continue;
        int any = 0, all = 1;
#pragma unroll
        for (int da = 0; da <= 2; ++da)
#pragma unroll
            for (int db = 0; db <= 2; ++db)
#pragma unroll
                for (int dc = 0; dc <= 2; ++dc) {
                    if ((da != 1) + (db != 1) + (dc != 1) > conn) continue;
                    const int v = t[((a + da) * (MO_T1 + 2) + b + db) * (MO_T2 + 2) + c + dc];
                    any |= v; all &= v;
                }
        O.p[i * O.s0 + j * O.s1 + k * O.s2] = (uint8_t)(erode ? all : any);
    }
}

// ------------------------------------------------------------------------------------------------ the merge
// grow: mask 1 and vol == background -> value; shrink: vol == value and mask 0 -> fill; every other voxel is copied (copy 0: out is vol itself)
__global__ __launch_bounds__(MO_THREADS) void morph_merge_kernel(MoSrc S, MoOut M, int A1, int A2, int N, int rule, double background, double fill,
                                                                 void* out, long long os0, long long os1, long long os2, int copy) {
    const long long gp = (long long)blockIdx.x * MO_THREADS + threadIdx.x;
    if (gp >= N) return;
    const int p = (int)gp;
    const int k = p % A2, j = (p / A2) % A1, i = p / (A2 * A1);
    const long long so = i * S.s0 + j * S.s1 + k * S.s2, oo = i * os0 + j * os1 + k * os2;
    const bool m = M.p[i * M.s0 + j * M.s1 + k * M.s2] != 0;
    if (rule == HV_MORPH_GROW ? (m && mo_eq(S.p, S.dt, so, background)) : (!m && mo_eq(S.p, S.dt, so, S.value)))
        mo_put(out, S.dt, oo, rule == HV_MORPH_GROW ? S.value : fill);
    else if (copy)
        mo_copy(S.p, so, out, oo, S.dt);
}

// ------------------------------------------------------------------------------------------------ host side
static inline bool mo_dims_ok(int A0, int A1, int A2) { return A0 > 0 && A1 > 0 && A2 > 0; }
static inline bool mo_dtype_ok(int dt) { return dt == HV_DT_U8 || dt == HV_DT_F32 || dt == HV_DT_F64; }
static inline bool mo_spacing_ok(const double* sp) {
    if (!sp) return false;
    for (int a = 0; a < 3; ++a)
        if (!(std::isfinite(sp[a]) && sp[a] > 0.0)) return false;
    return true;
}
// a radius the kernels take: finite, non-negative, and its square finite too ("no member" is +inf in the axis-1 pass)
static inline bool mo_radius_ok(double r) { return std::isfinite(r) && r >= 0.0 && std::isfinite(r * r); }
// the largest d in [0, cap] with (s d)^2 <= r2, by the expression the kernels use
static int mo_steps(double r2, double s, int cap) {
    int d = 0;
    while (d < cap) {
        const double t = s * (double)(d + 1);
        if (!(t * t <= r2)) break;
        ++d;
    }
    return d;
}
// the scan bounds (each capped by its extent: no member and no border voxel is further) and the carrier's bytes; false: beyond the 16-bit carrier
static bool mo_plan(int A0, int A1, int A2, double radius, const double* sp, int* R, int* cw) {
    const int dims[3] = {A0, A1, A2};
    const double r2 = radius * radius;
    for (int a = 0; a < 3; ++a) R[a] = mo_steps(r2, sp[a], dims[a] < MO_MAX_REACH + 1 ? dims[a] : MO_MAX_REACH + 1);
    if (R[0] > MO_MAX_REACH || R[2] > MO_MAX_REACH) return false;
    *cw = (R[0] > 254 || R[2] > 254) ? 2 : 1;
    return true;
}
struct MoWs { size_t a, m, total; };                       // a: the counts (ball) / the first byte volume (struct); m: the byte mask / the second
static MoWs mo_layout(int A0, int A1, int A2, int cw) {
    const size_t N = (size_t)A0 * A1 * A2;
    MoWs W;
    W.a = 0;
    W.m = hv_up16(N * cw);
    W.total = W.m + hv_up16(N);
    return W;
}
static const double mo_unit[3] = {1.0, 1.0, 1.0};

extern "C" size_t hv_morph_workspace_bytes(int A0, int A1, int A2, double radius, const double* spacing) {
    const double* sp = spacing ? spacing : mo_unit;
    if (!mo_dims_ok(A0, A1, A2) || !mo_radius_ok(radius) || !mo_spacing_ok(sp)) return 0;
    int R[3], cw = 2;
    if (!mo_plan(A0, A1, A2, radius, sp, R, &cw)) return 0;
    return mo_layout(A0, A1, A2, cw).total;
}

extern "C" int hv_morph_tile(int* dims) {
    if (!dims) return HV_ERR_ARG;
    dims[0] = MO_T0; dims[1] = MO_T1; dims[2] = MO_T2;
    return HV_OK;
}

static inline bool mo_op_ok(int op) { return op == HV_MORPH_DILATE || op == HV_MORPH_ERODE || op == HV_MORPH_OPEN || op == HV_MORPH_CLOSE; }
// the halves of an op in order: 1 = an erosion
static inline int mo_halves(int op, int* erode) {
    switch (op) {
        case HV_MORPH_DILATE: erode[0] = 0; return 1;
        case HV_MORPH_ERODE: erode[0] = 1; return 1;
        case HV_MORPH_OPEN: erode[0] = 1; erode[1] = 0; return 2;
        default: erode[0] = 0; erode[1] = 1; return 2;
    }
}

template <typename C>
static int mo_ball_half(const MoSrc& S, const MoBall& B, C* g, const MoOut& O, hipStream_t st) {
    hipLaunchKernelGGL(morph_axis0_kernel<C>, dim3(hv_cdiv((long long)B.A1 * B.A2, MO_THREADS)), dim3(MO_THREADS), 0, st, S, B, g);
    HV_LAUNCH_CHECK();
    int KT = MO_KT;
    while (KT > 1 && ((long long)B.A1 * KT * 2 > MO_LDS_BYTES || KT / 2 >= B.A2)) KT /= 2;
    hipLaunchKernelGGL(morph_axis1_kernel<C>, dim3((unsigned)((long long)B.A0 * hv_cdiv(B.A2, KT))), dim3(MO_THREADS), (size_t)B.A1 * KT * 2, st, B, g,
                       KT);
    HV_LAUNCH_CHECK();
    int LN = MO_LINES;
    while (LN > 1 && (long long)B.A2 * LN * 2 > MO_LDS_BYTES) LN /= 2;
    hipLaunchKernelGGL(morph_axis2_kernel<C>, dim3(hv_cdiv((long long)B.A0 * B.A1, LN)), dim3(MO_THREADS), (size_t)B.A2 * LN * 2, st, B, (const C*)g,
                       O, LN);
    HV_LAUNCH_CHECK();
    return HV_OK;
}

// what the two mask entries check alike; HV_OK, or the refusal
static int mo_check(const void* vol, int dtype, int A0, int A1, int A2, int mode, int op, int border_value, const void* out, const void* workspace) {
    if (!vol || !out || !workspace || !mo_dims_ok(A0, A1, A2) || !mo_dtype_ok(dtype) || (mode != HV_CCL_EQ && mode != HV_CCL_NE) || !mo_op_ok(op) ||
        (border_value != 0 && border_value != 1) || ((uintptr_t)workspace & 15))
        return HV_ERR_ARG;
    if ((long long)A0 * A1 * A2 > (1LL << 30)) return HV_ERR_UNSUPPORTED;
    return HV_OK;
}

extern "C" int hv_morph_ball(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, double value, int mode,
                             int op, double radius, const double* spacing, int border_value, void* out, long long os0, long long os1,
                             long long os2, void* workspace, size_t workspace_bytes, void* stream) {
    if (!mo_radius_ok(radius) || !mo_spacing_ok(spacing)) return HV_ERR_ARG;
    const int rc = mo_check(vol, dtype, A0, A1, A2, mode, op, border_value, out, workspace);
    if (rc != HV_OK) return rc;
    if (A1 > MO_MAX_LINE || A2 > MO_MAX_LINE) return HV_ERR_UNSUPPORTED;
    int R[3], cw = 2;
    if (!mo_plan(A0, A1, A2, radius, spacing, R, &cw)) return HV_ERR_UNSUPPORTED;
    const MoWs W = mo_layout(A0, A1, A2, cw);
    if (workspace_bytes < W.total) return HV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    MoSrc S0, SM;
    S0.p = vol; S0.dt = dtype; S0.s0 = s0; S0.s1 = s1; S0.s2 = s2; S0.value = value; S0.ne = mode == HV_CCL_NE;
    SM.p = ws + W.m; SM.dt = MO_MASK; SM.s0 = (long long)A1 * A2; SM.s1 = A2; SM.s2 = 1; SM.value = 0.0; SM.ne = 0;
    MoOut OF, OM;
    OF.p = (uint8_t*)out; OF.s0 = os0; OF.s1 = os1; OF.s2 = os2;
    OM.p = (uint8_t*)(ws + W.m); OM.s0 = SM.s0; OM.s1 = SM.s1; OM.s2 = 1;
    MoBall B;
    B.A0 = A0; B.A1 = A1; B.A2 = A2; B.R0 = R[0]; B.R1 = R[1]; B.R2 = R[2];
    B.s0 = spacing[0]; B.s1 = spacing[1]; B.s2 = spacing[2]; B.r2 = radius * radius;
    int erode[2];
    const int halves = mo_halves(op, erode);
    for (int h = 0; h < halves; ++h) {
        MoSrc S = h == 0 ? S0 : SM;
        if (erode[h]) S.ne = !S.ne;                // the erosion is the dilation of the complement, outside the volume included, inverted
        B.border = erode[h] ? 1 - border_value : border_value;
        B.inv_out = erode[h];
        const MoOut& O = h == halves - 1 ? OF : OM;
        const int e = cw == 1 ? mo_ball_half<uint8_t>(S, B, (uint8_t*)(ws + W.a), O, st) : mo_ball_half<uint16_t>(S, B, (uint16_t*)(ws + W.a), O, st);
        if (e != HV_OK) return e;
    }
    return HV_OK;
}

extern "C" int hv_morph_struct(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, double value, int mode,
                               int op, int connectivity, int iterations, int border_value, void* out, long long os0, long long os1,
                               long long os2, void* workspace, size_t workspace_bytes, void* stream) {
    if (connectivity < 1 || connectivity > 3 || iterations < 1) return HV_ERR_ARG;
    const int rc = mo_check(vol, dtype, A0, A1, A2, mode, op, border_value, out, workspace);
    if (rc != HV_OK) return rc;
    const MoWs W = mo_layout(A0, A1, A2, 1);
    if (workspace_bytes < W.total) return HV_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    uint8_t* buf[2] = {(uint8_t*)(ws + W.a), (uint8_t*)(ws + W.m)};
    int erode[2];
    const int halves = mo_halves(op, erode);
    const long long stages = (long long)halves * iterations;
    const int n0 = hv_cdiv(A0, MO_T0), n1 = hv_cdiv(A1, MO_T1), n2 = hv_cdiv(A2, MO_T2);
    const long long plane = (long long)A1 * A2;
    for (long long s = 0; s < stages; ++s) {
        MoSrc S;
        if (s == 0) {
            S.p = vol; S.dt = dtype; S.s0 = s0; S.s1 = s1; S.s2 = s2; S.value = value; S.ne = mode == HV_CCL_NE;
        } else {
            S.p = buf[(s - 1) & 1]; S.dt = MO_MASK; S.s0 = plane; S.s1 = A2; S.s2 = 1; S.value = 0.0; S.ne = 0;
        }
        MoOut O;
        if (s == stages - 1) {
            O.p = (uint8_t*)out; O.s0 = os0; O.s1 = os1; O.s2 = os2;
        } else {
            O.p = buf[s & 1]; O.s0 = plane; O.s1 = A2; O.s2 = 1;
        }
        hipLaunchKernelGGL(morph_stencil_kernel, dim3((unsigned)((long long)n0 * n1 * n2)), dim3(MO_THREADS), 0, st, S, O, A0, A1, A2, n1, n2,
                           connectivity, erode[s / iterations], border_value);
        HV_LAUNCH_CHECK();
    }
    return HV_OK;
}

extern "C" int hv_morph_merge(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, const void* mask,
                              long long ms0, long long ms1, long long ms2, int rule, double value, double background, double fill, void* out,
                              long long os0, long long os1, long long os2, void* stream) {
    if (!vol || !mask || !out || !mo_dims_ok(A0, A1, A2) || !mo_dtype_ok(dtype) || (rule != HV_MORPH_GROW && rule != HV_MORPH_SHRINK) ||
        (out == vol && (os0 != s0 || os1 != s1 || os2 != s2)))
        return HV_ERR_ARG;
    if ((long long)A0 * A1 * A2 > (1LL << 30)) return HV_ERR_UNSUPPORTED;
    MoSrc S;
    S.p = vol; S.dt = dtype; S.s0 = s0; S.s1 = s1; S.s2 = s2; S.value = value; S.ne = 0;
    MoOut M;
    M.p = (uint8_t*)const_cast<void*>(mask); M.s0 = ms0; M.s1 = ms1; M.s2 = ms2;
    const int N = A0 * A1 * A2;
    hipLaunchKernelGGL(morph_merge_kernel, dim3(hv_cdiv(N, MO_THREADS)), dim3(MO_THREADS), 0, (hipStream_t)stream, S, M, A1, A2, N, rule, background,
                       fill, out, os0, os1, os2, out != vol ? 1 : 0);
    HV_LAUNCH_CHECK();
    return HV_OK;
}
