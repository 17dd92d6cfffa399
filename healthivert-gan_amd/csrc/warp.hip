// Deformable 3-D resampling on the device: a volume sampled at coordinates that are not an affine lattice.
//   hv_map_coordinates  scipy.ndimage.map_coordinates: the coordinates are read from three planes over the output lattice, float32 (widened
//                       exactly) or float64, either as they are (HV_COORDS_ABSOLUTE, u_h = c_h(o)) or as a dense displacement field in source
//                       voxels (HV_COORDS_DISPLACEMENT, u_h = (double)o_h + c_h(o)).
//   hv_warp_grid        an affine lattice plus a free-form deformation from a coarse control grid [3][G0][G1][G2] of float64 displacements;
//                       no dense coordinates exist anywhere.  For output index o, in float64 without fused multiply-add, in this order:
//                         q_a = (o_a + gshift[a]) * gzoom[a], clamped to [0, G_a - 1] as q >= 0 ? (q <= hi ? q : hi) : 0
//                         d_h = the sampler's sum on grid[h] at q, order gorder: 1 the taps floor(q), floor(q) + 1 with 1 - y, 1 - (1 - y);
//                               3 the four taps and weights of hv_spline_taps on the control values themselves (no prefilter: the
//                               approximating cubic B-spline of free-form deformation, Rueckert et al. 1999).  Tap indices mirrored about the
//                               ends, last axis fastest, each term ((g w0) w1) w2, added from 0.0
//                         u_h = base_h(o) + d_h, base_h hv_resample's expression for the descriptor's form
// From u on both are hv_resample, word for word (resample_core.h): the outside test -- a NaN coordinate fails it and gives cval in mode
// constant, and is clamped to 0 by the nearest form, as in scipy -- the taps, weights, mirrored indices, term order and output conversion.
//
// One kernel template over source dtype x order x where the coordinates come from, one launch per entry.  The tile is resample_kernel's: 256
// lanes own RS_T^3 outputs; lanes run along role L, eight of them, then M; each lane computes two outputs RS_T / 2 apart along O.  The roles:
//   hv_warp_grid        as hv_resample: L is the output axis whose image under the base lattice has the smallest source stride.  The
//                       deformation is small against the lattice, so the source gathers decide.
//   hv_map_coordinates  L is the output axis along which the coordinate planes have the smallest stride (an axis of extent 1 last; a tie goes
//                       to the later axis).  Where a coordinate leads in the source is not known on the host, and the coordinate reads are
//                       the larger traffic (12 - 24 bytes per output against a 1 - 8 byte voxel), so they get the neighbouring lanes.
// The control grid is read from global memory through L1 / L2 (DESIGN.md row f17 says why it is not staged in LDS).  No atomics, no workspace,
// no LDS, no scratch; every source index is formed from a coordinate already tested or clamped, every grid index from a clamped q, every
// coordinate and output index from an output index below the extents: nothing outside the stated boxes is read or written.
#include "resample_core.h"

enum { WP_FROM_COORDS = 0, WP_FROM_GRID1 = 1, WP_FROM_GRID3 = 3 };

struct WpP {
    const void* src; void* dst;
    const void* aux;                    // the coordinate planes, or the control grid
    long long s0, s1, s2, d0, d1, d2;   // element strides by HOST axis
    long long xp, x0, x1, x2;           // aux: the plane (component) stride and the per-axis strides, in elements
    int A0, A1, A2, G0, G1, G2;
    int r0, r1, r2;                     // the role (0 = L, 1 = M, 2 = O) of host output axis 0 / 1 / 2
    int nL, nM, nO;                     // the output extents by role
    int dst_dt, aux_dt, kind;
    hv_warp_desc D;
};

// the three displacements at output index (c0, c1, c2): the taps and weights once, then the sampler's sum on each component of the grid
struct WpD { double d0, d1, d2; };
template <int GORDER>
__device__ __forceinline__ WpD wp_displace(const WpP& P, double c0, double c1, double c2) {
    constexpr int NT = GORDER + 1;
    double q0 = (c0 + P.D.gshift[0]) * P.D.gzoom[0], q1 = (c1 + P.D.gshift[1]) * P.D.gzoom[1], q2 = (c2 + P.D.gshift[2]) * P.D.gzoom[2];
    rs_inside(q0, P.G0, HV_FILT_NEAREST);
    rs_inside(q1, P.G1, HV_FILT_NEAREST);
    rs_inside(q2, P.G2, HV_FILT_NEAREST);
    long long o0[NT], o1[NT], o2[NT];
    double w0[NT], w1[NT], w2[NT];
    rs_taps<GORDER>(q0, P.G0, P.x0, o0, w0);
    rs_taps<GORDER>(q1, P.G1, P.x1, o1, w1);
    rs_taps<GORDER>(q2, P.G2, P.x2, o2, w2);
    WpD d = {0.0, 0.0, 0.0};
    // one component after the other, and within it one tap along axis 0 after the other (neither unrolled; the axis-0 tap is picked by
    // selects, so no array is indexed by a loop variable): at gorder 3 that keeps 16 loads in flight where the unrolled sum held all 64 x 3
    // in registers.  The order of the additions is the sampler's.
#pragma unroll 1
    for (int h = 0; h < 3; ++h) {
        const double* g = reinterpret_cast<const double*>(P.aux) + h * P.xp;
        double t = 0.0;
#pragma unroll 1
        for (int a = 0; a < NT; ++a) {
            long long oa = o0[0];
            double wa = w0[0];
#pragma unroll
            for (int k = 1; k < NT; ++k) {
                oa = a == k ? o0[k] : oa;
                wa = a == k ? w0[k] : wa;
            }
#pragma unroll
            for (int b = 0; b < NT; ++b) {
                const long long ob = oa + o1[b];
#pragma unroll
                for (int c = 0; c < NT; ++c) t += ((g[ob + o2[c]] * wa) * w1[b]) * w2[c];
            }
        }
        d.d0 = h == 0 ? t : d.d0;
        d.d1 = h == 1 ? t : d.d1;
        d.d2 = h == 2 ? t : d.d2;
    }
    return d;
}

// the sum over the taps at (u0, u1, u2), each already inside [0, A - 1]: last axis fastest, each term ((v w0) w1) w2, added from 0.0.  This is
// resample_kernel's tap loop restated: calling one shared function from resample_kernel changed its order-3 register allocation.
template <typename T, int ORDER>
__device__ __forceinline__ double wp_sample(const T* src, double u0, double u1, double u2, int A0, int A1, int A2, long long s0, long long s1,
                                            long long s2) {
    constexpr int NT = ORDER + 1;
    long long o0[NT], o1[NT], o2[NT];
    double w0[NT], w1[NT], w2[NT];
    rs_taps<ORDER>(u0, A0, s0, o0, w0);
    rs_taps<ORDER>(u1, A1, s1, o1, w1);
    rs_taps<ORDER>(u2, A2, s2, o2, w2);
    double t = 0.0;
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) {
            const long long ob = o0[a] + o1[b];
#pragma unroll
            for (int c = 0; c < NT; ++c) {
                const double v = rs_ld(src, ob + o2[c]);
                if constexpr (ORDER == 0) t += v;
                else t += ((v * w0[a]) * w1[b]) * w2[c];
            }
        }
    return t;
}

__device__ __forceinline__ double wp_coord(const void* c, int dt, long long off) {
    return dt == HV_DT_F32 ? (double)((const float*)c)[off] : ((const double*)c)[off];
}

// grid: the tiles, the one along L fastest
template <typename T, int ORDER, int FROM>
__global__ __launch_bounds__(RS_THREADS) void warp_kernel(WpP P) {
    const int ntL = (P.nL + RS_T - 1) / RS_T, ntM = (P.nM + RS_T - 1) / RS_T;
    const int tL = (int)(blockIdx.x % ntL), tM = (int)((blockIdx.x / ntL) % ntM), tO = (int)(blockIdx.x / ((unsigned)ntL * ntM));
    const int gL = tL * RS_T + (int)(threadIdx.x % RS_T), gM = tM * RS_T + (int)((threadIdx.x / RS_T) % RS_T);
    if (gL >= P.nL || gM >= P.nM) return;
    const T* src = reinterpret_cast<const T*>(P.src);
    const hv_resample_desc& D = P.D.base;
#pragma unroll 1
    for (int rep = 0; rep < 2; ++rep) {
        const int gO = tO * RS_T + (int)(threadIdx.x / (RS_T * RS_T)) + rep * (RS_T / 2);
        if (gO >= P.nO) return;
        const int i0 = rs_pick(P.r0, gL, gM, gO), i1 = rs_pick(P.r1, gL, gM, gO), i2 = rs_pick(P.r2, gL, gM, gO);
        const double c0 = (double)i0, c1 = (double)i1, c2 = (double)i2;
        double u0, u1, u2;
        if constexpr (FROM == WP_FROM_COORDS) {
            const long long off = i0 * P.x0 + i1 * P.x1 + i2 * P.x2;
            u0 = wp_coord(P.aux, P.aux_dt, off);
            u1 = wp_coord(P.aux, P.aux_dt, off + P.xp);
            u2 = wp_coord(P.aux, P.aux_dt, off + 2 * P.xp);
            if (P.kind == HV_COORDS_DISPLACEMENT) {
                u0 = c0 + u0;
                u1 = c1 + u1;
                u2 = c2 + u2;
            }
        } else {
            const WpD e = wp_displace<FROM>(P, c0, c1, c2);
            if (D.form == HV_RESAMPLE_MATRIX) {
                u0 = (((0.0 + c0 * D.matrix[0]) + c1 * D.matrix[1]) + c2 * D.matrix[2]) + D.offset[0];
                u1 = (((0.0 + c0 * D.matrix[3]) + c1 * D.matrix[4]) + c2 * D.matrix[5]) + D.offset[1];
                u2 = (((0.0 + c0 * D.matrix[6]) + c1 * D.matrix[7]) + c2 * D.matrix[8]) + D.offset[2];
            } else {
                u0 = (c0 + D.shift[0]) * D.zoom[0];
                u1 = (c1 + D.shift[1]) * D.zoom[1];
                u2 = (c2 + D.shift[2]) * D.zoom[2];
            }
            u0 = u0 + e.d0;
            u1 = u1 + e.d1;
            u2 = u2 + e.d2;
        }
        const bool in0 = rs_inside(u0, P.A0, D.mode), in1 = rs_inside(u1, P.A1, D.mode), in2 = rs_inside(u2, P.A2, D.mode);
        double t = D.cval;
        if (in0 && in1 && in2) t = wp_sample<T, ORDER>(src, u0, u1, u2, P.A0, P.A1, P.A2, P.s0, P.s1, P.s2);
        rs_store(P.dst, P.dst_dt, i0 * P.d0 + i1 * P.d1 + i2 * P.d2, t);
    }
}

// ------------------------------------------------------------------------------------------------ host side
template <typename T, int FROM>
static void wp_launch(int order, dim3 grid, hipStream_t st, const WpP& P) {
    if (order == 0) hipLaunchKernelGGL((warp_kernel<T, 0, FROM>), grid, dim3(RS_THREADS), 0, st, P);
    else if (order == 1) hipLaunchKernelGGL((warp_kernel<T, 1, FROM>), grid, dim3(RS_THREADS), 0, st, P);
}

template <int FROM>
static void wp_dispatch(int dtype, int order, dim3 grid, hipStream_t st, const WpP& P) {
    if (order == 3) hipLaunchKernelGGL((warp_kernel<double, 3, FROM>), grid, dim3(RS_THREADS), 0, st, P);
    else switch (dtype) {
        case HV_DT_U8: wp_launch<uint8_t, FROM>(order, grid, st, P); break;
        case HV_DT_I16: wp_launch<int16_t, FROM>(order, grid, st, P); break;
        case HV_DT_F32: wp_launch<float, FROM>(order, grid, st, P); break;
        default: wp_launch<double, FROM>(order, grid, st, P); break;
    }
}

// the parts of WpP every entry fills alike: the two boxes and the roles from `key` (rs_roles)
static void wp_fill(WpP& P, const void* vol, const int* A, const long long* ss, void* out, int out_dtype, const int* O, const long long* os,
                    const double* key) {
    P.src = vol; P.dst = out;
    P.s0 = ss[0]; P.s1 = ss[1]; P.s2 = ss[2]; P.d0 = os[0]; P.d1 = os[1]; P.d2 = os[2];
    P.A0 = A[0]; P.A1 = A[1]; P.A2 = A[2];
    int ord[3], role[3];
    rs_roles(O, key, ord);
    for (int r = 0; r < 3; ++r) role[ord[r]] = r;
    P.r0 = role[0]; P.r1 = role[1]; P.r2 = role[2];
    P.nL = O[ord[0]]; P.nM = O[ord[1]]; P.nO = O[ord[2]];
    P.dst_dt = out_dtype;
}

static dim3 wp_tiles(const int* O) { return dim3((unsigned)((long long)hv_cdiv(O[0], RS_T) * hv_cdiv(O[1], RS_T) * hv_cdiv(O[2], RS_T))); }

extern "C" int hv_map_coordinates_tile(int* dims) { return hv_resample_tile(dims); }
extern "C" int hv_warp_grid_tile(int* dims) { return hv_resample_tile(dims); }

extern "C" int hv_map_coordinates(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2,
                                  const void* coords, int coord_dtype, long long cp, long long c0, long long c1, long long c2, int coord_kind,
                                  void* out, int out_dtype, long long os0, long long os1, long long os2, int O0, int O1, int O2, int order,
                                  int mode, double cval, void* stream) {
    const int A[3] = {A0, A1, A2}, O[3] = {O0, O1, O2};
    const long long ss[3] = {s0, s1, s2}, os[3] = {os0, os1, os2};
    int rc = rs_check_args(vol, dtype, A, out, out_dtype, O, order, mode, cval);
    if (rc != HV_OK) return rc;
    if (!coords || (coord_dtype != HV_DT_F32 && coord_dtype != HV_DT_F64) ||
        (coord_kind != HV_COORDS_ABSOLUTE && coord_kind != HV_COORDS_DISPLACEMENT) || ((uintptr_t)coords & (rs_elem(coord_dtype) - 1)))
        return HV_ERR_ARG;
    rc = rs_check_support(vol, dtype, A, ss, out, out_dtype, O, os, order, mode);
    if (rc != HV_OK) return rc;
    const int C[4] = {3, O0, O1, O2};
    const long long cs[4] = {cp, c0, c1, c2};
    long long clo, chi, olo, ohi;
    rs_span(C, cs, rs_elem(coord_dtype), &clo, &chi, 4);
    rs_span(O, os, rs_elem(out_dtype), &olo, &ohi);
    if (rs_meet(coords, clo, chi, out, olo, ohi)) return HV_ERR_ARG;
    const double key[3] = {(double)rs_abs(c0), (double)rs_abs(c1), (double)rs_abs(c2)};
    WpP P = {};
    wp_fill(P, vol, A, ss, out, out_dtype, O, os, key);
    P.aux = coords; P.aux_dt = coord_dtype; P.kind = coord_kind;
    P.xp = cp; P.x0 = c0; P.x1 = c1; P.x2 = c2;
    P.D.base.order = order; P.D.base.mode = mode; P.D.base.cval = cval;
    wp_dispatch<WP_FROM_COORDS>(dtype, order, wp_tiles(O), (hipStream_t)stream, P);
    HV_LAUNCH_CHECK();
    return HV_OK;
}

extern "C" int hv_warp_grid(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, const double* grid,
                            long long gp, long long g0, long long g1, long long g2, int G0, int G1, int G2, void* out, int out_dtype,
                            long long os0, long long os1, long long os2, int O0, int O1, int O2, const hv_warp_desc* desc, void* stream) {
    if (!desc) return HV_ERR_ARG;
    const hv_resample_desc& D = desc->base;
    const int A[3] = {A0, A1, A2}, O[3] = {O0, O1, O2};
    const long long ss[3] = {s0, s1, s2}, os[3] = {os0, os1, os2};
    int rc = rs_check_args(vol, dtype, A, out, out_dtype, O, D.order, D.mode, D.cval);
    if (rc != HV_OK) return rc;
    if (!rs_desc_ok(D)) return HV_ERR_ARG;
    if (!grid || G0 <= 0 || G1 <= 0 || G2 <= 0 || (desc->gorder != 1 && desc->gorder != 3) || ((uintptr_t)grid & 7)) return HV_ERR_ARG;
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(desc->gzoom[i]) || !std::isfinite(desc->gshift[i])) return HV_ERR_ARG;
    rc = rs_check_support(vol, dtype, A, ss, out, out_dtype, O, os, D.order, D.mode);
    if (rc != HV_OK) return rc;
    if ((long long)G0 * G1 * G2 > (1LL << 30)) return HV_ERR_UNSUPPORTED;
    const int G[4] = {3, G0, G1, G2};
    const long long gs[4] = {gp, g0, g1, g2};
    long long glo, ghi, olo, ohi;
    rs_span(G, gs, sizeof(double), &glo, &ghi, 4);
    rs_span(O, os, rs_elem(out_dtype), &olo, &ohi);
    if (rs_meet(grid, glo, ghi, out, olo, ohi)) return HV_ERR_ARG;
    double key[3];
    rs_image(D, ss, key);
    WpP P = {};
    wp_fill(P, vol, A, ss, out, out_dtype, O, os, key);
    P.aux = grid; P.aux_dt = HV_DT_F64;
    P.xp = gp; P.x0 = g0; P.x1 = g1; P.x2 = g2;
    P.G0 = G0; P.G1 = G1; P.G2 = G2;
    P.D = *desc;
    const dim3 tiles = wp_tiles(O);
    if (desc->gorder == 1) wp_dispatch<WP_FROM_GRID1>(dtype, D.order, tiles, (hipStream_t)stream, P);
    else wp_dispatch<WP_FROM_GRID3>(dtype, D.order, tiles, (hipStream_t)stream, P);
    HV_LAUNCH_CHECK();
    return HV_OK;
}
