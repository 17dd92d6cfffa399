// Generation-quality evaluation of a synthesized vertebra volume on the device (reference evaluation/generation_eval_sagittal.py:11-103 and
// generation_eval_coronal.py:11-103, process_images and the three overlap metrics).
//
// A volume is seen as [R rows][C columns][S slices]: rows are axis 0, slices the view axis (2 sagittal, 1 coronal), columns the third
// axis.  Everything is float64 (-ffp-contract=off); the CT may be float32 / float64, the labels uint8 / float32 / float64.
//   ge_rows_kernel / ge_rows_cfast_kernel   pass 1: each volume read once.  Per (chunk of columns, slice, row): counts of ori, fake and
//                        ori & fake, min / max of the ori CT, sum of squared CT errors.  Lanes walk the axis with the smallest CT stride
//                        (rows or slices: a thread owns two neighbouring (slice, row) pairs and loops over a chunk of columns; columns: a
//                        wave owns one (slice, row) and reduces across lanes); two neighbours per lane -> 16-B fp64 loads where aligned
//   ge_slice_kernel      pass 2: grid (S): the chunks folded per row, then per slice the three counts, the ori's first / last row
//                        (x1, x2) and min / max / squared-error sum over the whole slice and over rows x1..x2
//   ge_select_kernel     <<<1,256>>>: the view axis extent of the ori, the 4/5 slice range, the > 400 voxel selection, IoU / Dice / RVD
//                        from the exact integer counts, the error flags
//   ge_ssim_kernel       pass 3: grid (column tiles, row tiles, S), selected slices only: the five 7x7 window sums of every interior
//                        pixel from an LDS tile; S evaluated with the slice's data range (every window) and with the patch's (windows whose
//                        centre row lies in [x1 + 3, x2 - 3], which lie inside the crop and have the crop's moments)
//   ge_slice_final_kernel  grid (S): per selected slice the SSIM means (fixed-order tile sums) and both PSNRs
//   ge_final_kernel      <<<1,256>>>: NaN-dropping means over the selected slices, the seven results, the per-slice records
#include "hv_common.h"

namespace {

constexpr int GE_TC = 64;     // ssim tile: output columns
constexpr int GE_TR = 16;     // ssim tile: output rows (4 per thread)
constexpr int GE_REC = 9;     // doubles per slice record

struct GeSlice {
    long long no, nf, ni;              // ori, fake, ori & fake voxels of the slice
    int x1, x2, sel, pad;
    double gmn, gmx, gsse, pmn, pmx, psse;
    double psnr_p, psnr_g, ssim_p, ssim_g;
};
struct GeParams { int empty, shorts, nsel, z0, z1, nz0, m, pad; long long no, nf, ni; };

template <typename T> __device__ __forceinline__ double ge_ld(const T* p) { return (double)*p; }
// two neighbours along a unit-stride axis, 16 / 8 / 2 bytes per lane (alignment checked by the host)
__device__ __forceinline__ void ge_ld2(const double* p, double& a, double& b) { const double2 v = *(const double2*)p; a = v.x; b = v.y; }
__device__ __forceinline__ void ge_ld2(const float* p, double& a, double& b) { const float2 v = *(const float2*)p; a = v.x; b = v.y; }
__device__ __forceinline__ void ge_ld2(const unsigned char* p, double& a, double& b) {
    const unsigned short v = *(const unsigned short*)p;
    a = (double)(v & 0xff); b = (double)(v >> 8);
}
template <typename T, bool VEC> __device__ __forceinline__ void ge_pair(const T* p, long long step, bool two, double& a, double& b) {
    if (VEC && two) { ge_ld2(p, a, b); return; }
    a = ge_ld(p);
    b = two ? ge_ld(p + step) : 0.0;
}

struct GeAcc {
    int no, nf, ni;
    double mn, mx, sse;
    __device__ __forceinline__ void init() { no = nf = ni = 0; mn = HUGE_VAL; mx = -HUGE_VAL; sse = 0.0; }
    __device__ __forceinline__ void add(double lo, double lf, double co, double cf, double label, bool ct) {
        const bool o = lo == label, f = lf == label;
        no += o; nf += f; ni += o && f;
        if (ct) { mn = fmin(mn, co); mx = fmax(mx, co); const double d = co - cf; sse += d * d; }
    }
};

struct GeTables { int *no, *nf, *ni; double *mn, *mx, *sse; };

__device__ __forceinline__ void ge_store(const GeTables& t, long long i, const GeAcc& a) {
    t.no[i] = a.no; t.nf[i] = a.nf; t.ni[i] = a.ni; t.mn[i] = a.mn; t.mx[i] = a.mx; t.sse[i] = a.sse;
}

// pass 1, lanes along rows or slices (the faster of the two, `fast_is_s`): thread = two neighbours along it x one index of the other
// x one chunk of CK columns (blockIdx.y)
template <typename TC, typename TL, bool VEC>
__global__ __launch_bounds__(256) void ge_rows_kernel(const TC* __restrict__ oct, const TC* __restrict__ fct, long long csr, long long csc,
                                                      long long css, const TL* __restrict__ olab, const TL* __restrict__ flab, long long lsr,
                                                      long long lsc, long long lss, int R, int C, int S, int fast_is_s, int CK, double label,
                                                      GeTables tab) {
    const int F = fast_is_s ? S : R, O = fast_is_s ? R : S, FP = (F + 1) >> 1;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)FP * O) return;
    const int f0 = 2 * (int)(t % FP), o = (int)(t / FP);
    const bool two = f0 + 1 < F;
    const int r = fast_is_s ? o : f0, s = fast_is_s ? f0 : o;
    const long long cstep = fast_is_s ? css : csr, lstep = fast_is_s ? lss : lsr;
    const int c0 = blockIdx.y * CK, c1 = min(C, c0 + CK);
    const bool ct = oct != nullptr;
    const TC* po = ct ? oct + (long long)r * csr + (long long)s * css : nullptr;
    const TC* pf = ct ? fct + (long long)r * csr + (long long)s * css : nullptr;
    const TL* pl = olab + (long long)r * lsr + (long long)s * lss;
    const TL* ql = flab + (long long)r * lsr + (long long)s * lss;
    GeAcc A, B;
    A.init(); B.init();
#pragma unroll 4
    for (int c = c0; c < c1; ++c) {
        double la, lb, ma, mb, ca = 0.0, cb = 0.0, da = 0.0, db = 0.0;
        ge_pair<TL, VEC>(pl + (long long)c * lsc, lstep, two, la, lb);
        ge_pair<TL, VEC>(ql + (long long)c * lsc, lstep, two, ma, mb);
        if (ct) {
            ge_pair<TC, VEC>(po + (long long)c * csc, cstep, two, ca, cb);
            ge_pair<TC, VEC>(pf + (long long)c * csc, cstep, two, da, db);
        }
        A.add(la, ma, ca, da, label, ct);
        B.add(lb, mb, cb, db, label, ct);
    }
    const long long base = (long long)blockIdx.y * S * R;
    ge_store(tab, base + (long long)s * R + r, A);
    if (two) ge_store(tab, base + (fast_is_s ? (long long)(s + 1) * R + r : (long long)s * R + r + 1), B);
}

__device__ __forceinline__ double ge_wsum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int ge_wsum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double ge_wmin(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double ge_wmax(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// pass 1, lanes along columns: a wave per (slice, row), two neighbouring columns per lane
template <typename TC, typename TL, bool VEC>
__global__ __launch_bounds__(256) void ge_rows_cfast_kernel(const TC* __restrict__ oct, const TC* __restrict__ fct, long long csr, long long csc,
                                                            long long css, const TL* __restrict__ olab, const TL* __restrict__ flab, long long lsr,
                                                            long long lsc, long long lss, int R, int C, int S, double label, GeTables tab) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)S * R) return;
    const int lane = threadIdx.x & 63, s = (int)(row / R), r = (int)(row - (long long)s * R);
    const bool ct = oct != nullptr;
    const TC* po = ct ? oct + (long long)r * csr + (long long)s * css : nullptr;
    const TC* pf = ct ? fct + (long long)r * csr + (long long)s * css : nullptr;
    const TL* pl = olab + (long long)r * lsr + (long long)s * lss;
    const TL* ql = flab + (long long)r * lsr + (long long)s * lss;
    GeAcc A;
    A.init();
    for (int c = 2 * lane; c < C; c += 128) {
        const bool two = c + 1 < C;
        double la, lb, ma, mb, ca = 0.0, cb = 0.0, da = 0.0, db = 0.0;
        ge_pair<TL, VEC>(pl + (long long)c * lsc, lsc, two, la, lb);
        ge_pair<TL, VEC>(ql + (long long)c * lsc, lsc, two, ma, mb);
        if (ct) {
            ge_pair<TC, VEC>(po + (long long)c * csc, csc, two, ca, cb);
            ge_pair<TC, VEC>(pf + (long long)c * csc, csc, two, da, db);
        }
        A.add(la, ma, ca, da, label, ct);
        if (two) A.add(lb, mb, cb, db, label, ct);
    }
    A.no = ge_wsum(A.no); A.nf = ge_wsum(A.nf); A.ni = ge_wsum(A.ni);
    A.mn = ge_wmin(A.mn); A.mx = ge_wmax(A.mx); A.sse = ge_wsum(A.sse);
    if (lane == 0) ge_store(tab, row, A);
}

// block reductions over 256 threads (4 waves)
__device__ __forceinline__ double ge_bsum(double v, double* sh) {
    v = ge_wsum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__device__ __forceinline__ double ge_bmin(double v, double* sh) {
    v = ge_wmin(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmin(fmin(sh[0], sh[1]), fmin(sh[2], sh[3]));
}
__device__ __forceinline__ double ge_bmax(double v, double* sh) { return -ge_bmin(-v, sh); }

// pass 2: one block per slice
__global__ __launch_bounds__(256) void ge_slice_kernel(GeTables tab, int K, int R, int S, GeSlice* __restrict__ sl) {
    __shared__ double sh[4];
    const int s = blockIdx.x;
    double no = 0.0, nf = 0.0, ni = 0.0, x1 = HUGE_VAL, x2 = -HUGE_VAL, mn = HUGE_VAL, mx = -HUGE_VAL, sse = 0.0;
    for (int r = threadIdx.x; r < R; r += 256) {
        long long o = 0;
        double rmn = HUGE_VAL, rmx = -HUGE_VAL, rs = 0.0;
        for (int k = 0; k < K; ++k) {
            const long long i = ((long long)k * S + s) * R + r;
            o += tab.no[i]; nf += tab.nf[i]; ni += tab.ni[i];
            rmn = fmin(rmn, tab.mn[i]); rmx = fmax(rmx, tab.mx[i]); rs += tab.sse[i];
        }
        no += (double)o;
        if (o > 0) { x1 = fmin(x1, (double)r); x2 = fmax(x2, (double)r); }
        mn = fmin(mn, rmn); mx = fmax(mx, rmx); sse += rs;
    }
    // counts are below 2^53: exact as doubles
    no = ge_bsum(no, sh); nf = ge_bsum(nf, sh); ni = ge_bsum(ni, sh);
    x1 = ge_bmin(x1, sh); x2 = ge_bmax(x2, sh);
    mn = ge_bmin(mn, sh); mx = ge_bmax(mx, sh); sse = ge_bsum(sse, sh);
    double pmn = HUGE_VAL, pmx = -HUGE_VAL, psse = 0.0;
    if (no > 0.0) {
        for (int r = (int)x1 + threadIdx.x; r <= (int)x2; r += 256) {
            for (int k = 0; k < K; ++k) {
                const long long i = ((long long)k * S + s) * R + r;
                pmn = fmin(pmn, tab.mn[i]); pmx = fmax(pmx, tab.mx[i]); psse += tab.sse[i];
            }
        }
    }
    pmn = ge_bmin(pmn, sh); pmx = ge_bmax(pmx, sh); psse = ge_bsum(psse, sh);
    if (threadIdx.x == 0) {
        GeSlice& g = sl[s];
        g.no = (long long)no; g.nf = (long long)nf; g.ni = (long long)ni;
        g.x1 = no > 0.0 ? (int)x1 : -1; g.x2 = no > 0.0 ? (int)x2 : -1; g.sel = 0; g.pad = 0;
        g.gmn = mn; g.gmx = mx; g.gsse = sse; g.pmn = pmn; g.pmx = pmx; g.psse = psse;
        g.psnr_p = g.psnr_g = g.ssim_p = g.ssim_g = 0.0;
    }
}

// the slice range and selection (process_images :60-71), the overlap metrics (:11-37); out[4] iou, out[5] rv_diff, out[6] dice.
// One block: the per-slice records are read in parallel (counts below 2^53 are exact as doubles)
__global__ __launch_bounds__(256) void ge_select_kernel(GeSlice* __restrict__ sl, int R, int C, int S, GeParams* __restrict__ prm,
                                                        double* __restrict__ out) {
    __shared__ double sh[4];
    double no = 0.0, nf = 0.0, ni = 0.0, z0 = HUGE_VAL, z1 = -HUGE_VAL;
    for (int s = threadIdx.x; s < S; s += 256) {
        const long long a = sl[s].no;
        no += (double)a; nf += (double)sl[s].nf; ni += (double)sl[s].ni;
        if (a > 0) { z0 = fmin(z0, (double)s); z1 = fmax(z1, (double)s); }
    }
    no = ge_bsum(no, sh); nf = ge_bsum(nf, sh); ni = ge_bsum(ni, sh);
    z0 = ge_bmin(z0, sh); z1 = ge_bmax(z1, sh);
    const bool empty = no == 0.0;
    int n = 0, m = 0, nz0 = 0;
    if (!empty) {
        n = (int)z1 - (int)z0 + 1; m = (4 * n) / 5; nz0 = (int)z0 + (n - m) / 2;   // int(n*4/5), z0 + (n - m)//2
    }
    double nsel = 0.0, shorts = 0.0;
    for (int s = nz0 + threadIdx.x; s < nz0 + m; s += 256) {
        if (sl[s].no > 400) {
            sl[s].sel = 1;
            nsel += 1.0;
            if (sl[s].x2 - sl[s].x1 + 1 < 7 || C < 7) shorts = 1.0;   // structural_similarity: a side shorter than win_size
        }
    }
    nsel = ge_bsum(nsel, sh);
    shorts = ge_bmax(shorts, sh);
    if (threadIdx.x != 0) return;
    GeParams p = {};
    p.no = (long long)no; p.nf = (long long)nf; p.ni = (long long)ni;
    p.empty = empty; p.shorts = shorts != 0.0; p.nsel = (int)nsel;
    p.z0 = empty ? 0 : (int)z0; p.z1 = empty ? 0 : (int)z1; p.nz0 = nz0; p.m = m;
    *prm = p;
    const long long u = p.no + p.nf - p.ni;
    out[4] = u == 0 ? 0.0 : (double)p.ni / (double)u;
    out[5] = p.no == 0 ? 0.0 : (double)(p.no > p.nf ? p.no - p.nf : p.nf - p.no) / (double)p.no;
    out[6] = p.no + p.nf == 0 ? 0.0 : 2.0 * (double)p.ni / (double)(p.no + p.nf);
    out[7] = (double)p.empty;
    out[8] = (double)p.shorts;
    out[9] = (double)p.nsel;
    out[10] = (double)p.no; out[11] = (double)p.nf; out[12] = (double)p.ni;
}

template <typename TC>
__device__ __forceinline__ double ge_ct(const TC* p, long long sr, long long sc, int r, int c) { return (double)p[(long long)r * sr + (long long)c * sc]; }

__device__ __forceinline__ double ge_S(double ux, double uy, double uxx, double uyy, double uxy, double C1, double C2) {
    const double cov = 49.0 / 48.0;
    const double vx = cov * (uxx - ux * ux), vy = cov * (uyy - uy * uy), vxy = cov * (uxy - ux * uy);
    const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2, B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
    return (A1 * A2) / (B1 * B2);
}

// pass 3: tile of GE_TR x GE_TC interior output pixels (centre rows 3.., columns 3..) of one selected slice; partial sums -> part[s][tile]
template <typename TC>
__global__ __launch_bounds__(256) void ge_ssim_kernel(const TC* __restrict__ oct, const TC* __restrict__ fct, long long csr, long long csc,
                                                      long long css, int R, int C, const GeSlice* __restrict__ sl, double* __restrict__ part) {
    constexpr int IR = GE_TR + 6, IC = GE_TC + 6, LD = IC + 1;
    __shared__ double X[IR * LD], Y[IR * LD];
    __shared__ double sh[4];
    const int s = blockIdx.z;
    const GeSlice g = sl[s];
    if (!g.sel) return;
    const int r0 = blockIdx.y * GE_TR, c0 = blockIdx.x * GE_TC;          // top-left input pixel of the tile
    const TC* po = oct + (long long)s * css;
    const TC* pf = fct + (long long)s * css;
    // stage (IR x IC) inputs, lanes along the faster of rows / columns
    const bool cfast = csc <= csr;
    for (int i = threadIdx.x; i < IR * IC; i += 256) {
        const int a = cfast ? i / IC : i % IR, b = cfast ? i % IC : i / IR;   // a row, b column
        const int r = r0 + a, c = c0 + b;
        double x = 0.0, y = 0.0;
        if (r < R && c < C) { x = ge_ct(po, csr, csc, r, c); y = ge_ct(pf, csr, csc, r, c); }
        X[a * LD + b] = x; Y[a * LD + b] = y;
    }
    __syncthreads();
    const double Rg = g.gmx - g.gmn, Rp = g.pmx - g.pmn;
    const double C1g = (0.01 * Rg) * (0.01 * Rg), C2g = (0.03 * Rg) * (0.03 * Rg);
    const double C1p = (0.01 * Rp) * (0.01 * Rp), C2p = (0.03 * Rp) * (0.03 * Rp);
    const int tc = threadIdx.x & 63, tr = (threadIdx.x >> 6) * 4;        // output column tc, output rows tr..tr+3 of the tile
    const int oc = c0 + 3 + tc;                                            // centre column in the slice
    const bool patch_ok = g.x2 - g.x1 + 1 >= 7;
    double gs = 0.0, ps = 0.0;
    if (oc <= C - 4) {
        double h[10][5];
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                const double x = X[(tr + i) * LD + tc + j], y = Y[(tr + i) * LD + tc + j];
                sx += x; sy += y; sxx += x * x; syy += y * y; sxy += x * y;
            }
            h[i][0] = sx; h[i][1] = sy; h[i][2] = sxx; h[i][3] = syy; h[i][4] = sxy;
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int orow = r0 + 3 + tr + o;                              // centre row in the slice
            if (orow > R - 4) break;
            double m[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                double v = 0.0;
#pragma unroll
                for (int i = 0; i < 7; ++i) v += h[o + i][q];
                m[q] = v / 49.0;
            }
            gs += ge_S(m[0], m[1], m[2], m[3], m[4], C1g, C2g);
            if (patch_ok && orow >= g.x1 + 3 && orow <= g.x2 - 3) ps += ge_S(m[0], m[1], m[2], m[3], m[4], C1p, C2p);
        }
    }
    gs = ge_bsum(gs, sh);
    ps = ge_bsum(ps, sh);
    if (threadIdx.x == 0) {
        const long long t = ((long long)s * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        part[2 * t] = gs;
        part[2 * t + 1] = ps;
    }
}

__device__ __forceinline__ double ge_psnr(double R, double sse, double n) {
    const double err = sse / n;
    return 10.0 * log10((R * R) / err);
}

// per selected slice: SSIM means (tile partials summed in a fixed order) and both PSNRs
__global__ __launch_bounds__(256) void ge_slice_final_kernel(GeSlice* __restrict__ sl, const double* __restrict__ part, int tiles, int R, int C) {
    __shared__ double sh[4];
    const int s = blockIdx.x;
    if (!sl[s].sel) return;
    double gs = 0.0, ps = 0.0;
    for (int t = threadIdx.x; t < tiles; t += 256) {
        gs += part[2 * ((long long)s * tiles + t)];
        ps += part[2 * ((long long)s * tiles + t) + 1];
    }
    gs = ge_bsum(gs, sh);
    ps = ge_bsum(ps, sh);
    if (threadIdx.x == 0) {
        GeSlice& g = sl[s];
        const int rows = g.x2 - g.x1 + 1;
        g.ssim_g = gs / ((double)(R - 6) * (double)(C - 6));
        g.ssim_p = ps / ((double)(rows - 6) * (double)(C - 6));
        g.psnr_g = ge_psnr(g.gmx - g.gmn, g.gsse, (double)R * (double)C);
        g.psnr_p = ge_psnr(g.pmx - g.pmn, g.psse, (double)rows * (double)C);
    }
}

// out[0..3] global psnr, global ssim, patch psnr, patch ssim (np.mean over the non-NaN values, 0 if none); records [z, x1, x2, R_patch,
// R_global, psnr_patch, ssim_patch, psnr_global, ssim_global] for the slices of the 4/5 range in order, z = -1 where a slice is not evaluated.
// One block: the selected slices are read in parallel, sums by a fixed-order tree
__global__ __launch_bounds__(256) void ge_final_kernel(const GeSlice* __restrict__ sl, const GeParams* __restrict__ prm, double* __restrict__ out,
                                                       double* __restrict__ rec) {
    __shared__ double sh[4];
    const GeParams p = *prm;
    const bool ok = !p.empty && !p.shorts;
    double sum[4] = {0.0, 0.0, 0.0, 0.0}, cnt[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; ok && i < p.m; i += 256) {
        const int s = p.nz0 + i;
        const GeSlice& g = sl[s];
        if (g.sel) {
            const double v[4] = {g.psnr_g, g.ssim_g, g.psnr_p, g.ssim_p};
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (!isnan(v[q])) { sum[q] += v[q]; cnt[q] += 1.0; }
        }
        if (rec) {
            double* o = rec + (long long)GE_REC * i;
            o[0] = g.sel ? s : -1; o[1] = g.x1; o[2] = g.x2; o[3] = g.pmx - g.pmn; o[4] = g.gmx - g.gmn;
            o[5] = g.psnr_p; o[6] = g.ssim_p; o[7] = g.psnr_g; o[8] = g.ssim_g;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) { sum[q] = ge_bsum(sum[q], sh); cnt[q] = ge_bsum(cnt[q], sh); }
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) out[q] = cnt[q] > 0.0 ? sum[q] / cnt[q] : 0.0;
    out[13] = p.z0; out[14] = p.z1; out[15] = ok ? p.m : 0;
}

struct GeLayout {
    int R, C, S, K, CK, tr, tc;
    long long sr, sc, ss, lr, lc, ls;
};

GeLayout ge_layout(int H, int W, int Z, int view, long long s0, long long s1, long long s2, long long l0, long long l1, long long l2) {
    GeLayout g;
    g.R = H;
    if (view == 2) { g.C = W; g.S = Z; g.sr = s0; g.sc = s1; g.ss = s2; g.lr = l0; g.lc = l1; g.ls = l2; }
    else { g.C = Z; g.S = W; g.sr = s0; g.sc = s2; g.ss = s1; g.lr = l0; g.lc = l2; g.ls = l1; }
    // pass 1 (rows kernel): enough (pair, chunk) threads to fill the chip, at least 8 columns per chunk
    const long long pairs = (long long)((std::max(g.R, g.S) + 1) / 2) * std::min(g.R, g.S);
    int K = (int)std::min<long long>(64, std::max<long long>(1, (131072 + pairs - 1) / pairs));
    K = std::max(1, std::min(K, g.C / 8));
    g.CK = (g.C + K - 1) / K;
    g.K = (g.C + g.CK - 1) / g.CK;
    g.tr = hv_cdiv(std::max(1, g.R - 6), GE_TR);
    g.tc = hv_cdiv(std::max(1, g.C - 6), GE_TC);
    return g;
}

size_t ge_ws(const GeLayout& g) {
    const size_t cells = (size_t)g.K * g.S * g.R;
    return cells * (3 * sizeof(int) + 3 * sizeof(double)) + (size_t)g.S * sizeof(GeSlice) + sizeof(GeParams) +
           (size_t)g.S * g.tr * g.tc * 2 * sizeof(double) + 256;
}

template <typename TC, typename TL>
void ge_pass1(const void* oct, const void* fct, const void* olab, const void* flab, const GeLayout& g, double label, const GeTables& tab,
              bool cfast, int fast_is_s, bool vec, hipStream_t s) {
    const TC *o = (const TC*)oct, *f = (const TC*)fct;
    const TL *a = (const TL*)olab, *b = (const TL*)flab;
    if (cfast) {
        const dim3 grid(hv_cdiv((long long)g.S * g.R, 4));
        if (vec) hipLaunchKernelGGL((ge_rows_cfast_kernel<TC, TL, true>), grid, dim3(256), 0, s, o, f, g.sr, g.sc, g.ss, a, b, g.lr, g.lc, g.ls, g.R, g.C, g.S, label, tab);
        else hipLaunchKernelGGL((ge_rows_cfast_kernel<TC, TL, false>), grid, dim3(256), 0, s, o, f, g.sr, g.sc, g.ss, a, b, g.lr, g.lc, g.ls, g.R, g.C, g.S, label, tab);
    } else {
        const int F = fast_is_s ? g.S : g.R, O = fast_is_s ? g.R : g.S;
        const dim3 grid(hv_cdiv((long long)((F + 1) / 2) * O, 256), g.K);
        if (vec) hipLaunchKernelGGL((ge_rows_kernel<TC, TL, true>), grid, dim3(256), 0, s, o, f, g.sr, g.sc, g.ss, a, b, g.lr, g.lc, g.ls, g.R, g.C, g.S, fast_is_s, g.CK, label, tab);
        else hipLaunchKernelGGL((ge_rows_kernel<TC, TL, false>), grid, dim3(256), 0, s, o, f, g.sr, g.sc, g.ss, a, b, g.lr, g.lc, g.ls, g.R, g.C, g.S, fast_is_s, g.CK, label, tab);
    }
}

template <typename TC>
void ge_pass1_l(const void* oct, const void* fct, const void* olab, const void* flab, int label_dtype, const GeLayout& g, double label,
                const GeTables& tab, bool cfast, int fast_is_s, bool vec, hipStream_t s) {
    if (label_dtype == HV_DT_U8) ge_pass1<TC, unsigned char>(oct, fct, olab, flab, g, label, tab, cfast, fast_is_s, vec, s);
    else if (label_dtype == HV_DT_F32) ge_pass1<TC, float>(oct, fct, olab, flab, g, label, tab, cfast, fast_is_s, vec, s);
    else ge_pass1<TC, double>(oct, fct, olab, flab, g, label, tab, cfast, fast_is_s, vec, s);
}

bool ge_aligned(const void* p, size_t bytes) { return p == nullptr || ((uintptr_t)p % bytes) == 0; }

}  // namespace

extern "C" size_t hv_gen_eval_workspace_bytes(int H, int W, int Z, int view) {
    if (H <= 0 || W <= 0 || Z <= 0 || (view != 1 && view != 2)) return 0;
    return ge_ws(ge_layout(H, W, Z, view, 0, 0, 0, 0, 0, 0));
}

extern "C" int hv_gen_eval(const void* ori_ct, const void* fake_ct, int ct_dtype, long long cs0, long long cs1, long long cs2, const void* ori_seg,
                           const void* fake_seg, int label_dtype, long long ls0, long long ls1, long long ls2, int H, int W, int Z, int view,
                           double label, double* out, double* slices, void* workspace, size_t workspace_bytes, void* stream) {
    if (!ori_seg || !fake_seg || !out || H <= 0 || W <= 0 || Z <= 0 || (view != 1 && view != 2) || (!ori_ct) != (!fake_ct)) return HV_ERR_ARG;
    if ((ct_dtype != HV_DT_F32 && ct_dtype != HV_DT_F64) || (label_dtype != HV_DT_U8 && label_dtype != HV_DT_F32 && label_dtype != HV_DT_F64))
        return HV_ERR_ARG;
    const GeLayout g = ge_layout(H, W, Z, view, cs0, cs1, cs2, ls0, ls1, ls2);
    if (g.K > 65535 || g.S > 65535 || g.tr > 65535) return HV_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < ge_ws(g) || ((uintptr_t)workspace & 15)) return HV_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const size_t cells = (size_t)g.K * g.S * g.R;
    GeTables tab;
    tab.mn = (double*)ws; ws += cells * sizeof(double);
    tab.mx = (double*)ws; ws += cells * sizeof(double);
    tab.sse = (double*)ws; ws += cells * sizeof(double);
    GeSlice* sl = (GeSlice*)ws; ws += (size_t)g.S * sizeof(GeSlice);
    GeParams* prm = (GeParams*)ws; ws += sizeof(GeParams);
    double* part = (double*)ws; ws += (size_t)g.S * g.tr * g.tc * 2 * sizeof(double);
    tab.no = (int*)ws; ws += cells * sizeof(int);
    tab.nf = (int*)ws; ws += cells * sizeof(int);
    tab.ni = (int*)ws;
    const bool ct = ori_ct != nullptr;
    const size_t cb = ct_dtype == HV_DT_F64 ? 8 : 4, lb = label_dtype == HV_DT_F64 ? 8 : label_dtype == HV_DT_F32 ? 4 : 1;
    // pass 1 layout: lanes along the axis with the smallest CT stride (the label's when there is no CT)
    const long long ar = std::llabs(ct ? g.sr : g.lr), ac = std::llabs(ct ? g.sc : g.lc), as = std::llabs(ct ? g.ss : g.ls);
    const bool cfast = ac < ar && ac < as;
    const int fast_is_s = as < ar;
    // 2-wide loads: unit stride along the fast axis in both kinds of volume, and every pair start aligned to the pair's bytes
    const long long fc = cfast ? g.sc : fast_is_s ? g.ss : g.sr, fl = cfast ? g.lc : fast_is_s ? g.ls : g.lr;
    const long long oc1 = cfast ? g.sr : fast_is_s ? g.sr : g.ss, oc2 = cfast ? g.ss : g.sc;
    const long long ol1 = cfast ? g.lr : fast_is_s ? g.lr : g.ls, ol2 = cfast ? g.ls : g.lc;
    const bool vec = fl == 1 && (!ct || fc == 1) && (ol1 % 2) == 0 && (ol2 % 2) == 0 && (!ct || ((oc1 % 2) == 0 && (oc2 % 2) == 0)) &&
                     ge_aligned(ori_ct, 2 * cb) && ge_aligned(fake_ct, 2 * cb) && ge_aligned(ori_seg, 2 * lb) && ge_aligned(fake_seg, 2 * lb);
    if (ct_dtype == HV_DT_F64) ge_pass1_l<double>(ori_ct, fake_ct, ori_seg, fake_seg, label_dtype, g, label, tab, cfast, fast_is_s, vec, s);
    else ge_pass1_l<float>(ori_ct, fake_ct, ori_seg, fake_seg, label_dtype, g, label, tab, cfast, fast_is_s, vec, s);
    HV_LAUNCH_CHECK();
    hipLaunchKernelGGL(ge_slice_kernel, dim3(g.S), dim3(256), 0, s, tab, cfast ? 1 : g.K, g.R, g.S, sl);
    HV_LAUNCH_CHECK();
    hipLaunchKernelGGL(ge_select_kernel, dim3(1), dim3(256), 0, s, sl, g.R, g.C, g.S, prm, out);
    HV_LAUNCH_CHECK();
    if (!ct) return HV_OK;
    if (g.R >= 7 && g.C >= 7) {
        const dim3 grid(g.tc, g.tr, g.S);
        if (ct_dtype == HV_DT_F64)
            hipLaunchKernelGGL((ge_ssim_kernel<double>), grid, dim3(256), 0, s, (const double*)ori_ct, (const double*)fake_ct, g.sr, g.sc, g.ss, g.R, g.C, sl, part);
        else
            hipLaunchKernelGGL((ge_ssim_kernel<float>), grid, dim3(256), 0, s, (const float*)ori_ct, (const float*)fake_ct, g.sr, g.sc, g.ss, g.R, g.C, sl, part);
        HV_LAUNCH_CHECK();
        hipLaunchKernelGGL(ge_slice_final_kernel, dim3(g.S), dim3(256), 0, s, sl, part, g.tr * g.tc, g.R, g.C);
        HV_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(ge_final_kernel, dim3(1), dim3(256), 0, s, sl, prm, out, slices);
    HV_LAUNCH_CHECK();
    return HV_OK;
}
