// Generation-quality evaluation of a synthesized vertebra volume on the device (reference evaluation/generation_eval_sagittal.py:11-103 and
// generation_eval_coronal.py:11-103, process_images and the three overlap metrics, and main() :124-162, every experiment's volumes against
// the same original).
//
// A volume is seen as [R rows][C columns][S slices]: rows are axis 0, slices the view axis (2 sagittal, 1 coronal), columns the third
// axis.  Everything is float64 (-ffp-contract=off); the CT may be float32 / float64, the labels uint8 / float32 / float64.
// hv_gen_eval, one (original, synthesized) pair:
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
// hv_gen_eval_batch, N originals x E synthesized volumes each (device pointer tables), seven launches whatever N and E are.  Every kernel
// calls the __device__ functions the single-pair kernels call, so a pair's results are the same bits as hv_gen_eval's:
//   ge_rows_batch_kernel / ge_rows_cfast_batch_kernel   pass 1, grid z = (item, group of GE_EB experiments): the ori's label and CT element
//                        loaded once and kept in registers, an inner loop over the group's experiments loads the synthesized ones.  The
//                        ori-only partials (|ori|, CT min / max) are written by an item's first group, |fake|, |ori & fake| and the
//                        squared-error sum per (item, experiment).  The 2-wide loads are taken where the block's own pointers are aligned
//   ge_slice_ori_kernel  grid (S, N): |ori|, x1, x2, min / max over the slice and over rows x1..x2, once per item
//   ge_slice_exp_kernel  grid (S, N * E): |fake|, |ori & fake|, the squared-error sums over the slice and over rows x1..x2
//   ge_select_batch_kernel  grid (N): the selection once per item, then the overlap metrics and flags of each of its experiments
//   ge_ssim_batch_kernel grid (tiles, S, N): the ori tile staged in LDS and its window sums of x and x^2 formed once, then per experiment
//                        the synthesized tile staged, the sums of y, y^2, xy and both S evaluations (one ori and one synthesized tile in LDS)
//   ge_slice_final_batch_kernel  grid (S, N * E);  ge_final_batch_kernel  grid (N * E)
#include "hv_common.h"

namespace {

constexpr int GE_TC = 64;     // ssim tile: output columns
constexpr int GE_TR = 16;     // ssim tile: output rows (4 per thread)
constexpr int GE_REC = 9;     // doubles per slice record
constexpr int GE_EB = 4;      // batch pass 1: experiments that share one read of the original (their accumulators stay in registers)

struct GeSlice {
    long long no, nf, ni;              // ori, fake, ori & fake voxels of the slice
    int x1, x2, sel, pad;
    double gmn, gmx, gsse, pmn, pmx, psse;
    double psnr_p, psnr_g, ssim_p, ssim_g;
};
struct GeParams { int empty, shorts, nsel, z0, z1, nz0, m, pad; long long no, nf, ni; };
// the batch form's slice records: what depends on the original alone (one per item) and the rest (one per item and experiment)
struct GeSliceO {
    long long no;
    int x1, x2, sel, pad;
    double gmn, gmx, pmn, pmx;
};
struct GeSliceE {
    long long nf, ni;
    double gsse, psse, psnr_p, psnr_g, ssim_p, ssim_g;
};

template <typename T> __device__ __forceinline__ double ge_ld(const T* p) { return (double)*p; }
// two neighbours along a unit-stride axis, 16 / 8 / 2 bytes per lane (alignment checked by the host, in the batch form by the block)
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

// pass 1 accumulators: what the original alone decides, and what one synthesized volume adds
struct GeAccO {
    int no;
    double mn, mx;
    __device__ __forceinline__ void init() { no = 0; mn = HUGE_VAL; mx = -HUGE_VAL; }
    __device__ __forceinline__ void add(bool o, double co, bool ct) {
        no += o;
        if (ct) { mn = fmin(mn, co); mx = fmax(mx, co); }
    }
};
struct GeAccE {
    int nf, ni;
    double sse;
    __device__ __forceinline__ void init() { nf = ni = 0; sse = 0.0; }
    __device__ __forceinline__ void add(bool o, bool f, double co, double cf, bool ct) {
        nf += f; ni += o && f;
        if (ct) { const double d = co - cf; sse += d * d; }
    }
};

struct GeTables { int *no, *nf, *ni; double *mn, *mx, *sse; };
struct GeTabO { int* no; double *mn, *mx; };       // [K][S][R] of one item
struct GeTabE { int *nf, *ni; double* sse; };      // [K][S][R] of one (item, experiment)

__device__ __forceinline__ void ge_store(const GeTabO& t, long long i, const GeAccO& a) { t.no[i] = a.no; t.mn[i] = a.mn; t.mx[i] = a.mx; }
__device__ __forceinline__ void ge_store(const GeTabE& t, long long i, const GeAccE& a) { t.nf[i] = a.nf; t.ni[i] = a.ni; t.sse[i] = a.sse; }

// one original and up to EB synthesized volumes of one stride triple per kind
template <typename TC, typename TL, int EB> struct GeVols {
    const TC* oct;
    const TL* olab;
    const TC* fct[EB];
    const TL* flab[EB];
    GeTabO to;
    GeTabE te[EB];
    int ne;              // synthesized volumes in use
    bool write_ori;      // this block stores the ori-only partials
};

// pass 1, lanes along rows or slices (the faster of the two, `fast_is_s`): thread t = two neighbours along it x one index of the other
// x one chunk of CK columns (`chunk`).  Per column the ori's elements are loaded once, then each synthesized volume's
template <typename TC, typename TL, bool VEC, int EB>
__device__ __forceinline__ void ge_rows_body(const GeVols<TC, TL, EB>& v, long long csr, long long csc, long long css, long long lsr, long long lsc,
                                             long long lss, int R, int C, int S, int fast_is_s, int CK, int chunk, long long t, double label) {
    const int F = fast_is_s ? S : R, O = fast_is_s ? R : S, FP = (F + 1) >> 1;
    if (t >= (long long)FP * O) return;
    const int f0 = 2 * (int)(t % FP), o = (int)(t / FP);
    const bool two = f0 + 1 < F;
    const int r = fast_is_s ? o : f0, s = fast_is_s ? f0 : o;
    const long long cstep = fast_is_s ? css : csr, lstep = fast_is_s ? lss : lsr;
    const int c0 = chunk * CK, c1 = min(C, c0 + CK);
    const bool ct = v.oct != nullptr;
    const long long coff = (long long)r * csr + (long long)s * css, loff = (long long)r * lsr + (long long)s * lss;
    GeAccO A, B;
    GeAccE Ae[EB], Be[EB];
    A.init(); B.init();
#pragma unroll
    for (int j = 0; j < EB; ++j) { Ae[j].init(); Be[j].init(); }
#pragma unroll(EB == 1 ? 4 : 2)
    for (int c = c0; c < c1; ++c) {
        double la, lb, ca = 0.0, cb = 0.0;
        ge_pair<TL, VEC>(v.olab + loff + (long long)c * lsc, lstep, two, la, lb);
        if (ct) ge_pair<TC, VEC>(v.oct + coff + (long long)c * csc, cstep, two, ca, cb);
        const bool oa = la == label, ob = lb == label;
        A.add(oa, ca, ct);
        B.add(ob, cb, ct);
#pragma unroll
        for (int j = 0; j < EB; ++j) {
            if (j < v.ne) {
                double ma, mb, da = 0.0, db = 0.0;
                ge_pair<TL, VEC>(v.flab[j] + loff + (long long)c * lsc, lstep, two, ma, mb);
                if (ct) ge_pair<TC, VEC>(v.fct[j] + coff + (long long)c * csc, cstep, two, da, db);
                Ae[j].add(oa, ma == label, ca, da, ct);
                Be[j].add(ob, mb == label, cb, db, ct);
            }
        }
    }
    const long long ia = (long long)chunk * S * R + (long long)s * R + r;
    const long long ib = (long long)chunk * S * R + (fast_is_s ? (long long)(s + 1) * R + r : (long long)s * R + r + 1);
    if (v.write_ori) {
        ge_store(v.to, ia, A);
        if (two) ge_store(v.to, ib, B);
    }
#pragma unroll
    for (int j = 0; j < EB; ++j) {
        if (j < v.ne) {
            ge_store(v.te[j], ia, Ae[j]);
            if (two) ge_store(v.te[j], ib, Be[j]);
        }
    }
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

// pass 1, lanes along columns: a wave per (slice, row) `row`, two neighbouring columns per lane
template <typename TC, typename TL, bool VEC, int EB>
__device__ __forceinline__ void ge_rows_cfast_body(const GeVols<TC, TL, EB>& v, long long csr, long long csc, long long css, long long lsr,
                                                   long long lsc, long long lss, int R, int C, int S, long long row, int lane, double label) {
    if (row >= (long long)S * R) return;
    const int s = (int)(row / R), r = (int)(row - (long long)s * R);
    const bool ct = v.oct != nullptr;
    const long long coff = (long long)r * csr + (long long)s * css, loff = (long long)r * lsr + (long long)s * lss;
    GeAccO A;
    GeAccE Ae[EB];
    A.init();
#pragma unroll
    for (int j = 0; j < EB; ++j) Ae[j].init();
    for (int c = 2 * lane; c < C; c += 128) {
        const bool two = c + 1 < C;
        double la, lb, ca = 0.0, cb = 0.0;
        ge_pair<TL, VEC>(v.olab + loff + (long long)c * lsc, lsc, two, la, lb);
        if (ct) ge_pair<TC, VEC>(v.oct + coff + (long long)c * csc, csc, two, ca, cb);
        const bool oa = la == label, ob = lb == label;
        A.add(oa, ca, ct);
        if (two) A.add(ob, cb, ct);
#pragma unroll
        for (int j = 0; j < EB; ++j) {
            if (j < v.ne) {
                double ma, mb, da = 0.0, db = 0.0;
                ge_pair<TL, VEC>(v.flab[j] + loff + (long long)c * lsc, lsc, two, ma, mb);
                if (ct) ge_pair<TC, VEC>(v.fct[j] + coff + (long long)c * csc, csc, two, da, db);
                Ae[j].add(oa, ma == label, ca, da, ct);
                if (two) Ae[j].add(ob, mb == label, cb, db, ct);
            }
        }
    }
    A.no = ge_wsum(A.no); A.mn = ge_wmin(A.mn); A.mx = ge_wmax(A.mx);
    if (lane == 0 && v.write_ori) ge_store(v.to, row, A);
#pragma unroll
    for (int j = 0; j < EB; ++j) {
        if (j < v.ne) {
            Ae[j].nf = ge_wsum(Ae[j].nf); Ae[j].ni = ge_wsum(Ae[j].ni); Ae[j].sse = ge_wsum(Ae[j].sse);
            if (lane == 0) ge_store(v.te[j], row, Ae[j]);
        }
    }
}

template <typename TC, typename TL>
__device__ __forceinline__ GeVols<TC, TL, 1> ge_single_vols(const TC* oct, const TC* fct, const TL* olab, const TL* flab, const GeTables& tab) {
    GeVols<TC, TL, 1> v;
    v.oct = oct; v.olab = olab; v.fct[0] = fct; v.flab[0] = flab;
    v.to.no = tab.no; v.to.mn = tab.mn; v.to.mx = tab.mx;
    v.te[0].nf = tab.nf; v.te[0].ni = tab.ni; v.te[0].sse = tab.sse;
    v.ne = 1; v.write_ori = true;
    return v;
}

template <typename TC, typename TL, bool VEC>
__global__ __launch_bounds__(256) void ge_rows_kernel(const TC* __restrict__ oct, const TC* __restrict__ fct, long long csr, long long csc,
                                                      long long css, const TL* __restrict__ olab, const TL* __restrict__ flab, long long lsr,
                                                      long long lsc, long long lss, int R, int C, int S, int fast_is_s, int CK, double label,
                                                      GeTables tab) {
    ge_rows_body<TC, TL, VEC, 1>(ge_single_vols(oct, fct, olab, flab, tab), csr, csc, css, lsr, lsc, lss, R, C, S, fast_is_s, CK, blockIdx.y,
                                 (long long)blockIdx.x * 256 + threadIdx.x, label);
}

template <typename TC, typename TL, bool VEC>
__global__ __launch_bounds__(256) void ge_rows_cfast_kernel(const TC* __restrict__ oct, const TC* __restrict__ fct, long long csr, long long csc,
                                                            long long css, const TL* __restrict__ olab, const TL* __restrict__ flab, long long lsr,
                                                            long long lsc, long long lss, int R, int C, int S, double label, GeTables tab) {
    ge_rows_cfast_body<TC, TL, VEC, 1>(ge_single_vols(oct, fct, olab, flab, tab), csr, csc, css, lsr, lsc, lss, R, C, S,
                                       (long long)blockIdx.x * 4 + (threadIdx.x >> 6), threadIdx.x & 63, label);
}

// the batch call's operands: device tables of N (ori) and N * E (fake, [item * E + experiment]) volume pointers, N labels
struct GeBatch {
    const void* const* oct;
    const void* const* fct;
    const void* const* olab;
    const void* const* flab;
    const double* labels;
    int N, E, EG, pad;       // EG = groups of GE_EB experiments
    long long cells;         // pass-1 table cells of one volume (K * S * R)
};
struct GeTabsB { GeTabO to; GeTabE te; };   // item 0 / pair 0; the others follow at multiples of `cells`

// the volumes of grid z = item * EG + group; `aligned`: every pointer in use allows the 2-wide loads
template <typename TC, typename TL>
__device__ __forceinline__ GeVols<TC, TL, GE_EB> ge_batch_vols(const GeBatch& b, const GeTabsB& tabs, int z, double& label, bool& aligned) {
    const int item = z / b.EG, e0 = (z - item * b.EG) * GE_EB;
    GeVols<TC, TL, GE_EB> v;
    v.ne = min(GE_EB, b.E - e0);
    v.write_ori = e0 == 0;
    v.oct = b.oct ? (const TC*)b.oct[item] : nullptr;
    v.olab = (const TL*)b.olab[item];
    const long long io = (long long)item * b.cells;
    v.to.no = tabs.to.no + io; v.to.mn = tabs.to.mn + io; v.to.mx = tabs.to.mx + io;
    uintptr_t bits = (uintptr_t)v.oct % (2 * sizeof(TC)) | (uintptr_t)v.olab % (2 * sizeof(TL));
#pragma unroll
    for (int j = 0; j < GE_EB; ++j) {
        const long long pair = (long long)item * b.E + e0 + min(j, v.ne - 1);
        v.fct[j] = b.oct ? (const TC*)b.fct[pair] : nullptr;
        v.flab[j] = (const TL*)b.flab[pair];
        const long long ie = pair * b.cells;
        v.te[j].nf = tabs.te.nf + ie; v.te[j].ni = tabs.te.ni + ie; v.te[j].sse = tabs.te.sse + ie;
        bits |= (uintptr_t)v.fct[j] % (2 * sizeof(TC)) | (uintptr_t)v.flab[j] % (2 * sizeof(TL));
    }
    label = b.labels[item];
    aligned = bits == 0;
    return v;
}

template <typename TC, typename TL, bool VEC>
__global__ __launch_bounds__(256) void ge_rows_batch_kernel(GeBatch b, GeTabsB tabs, long long csr, long long csc, long long css, long long lsr,
                                                            long long lsc, long long lss, int R, int C, int S, int fast_is_s, int CK) {
    double label;
    bool aligned;
    const GeVols<TC, TL, GE_EB> v = ge_batch_vols<TC, TL>(b, tabs, blockIdx.z, label, aligned);
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if constexpr (VEC) {
        if (aligned) {
            ge_rows_body<TC, TL, true, GE_EB>(v, csr, csc, css, lsr, lsc, lss, R, C, S, fast_is_s, CK, blockIdx.y, t, label);
            return;
        }
    }
    ge_rows_body<TC, TL, false, GE_EB>(v, csr, csc, css, lsr, lsc, lss, R, C, S, fast_is_s, CK, blockIdx.y, t, label);
}

template <typename TC, typename TL, bool VEC>
__global__ __launch_bounds__(256) void ge_rows_cfast_batch_kernel(GeBatch b, GeTabsB tabs, long long csr, long long csc, long long css,
                                                                  long long lsr, long long lsc, long long lss, int R, int C, int S) {
    double label;
    bool aligned;
    const GeVols<TC, TL, GE_EB> v = ge_batch_vols<TC, TL>(b, tabs, blockIdx.z, label, aligned);
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if constexpr (VEC) {
        if (aligned) {
            ge_rows_cfast_body<TC, TL, true, GE_EB>(v, csr, csc, css, lsr, lsc, lss, R, C, S, row, lane, label);
            return;
        }
    }
    ge_rows_cfast_body<TC, TL, false, GE_EB>(v, csr, csc, css, lsr, lsc, lss, R, C, S, row, lane, label);
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

// pass 2 of one slice, the original's part: the chunks folded per row, |ori|, first / last row, CT min / max over the slice and over
// rows x1..x2.  Counts are below 2^53: exact as doubles.  Every thread of the block gets the result
struct GeSlO { double no, x1, x2, mn, mx, pmn, pmx; };
__device__ __forceinline__ GeSlO ge_slice_ori(const GeTabO& tab, int K, int R, int S, int s, double* sh) {
    GeSlO q;
    double no = 0.0, x1 = HUGE_VAL, x2 = -HUGE_VAL, mn = HUGE_VAL, mx = -HUGE_VAL;
    for (int r = threadIdx.x; r < R; r += 256) {
        long long o = 0;
        double rmn = HUGE_VAL, rmx = -HUGE_VAL;
        for (int k = 0; k < K; ++k) {
            const long long i = ((long long)k * S + s) * R + r;
            o += tab.no[i];
            rmn = fmin(rmn, tab.mn[i]); rmx = fmax(rmx, tab.mx[i]);
        }
        no += (double)o;
        if (o > 0) { x1 = fmin(x1, (double)r); x2 = fmax(x2, (double)r); }
        mn = fmin(mn, rmn); mx = fmax(mx, rmx);
    }
    q.no = ge_bsum(no, sh);
    q.x1 = ge_bmin(x1, sh); q.x2 = ge_bmax(x2, sh);
    q.mn = ge_bmin(mn, sh); q.mx = ge_bmax(mx, sh);
    double pmn = HUGE_VAL, pmx = -HUGE_VAL;
    if (q.no > 0.0) {
        for (int r = (int)q.x1 + threadIdx.x; r <= (int)q.x2; r += 256) {
            for (int k = 0; k < K; ++k) {
                const long long i = ((long long)k * S + s) * R + r;
                pmn = fmin(pmn, tab.mn[i]); pmx = fmax(pmx, tab.mx[i]);
            }
        }
    }
    q.pmn = ge_bmin(pmn, sh); q.pmx = ge_bmax(pmx, sh);
    return q;
}

// pass 2 of one slice, one synthesized volume's part: |fake|, |ori & fake|, the squared-error sums over the slice and over rows x1..x2
// (`patch`: the slice has an original voxel)
struct GeSlE { double nf, ni, sse, psse; };
__device__ __forceinline__ GeSlE ge_slice_exp(const GeTabE& tab, int K, int R, int S, int s, bool patch, int x1, int x2, double* sh) {
    GeSlE q;
    double nf = 0.0, ni = 0.0, sse = 0.0;
    for (int r = threadIdx.x; r < R; r += 256) {
        double rs = 0.0;
        for (int k = 0; k < K; ++k) {
            const long long i = ((long long)k * S + s) * R + r;
            nf += tab.nf[i]; ni += tab.ni[i];
            rs += tab.sse[i];
        }
        sse += rs;
    }
    q.nf = ge_bsum(nf, sh); q.ni = ge_bsum(ni, sh);
    q.sse = ge_bsum(sse, sh);
    double psse = 0.0;
    if (patch) {
        for (int r = x1 + threadIdx.x; r <= x2; r += 256) {
            for (int k = 0; k < K; ++k) psse += tab.sse[((long long)k * S + s) * R + r];
        }
    }
    q.psse = ge_bsum(psse, sh);
    return q;
}

// pass 2: one block per slice
__global__ __launch_bounds__(256) void ge_slice_kernel(GeTables tab, int K, int R, int S, GeSlice* __restrict__ sl) {
    __shared__ double sh[4];
    const int s = blockIdx.x;
    const GeTabO to = {tab.no, tab.mn, tab.mx};
    const GeTabE te = {tab.nf, tab.ni, tab.sse};
    const GeSlO o = ge_slice_ori(to, K, R, S, s, sh);
    const GeSlE e = ge_slice_exp(te, K, R, S, s, o.no > 0.0, (int)o.x1, (int)o.x2, sh);
    if (threadIdx.x == 0) {
        GeSlice& g = sl[s];
        g.no = (long long)o.no; g.nf = (long long)e.nf; g.ni = (long long)e.ni;
        g.x1 = o.no > 0.0 ? (int)o.x1 : -1; g.x2 = o.no > 0.0 ? (int)o.x2 : -1; g.sel = 0; g.pad = 0;
        g.gmn = o.mn; g.gmx = o.mx; g.gsse = e.sse; g.pmn = o.pmn; g.pmx = o.pmx; g.psse = e.psse;
        g.psnr_p = g.psnr_g = g.ssim_p = g.ssim_g = 0.0;
    }
}

__global__ __launch_bounds__(256) void ge_slice_ori_kernel(GeTabO tab, long long cells, int K, int R, int S, GeSliceO* __restrict__ so) {
    __shared__ double sh[4];
    const int s = blockIdx.x, item = blockIdx.y;
    const long long io = (long long)item * cells;
    const GeTabO to = {tab.no + io, tab.mn + io, tab.mx + io};
    const GeSlO o = ge_slice_ori(to, K, R, S, s, sh);
    if (threadIdx.x == 0) {
        GeSliceO& g = so[(long long)item * S + s];
        g.no = (long long)o.no;
        g.x1 = o.no > 0.0 ? (int)o.x1 : -1; g.x2 = o.no > 0.0 ? (int)o.x2 : -1; g.sel = 0; g.pad = 0;
        g.gmn = o.mn; g.gmx = o.mx; g.pmn = o.pmn; g.pmx = o.pmx;
    }
}

__global__ __launch_bounds__(256) void ge_slice_exp_kernel(GeTabE tab, long long cells, int E, int K, int R, int S,
                                                           const GeSliceO* __restrict__ so, GeSliceE* __restrict__ se) {
    __shared__ double sh[4];
    const int s = blockIdx.x, pair = blockIdx.y, item = pair / E;
    const long long ie = (long long)pair * cells;
    const GeTabE te = {tab.nf + ie, tab.ni + ie, tab.sse + ie};
    const GeSliceO o = so[(long long)item * S + s];
    const GeSlE e = ge_slice_exp(te, K, R, S, s, o.no > 0, o.x1, o.x2, sh);
    if (threadIdx.x == 0) {
        GeSliceE& g = se[(long long)pair * S + s];
        g.nf = (long long)e.nf; g.ni = (long long)e.ni;
        g.gsse = e.sse; g.psse = e.psse;
        g.psnr_p = g.psnr_g = g.ssim_p = g.ssim_g = 0.0;
    }
}

// the slice range and selection of one original (process_images :60-71): marks sl[].sel; every thread of the block gets the parameters
// (nf, ni left 0).  SL: GeSlice or GeSliceO
template <typename SL>
__device__ __forceinline__ GeParams ge_select_ori(SL* __restrict__ sl, int C, int S, double* sh) {
    double no = 0.0, z0 = HUGE_VAL, z1 = -HUGE_VAL;
    for (int s = threadIdx.x; s < S; s += 256) {
        const long long a = sl[s].no;
        no += (double)a;
        if (a > 0) { z0 = fmin(z0, (double)s); z1 = fmax(z1, (double)s); }
    }
    no = ge_bsum(no, sh);
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
    GeParams p = {};
    p.no = (long long)no;
    p.empty = empty; p.shorts = shorts != 0.0; p.nsel = (int)nsel;
    p.z0 = empty ? 0 : (int)z0; p.z1 = empty ? 0 : (int)z1; p.nz0 = nz0; p.m = m;
    return p;
}

// |fake| and |ori & fake| of one synthesized volume (counts below 2^53 are exact as doubles).  SE: GeSlice or GeSliceE
template <typename SE>
__device__ __forceinline__ void ge_select_exp(const SE* __restrict__ se, int S, double* sh, long long& nf, long long& ni) {
    double f = 0.0, i = 0.0;
    for (int s = threadIdx.x; s < S; s += 256) { f += (double)se[s].nf; i += (double)se[s].ni; }
    nf = (long long)ge_bsum(f, sh);
    ni = (long long)ge_bsum(i, sh);
}

// the overlap metrics (:11-37) from the exact integer counts; out[4] iou, out[5] rv_diff, out[6] dice, the flags and counts
__device__ __forceinline__ void ge_write_counts(const GeParams& p, double* __restrict__ out) {
    const long long u = p.no + p.nf - p.ni;
    out[4] = u == 0 ? 0.0 : (double)p.ni / (double)u;
    out[5] = p.no == 0 ? 0.0 : (double)(p.no > p.nf ? p.no - p.nf : p.nf - p.no) / (double)p.no;
    out[6] = p.no + p.nf == 0 ? 0.0 : 2.0 * (double)p.ni / (double)(p.no + p.nf);
    out[7] = (double)p.empty;
    out[8] = (double)p.shorts;
    out[9] = (double)p.nsel;
    out[10] = (double)p.no; out[11] = (double)p.nf; out[12] = (double)p.ni;
}

// One block: the per-slice records are read in parallel
__global__ __launch_bounds__(256) void ge_select_kernel(GeSlice* __restrict__ sl, int R, int C, int S, GeParams* __restrict__ prm,
                                                        double* __restrict__ out) {
    __shared__ double sh[4];
    GeParams p = ge_select_ori(sl, C, S, sh);
    ge_select_exp(sl, S, sh, p.nf, p.ni);
    if (threadIdx.x != 0) return;
    *prm = p;
    ge_write_counts(p, out);
}

// one block per item: the selection once, then each experiment's counts
__global__ __launch_bounds__(256) void ge_select_batch_kernel(GeSliceO* __restrict__ so, const GeSliceE* __restrict__ se, int E, int C, int S,
                                                              GeParams* __restrict__ prm, double* __restrict__ out) {
    __shared__ double sh[4];
    const int item = blockIdx.x;
    GeParams p = ge_select_ori(so + (long long)item * S, C, S, sh);
    if (threadIdx.x == 0) prm[item] = p;
    for (int e = 0; e < E; ++e) {
        const long long pair = (long long)item * E + e;
        ge_select_exp(se + pair * S, S, sh, p.nf, p.ni);
        if (threadIdx.x == 0) ge_write_counts(p, out + 16 * pair);
    }
}

template <typename TC>
__device__ __forceinline__ double ge_ct(const TC* p, long long sr, long long sc, int r, int c) { return (double)p[(long long)r * sr + (long long)c * sc]; }

__device__ __forceinline__ double ge_S(double ux, double uy, double uxx, double uyy, double uxy, double C1, double C2) {
    const double cov = 49.0 / 48.0;
    const double vx = cov * (uxx - ux * ux), vy = cov * (uyy - uy * uy), vxy = cov * (uxy - ux * uy);
    const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2, B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
    return (A1 * A2) / (B1 * B2);
}

constexpr int GE_IR = GE_TR + 6, GE_IC = GE_TC + 6, GE_LD = GE_IC + 1;   // ssim tile: input rows, input columns, LDS row pitch

// stage the (GE_IR x GE_IC) inputs of the tile whose top-left input pixel is (r0, c0), zeros outside the slice; lanes along the faster
// of rows / columns
template <typename TC>
__device__ __forceinline__ void ge_stage(const TC* __restrict__ p, long long csr, long long csc, int R, int C, int r0, int c0, double* __restrict__ X) {
    const bool cfast = csc <= csr;
    for (int i = threadIdx.x; i < GE_IR * GE_IC; i += 256) {
        const int a = cfast ? i / GE_IC : i % GE_IR, b = cfast ? i % GE_IC : i / GE_IR;   // a row, b column
        const int r = r0 + a, c = c0 + b;
        X[a * GE_LD + b] = r < R && c < C ? ge_ct(p, csr, csc, r, c) : 0.0;
    }
}

// 7x7 window mean of the horizontal sums h of 10 consecutive rows, output row o of the thread's four
__device__ __forceinline__ double ge_vwin(const double (&h)[10], int o) {
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < 7; ++i) v += h[o + i];
    return v / 49.0;
}

// the original's window means of x and x^2 at the thread's four outputs (output column tc, output rows tr..tr+3 of the tile)
struct GeWinX { double ux[4], uxx[4]; };
__device__ __forceinline__ GeWinX ge_tile_x(const double* __restrict__ X, int tr, int tc) {
    double hx[10], hxx[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        double sx = 0.0, sxx = 0.0;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const double x = X[(tr + i) * GE_LD + tc + j];
            sx += x; sxx += x * x;
        }
        hx[i] = sx; hxx[i] = sxx;
    }
    GeWinX w;
#pragma unroll
    for (int o = 0; o < 4; ++o) { w.ux[o] = ge_vwin(hx, o); w.uxx[o] = ge_vwin(hxx, o); }
    return w;
}

// SSIM constants and crop rows of one slice: all decided by the original
struct GeSsimC { double C1g, C2g, C1p, C2p; int x1, x2; bool patch_ok; };
template <typename SL> __device__ __forceinline__ GeSsimC ge_ssim_consts(const SL& g) {
    GeSsimC k;
    const double Rg = g.gmx - g.gmn, Rp = g.pmx - g.pmn;
    k.C1g = (0.01 * Rg) * (0.01 * Rg); k.C2g = (0.03 * Rg) * (0.03 * Rg);
    k.C1p = (0.01 * Rp) * (0.01 * Rp); k.C2p = (0.03 * Rp) * (0.03 * Rp);
    k.x1 = g.x1; k.x2 = g.x2;
    k.patch_ok = g.x2 - g.x1 + 1 >= 7;
    return k;
}

// one synthesized tile against the original's: window means of y, y^2 and xy, S with the slice's data range (every window) and with the
// patch's (centre rows x1 + 3 .. x2 - 3) summed over the thread's outputs that lie in the slice
__device__ __forceinline__ void ge_tile_y(const double* __restrict__ X, const double* __restrict__ Y, const GeWinX& w, int tr, int tc, int r0, int R,
                                          const GeSsimC& k, double& gs, double& ps) {
    double hy[10], hyy[10], hxy[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        double sy = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const double x = X[(tr + i) * GE_LD + tc + j], y = Y[(tr + i) * GE_LD + tc + j];
            sy += y; syy += y * y; sxy += x * y;
        }
        hy[i] = sy; hyy[i] = syy; hxy[i] = sxy;
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int orow = r0 + 3 + tr + o;                              // centre row in the slice
        if (orow > R - 4) break;
        const double uy = ge_vwin(hy, o), uyy = ge_vwin(hyy, o), uxy = ge_vwin(hxy, o);
        gs += ge_S(w.ux[o], uy, w.uxx[o], uyy, uxy, k.C1g, k.C2g);
        if (k.patch_ok && orow >= k.x1 + 3 && orow <= k.x2 - 3) ps += ge_S(w.ux[o], uy, w.uxx[o], uyy, uxy, k.C1p, k.C2p);
    }
}

// pass 3: tile of GE_TR x GE_TC interior output pixels (centre rows 3.., columns 3..) of one selected slice; partial sums -> part[s][tile]
template <typename TC>
__global__ __launch_bounds__(256) void ge_ssim_kernel(const TC* __restrict__ oct, const TC* __restrict__ fct, long long csr, long long csc,
                                                      long long css, int R, int C, const GeSlice* __restrict__ sl, double* __restrict__ part) {
    __shared__ double X[GE_IR * GE_LD], Y[GE_IR * GE_LD];
    __shared__ double sh[4];
    const int s = blockIdx.z;
    const GeSlice g = sl[s];
    if (!g.sel) return;
    const int r0 = blockIdx.y * GE_TR, c0 = blockIdx.x * GE_TC;          // top-left input pixel of the tile
    ge_stage(oct + (long long)s * css, csr, csc, R, C, r0, c0, X);
    ge_stage(fct + (long long)s * css, csr, csc, R, C, r0, c0, Y);
    __syncthreads();
    const GeSsimC k = ge_ssim_consts(g);
    const int tc = threadIdx.x & 63, tr = (threadIdx.x >> 6) * 4;        // output column tc, output rows tr..tr+3 of the tile
    double gs = 0.0, ps = 0.0;
    if (c0 + 3 + tc <= C - 4) {                                            // centre column in the slice
        const GeWinX w = ge_tile_x(X, tr, tc);
        asm volatile("" ::: "memory");   // the x tile is read again below, not kept: 70 live doubles would halve the occupancy
        ge_tile_y(X, Y, w, tr, tc, r0, R, k, gs, ps);
    }
    gs = ge_bsum(gs, sh);
    ps = ge_bsum(ps, sh);
    if (threadIdx.x == 0) {
        const long long t = ((long long)s * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        part[2 * t] = gs;
        part[2 * t + 1] = ps;
    }
}

// pass 3 of the batch form: grid (tile, slice, item), tile = row tile * tcs + column tile.  The original's tile and its two window sums
// once, then one synthesized tile at a time; partial sums -> part[pair][s][tile]
template <typename TC>
__global__ __launch_bounds__(256) void ge_ssim_batch_kernel(GeBatch b, long long csr, long long csc, long long css, int R, int C, int S, int tcs,
                                                            const GeSliceO* __restrict__ so, double* __restrict__ part) {
    __shared__ double X[GE_IR * GE_LD], Y[GE_IR * GE_LD];
    __shared__ double sh[4];
    const int s = blockIdx.y, item = blockIdx.z;
    const GeSliceO g = so[(long long)item * S + s];
    if (!g.sel) return;
    const int r0 = (blockIdx.x / tcs) * GE_TR, c0 = (blockIdx.x % tcs) * GE_TC;
    ge_stage((const TC*)b.oct[item] + (long long)s * css, csr, csc, R, C, r0, c0, X);
    __syncthreads();
    const GeSsimC k = ge_ssim_consts(g);
    const int tc = threadIdx.x & 63, tr = (threadIdx.x >> 6) * 4;
    const bool in = c0 + 3 + tc <= C - 4;
    GeWinX w = {};
    if (in) w = ge_tile_x(X, tr, tc);
    for (int e = 0; e < b.E; ++e) {
        const long long pair = (long long)item * b.E + e;
        // every thread is past its reads of the previous Y: it has been through the barriers of the sums below
        ge_stage((const TC*)b.fct[pair] + (long long)s * css, csr, csc, R, C, r0, c0, Y);
        __syncthreads();
        double gs = 0.0, ps = 0.0;
        if (in) ge_tile_y(X, Y, w, tr, tc, r0, R, k, gs, ps);
        gs = ge_bsum(gs, sh);
        ps = ge_bsum(ps, sh);
        if (threadIdx.x == 0) {
            const long long t = (pair * S + s) * gridDim.x + blockIdx.x;
            part[2 * t] = gs;
            part[2 * t + 1] = ps;
        }
    }
}

__device__ __forceinline__ double ge_psnr(double R, double sse, double n) {
    const double err = sse / n;
    return 10.0 * log10((R * R) / err);
}

// one selected slice: the tile partials part[2 * t], part[2 * t + 1] summed in a fixed order, then (thread 0) the SSIM means and both PSNRs.
// SO / SE: GeSlice, or GeSliceO and GeSliceE
template <typename SO, typename SE>
__device__ __forceinline__ void ge_slice_metrics(const SO& o, SE& e, const double* __restrict__ part, int tiles, int R, int C, double* sh) {
    double gs = 0.0, ps = 0.0;
    for (int t = threadIdx.x; t < tiles; t += 256) {
        gs += part[2 * (long long)t];
        ps += part[2 * (long long)t + 1];
    }
    gs = ge_bsum(gs, sh);
    ps = ge_bsum(ps, sh);
    if (threadIdx.x == 0) {
        const int rows = o.x2 - o.x1 + 1;
        e.ssim_g = gs / ((double)(R - 6) * (double)(C - 6));
        e.ssim_p = ps / ((double)(rows - 6) * (double)(C - 6));
        e.psnr_g = ge_psnr(o.gmx - o.gmn, e.gsse, (double)R * (double)C);
        e.psnr_p = ge_psnr(o.pmx - o.pmn, e.psse, (double)rows * (double)C);
    }
}

// per selected slice: SSIM means (tile partials summed in a fixed order) and both PSNRs
__global__ __launch_bounds__(256) void ge_slice_final_kernel(GeSlice* __restrict__ sl, const double* __restrict__ part, int tiles, int R, int C) {
    __shared__ double sh[4];
    const int s = blockIdx.x;
    if (!sl[s].sel) return;
    ge_slice_metrics(sl[s], sl[s], part + 2 * ((long long)s * tiles), tiles, R, C, sh);
}

__global__ __launch_bounds__(256) void ge_slice_final_batch_kernel(const GeSliceO* __restrict__ so, GeSliceE* __restrict__ se, int E, int S,
                                                                   const double* __restrict__ part, int tiles, int R, int C) {
    __shared__ double sh[4];
    const int s = blockIdx.x, pair = blockIdx.y, item = pair / E;
    const GeSliceO& o = so[(long long)item * S + s];
    if (!o.sel) return;
    ge_slice_metrics(o, se[(long long)pair * S + s], part + 2 * (((long long)pair * S + s) * tiles), tiles, R, C, sh);
}

// out[0..3] global psnr, global ssim, patch psnr, patch ssim (np.mean over the non-NaN values, 0 if none); records [z, x1, x2, R_patch,
// R_global, psnr_patch, ssim_patch, psnr_global, ssim_global] for the slices of the 4/5 range in order, z = -1 where a slice is not evaluated.
// One block: the selected slices are read in parallel, sums by a fixed-order tree.  SO / SE: GeSlice, or GeSliceO and GeSliceE
template <typename SO, typename SE>
__device__ __forceinline__ void ge_final(const SO* __restrict__ so, const SE* __restrict__ se, const GeParams& p, double* __restrict__ out,
                                         double* __restrict__ rec, double* sh) {
    const bool ok = !p.empty && !p.shorts;
    double sum[4] = {0.0, 0.0, 0.0, 0.0}, cnt[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; ok && i < p.m; i += 256) {
        const int s = p.nz0 + i;
        const SO& g = so[s];
        const SE& q = se[s];
        if (g.sel) {
            const double v[4] = {q.psnr_g, q.ssim_g, q.psnr_p, q.ssim_p};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (!isnan(v[j])) { sum[j] += v[j]; cnt[j] += 1.0; }
        }
        if (rec) {
            double* o = rec + (long long)GE_REC * i;
            o[0] = g.sel ? s : -1; o[1] = g.x1; o[2] = g.x2; o[3] = g.pmx - g.pmn; o[4] = g.gmx - g.gmn;
            o[5] = q.psnr_p; o[6] = q.ssim_p; o[7] = q.psnr_g; o[8] = q.ssim_g;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { sum[j] = ge_bsum(sum[j], sh); cnt[j] = ge_bsum(cnt[j], sh); }
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = cnt[j] > 0.0 ? sum[j] / cnt[j] : 0.0;
    out[13] = p.z0; out[14] = p.z1; out[15] = ok ? p.m : 0;
}

__global__ __launch_bounds__(256) void ge_final_kernel(const GeSlice* __restrict__ sl, const GeParams* __restrict__ prm, double* __restrict__ out,
                                                       double* __restrict__ rec) {
    __shared__ double sh[4];
    ge_final(sl, sl, *prm, out, rec, sh);
}

// one block per (item, experiment)
__global__ __launch_bounds__(256) void ge_final_batch_kernel(const GeSliceO* __restrict__ so, const GeSliceE* __restrict__ se,
                                                             const GeParams* __restrict__ prm, int E, int S, double* __restrict__ out,
                                                             double* __restrict__ rec) {
    __shared__ double sh[4];
    const int pair = blockIdx.x, item = pair / E;
    ge_final(so + (long long)item * S, se + (long long)pair * S, prm[item], out + 16 * (long long)pair,
             rec ? rec + (long long)pair * S * GE_REC : nullptr, sh);
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

// the batch workspace: the chunking (K, and so the summation order) is the single pair's, whatever N and E are
size_t ge_ws_batch(const GeLayout& g, size_t N, size_t E) {
    const size_t cells = (size_t)g.K * g.S * g.R, P = N * E;
    return N * cells * (sizeof(int) + 2 * sizeof(double)) + P * cells * (2 * sizeof(int) + sizeof(double)) +
           N * g.S * sizeof(GeSliceO) + P * g.S * sizeof(GeSliceE) + N * sizeof(GeParams) + P * g.S * g.tr * g.tc * 2 * sizeof(double) + 256;
}

// pass 1 layout of one stride pair: lanes along the axis with the smallest CT stride (the label's when there is no CT); `strides_vec`:
// the strides allow the 2-wide loads (unit stride along the fast axis in both kinds of volume, every pair start a multiple of 2 elements
// from the base), which the bases' alignment then decides
struct GePass1 { bool cfast, strides_vec; int fast_is_s; };
GePass1 ge_pass1_layout(const GeLayout& g, bool ct) {
    GePass1 p;
    const long long ar = std::llabs(ct ? g.sr : g.lr), ac = std::llabs(ct ? g.sc : g.lc), as = std::llabs(ct ? g.ss : g.ls);
    p.cfast = ac < ar && ac < as;
    p.fast_is_s = as < ar;
    const long long fc = p.cfast ? g.sc : p.fast_is_s ? g.ss : g.sr, fl = p.cfast ? g.lc : p.fast_is_s ? g.ls : g.lr;
    const long long oc1 = p.cfast ? g.sr : p.fast_is_s ? g.sr : g.ss, oc2 = p.cfast ? g.ss : g.sc;
    const long long ol1 = p.cfast ? g.lr : p.fast_is_s ? g.lr : g.ls, ol2 = p.cfast ? g.ls : g.lc;
    p.strides_vec = fl == 1 && (!ct || fc == 1) && (ol1 % 2) == 0 && (ol2 % 2) == 0 && (!ct || ((oc1 % 2) == 0 && (oc2 % 2) == 0));
    return p;
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

template <typename TC, typename TL>
void ge_pass1_batch(const GeBatch& b, const GeTabsB& tabs, const GeLayout& g, const GePass1& p, hipStream_t s) {
    const unsigned gz = (unsigned)b.N * b.EG;
    if (p.cfast) {
        const dim3 grid(hv_cdiv((long long)g.S * g.R, 4), 1, gz);
        if (p.strides_vec) hipLaunchKernelGGL((ge_rows_cfast_batch_kernel<TC, TL, true>), grid, dim3(256), 0, s, b, tabs, g.sr, g.sc, g.ss, g.lr, g.lc, g.ls, g.R, g.C, g.S);
        else hipLaunchKernelGGL((ge_rows_cfast_batch_kernel<TC, TL, false>), grid, dim3(256), 0, s, b, tabs, g.sr, g.sc, g.ss, g.lr, g.lc, g.ls, g.R, g.C, g.S);
    } else {
        const int F = p.fast_is_s ? g.S : g.R, O = p.fast_is_s ? g.R : g.S;
        const dim3 grid(hv_cdiv((long long)((F + 1) / 2) * O, 256), g.K, gz);
        if (p.strides_vec) hipLaunchKernelGGL((ge_rows_batch_kernel<TC, TL, true>), grid, dim3(256), 0, s, b, tabs, g.sr, g.sc, g.ss, g.lr, g.lc, g.ls, g.R, g.C, g.S, p.fast_is_s, g.CK);
        else hipLaunchKernelGGL((ge_rows_batch_kernel<TC, TL, false>), grid, dim3(256), 0, s, b, tabs, g.sr, g.sc, g.ss, g.lr, g.lc, g.ls, g.R, g.C, g.S, p.fast_is_s, g.CK);
    }
}

template <typename TC>
void ge_pass1_batch_l(int label_dtype, const GeBatch& b, const GeTabsB& tabs, const GeLayout& g, const GePass1& p, hipStream_t s) {
    if (label_dtype == HV_DT_U8) ge_pass1_batch<TC, unsigned char>(b, tabs, g, p, s);
    else if (label_dtype == HV_DT_F32) ge_pass1_batch<TC, float>(b, tabs, g, p, s);
    else ge_pass1_batch<TC, double>(b, tabs, g, p, s);
}

bool ge_aligned(const void* p, size_t bytes) { return p == nullptr || ((uintptr_t)p % bytes) == 0; }

bool ge_dtypes_ok(int ct_dtype, int label_dtype) {
    return (ct_dtype == HV_DT_F32 || ct_dtype == HV_DT_F64) && (label_dtype == HV_DT_U8 || label_dtype == HV_DT_F32 || label_dtype == HV_DT_F64);
}

}  // namespace

extern "C" size_t hv_gen_eval_workspace_bytes(int H, int W, int Z, int view) {
    if (H <= 0 || W <= 0 || Z <= 0 || (view != 1 && view != 2)) return 0;
    return ge_ws(ge_layout(H, W, Z, view, 0, 0, 0, 0, 0, 0));
}

extern "C" int hv_gen_eval(const void* ori_ct, const void* fake_ct, int ct_dtype, long long cs0, long long cs1, long long cs2, const void* ori_seg,
                           const void* fake_seg, int label_dtype, long long ls0, long long ls1, long long ls2, int H, int W, int Z, int view,
                           double label, double* out, double* slices, void* workspace, size_t workspace_bytes, void* stream) {
    if (!ori_seg || !fake_seg || !out || H <= 0 || W <= 0 || Z <= 0 || (view != 1 && view != 2) || (!ori_ct) != (!fake_ct)) return HV_ERR_ARG;
    if (!ge_dtypes_ok(ct_dtype, label_dtype)) return HV_ERR_ARG;
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
    const GePass1 p1 = ge_pass1_layout(g, ct);
    const bool cfast = p1.cfast;
    const int fast_is_s = p1.fast_is_s;
    const bool vec = p1.strides_vec && ge_aligned(ori_ct, 2 * cb) && ge_aligned(fake_ct, 2 * cb) && ge_aligned(ori_seg, 2 * lb) &&
                     ge_aligned(fake_seg, 2 * lb);
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

extern "C" size_t hv_gen_eval_batch_workspace_bytes(int H, int W, int Z, int view, int N, int E) {
    if (H <= 0 || W <= 0 || Z <= 0 || (view != 1 && view != 2) || N < 1 || E < 1) return 0;
    return ge_ws_batch(ge_layout(H, W, Z, view, 0, 0, 0, 0, 0, 0), (size_t)N, (size_t)E);
}

extern "C" int hv_gen_eval_batch(const void* const* ori_ct, const void* const* fake_ct, int ct_dtype, long long cs0, long long cs1, long long cs2,
                                 const void* const* ori_seg, const void* const* fake_seg, int label_dtype, long long ls0, long long ls1,
                                 long long ls2, int H, int W, int Z, int view, const double* labels, int N, int E, double* out, double* slices,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    if (!ori_seg || !fake_seg || !labels || !out || H <= 0 || W <= 0 || Z <= 0 || (view != 1 && view != 2) || (!ori_ct) != (!fake_ct) ||
        N < 1 || E < 1)
        return HV_ERR_ARG;
    if (!ge_dtypes_ok(ct_dtype, label_dtype)) return HV_ERR_ARG;
    const GeLayout g = ge_layout(H, W, Z, view, cs0, cs1, cs2, ls0, ls1, ls2);
    const int EG = hv_cdiv(E, GE_EB), tiles = g.tr * g.tc;
    const long long P = (long long)N * E;
    if (g.K > 65535 || g.S > 65535 || (long long)N * EG > 65535 || P > 65535) return HV_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < ge_ws_batch(g, N, E) || ((uintptr_t)workspace & 15)) return HV_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const size_t cells = (size_t)g.K * g.S * g.R;
    // doubles and records first (every size a multiple of 8 bytes), the int tables last
    GeTabsB tabs;
    tabs.to.mn = (double*)ws; ws += N * cells * sizeof(double);
    tabs.to.mx = (double*)ws; ws += N * cells * sizeof(double);
    tabs.te.sse = (double*)ws; ws += P * cells * sizeof(double);
    double* part = (double*)ws; ws += (size_t)P * g.S * tiles * 2 * sizeof(double);
    GeSliceO* so = (GeSliceO*)ws; ws += (size_t)N * g.S * sizeof(GeSliceO);
    GeSliceE* se = (GeSliceE*)ws; ws += (size_t)P * g.S * sizeof(GeSliceE);
    GeParams* prm = (GeParams*)ws; ws += (size_t)N * sizeof(GeParams);
    tabs.to.no = (int*)ws; ws += N * cells * sizeof(int);
    tabs.te.nf = (int*)ws; ws += P * cells * sizeof(int);
    tabs.te.ni = (int*)ws;
    const bool ct = ori_ct != nullptr;
    GeBatch b;
    b.oct = ori_ct; b.fct = fake_ct; b.olab = ori_seg; b.flab = fake_seg; b.labels = labels;
    b.N = N; b.E = E; b.EG = EG; b.pad = 0; b.cells = (long long)cells;
    const GePass1 p1 = ge_pass1_layout(g, ct);
    const int K = p1.cfast ? 1 : g.K;
    if (ct_dtype == HV_DT_F64) ge_pass1_batch_l<double>(label_dtype, b, tabs, g, p1, s);
    else ge_pass1_batch_l<float>(label_dtype, b, tabs, g, p1, s);
    HV_LAUNCH_CHECK();
    hipLaunchKernelGGL(ge_slice_ori_kernel, dim3(g.S, N), dim3(256), 0, s, tabs.to, b.cells, K, g.R, g.S, so);
    HV_LAUNCH_CHECK();
    hipLaunchKernelGGL(ge_slice_exp_kernel, dim3(g.S, (unsigned)P), dim3(256), 0, s, tabs.te, b.cells, E, K, g.R, g.S, so, se);
    HV_LAUNCH_CHECK();
    hipLaunchKernelGGL(ge_select_batch_kernel, dim3(N), dim3(256), 0, s, so, se, E, g.C, g.S, prm, out);
    HV_LAUNCH_CHECK();
    if (!ct) return HV_OK;
    if (g.R >= 7 && g.C >= 7) {
        const dim3 grid(tiles, g.S, N);
        if (ct_dtype == HV_DT_F64) hipLaunchKernelGGL((ge_ssim_batch_kernel<double>), grid, dim3(256), 0, s, b, g.sr, g.sc, g.ss, g.R, g.C, g.S, g.tc, so, part);
        else hipLaunchKernelGGL((ge_ssim_batch_kernel<float>), grid, dim3(256), 0, s, b, g.sr, g.sc, g.ss, g.R, g.C, g.S, g.tc, so, part);
        HV_LAUNCH_CHECK();
        hipLaunchKernelGGL(ge_slice_final_batch_kernel, dim3(g.S, (unsigned)P), dim3(256), 0, s, so, se, E, g.S, part, tiles, g.R, g.C);
        HV_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(ge_final_batch_kernel, dim3((unsigned)P), dim3(256), 0, s, so, se, prm, E, g.S, out, slices);
    HV_LAUNCH_CHECK();
    return HV_OK;
}
