// SVM grading of the RHLV features at every point of a parameter grid (reference evaluation/SVM_grading.py:21-52,63-71 and
// evaluation/SVM_grading_2.5d.py:33-59: StandardScaler on the train + test rows, SVC(kernel='linear', class_weight='balanced'),
// StratifiedKFold(5), every fold's model applied to the val rows, confusion matrix / macro F1 / precision / recall / accuracy per fold, their
// mean and variance over the folds).  All arithmetic in float64, every reduction in a fixed order: a grid point's
// results are the same bits whether it is graded alone or inside a larger grid (nothing a workgroup computes depends on G or on its place in
// the grid, and no workgroup reads what another one of the same kernel wrote).
//
//   svm_smo_kernel<F, CAP>   one workgroup per (class pair, fold, grid point): libsvm's C-SVC dual of that pair's training rows of that fold
//                            (Fan, Chen, Lin 2005: maximal violating pair, second-order choice of the second variable, ties to the lowest
//                            row; two-variable update with clipping; calculate_rho).  The scaler is fused into the staging: every workgroup
//                            computes the grid point's column means and standard deviations itself (M * F loads, L2-resident after the first
//                            of the grid point's workgroups), so there is no workspace and no kernel in front.
//   svm_vote_kernel<F>       one workgroup per (fold, grid point): pairwise decisions w.x - b of every val row, libsvm's vote, the prediction,
//                            the K x K confusion matrix (LDS integer atomics: order-free), the four scores by one lane.
//   svm_fold_stats_kernel    one thread per (grid point, score): mean and population variance over the five folds.
//   svm_fit_kernel / svm_predict_kernel / svm_features_kernel   the same grader fitted once on chosen rows, kept and applied to new rows (further
//                            down).  The staging, the solver and the row vote are device functions (svm_stage, svm_solve, svm_vote_row) that both
//                            families call: there is one body of each, so the two families give the same bits.
//
// Block size: ONE wave.  An SMO iteration is two dependent arg-reductions over the pair's rows and a two-variable update, about 40 flops per
// row (F <= 6): there is no work to hide a workgroup barrier behind, and with one wave there is none -- a barrier of a workgroup that fits a
// wave compiles to nothing, the reductions are six cross-lane steps, and a lane strip-mines rows lane, lane + 64, ...  (a few hundred rows per
// pair at the reference's table sizes: 2-6 rows per lane).  Parallelism comes from the grid: 512 grid points x 5 folds x up to 6 pairs are
// 15 360 independent waves, eight or more resident per CU.  Not measured yet against a multi-wave form.
// LDS: per row F scaled features (column-major: lanes read consecutive doubles, the broadcast of row i is conflict-free), alpha, gradient,
// signed bound (the sign is the row's y) and x.x: (F + 4) * 8 bytes.  CAP is one of 256 / 512 / 1024 / 1792 rows, the smallest that holds the
// largest pair of the call, so the resident waves per CU follow the problem size; 1792 rows x 80 B = 140 KiB of the 160 KiB a workgroup may
// declare is the cap hv_svm_grade_plan refuses beyond (HV_SVM_MAX_ROWS).
// Termination: the SMO loop ends at the KKT gap m(alpha) - M(alpha) <= tol or after max_iter iterations (a launch argument, >= 1, finite);
// nothing waits on another wave.
#include "hv_common.h"
#include <math.h>
#include <string.h>

#define SVM_FOLDS HV_SVM_FOLDS
#define SVM_MAXK HV_SVM_MAX_CLASSES
#define SVM_MAXP 6
#define SVM_MAGIC 0x53564d31
#define SVM_TAU 1e-12
#define SVM_HDR 8
// the plan (hv_svm_grade_plan): bound[5][4] doubles, then ints: header[8] = {magic, M, Mv, K, largest pair, 0, 0, 0}, present[5][4], y_tt[M] (class
// index), fold[M], y_val[Mv] (class index)
#define SVM_PLAN_INTS(M, Mv) (SVM_HDR + SVM_FOLDS * SVM_MAXK + 2 * (size_t)(M) + (size_t)(Mv))
#define SVM_PLAN_BYTES(M, Mv) (SVM_FOLDS * SVM_MAXK * sizeof(double) + ((SVM_PLAN_INTS(M, Mv) + 1) / 2) * 2 * sizeof(int))

struct SvmArgs {
    const double* xtt; const double* xval; const double* bound; const int* hdr;
    int G, M, Mv, K, P, max_iter;
    double tol;
    double* w; double* b; double* gap; int* info;
    int* pred; int* confusion; double* scores; int* unusable; double* decision;
};

__device__ __forceinline__ double svm_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double svm_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double svm_wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int svm_wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// the largest v of the wave and its row; equal values: the lowest row (idx 0x7fffffff = none)
__device__ __forceinline__ void svm_wave_argmax(double& v, int& idx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
}

// StandardScaler of one grid point by one wave: mean[c] and scale[c] (1 for a column indistinguishable from a constant, scikit-learn's
// _is_constant_feature / _handle_zeros_in_scale) over the M train + test rows; false where a feature of the train + test or of the val rows is
// not finite.  Same instructions in both kernels: the two see the same bits.
template <int F>
__device__ __forceinline__ bool svm_scaler(const double* __restrict__ xtt, int M, const double* __restrict__ xval, int Mv, int lane,
                                           double (&mean)[F], double (&scale)[F]) {
    double s[F], t[F];
#pragma unroll
    for (int c = 0; c < F; ++c) { s[c] = 0.0; t[c] = 0.0; }
    for (int k = lane; k < M; k += 64)
#pragma unroll
        for (int c = 0; c < F; ++c) s[c] += xtt[(long long)k * F + c];
    for (int k = lane; k < Mv; k += 64)
#pragma unroll
        for (int c = 0; c < F; ++c) t[c] += xval[(long long)k * F + c];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < F; ++c) {
        s[c] = svm_wave_sum(s[c]);
        t[c] = svm_wave_sum(t[c]);
        ok = ok && isfinite(s[c]) && isfinite(t[c]);
        mean[c] = s[c] / (double)M;
    }
    if (!ok) return false;
    double d1[F], d2[F];
#pragma unroll
    for (int c = 0; c < F; ++c) { d1[c] = 0.0; d2[c] = 0.0; }
    for (int k = lane; k < M; k += 64)
#pragma unroll
        for (int c = 0; c < F; ++c) {
            const double d = xtt[(long long)k * F + c] - mean[c];
            d1[c] += d;
            d2[c] += d * d;
        }
    const double eps = 2.220446049250313e-16, n = (double)M;
#pragma unroll
    for (int c = 0; c < F; ++c) {
        d1[c] = svm_wave_sum(d1[c]);
        d2[c] = svm_wave_sum(d2[c]);
        const double var = (d2[c] - d1[c] * d1[c] / n) / n;
        const double ne = n * mean[c] * eps;
        const bool constant = var <= n * eps * var + ne * ne;
        const double sd = sqrt(var);
        scale[c] = (constant || !(sd > 0.0)) ? 1.0 : sd;
        ok = ok && isfinite(var);
    }
    return ok;
}

__device__ __forceinline__ void svm_pair(int p, int K, int& a, int& b) {
    a = 0;
    int left = p;
    while (a < K - 2 && left >= K - 1 - a) { left -= K - 1 - a; ++a; }
    b = a + 1 + left;
}

__device__ __forceinline__ bool svm_plan_ok(const SvmArgs& A) {
    return A.hdr[0] == SVM_MAGIC && A.hdr[1] == A.M && A.hdr[2] == A.Mv && A.hdr[3] == A.K;
}

// Staging of one pair's problem by one wave (svm_smo_kernel and svm_fit_kernel): the rows k of X [M][F] with sel[k] != skip and class ca, then those
// of class cb (libsvm groups the rows by class: the lower class first, each class in row order), scaled, into the LDS arrays of CAP rows.
// -> the number of rows that were selected (rows past CAP are counted, not stored: the caller refuses n > CAP).
template <int F, int CAP>
__device__ __forceinline__ int svm_stage(const double* __restrict__ X, int M, const int* __restrict__ y, const int* __restrict__ sel, int skip, int ca,
                                         int cb, double bound_a, double bound_b, const double (&mean)[F], const double (&scale)[F], int lane,
                                         double* sx, double* sa, double* sg, double* sc, double* sq) {
    int n = 0;
    for (int side = 0; side < 2; ++side) {
        const int cls = side ? cb : ca;
        const double bound = side ? bound_b * -1.0 : bound_a * 1.0;
        for (int base = 0; base < M; base += 64) {
            const int k = base + lane;
            const bool take = k < M && sel[k] != skip && y[k] == cls;
            const unsigned long long mask = __ballot(take);
            const int pos = n + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
            if (take && pos < CAP) {
                double q = 0.0;
#pragma unroll
                for (int c = 0; c < F; ++c) {
                    const double v = (X[(long long)k * F + c] - mean[c]) / scale[c];
                    sx[c * CAP + pos] = v;
                    q += v * v;
                }
                sa[pos] = 0.0;
                sg[pos] = -1.0;
                sc[pos] = bound;
                sq[pos] = q;
            }
            n += __popcll(mask);
        }
    }
    return n;
}

// THE solver body (svm_smo_kernel and svm_fit_kernel): SMO over the n staged rows by one wave, then calculate_rho.  w leaves as the primal weights,
// gap as the final KKT gap, rho as libsvm's rho, iter / nsv / status as info reports them.
template <int F, int CAP>
__device__ __forceinline__ void svm_solve(double* sx, double* sa, double* sg, const double* sc, const double* sq, int n, int lane, double tol,
                                          int max_iter, double (&w)[F], double& gap, double& rho, int& iter, int& nsv, int& status) {
    __syncthreads();
#pragma unroll
    for (int c = 0; c < F; ++c) w[c] = 0.0;
    const double inf = __builtin_inf();
    for (;;) {
        // gradient of every row from w, the most violating row of I_up and the largest y G of I_low
        double gmax = -inf, gmax2 = -inf;
        int gi = 0x7fffffff;
        for (int k = lane; k < n; k += 64) {
            const double cs = sc[k], a = sa[k], C = fabs(cs);
            const bool pos = cs > 0.0;
            double d = 0.0;
#pragma unroll
            for (int c = 0; c < F; ++c) d += w[c] * sx[c * CAP + k];
            const double yg = d - (pos ? 1.0 : -1.0);          // y G = w.x - y
            sg[k] = pos ? yg : -yg;
            const bool up = pos ? a < C : a > 0.0, low = pos ? a > 0.0 : a < C;
            if (up && -yg > gmax) { gmax = -yg; gi = k; }
            if (low && yg > gmax2) gmax2 = yg;
        }
        svm_wave_argmax(gmax, gi);
        gmax2 = svm_wave_max(gmax2);
        gap = gmax + gmax2;
        if (gi == 0x7fffffff || !(gap > tol)) { status = HV_SVM_CONVERGED; break; }
        if (iter >= max_iter) { status = HV_SVM_MAX_ITER; break; }
        __syncthreads();
        const int i = gi;
        double xi[F];
#pragma unroll
        for (int c = 0; c < F; ++c) xi[c] = sx[c * CAP + i];
        const double qi = sq[i];
        // second variable: the row of I_low with the largest second-order decrease of the objective
        double best = -inf;
        int bj = 0x7fffffff;
        for (int k = lane; k < n; k += 64) {
            const double cs = sc[k], a = sa[k], C = fabs(cs);
            const bool pos = cs > 0.0;
            const bool low = pos ? a > 0.0 : a < C;
            const double diff = gmax + (pos ? sg[k] : -sg[k]);
            if (low && diff > 0.0) {
                double kij = 0.0;
#pragma unroll
                for (int c = 0; c < F; ++c) kij += xi[c] * sx[c * CAP + k];
                double quad = qi + sq[k] - 2.0 * kij;
                if (!(quad > 0.0)) quad = SVM_TAU;
                const double gain = diff * diff / quad;
                if (gain > best) { best = gain; bj = k; }
            }
        }
        svm_wave_argmax(best, bj);
        if (bj == 0x7fffffff) { status = HV_SVM_CONVERGED; break; }
        const int j = bj;
        double xj[F], kij = 0.0;
#pragma unroll
        for (int c = 0; c < F; ++c) { xj[c] = sx[c * CAP + j]; kij += xi[c] * xj[c]; }
        const double ci = fabs(sc[i]), cj = fabs(sc[j]), yi = sc[i] > 0.0 ? 1.0 : -1.0, yj = sc[j] > 0.0 ? 1.0 : -1.0;
        const double Gi = sg[i], Gj = sg[j], oi = sa[i], oj = sa[j];
        double ai = oi, aj = oj;
        double quad = qi + sq[j] - 2.0 * kij;
        if (!(quad > 0.0)) quad = SVM_TAU;
        if (yi != yj) {
            const double delta = (-Gi - Gj) / quad, diff = ai - aj;
            ai += delta;
            aj += delta;
            if (diff > 0.0) { if (aj < 0.0) { aj = 0.0; ai = diff; } }
            else { if (ai < 0.0) { ai = 0.0; aj = -diff; } }
            if (diff > ci - cj) { if (ai > ci) { ai = ci; aj = ci - diff; } }
            else { if (aj > cj) { aj = cj; ai = cj + diff; } }
        } else {
            const double delta = (Gi - Gj) / quad, sum = ai + aj;
            ai -= delta;
            aj += delta;
            if (sum > ci) { if (ai > ci) { ai = ci; aj = sum - ci; } }
            else { if (aj < 0.0) { aj = 0.0; ai = sum; } }
            if (sum > cj) { if (aj > cj) { aj = cj; ai = sum - cj; } }
            else { if (ai < 0.0) { ai = 0.0; aj = sum; } }
        }
        __syncthreads();          // every lane has read alpha_i / alpha_j (one wave: no instruction)
        if (lane == 0) { sa[i] = ai; sa[j] = aj; }
        const double ti = yi * (ai - oi), tj = yj * (aj - oj);
#pragma unroll
        for (int c = 0; c < F; ++c) w[c] += ti * xi[c] + tj * xj[c];
        ++iter;
        __syncthreads();
    }
    // calculate_rho: the mean of y G over the free rows, else the midpoint of the two bounds
    double fsum = 0.0, ub = inf, lb = -inf;
    int nfree = 0;
    for (int k = lane; k < n; k += 64) {
        const double cs = sc[k], a = sa[k], C = fabs(cs);
        const bool pos = cs > 0.0;
        const double yg = pos ? sg[k] : -sg[k];
        if (a > 0.0) ++nsv;
        if (a >= C) { if (pos) lb = fmax(lb, yg); else ub = fmin(ub, yg); }
        else if (a <= 0.0) { if (pos) ub = fmin(ub, yg); else lb = fmax(lb, yg); }
        else { ++nfree; fsum += yg; }
    }
    fsum = svm_wave_sum(fsum);
    nfree = svm_wave_sum_int(nfree);
    nsv = svm_wave_sum_int(nsv);
    ub = svm_wave_min(ub);
    lb = svm_wave_max(lb);
    rho = nfree > 0 ? fsum / (double)nfree : (ub + lb) / 2.0;
}

// THE row vote (svm_vote_kernel and svm_predict_kernel), one lane per row: scale the row, the P decisions w.x_scaled summed in column order then
// - b (NaN for a pair that was not solved), libsvm's vote -- a decision > 0 votes for the pair's lower class, the most votes win, ties to the
// lowest class, only classes present in the training rows are candidates.  -> the class index, -1 if no class is present.  decision [P], votes [K]
// and contrib [P][F] (w[p][c] * x_scaled[c], the very products the decision sums) are written where the pointer is not null.
template <int F>
__device__ __forceinline__ int svm_vote_row(const double* __restrict__ xrow, const double (&mean)[F], const double (&scale)[F], const double* sw,
                                            const double* sb, const int* sok, const int* __restrict__ present, int K, double* __restrict__ decision,
                                            int* __restrict__ votes_out, double* __restrict__ contrib) {
    const double nan = __builtin_nan("");
    double x[F];
#pragma unroll
    for (int c = 0; c < F; ++c) x[c] = (xrow[c] - mean[c]) / scale[c];
    int votes[SVM_MAXK] = {0, 0, 0, 0};
    int q = 0;
    for (int a = 0; a < K; ++a)
        for (int b = a + 1; b < K; ++b, ++q) {
            double d = nan;
            if (sok[q]) {
                d = 0.0;
#pragma unroll
                for (int c = 0; c < F; ++c) {
                    const double t = sw[q * F + c] * x[c];
                    if (contrib) contrib[q * F + c] = t;
                    d += t;
                }
                d -= sb[q];
                const int win = d > 0.0 ? a : b;
#pragma unroll
                for (int v = 0; v < SVM_MAXK; ++v) votes[v] += v == win;
            } else if (contrib) {
#pragma unroll
                for (int c = 0; c < F; ++c) contrib[q * F + c] = nan;
            }
            if (decision) decision[q] = d;
        }
    int best = -1, bv = -1;
#pragma unroll
    for (int v = 0; v < SVM_MAXK; ++v) {
        if (v < K && present[v] && votes[v] > bv) { bv = votes[v]; best = v; }
        if (votes_out && v < K) votes_out[v] = votes[v];
    }
    return best;
}

template <int F, int CAP>
__global__ __launch_bounds__(64) void svm_smo_kernel(SvmArgs A) {
    __shared__ double sx[F * CAP];
    __shared__ double sa[CAP], sg[CAP], sc[CAP], sq[CAP];
    const int lane = threadIdx.x, p = blockIdx.x, f = blockIdx.y, g = blockIdx.z;
    const long long prob = ((long long)g * SVM_FOLDS + f) * A.P + p;
    double* wout = A.w + prob * F;
    int* info = A.info + prob * 4;
    int ca, cb;
    svm_pair(p, A.K, ca, cb);
    const int* present = A.hdr + SVM_HDR + f * SVM_MAXK;
    const int* ytt = A.hdr + SVM_HDR + SVM_FOLDS * SVM_MAXK;
    const int* fold = ytt + A.M;
    const double nan = __builtin_nan("");
    int status = HV_SVM_CONVERGED, n = 0, iter = 0, nsv = 0;
    double w[F], mean[F], scale[F], gap = nan, rho = nan;
#pragma unroll
    for (int c = 0; c < F; ++c) w[c] = nan;
    bool solve = true;
    if (!svm_plan_ok(A)) { status = HV_SVM_BAD_PLAN; solve = false; }
    else if (!present[ca] || !present[cb]) { status = HV_SVM_ABSENT; solve = false; }
    else if (!svm_scaler<F>(A.xtt + (long long)g * A.M * F, A.M, A.xval + (long long)g * A.Mv * F, A.Mv, lane, mean, scale)) {
        status = HV_SVM_UNUSABLE;
        solve = false;
    }
    if (solve) {
        n = svm_stage<F, CAP>(A.xtt + (long long)g * A.M * F, A.M, ytt, fold, f, ca, cb, A.bound[f * SVM_MAXK + ca], A.bound[f * SVM_MAXK + cb], mean,
                              scale, lane, sx, sa, sg, sc, sq);
        if (n > CAP) { status = HV_SVM_BAD_PLAN; solve = false; }
    }
    if (solve) svm_solve<F, CAP>(sx, sa, sg, sc, sq, n, lane, A.tol, A.max_iter, w, gap, rho, iter, nsv, status);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < F; ++c) wout[c] = w[c];
        A.b[prob] = rho;
        A.gap[prob] = gap;
        info[0] = iter; info[1] = status; info[2] = nsv; info[3] = n;
    }
}

template <int F>
__global__ __launch_bounds__(64) void svm_vote_kernel(SvmArgs A) {
    __shared__ double sw[SVM_MAXP * F], sb[SVM_MAXP];
    __shared__ int sok[SVM_MAXP], scm[SVM_MAXK * SVM_MAXK];
    const int lane = threadIdx.x, f = blockIdx.x, g = blockIdx.y, K = A.K, P = A.P;
    const long long gf = (long long)g * SVM_FOLDS + f;
    const int* present = A.hdr + SVM_HDR + f * SVM_MAXK;
    const int* yval = A.hdr + SVM_HDR + SVM_FOLDS * SVM_MAXK + 2 * A.M;
    const double nan = __builtin_nan("");
    double mean[F], scale[F];
    bool ok = svm_plan_ok(A);
    if (ok) ok = svm_scaler<F>(A.xtt + (long long)g * A.M * F, A.M, A.xval + (long long)g * A.Mv * F, A.Mv, lane, mean, scale);
    if (lane < SVM_MAXK * SVM_MAXK) scm[lane] = 0;
    if (lane < P) {
        const int st = A.info[(gf * P + lane) * 4 + 1];
        sok[lane] = st == HV_SVM_CONVERGED || st == HV_SVM_MAX_ITER;
        sb[lane] = A.b[gf * P + lane];
        for (int c = 0; c < F; ++c) sw[lane * F + c] = A.w[(gf * P + lane) * F + c];
    }
    __syncthreads();
    if (!ok) {
        for (int r = lane; r < A.Mv; r += 64) {
            A.pred[gf * A.Mv + r] = -1;
            if (A.decision)
                for (int q = 0; q < P; ++q) A.decision[(gf * A.Mv + r) * P + q] = nan;
        }
        if (lane < K * K) A.confusion[gf * K * K + lane] = 0;
        if (lane < 4) A.scores[gf * 4 + lane] = nan;
        if (lane == 0 && f == 0) A.unusable[g] = 1;
        return;
    }
    const double* X = A.xval + (long long)g * A.Mv * F;
    for (int r = lane; r < A.Mv; r += 64) {
        const int best = svm_vote_row<F>(X + (long long)r * F, mean, scale, sw, sb, sok, present, K,
                                         A.decision ? A.decision + (gf * A.Mv + r) * P : nullptr, nullptr, nullptr);
        A.pred[gf * A.Mv + r] = best;
        const int t = yval[r];
        if (best >= 0 && t >= 0 && t < K) atomicAdd(&scm[t * K + best], 1);
    }
    __syncthreads();
    if (lane < K * K) A.confusion[gf * K * K + lane] = scm[lane];
    if (lane == 0) {
        // macro scores over the classes that occur among the true or the predicted labels; an empty denominator contributes 0
        double f1 = 0.0, prec = 0.0, rec = 0.0;
        int used = 0, hit = 0, total = 0;
        for (int c = 0; c < K; ++c) {
            int nt = 0, np = 0;
            for (int o = 0; o < K; ++o) { nt += scm[c * K + o]; np += scm[o * K + c]; }
            const int tp = scm[c * K + c];
            hit += tp;
            total += nt;
            if (nt + np == 0) continue;
            ++used;
            f1 += 2.0 * (double)tp / (double)(nt + np);
            if (np > 0) prec += (double)tp / (double)np;
            if (nt > 0) rec += (double)tp / (double)nt;
        }
        double* s = A.scores + gf * 4;
        s[0] = used ? f1 / (double)used : nan;
        s[1] = used ? prec / (double)used : nan;
        s[2] = used ? rec / (double)used : nan;
        s[3] = total ? (double)hit / (double)total : nan;
        if (f == 0) A.unusable[g] = 0;
    }
}

__global__ __launch_bounds__(64) void svm_fold_stats_kernel(const double* __restrict__ scores, double* __restrict__ mean, double* __restrict__ var,
                                                            long long n) {
    const long long t = (long long)blockIdx.x * 64 + threadIdx.x;
    if (t >= n) return;
    const long long g = t >> 2;
    const int s = (int)(t & 3);
    double v[SVM_FOLDS], m = 0.0, q = 0.0;
#pragma unroll
    for (int f = 0; f < SVM_FOLDS; ++f) { v[f] = scores[(g * SVM_FOLDS + f) * 4 + s]; m += v[f]; }
    m /= (double)SVM_FOLDS;
#pragma unroll
    for (int f = 0; f < SVM_FOLDS; ++f) q += (v[f] - m) * (v[f] - m);
    mean[t] = m;
    var[t] = q / (double)SVM_FOLDS;
}

extern "C" size_t hv_svm_grade_plan_bytes(int M, int Mv) {
    if (M <= 0 || Mv <= 0) return 0;
    return SVM_PLAN_BYTES(M, Mv);
}

extern "C" int hv_svm_grade_plan(const int* y_tt, const int* fold, int M, const int* y_val, int Mv, const int* classes, int K, void* plan,
                                 size_t plan_bytes, int* max_rows) {
    if (!y_tt || !fold || !y_val || !classes || !plan || !max_rows || M <= 0 || Mv <= 0) return HV_ERR_ARG;
    if (K < 2 || K > SVM_MAXK) return HV_ERR_UNSUPPORTED;
    if (plan_bytes < SVM_PLAN_BYTES(M, Mv)) return HV_ERR_WORKSPACE;
    for (int c = 0; c < K; ++c)
        if (classes[c] < 0 || (c && classes[c] <= classes[c - 1])) return HV_ERR_ARG;
    memset(plan, 0, SVM_PLAN_BYTES(M, Mv));
    double* bound = (double*)plan;
    int* hdr = (int*)(bound + SVM_FOLDS * SVM_MAXK);
    int* present = hdr + SVM_HDR;
    int* ytt = present + SVM_FOLDS * SVM_MAXK;
    int* fo = ytt + M;
    int* yv = fo + M;
    auto index = [&](int label) { for (int c = 0; c < K; ++c) if (classes[c] == label) return c; return -1; };
    int count[SVM_FOLDS][SVM_MAXK] = {};
    for (int k = 0; k < M; ++k) {
        const int c = index(y_tt[k]);
        if (c < 0 || fold[k] < 0 || fold[k] >= SVM_FOLDS) return HV_ERR_ARG;
        ytt[k] = c;
        fo[k] = fold[k];
        for (int f = 0; f < SVM_FOLDS; ++f)
            if (f != fold[k]) ++count[f][c];
    }
    for (int k = 0; k < Mv; ++k) {
        const int c = index(y_val[k]);
        if (c < 0) return HV_ERR_ARG;
        yv[k] = c;
    }
    int largest = 0;
    for (int f = 0; f < SVM_FOLDS; ++f) {
        int n = 0, ncls = 0;
        for (int c = 0; c < K; ++c) { n += count[f][c]; ncls += count[f][c] > 0; }
        for (int c = 0; c < K; ++c) {
            present[f * SVM_MAXK + c] = count[f][c] > 0;
            // class_weight='balanced' with C = 1: n_train / (n_classes_in_train * count(class))
            bound[f * SVM_MAXK + c] = count[f][c] > 0 ? (double)n / ((double)ncls * (double)count[f][c]) : 0.0;
            for (int d = c + 1; d < K; ++d)
                if (count[f][c] > 0 && count[f][d] > 0 && count[f][c] + count[f][d] > largest) largest = count[f][c] + count[f][d];
        }
    }
    *max_rows = largest;
    if (largest > HV_SVM_MAX_ROWS) return HV_ERR_UNSUPPORTED;
    hdr[0] = SVM_MAGIC; hdr[1] = M; hdr[2] = Mv; hdr[3] = K; hdr[4] = largest;
    return HV_OK;
}

extern "C" int hv_svm_grade_grid(const double* X_tt, const double* X_val, const void* plan, int G, int M, int Mv, int F, int K, int max_rows,
                                 double tol, int max_iter, double* w, double* b, double* gap, int* info, int* pred, int* confusion,
                                 double* scores, double* mean, double* var, int* unusable, double* decision, void* stream) {
    if (!X_tt || !X_val || !plan || !w || !b || !gap || !info || !pred || !confusion || !scores || !mean || !var || !unusable || G <= 0 ||
        M <= 0 || Mv <= 0 || max_rows < 0 || max_iter < 1 || !(tol > 0.0))
        return HV_ERR_ARG;
    if ((F != 3 && F != 6) || K < 2 || K > SVM_MAXK || max_rows > HV_SVM_MAX_ROWS || G > 65535) return HV_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    SvmArgs A;
    A.xtt = X_tt; A.xval = X_val;
    A.bound = (const double*)plan;
    A.hdr = (const int*)(A.bound + SVM_FOLDS * SVM_MAXK);
    A.G = G; A.M = M; A.Mv = Mv; A.K = K; A.P = K * (K - 1) / 2; A.max_iter = max_iter; A.tol = tol;
    A.w = w; A.b = b; A.gap = gap; A.info = info; A.pred = pred; A.confusion = confusion; A.scores = scores; A.unusable = unusable;
    A.decision = decision;
    const dim3 grid(A.P, SVM_FOLDS, G);
#define SVM_RUN(FF, CAP) hipLaunchKernelGGL((svm_smo_kernel<FF, CAP>), grid, dim3(64), 0, s, A)
#define SVM_CAPS(FF) do { if (max_rows <= 256) SVM_RUN(FF, 256); else if (max_rows <= 512) SVM_RUN(FF, 512); \
                          else if (max_rows <= 1024) SVM_RUN(FF, 1024); else SVM_RUN(FF, HV_SVM_MAX_ROWS); } while (0)
    if (F == 3) SVM_CAPS(3); else SVM_CAPS(6);
#undef SVM_CAPS
#undef SVM_RUN
    HV_LAUNCH_CHECK();
    if (F == 3) hipLaunchKernelGGL(svm_vote_kernel<3>, dim3(SVM_FOLDS, G), dim3(64), 0, s, A);
    else hipLaunchKernelGGL(svm_vote_kernel<6>, dim3(SVM_FOLDS, G), dim3(64), 0, s, A);
    HV_LAUNCH_CHECK();
    const long long n = (long long)G * 4;
    hipLaunchKernelGGL(svm_fold_stats_kernel, dim3(hv_cdiv(n, 64)), dim3(64), 0, s, (const double*)scores, mean, var, n);
    HV_LAUNCH_CHECK();
    return HV_OK;
}

// ---------------------------------------------------------------- fit at a chosen setting, keep the model, grade new rows
//   svm_fit_kernel<F, CAP>   one wave per (class pair, grid point): svm_scaler over ALL M rows of the grid point (the reference scales before it
//                            splits), svm_stage of the rows with train[k] != 0, svm_solve -- the grading kernels' own bodies, so a fit on the rows
//                            `fold != f` is bit for bit svm_smo_kernel's problem of fold f.  The pair-0 wave also writes the grid point's scaler.
//   svm_predict_kernel<F>    one lane per row, 256-lane blocks, the grid point's model staged in LDS once per block; svm_vote_row per row.  No
//                            atomics, no cross-lane traffic, no workspace: a row's outputs depend on that row and the model alone.
//   svm_features_kernel      hv_rhlv_views_batch's records -> the feature rows, one lane per row.
// the fit plan (hv_svm_fit_plan): bound[4] doubles, then ints: header[8] = {magic, M, K, largest pair, 0, 0, 0, 0}, present[4], y[M] (class index),
// train[M] (0 / 1)
#define SVM_FIT_MAGIC 0x53564d32
#define SVM_FIT_PLAN_INTS(M) (SVM_HDR + SVM_MAXK + 2 * (size_t)(M))
#define SVM_FIT_PLAN_BYTES(M) (SVM_MAXK * sizeof(double) + ((SVM_FIT_PLAN_INTS(M) + 1) / 2) * 2 * sizeof(int))

struct SvmFitArgs {
    const double* x; const double* bound; const int* hdr;
    int G, M, K, P, max_iter;
    double tol;
    double* mean; double* scale; double* w; double* b; double* gap; int* info;
};

template <int F, int CAP>
__global__ __launch_bounds__(64) void svm_fit_kernel(SvmFitArgs A) {
    __shared__ double sx[F * CAP];
    __shared__ double sa[CAP], sg[CAP], sc[CAP], sq[CAP];
    const int lane = threadIdx.x, p = blockIdx.x, g = blockIdx.z;
    const long long prob = (long long)g * A.P + p;
    int ca, cb;
    svm_pair(p, A.K, ca, cb);
    const int* present = A.hdr + SVM_HDR;
    const int* y = present + SVM_MAXK;
    const int* train = y + A.M;
    const double* X = A.x + (long long)g * A.M * F;
    const double nan = __builtin_nan("");
    int status = HV_SVM_CONVERGED, n = 0, iter = 0, nsv = 0;
    double w[F], mean[F], scale[F], gap = nan, rho = nan;
#pragma unroll
    for (int c = 0; c < F; ++c) w[c] = nan;
    bool solve = true, scaled = false;
    if (!(A.hdr[0] == SVM_FIT_MAGIC && A.hdr[1] == A.M && A.hdr[2] == A.K)) { status = HV_SVM_BAD_PLAN; solve = false; }
    else if (!(scaled = svm_scaler<F>(X, A.M, X, 0, lane, mean, scale))) { status = HV_SVM_UNUSABLE; solve = false; }
    else if (!present[ca] || !present[cb]) { status = HV_SVM_ABSENT; solve = false; }
    if (solve) {
        n = svm_stage<F, CAP>(X, A.M, y, train, 0, ca, cb, A.bound[ca], A.bound[cb], mean, scale, lane, sx, sa, sg, sc, sq);
        if (n > CAP) { status = HV_SVM_BAD_PLAN; solve = false; }
    }
    if (solve) svm_solve<F, CAP>(sx, sa, sg, sc, sq, n, lane, A.tol, A.max_iter, w, gap, rho, iter, nsv, status);
    if (lane == 0) {
        int* info = A.info + prob * 4;
#pragma unroll
        for (int c = 0; c < F; ++c) A.w[prob * F + c] = w[c];
        A.b[prob] = rho;
        A.gap[prob] = gap;
        info[0] = iter; info[1] = status; info[2] = nsv; info[3] = n;
        if (p == 0) {
#pragma unroll
            for (int c = 0; c < F; ++c) {
                A.mean[(long long)g * F + c] = scaled ? mean[c] : nan;
                A.scale[(long long)g * F + c] = scaled ? scale[c] : nan;
            }
        }
    }
}

struct SvmPredictArgs {
    const double* x; const int* present; const double* mean; const double* scale; const double* w; const double* b; const int* info;
    int G, N, K, P;
    int* pred; double* decision; int* votes; double* contrib;
};

template <int F>
__global__ __launch_bounds__(256) void svm_predict_kernel(SvmPredictArgs A) {
    __shared__ double sw[SVM_MAXP * F], sb[SVM_MAXP], sms[2 * F];
    __shared__ int sok[SVM_MAXP], spresent[SVM_MAXK], sbad;
    const int t = threadIdx.x, g = blockIdx.y, K = A.K, P = A.P;
    if (t == 0) sbad = 0;
    __syncthreads();
    if (t < P * F) sw[t] = A.w[(long long)g * P * F + t];
    if (t < 2 * F) sms[t] = t < F ? A.mean[(long long)g * F + t] : A.scale[(long long)g * F + t - F];
    if (t < SVM_MAXK) spresent[t] = t < K ? A.present[t] : 0;
    if (t < P) {
        const int st = A.info[((long long)g * P + t) * 4 + 1];
        sok[t] = st == HV_SVM_CONVERGED || st == HV_SVM_MAX_ITER;
        sb[t] = A.b[(long long)g * P + t];
        if (st == HV_SVM_UNUSABLE || st == HV_SVM_BAD_PLAN) sbad = 1;          // every writer stores the same value
    }
    __syncthreads();
    const long long r = (long long)blockIdx.x * 256 + t;
    if (r >= A.N) return;
    const double nan = __builtin_nan("");
    const double* xrow = A.x + ((long long)g * A.N + r) * F;
    const long long row = (long long)g * A.N + r;
    double mean[F], scale[F];
    bool ok = !sbad;
#pragma unroll
    for (int c = 0; c < F; ++c) {
        mean[c] = sms[c];
        scale[c] = sms[F + c];
        ok = ok && isfinite(xrow[c]) && isfinite(mean[c]) && isfinite(scale[c]);
    }
    double* dec = A.decision ? A.decision + row * P : nullptr;
    int* votes = A.votes ? A.votes + row * K : nullptr;
    double* contrib = A.contrib ? A.contrib + row * P * F : nullptr;
    if (!ok) {
        A.pred[row] = -1;
        if (dec) for (int q = 0; q < P; ++q) dec[q] = nan;
        if (votes) for (int v = 0; v < K; ++v) votes[v] = 0;
        if (contrib) for (int q = 0; q < P * F; ++q) contrib[q] = nan;
        return;
    }
    A.pred[row] = svm_vote_row<F>(xrow, mean, scale, sw, sb, sok, spresent, K, dec, votes, contrib);
}

// records [N][2][16] -> X [N][F]: columns 1..3 (Pre / Mid / Post RHLV) of view `first` (0 sagittal, 1 coronal), with F = 6 then the other view's.
// The row is NaN where the original lacks the vertebra (sagittal [13] == 0) or the coronal script would have raised (coronal [14] != 0).
__global__ __launch_bounds__(256) void svm_features_kernel(const double* __restrict__ records, long long N, int first, int F, double* __restrict__ X) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    const double* rec = records + r * 32;
    const bool bad = rec[13] == 0.0 || rec[16 + 14] != 0.0;
    const double nan = __builtin_nan("");
    for (int c = 0; c < F; ++c) {
        const int view = c < 3 ? first : 1 - first;
        X[r * F + c] = bad ? nan : rec[view * 16 + 1 + c % 3];
    }
}

extern "C" size_t hv_svm_fit_plan_bytes(int M) {
    if (M <= 0) return 0;
    return SVM_FIT_PLAN_BYTES(M);
}

extern "C" int hv_svm_fit_plan(const int* y, const int* train, int M, const int* classes, int K, void* plan, size_t plan_bytes, int* max_rows) {
    if (!y || !classes || !plan || !max_rows || M <= 0) return HV_ERR_ARG;
    if (K < 2 || K > SVM_MAXK) return HV_ERR_UNSUPPORTED;
    if (plan_bytes < SVM_FIT_PLAN_BYTES(M)) return HV_ERR_WORKSPACE;
    for (int c = 0; c < K; ++c)
        if (classes[c] < 0 || (c && classes[c] <= classes[c - 1])) return HV_ERR_ARG;
    auto index = [&](int label) { for (int c = 0; c < K; ++c) if (classes[c] == label) return c; return -1; };
    // every check first: a refusal leaves the plan as it was
    int count[SVM_MAXK] = {};
    for (int k = 0; k < M; ++k) {
        const int c = index(y[k]);
        if (c < 0) return HV_ERR_ARG;
        if (!train || train[k] != 0) ++count[c];
    }
    int n = 0, ncls = 0, largest = 0;
    for (int c = 0; c < K; ++c) { n += count[c]; ncls += count[c] > 0; }
    for (int c = 0; c < K; ++c)
        for (int d = c + 1; d < K; ++d)
            if (count[c] > 0 && count[d] > 0 && count[c] + count[d] > largest) largest = count[c] + count[d];
    *max_rows = largest;
    if (largest > HV_SVM_MAX_ROWS) return HV_ERR_UNSUPPORTED;
    memset(plan, 0, SVM_FIT_PLAN_BYTES(M));
    double* bound = (double*)plan;
    int* hdr = (int*)(bound + SVM_MAXK);
    int* present = hdr + SVM_HDR;
    int* yi = present + SVM_MAXK;
    int* tr = yi + M;
    for (int c = 0; c < K; ++c) {
        present[c] = count[c] > 0;
        // class_weight='balanced' with C = 1: n_train / (n_classes_in_train * count(class))
        bound[c] = count[c] > 0 ? (double)n / ((double)ncls * (double)count[c]) : 0.0;
    }
    for (int k = 0; k < M; ++k) {
        yi[k] = index(y[k]);
        tr[k] = !train || train[k] != 0;
    }
    hdr[0] = SVM_FIT_MAGIC; hdr[1] = M; hdr[2] = K; hdr[3] = largest;
    return HV_OK;
}

extern "C" int hv_svm_fit(const double* X, const void* plan, int G, int M, int F, int K, int max_rows, double tol, int max_iter, double* mean,
                          double* scale, double* w, double* b, double* gap, int* info, void* stream) {
    if (!X || !plan || !mean || !scale || !w || !b || !gap || !info || G <= 0 || M <= 0 || max_rows < 0 || max_iter < 1 || !(tol > 0.0))
        return HV_ERR_ARG;
    if ((F != 3 && F != 6) || K < 2 || K > SVM_MAXK || max_rows > HV_SVM_MAX_ROWS || G > 65535) return HV_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    SvmFitArgs A;
    A.x = X;
    A.bound = (const double*)plan;
    A.hdr = (const int*)(A.bound + SVM_MAXK);
    A.G = G; A.M = M; A.K = K; A.P = K * (K - 1) / 2; A.max_iter = max_iter; A.tol = tol;
    A.mean = mean; A.scale = scale; A.w = w; A.b = b; A.gap = gap; A.info = info;
    const dim3 grid(A.P, 1, G);
#define SVM_RUN(FF, CAP) hipLaunchKernelGGL((svm_fit_kernel<FF, CAP>), grid, dim3(64), 0, s, A)
#define SVM_CAPS(FF) do { if (max_rows <= 256) SVM_RUN(FF, 256); else if (max_rows <= 512) SVM_RUN(FF, 512); \
                          else if (max_rows <= 1024) SVM_RUN(FF, 1024); else SVM_RUN(FF, HV_SVM_MAX_ROWS); } while (0)
    if (F == 3) SVM_CAPS(3); else SVM_CAPS(6);
#undef SVM_CAPS
#undef SVM_RUN
    HV_LAUNCH_CHECK();
    return HV_OK;
}

extern "C" int hv_svm_predict(const double* X, int G, int N, int F, int K, const int* present, const double* mean, const double* scale, const double* w,
                              const double* b, const int* info, int* pred, double* decision, int* votes, double* contrib, void* stream) {
    if (!X || !present || !mean || !scale || !w || !b || !info || !pred || G <= 0 || N <= 0) return HV_ERR_ARG;
    if ((F != 3 && F != 6) || K < 2 || K > SVM_MAXK || G > 65535) return HV_ERR_UNSUPPORTED;
    SvmPredictArgs A;
    A.x = X; A.present = present; A.mean = mean; A.scale = scale; A.w = w; A.b = b; A.info = info;
    A.G = G; A.N = N; A.K = K; A.P = K * (K - 1) / 2;
    A.pred = pred; A.decision = decision; A.votes = votes; A.contrib = contrib;
    const dim3 grid((unsigned)hv_cdiv((long long)N, 256), G);
    if (F == 3) hipLaunchKernelGGL(svm_predict_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, A);
    else hipLaunchKernelGGL(svm_predict_kernel<6>, grid, dim3(256), 0, (hipStream_t)stream, A);
    HV_LAUNCH_CHECK();
    return HV_OK;
}

extern "C" int hv_svm_features(const double* records, int N, int first_view, int F, double* X, void* stream) {
    if (!records || !X || N <= 0 || first_view < 0 || first_view > 1) return HV_ERR_ARG;
    if (F != 3 && F != 6) return HV_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(svm_features_kernel, dim3((unsigned)hv_cdiv((long long)N, 256)), dim3(256), 0, (hipStream_t)stream, records, (long long)N,
                       first_view, F, X);
    HV_LAUNCH_CHECK();
    return HV_OK;
}
