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
        // the pair's training rows of this fold, the lower class first (libsvm groups the rows by class), each class in row order
        const double* X = A.xtt + (long long)g * A.M * F;
        for (int side = 0; side < 2; ++side) {
            const int cls = side ? cb : ca;
            const double bound = A.bound[f * SVM_MAXK + cls] * (side ? -1.0 : 1.0);
            for (int base = 0; base < A.M; base += 64) {
                const int k = base + lane;
                const bool take = k < A.M && fold[k] != f && ytt[k] == cls;
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
        if (n > CAP) { status = HV_SVM_BAD_PLAN; solve = false; }
    }
    if (solve) {
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
            if (gi == 0x7fffffff || !(gap > A.tol)) { status = HV_SVM_CONVERGED; break; }
            if (iter >= A.max_iter) { status = HV_SVM_MAX_ITER; break; }
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
        double x[F];
#pragma unroll
        for (int c = 0; c < F; ++c) x[c] = (X[(long long)r * F + c] - mean[c]) / scale[c];
        int votes[SVM_MAXK] = {0, 0, 0, 0};
        int q = 0;
        for (int a = 0; a < K; ++a)
            for (int b = a + 1; b < K; ++b, ++q) {
                double d = nan;
                if (sok[q]) {
                    d = 0.0;
#pragma unroll
                    for (int c = 0; c < F; ++c) d += sw[q * F + c] * x[c];
                    d -= sb[q];
                    const int win = d > 0.0 ? a : b;
#pragma unroll
                    for (int v = 0; v < SVM_MAXK; ++v) votes[v] += v == win;
                }
                if (A.decision) A.decision[(gf * A.Mv + r) * P + q] = d;
            }
        int best = -1, bv = -1;
#pragma unroll
        for (int v = 0; v < SVM_MAXK; ++v)
            if (v < K && present[v] && votes[v] > bv) { bv = votes[v]; best = v; }
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
