// Relative height loss value (RHLV) of a generated vs the original vertebra label volume, on the device, in the sagittal view
// (reference evaluation/RHLV_quantification.py:41-147 and the per-vertebra body of process_datasets_to_excel :160-178), the coronal view
// (evaluation/RHLV_quantification_coronal.py, same lines) or both from one pass over the volumes (the six features of SVM_grading_2.5d.py).
//
// Integer / HBM-byte work: both volumes are read once into the column-count table both views start from, everything after that is a few KB.
//   rhlv_counts_kernel   grid (Z, 2, N): cnt[v][z][w] = #{h : vol_v[h][w][z] == label_index}, tot[v][z]   (lanes along w; a z-fastest
//                        variant with lanes along z serves the reference's [H][W][Z] arrays)
//   rhlv_tot_kernel      grid (S, 2, N): voxels per slice of one view from the table (coronal: slice w = sum over z; sagittal after the z-fastest counts)
//   rhlv_range_kernel    grid (1, views, N): slice extent of the original vertebra -> centre, half-length -> [lo, hi) (numpy slice rules)
//   rhlv_slice_kernel    grid (S, views, N): thirds of the generated vertebra's column extent, centre columns, rescale ratios,
//                        thresholded integer sums per (all | pre | mid | post) x (generated | original)
//   rhlv_final_kernel    grid (1, views, N): means over the slices, the four RHLVs and the relative height of the original
// and, for the hv_rhlv_maps entries only, the per-column picture those numbers are folded from (two more launches, any views and pairs):
//   rhlv_map_kernel      grid (S, views, N): one row per slice of the whole-slice ("all") heights and what was selected from them
//   rhlv_profile_kernel  grid (ceil((S + C) / 256), views, N): one lane per column / per slice, the selected heights averaged along the other axis
// A view (RhlvView) is a way to walk the one table: the sagittal view takes slices z with columns w, the coronal view slices w with columns z
// (read strided: the table is at most 2*Z*W ints), and each carries its script's ratio arithmetic.  N > 1 is the batched form: blockIdx.z
// picks the volume pair and its slab of the workspace.
// All floating-point steps are doubles in the reference's operation order (-ffp-contract=off); the only deviation is that a
// slice's selected heights are summed as integers and scaled once (sum(c)*r instead of sum(c*r)): ~1e-16 relative.
//
// A map row (slice s of a view, column c), from the slice's RhlvMapRec {ratio_all, thr_f, thr_l, t1, t2, on}:
//   height_fake[s][c]  = cnt_fake[s][c] * ratio_all          (all_height_fake * all_scale_ratio, :93)
//   height_label[s][c] = cnt_label[s][c]                     (:70)
//   flags[s][c]        = region (bits 0-1: 0 pre c < t1, 1 mid c < t2, 2 post) | sel_f << 2 | sel_l << 3 | 1 << 4 (the script visits the slice),
//                        sel_f = height_fake > thr_f (:99), sel_l = height_label > thr_l (:100)
//   loss[s][c]         = (height_fake - height_label) / (height_fake + 1e-6) where sel_f, else NaN    (:139 per column)
// A slice the script does not visit (outside [lo, hi), or empty in either volume) is a row of NaN losses, zero heights and zero flags.
// A profile is {sum of selected height_fake / their number, the same of height_label, (pf - pl) / (pf + 1e-6)}, NaN where nothing is
// selected; each lane walks its slices or columns in ascending order and recomputes the heights from the table, so the profiles do not
// depend on which maps were asked for, on the launch shape or on the batch.
#include "hv_common.h"

struct RhlvRec { double ratio[4]; long long Sf[4], nf[4], Sl[4], nl[4], raises; };
struct RhlvMapRec { double ratio, thr_f, thr_l; int t1, t2, on, pad; };   // what rhlv_map_kernel / rhlv_profile_kernel need of a slice

struct RhlvView {
    int S, C;                  // slices, columns per slice
    int ss, sc;                // element strides of a slice / a column in one volume's table cnt[Z][W]
    int coronal;               // the coronal script's ratios (no epsilon) and its max() of an empty third
    int divisor, lo, hi;       // lo == INT_MIN: [lo, hi) from the original vertebra's extent and length_divisor
    double thr;
    long long tot, params, recs;   // byte offsets into a pair's workspace slab: tot[2][S], params[8], recs[S]
};
struct RhlvPlan {
    RhlvView view[2];
    int nviews, W, Z;
    long long cnt, pair_bytes;     // byte offset of cnt[2][Z][W]; size of one pair's slab
    long long maprecs[2];          // per view: byte offset of RhlvMapRec[S] (the hv_rhlv_maps entries only)
};

__device__ __forceinline__ char* rhlv_slab(char* ws, const RhlvPlan& P) { return ws + (long long)blockIdx.z * P.pair_bytes; }
// volume v (0 generated, 1 original) of pair blockIdx.z: from the device table of pointer pairs, or the single pair passed by value
template <typename T>
__device__ __forceinline__ const T* rhlv_volume_ptr(const T* fake, const T* label, const void* const* pairs, int v) {
    return pairs ? (const T*)pairs[2 * (long long)blockIdx.z + v] : (v == 0 ? fake : label);
}

template <typename T>
__global__ __launch_bounds__(256) void rhlv_counts_kernel(const T* __restrict__ fake, const T* __restrict__ label, const void* const* __restrict__ pairs,
                                                          const float* __restrict__ label_indices, long long sh, long long sw, long long sz, int H,
                                                          float label_index, char* __restrict__ ws, RhlvPlan P) {
    __shared__ int red[256];
    const int z = blockIdx.x, v = blockIdx.y, Z = P.Z, W = P.W;
    const T* vol = rhlv_volume_ptr(fake, label, pairs, v);
    if (label_indices) label_index = label_indices[blockIdx.z];
    int* cnt = (int*)(rhlv_slab(ws, P) + P.cnt);
    int* tot = (int*)(rhlv_slab(ws, P) + P.view[0].tot);       // view[0] is the sagittal one whenever it is asked for
    int mine = 0;
    for (int w = threadIdx.x; w < W; w += 256) {
        int c = 0;
        const T* p = vol + (long long)w * sw + (long long)z * sz;
        for (int h = 0; h < H; ++h) {
            const float val = (float)p[(long long)h * sh];
            c += label_index < 0.f ? (val != 0.f) : (val == label_index);
        }
        cnt[((long long)v * Z + z) * W + w] = c;
        mine += c;
    }
    if (P.view[0].coronal) return;                              // coronal only: its totals come from rhlv_tot_kernel
    red[threadIdx.x] = mine;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) tot[v * Z + z] = red[0];
}

// the same for volumes whose z index is the fastest-varying one in memory (the reference's [H][W][Z] arrays): a lane owns one (w, z)
// column and walks h, 64 consecutive lanes read 64 consecutive z -- coalesced.  grid (ceil(W*Z/256), 2, N); tot by rhlv_tot_kernel.
template <typename T>
__global__ __launch_bounds__(256) void rhlv_counts_zfast_kernel(const T* __restrict__ fake, const T* __restrict__ label,
                                                                const void* const* __restrict__ pairs, const float* __restrict__ label_indices,
                                                                long long sh, long long sw, long long sz, int H, float label_index,
                                                                char* __restrict__ ws, RhlvPlan P) {
    const int Z = P.Z, W = P.W;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)W * Z) return;
    const int v = blockIdx.y, w = (int)(i / Z), z = (int)(i - (long long)w * Z);
    const T* p = rhlv_volume_ptr(fake, label, pairs, v) + (long long)w * sw + (long long)z * sz;
    if (label_indices) label_index = label_indices[blockIdx.z];
    int* cnt = (int*)(rhlv_slab(ws, P) + P.cnt);
    int c = 0;
    for (int h = 0; h < H; ++h) {
        const float val = (float)p[(long long)h * sh];
        c += label_index < 0.f ? (val != 0.f) : (val == label_index);
    }
    cnt[((long long)v * Z + z) * W + w] = c;
}
// tot[v][s] of view `vi`: the table summed over the view's columns.  grid (S, 2, N)
__global__ __launch_bounds__(256) void rhlv_tot_kernel(char* __restrict__ ws, RhlvPlan P, int vi) {
    __shared__ int red[256];
    const RhlvView& V = P.view[vi];
    const int s = blockIdx.x, v = blockIdx.y;
    const int* cv = (const int*)(rhlv_slab(ws, P) + P.cnt) + (long long)v * P.Z * P.W + (long long)s * V.ss;
    int* tot = (int*)(rhlv_slab(ws, P) + V.tot);
    int mine = 0;
    for (int c = threadIdx.x; c < V.C; c += 256) mine += cv[(long long)c * V.sc];
    red[threadIdx.x] = mine;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) tot[v * V.S + s] = red[0];
}

// The slices [lo, hi) a script walks on an axis of Z slices, from the original vertebra's voxels per slice (tot_label[Z]): lo_in == INT_MIN: centre
// = int(mean slice index), half-length = extent // divisor like process_datasets_to_excel, else the explicit [lo_in, hi_in); numpy's slice
// normalisation either way.  One lane walks the axis: rhlv_range_kernel per view, rhlv_sweep_final_kernel per divisor.
struct RhlvRange { int lo, hi, cz, len, valid; };
__device__ __forceinline__ RhlvRange rhlv_slice_range(const int* __restrict__ tot_label, int Z, int divisor, int lo_in, int hi_in) {
    int lo, hi, cz = 0, len = 0, valid = 1;
    if (lo_in == INT_MIN) {
        long long n = 0, sz = 0;
        int mn = Z, mx = -1;
        for (int z = 0; z < Z; ++z) {
            const int t = tot_label[z];
            if (t > 0) { n += t; sz += (long long)t * z; mn = min(mn, z); mx = max(mx, z); }
        }
        if (n == 0) { valid = 0; lo = hi = 0; }
        else {
            cz = (int)((double)sz / (double)n);          // int(np.mean(loc))
            len = (mx - mn) / divisor;                  // (max_z - min_z) // length_divisor
            lo = cz - len; hi = cz + len;
        }
    } else { lo = lo_in; hi = hi_in; cz = (lo_in + hi_in) / 2; len = (hi_in - lo_in) / 2; }
    // numpy slice normalisation of [lo:hi] on an axis of length Z
    if (lo < 0) lo = max(lo + Z, 0);
    if (hi < 0) hi = max(hi + Z, 0);
    lo = min(lo, Z); hi = min(hi, Z);
    return {lo, hi, cz, len, valid};
}

// params: [0] lo, [1] hi, [2] centre slice, [3] length, [4] valid (label has voxels)
__global__ void rhlv_range_kernel(char* __restrict__ ws, RhlvPlan P) {
    if (threadIdx.x != 0) return;
    const RhlvView& V = P.view[blockIdx.y];
    const int* tot = (const int*)(rhlv_slab(ws, P) + V.tot);
    int* params = (int*)(rhlv_slab(ws, P) + V.params);
    const RhlvRange R = rhlv_slice_range(tot + V.S, V.S, V.divisor, V.lo, V.hi);
    params[0] = R.lo; params[1] = R.hi; params[2] = R.cz; params[3] = R.len; params[4] = R.valid;
}

__device__ __forceinline__ long long rhlv_block_sum(long long v, long long* sh) {
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}
__device__ __forceinline__ int rhlv_block_max(int v, long long* sh) {
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] = max(sh[threadIdx.x], sh[threadIdx.x + o]);
        __syncthreads();
    }
    return (int)sh[0];
}

// MAPS: also leave the slice's RhlvMapRec (the hv_rhlv_maps entries); the other entries run the instantiation without it
template <bool MAPS>
__global__ __launch_bounds__(256) void rhlv_slice_kernel(char* __restrict__ ws, RhlvPlan P) {
    __shared__ long long sh[256];
    const RhlvView& V = P.view[blockIdx.y];
    const int z = blockIdx.x, Z = V.S, W = V.C, tid = threadIdx.x;
    if (z >= Z) return;                                  // the grid is as wide as the longer view
    const long long sc = V.sc;
    const int* tot = (const int*)(rhlv_slab(ws, P) + V.tot);
    const int* params = (const int*)(rhlv_slab(ws, P) + V.params);
    RhlvRec* rec = (RhlvRec*)(rhlv_slab(ws, P) + V.recs) + z;
    RhlvMapRec* mrec = MAPS ? (RhlvMapRec*)(rhlv_slab(ws, P) + P.maprecs[blockIdx.y]) + z : nullptr;
    const int* cf = (const int*)(rhlv_slab(ws, P) + P.cnt) + (long long)z * V.ss;     // column w of this slice: cf[w * sc]
    const int* cl = cf + (long long)P.Z * P.W;
    const bool on = z >= params[0] && z < params[1] && tot[z] > 0 && tot[Z + z] > 0 && params[4];
    if (!on) {
        if (tid < 4) { rec->ratio[tid] = 1.0; rec->Sf[tid] = rec->nf[tid] = rec->Sl[tid] = rec->nl[tid] = 0; }
        if (tid == 0) rec->raises = 0;
        if (MAPS && tid == 0) { mrec->ratio = 1.0; mrec->thr_f = mrec->thr_l = 0.0; mrec->t1 = mrec->t2 = mrec->on = mrec->pad = 0; }
        return;
    }
    // column statistics of the generated and the original vertebra
    int ymin = W, ymax = -1;
    long long swf = 0, swl = 0;
    for (int w = tid; w < W; w += 256) {
        if (cf[w * sc] > 0) { ymin = min(ymin, w); ymax = max(ymax, w); }
        swf += (long long)cf[w * sc] * w;
        swl += (long long)cl[w * sc] * w;
    }
    ymax = rhlv_block_max(ymax, sh);
    ymin = -rhlv_block_max(-ymin, sh);
    swf = rhlv_block_sum(swf, sh);
    swl = rhlv_block_sum(swl, sh);
    const int y_range = ymax - ymin;
    const int t1 = (int)((double)ymin + (double)y_range / 3.0);            // int(y_min + y_range/3)
    const int t2 = (int)((double)ymin + (double)(2 * y_range) / 3.0);      // int(y_min + 2*y_range/3)
    const int ccf = (int)((double)swf / (double)tot[z]);                   // int(np.mean(loc))
    const int ccl = (int)((double)swl / (double)tot[Z + z]);
    const int center_f_i = cf[ccf * sc], center_l = cl[ccl * sc];
    const int r0[4] = {0, 0, t1, t2}, r1[4] = {W, t1, t2, W};
    double ratio[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        int mf = -1, ml = -1;
        for (int w = r0[c] + tid; w < r1[c]; w += 256) { mf = max(mf, cf[w * sc]); ml = max(ml, cl[w * sc]); }
        mf = rhlv_block_max(mf, sh);
        ml = rhlv_block_max(ml, sh);
        // sagittal: label.max() / (fake.max() + 1e-6) behind .size > 0 guards; coronal: label.max() / fake.max(), inf where a third of the
        // generated vertebra is empty (0 * inf = nan then selects nothing below)
        const double den = V.coronal ? (double)mf : (double)mf + 1e-6;
        ratio[c] = (r1[c] > r0[c] && ml > mf) ? (double)ml / den : 1.0;
    }
    // the coronal script takes max() of the pre and mid thirds unguarded: an empty one (the post third never is) raises ValueError
    const long long raises = V.coronal && (t1 <= 0 || t2 <= t1);
    const double center_f = (double)center_f_i * ratio[0];
    const double thr_f = center_f * V.thr, thr_l = (double)center_l * V.thr;
    if (MAPS && tid == 0) { mrec->ratio = ratio[0]; mrec->thr_f = thr_f; mrec->thr_l = thr_l; mrec->t1 = t1; mrec->t2 = t2; mrec->on = 1; mrec->pad = 0; }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        long long Sf = 0, nf = 0, Sl = 0, nl = 0;
        for (int w = r0[c] + tid; w < r1[c]; w += 256) {
            if ((double)cf[w * sc] * ratio[c] > thr_f) { Sf += cf[w * sc]; ++nf; }
            if ((double)cl[w * sc] > thr_l) { Sl += cl[w * sc]; ++nl; }
        }
        Sf = rhlv_block_sum(Sf, sh); nf = rhlv_block_sum(nf, sh);
        Sl = rhlv_block_sum(Sl, sh); nl = rhlv_block_sum(nl, sh);
        if (tid == 0) { rec->ratio[c] = ratio[c]; rec->Sf[c] = Sf; rec->nf[c] = nf; rec->Sl[c] = Sl; rec->nl[c] = nl; }
    }
    if (tid == 0) rec->raises = raises;
}

// out[0..4] = all, pre, mid, post RHLV, relative height of the original; out[5..12] = the eight mean heights
// (all_f, all_l, pre_f, pre_l, mid_f, mid_l, post_f, post_l); out[13] = 1 if the original vertebra exists, else 0;
// 16-double records: out[14] = 1 if the reference would have raised (coronal view), out[15] = 0
__device__ __forceinline__ void rhlv_write_record(double* __restrict__ out, const double (&m)[8], int valid, long long raises, int out_len) {
    for (int c = 0; c < 4; ++c) out[c] = (m[2 * c] - m[2 * c + 1]) / (m[2 * c] + 1e-6);
    const double mn = fmin(m[3], fmin(m[5], m[7])), mx = fmax(m[3], fmax(m[5], m[7]));
    out[4] = mn / (mx + 1e-6);
    for (int i = 0; i < 8; ++i) out[5 + i] = m[i];
    out[13] = (double)valid;
    if (out_len > 14) { out[14] = (double)raises; out[15] = 0.0; }
}

__global__ void rhlv_final_kernel(char* __restrict__ ws, RhlvPlan P, double* __restrict__ out, int out_len) {
    if (threadIdx.x != 0) return;
    const RhlvView& V = P.view[blockIdx.y];
    const RhlvRec* recs = (const RhlvRec*)(rhlv_slab(ws, P) + V.recs);
    const int* params = (const int*)(rhlv_slab(ws, P) + V.params);
    const int Z = V.S;
    out += ((long long)blockIdx.z * P.nviews + blockIdx.y) * out_len;
    double m[8];
    long long raises = 0;
    for (int c = 0; c < 4; ++c) {
        double sf = 0.0, sl = 0.0;
        long long nf = 0, nl = 0;
        for (int z = 0; z < Z; ++z) {
            if (recs[z].nf[c] > 0) sf += (double)recs[z].Sf[c] * recs[z].ratio[c];      // nothing selected: nothing added (the ratio may be inf)
            sl += (double)recs[z].Sl[c];
            nf += recs[z].nf[c];
            nl += recs[z].nl[c];
            raises |= recs[z].raises;
        }
        m[2 * c] = nf > 0 ? sf / (double)nf : 0.0;
        m[2 * c + 1] = nl > 0 ? sl / (double)nl : 0.0;
    }
    rhlv_write_record(out, m, params[4], raises, out_len);
}

// ---- the parameter sweep (hv_rhlv_sweep): every (length_divisor, height_threshold) of a grid from one pass over the volumes.  Neither parameter
// touches the table or a slice's thirds, maxima, ratios and centre heights; the threshold selects columns, the divisor selects slices.
//   rhlv_sweep_slice_kernel   grid (S, views, N): EVERY slice where both vertebrae have voxels (the range differs per divisor): the
//                             threshold-independent state once (RhlvSweepSlice), then per threshold the integer sums of rhlv_slice_kernel
//   rhlv_sweep_final_kernel   grid (ceil(D*T/64), views, N): one lane per grid point: that divisor's range, the ordered fold of rhlv_final_kernel
// A pair's slab is the other entries' (rhlv_plan) followed by, per view, RhlvSweepSlice[S] and RhlvSweepRec[S][T].
struct RhlvSweepSlice { double ratio[4]; int on, raises; };
struct RhlvSweepRec { int Sf[4], nf[4], Sl[4], nl[4]; };    // a slice's sums are at most H * C: hv_rhlv_sweep refuses shapes where that passes INT_MAX
struct RhlvSweepPlan { long long state[2], recs[2]; };       // per view: byte offsets in a pair's slab

__device__ __forceinline__ int rhlv_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int rhlv_wave_count(bool p) { return __popcll(__ballot(p)); }

__global__ __launch_bounds__(256) void rhlv_sweep_slice_kernel(char* __restrict__ ws, RhlvPlan P, RhlvSweepPlan Q, hv_rhlv_grid G) {
    __shared__ long long sh[256];
    __shared__ int part[HV_RHLV_MAX_THRESHOLDS][4][14];   // per threshold and wave: Sf all, pre, mid, post | nf the same | Sl pre, mid, post | nl the same
    const RhlvView& V = P.view[blockIdx.y];
    const int z = blockIdx.x, Z = V.S, W = V.C, tid = threadIdx.x, T = G.n_thresholds;
    if (z >= Z) return;                                  // the grid is as wide as the longer view
    const long long sc = V.sc;
    const int* tot = (const int*)(rhlv_slab(ws, P) + V.tot);
    RhlvSweepSlice* st = (RhlvSweepSlice*)(rhlv_slab(ws, P) + Q.state[blockIdx.y]) + z;
    RhlvSweepRec* recs = (RhlvSweepRec*)(rhlv_slab(ws, P) + Q.recs[blockIdx.y]) + (long long)z * T;
    const int* cf = (const int*)(rhlv_slab(ws, P) + P.cnt) + (long long)z * V.ss;     // column w of this slice: cf[w * sc]
    const int* cl = cf + (long long)P.Z * P.W;
    if (!(tot[z] > 0 && tot[Z + z] > 0)) {               // no script visits it, whatever the range: the fold skips its records
        if (tid < 4) st->ratio[tid] = 1.0;
        if (tid == 0) { st->on = 0; st->raises = 0; }
        return;
    }
    // the threshold-independent state, in rhlv_slice_kernel's expressions
    int ymin = W, ymax = -1;
    long long swf = 0, swl = 0;
    for (int w = tid; w < W; w += 256) {
        if (cf[w * sc] > 0) { ymin = min(ymin, w); ymax = max(ymax, w); }
        swf += (long long)cf[w * sc] * w;
        swl += (long long)cl[w * sc] * w;
    }
    ymax = rhlv_block_max(ymax, sh);
    ymin = -rhlv_block_max(-ymin, sh);
    swf = rhlv_block_sum(swf, sh);
    swl = rhlv_block_sum(swl, sh);
    const int y_range = ymax - ymin;
    const int t1 = (int)((double)ymin + (double)y_range / 3.0);            // int(y_min + y_range/3)
    const int t2 = (int)((double)ymin + (double)(2 * y_range) / 3.0);      // int(y_min + 2*y_range/3)
    const int ccf = (int)((double)swf / (double)tot[z]);                   // int(np.mean(loc))
    const int ccl = (int)((double)swl / (double)tot[Z + z]);
    const int center_f_i = cf[ccf * sc], center_l = cl[ccl * sc];
    const int r0[4] = {0, 0, t1, t2}, r1[4] = {W, t1, t2, W};
    double ratio[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        int mf = -1, ml = -1;
        for (int w = r0[c] + tid; w < r1[c]; w += 256) { mf = max(mf, cf[w * sc]); ml = max(ml, cl[w * sc]); }
        mf = rhlv_block_max(mf, sh);
        ml = rhlv_block_max(ml, sh);
        const double den = V.coronal ? (double)mf : (double)mf + 1e-6;    // see rhlv_slice_kernel
        ratio[c] = (r1[c] > r0[c] && ml > mf) ? (double)ml / den : 1.0;
    }
    const double center_f = (double)center_f_i * ratio[0];
    if (tid == 0) {
        for (int c = 0; c < 4; ++c) st->ratio[c] = ratio[c];
        st->on = 1;
        st->raises = V.coronal && (t1 <= 0 || t2 <= t1);
    }
    // per threshold: a column counts for the whole slice (ratio[0]) and for its own third (that third's ratio); the original's test is the same in
    // both, so its whole-slice sums are the thirds' added up.  Integer sums: a wave folds its 64 columns by shuffles, the counts by ballots,
    // lane 0 keeps the wave's running sums in LDS; one barrier, then one lane per threshold adds the four waves.
    const int wave = tid >> 6, lane = tid & 63;
    for (int k = 0; k < W; k += 256) {                   // block-uniform: every lane takes part in the shuffles
        const int w = k + tid;
        const bool live = w < W;
        const int f = live ? cf[w * sc] : 0, l = live ? cl[w * sc] : 0;
        const int reg = w < t1 ? 1 : w < t2 ? 2 : 3;
        const double hf_all = (double)f * ratio[0], hf_reg = (double)f * (reg == 1 ? ratio[1] : reg == 2 ? ratio[2] : ratio[3]), hl = (double)l;
        for (int t = 0; t < T; ++t) {
            const double thr_f = center_f * G.threshold[t], thr_l = (double)center_l * G.threshold[t];
            const bool sa = live && hf_all > thr_f, sr = live && hf_reg > thr_f, sl = live && hl > thr_l;
            int v[14];
            v[0] = rhlv_wave_sum(sa ? f : 0);
            v[4] = rhlv_wave_count(sa);
#pragma unroll
            for (int c = 1; c < 4; ++c) {
                v[c] = rhlv_wave_sum(sr && reg == c ? f : 0);
                v[4 + c] = rhlv_wave_count(sr && reg == c);
                v[7 + c] = rhlv_wave_sum(sl && reg == c ? l : 0);
                v[10 + c] = rhlv_wave_count(sl && reg == c);
            }
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 14; ++i) part[t][wave][i] = k == 0 ? v[i] : part[t][wave][i] + v[i];
            }
        }
    }
    __syncthreads();
    for (int t = tid; t < T; t += 256) {
        int v[14];
#pragma unroll
        for (int i = 0; i < 14; ++i) v[i] = part[t][0][i] + part[t][1][i] + part[t][2][i] + part[t][3][i];
        RhlvSweepRec r;
        r.Sl[0] = r.nl[0] = 0;
#pragma unroll
        for (int c = 1; c < 4; ++c) { r.Sl[c] = v[7 + c]; r.nl[c] = v[10 + c]; r.Sl[0] += v[7 + c]; r.nl[0] += v[10 + c]; }
#pragma unroll
        for (int c = 0; c < 4; ++c) { r.Sf[c] = v[c]; r.nf[c] = v[4 + c]; }
        recs[t] = r;
    }
}

// out [N][D][T][views][16]: hv_rhlv_views' records
__global__ __launch_bounds__(64) void rhlv_sweep_final_kernel(const char* __restrict__ ws, RhlvPlan P, RhlvSweepPlan Q, hv_rhlv_grid G,
                                                              double* __restrict__ out) {
    const int D = G.n_divisors, T = G.n_thresholds;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= D * T) return;
    const int d = i / T, t = i - d * T;
    const RhlvView& V = P.view[blockIdx.y];
    const char* slab = ws + (long long)blockIdx.z * P.pair_bytes;
    const RhlvSweepSlice* st = (const RhlvSweepSlice*)(slab + Q.state[blockIdx.y]);
    const RhlvSweepRec* recs = (const RhlvSweepRec*)(slab + Q.recs[blockIdx.y]);
    const RhlvRange R = rhlv_slice_range((const int*)(slab + V.tot) + V.S, V.S, G.divisor[d], INT_MIN, 0);
    double m[8];
    long long raises = 0;
    for (int c = 0; c < 4; ++c) {
        double sf = 0.0, sl = 0.0;
        long long nf = 0, nl = 0;
        for (int z = R.lo; z < R.hi; ++z) {              // rhlv_final_kernel's fold: the slices outside add nothing there
            if (!st[z].on) continue;
            const RhlvSweepRec& r = recs[(long long)z * T + t];
            if (r.nf[c] > 0) sf += (double)r.Sf[c] * st[z].ratio[c];
            sl += (double)r.Sl[c];
            nf += r.nf[c];
            nl += r.nl[c];
            raises |= st[z].raises;
        }
        m[2 * c] = nf > 0 ? sf / (double)nf : 0.0;
        m[2 * c + 1] = nl > 0 ? sl / (double)nl : 0.0;
    }
    out += ((((long long)blockIdx.z * D + d) * T + t) * P.nviews + blockIdx.y) * 16;
    rhlv_write_record(out, m, R.valid, raises, 16);
}

// Output pointers of one view for n_pairs pairs, each NULL = not wanted: loss / hf / hl / flags [N][S][C], colp [N][3][C], slicep [N][3][S],
// range [N][2]
struct RhlvMapOut { double *loss, *hf, *hl; unsigned char* flags; double *colp, *slicep; int* range; };
struct RhlvMapOuts { RhlvMapOut view[2]; };

__global__ __launch_bounds__(256) void rhlv_map_kernel(const char* __restrict__ ws, RhlvPlan P, RhlvMapOuts O) {
    const RhlvView& V = P.view[blockIdx.y];
    const RhlvMapOut& o = O.view[blockIdx.y];
    const int s = blockIdx.x, S = V.S, C = V.C;
    if (s >= S) return;                                  // the grid is as wide as the longer view
    const char* slab = ws + (long long)blockIdx.z * P.pair_bytes;
    const RhlvMapRec r = ((const RhlvMapRec*)(slab + P.maprecs[blockIdx.y]))[s];
    const int* cf = (const int*)(slab + P.cnt) + (long long)s * V.ss;
    const int* cl = cf + (long long)P.Z * P.W;
    const long long sc = V.sc, row = ((long long)blockIdx.z * S + s) * C;
    if (s == 0 && threadIdx.x == 0 && o.range) {
        const int* params = (const int*)(slab + V.params);
        o.range[2 * (long long)blockIdx.z] = params[0];
        o.range[2 * (long long)blockIdx.z + 1] = params[1];
    }
    for (int c = threadIdx.x; c < C; c += 256) {
        double hf = 0.0, hl = 0.0, loss = __builtin_nan("");
        unsigned flags = 0;
        if (r.on) {
            hf = (double)cf[c * sc] * r.ratio;
            hl = (double)cl[c * sc];
            const bool sel_f = hf > r.thr_f, sel_l = hl > r.thr_l;
            flags = (c < r.t1 ? 0u : c < r.t2 ? 1u : 2u) | (sel_f ? 4u : 0u) | (sel_l ? 8u : 0u) | 16u;
            if (sel_f) loss = (hf - hl) / (hf + 1e-6);
        }
        if (o.hf) o.hf[row + c] = hf;
        if (o.hl) o.hl[row + c] = hl;
        if (o.loss) o.loss[row + c] = loss;
        if (o.flags) o.flags[row + c] = (unsigned char)flags;
    }
}

// lanes [0, C): column c over the slices of [lo, hi); lanes [C, C + S): slice s over its columns.  Sequential sums in ascending order.
__global__ __launch_bounds__(256) void rhlv_profile_kernel(const char* __restrict__ ws, RhlvPlan P, RhlvMapOuts O) {
    const RhlvView& V = P.view[blockIdx.y];
    const RhlvMapOut& o = O.view[blockIdx.y];
    const int S = V.S, C = V.C;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S + C) return;
    const bool column = i < C;
    double* out = column ? o.colp : o.slicep;
    if (!out) return;
    const char* slab = ws + (long long)blockIdx.z * P.pair_bytes;
    const RhlvMapRec* recs = (const RhlvMapRec*)(slab + P.maprecs[blockIdx.y]);
    const int* params = (const int*)(slab + V.params);
    const int* cf = (const int*)(slab + P.cnt);
    const int* cl = cf + (long long)P.Z * P.W;
    const long long ss = V.ss, sc = V.sc;
    double sf = 0.0, sl = 0.0;
    long long nf = 0, nl = 0;
    if (column) {
        for (int s = params[0]; s < params[1]; ++s) {
            const RhlvMapRec r = recs[s];
            if (!r.on) continue;
            const double hf = (double)cf[s * ss + i * sc] * r.ratio, hl = (double)cl[s * ss + i * sc];
            if (hf > r.thr_f) { sf += hf; ++nf; }
            if (hl > r.thr_l) { sl += hl; ++nl; }
        }
    } else {
        const int s = i - C;
        const RhlvMapRec r = recs[s];
        if (r.on)
            for (int c = 0; c < C; ++c) {
                const double hf = (double)cf[s * ss + c * sc] * r.ratio, hl = (double)cl[s * ss + c * sc];
                if (hf > r.thr_f) { sf += hf; ++nf; }
                if (hl > r.thr_l) { sl += hl; ++nl; }
            }
    }
    const int n = column ? C : S, j = column ? i : i - C;
    const double pf = nf > 0 ? sf / (double)nf : __builtin_nan(""), pl = nl > 0 ? sl / (double)nl : __builtin_nan("");
    out += (long long)blockIdx.z * 3 * n;
    out[j] = pf;
    out[n + j] = pl;
    out[2 * n + j] = (pf - pl) / (pf + 1e-6);
}


// One pair's workspace slab: recs per view | cnt[2][Z][W] | tot[2][S] per view | params[8] per view | maprecs per view (maps only); view[0] is the sagittal one when asked for
static RhlvPlan rhlv_plan(int W, int Z, int views, const hv_rhlv_view* sagittal, const hv_rhlv_view* coronal, bool maps = false) {
    RhlvPlan P = {};
    P.W = W; P.Z = Z;
    if (views & HV_RHLV_SAGITTAL) { RhlvView& V = P.view[P.nviews++]; V.S = Z; V.C = W; V.ss = W; V.sc = 1; V.coronal = 0; }
    if (views & HV_RHLV_CORONAL) { RhlvView& V = P.view[P.nviews++]; V.S = W; V.C = Z; V.ss = 1; V.sc = W; V.coronal = 1; }
    long long off = 0;
    for (int i = 0; i < P.nviews; ++i) { P.view[i].recs = off; off += (long long)P.view[i].S * sizeof(RhlvRec); }
    P.cnt = off; off += (long long)2 * Z * W * sizeof(int);
    for (int i = 0; i < P.nviews; ++i) { P.view[i].tot = off; off += (long long)2 * P.view[i].S * sizeof(int); }
    for (int i = 0; i < P.nviews; ++i) {
        RhlvView& V = P.view[i];
        V.params = off; off += 8 * sizeof(int);
        const hv_rhlv_view* a = V.coronal ? coronal : sagittal;
        if (a) { V.divisor = a->length_divisor; V.lo = a->lo; V.hi = a->hi; V.thr = a->height_threshold; }
    }
    for (int i = 0; i < P.nviews; ++i) {
        P.maprecs[i] = -1;
        if (maps) { P.maprecs[i] = off; off += (long long)P.view[i].S * sizeof(RhlvMapRec); }
    }
    P.pair_bytes = (off + 7) & ~7LL;
    return P;
}

// the pass over the volumes and the per-slice totals, the start of every entry: one pair passed by value (pairs == NULL, n_pairs 1) or a device
// table of n_pairs pointer pairs
static int rhlv_launch_table(const void* fake, const void* label, const void* pairs, const float* label_indices, int n_pairs, int dtype,
                             long long stride_h, long long stride_w, long long stride_z, int H, float label_index, const RhlvPlan& P, char* ws,
                             hipStream_t s) {
    const void* const* pp = (const void* const*)pairs;
    const bool zfast = stride_z == 1 && stride_w != 1;   // z fastest in memory: lanes along z
    const dim3 grid = zfast ? dim3(hv_cdiv((long long)P.W * P.Z, 256), 2, n_pairs) : dim3(P.Z, 2, n_pairs);
    if (zfast && dtype == 0)
        hipLaunchKernelGGL((rhlv_counts_zfast_kernel<float>), grid, dim3(256), 0, s, (const float*)fake, (const float*)label, pp, label_indices, stride_h,
                           stride_w, stride_z, H, label_index, ws, P);
    else if (zfast)
        hipLaunchKernelGGL((rhlv_counts_zfast_kernel<unsigned char>), grid, dim3(256), 0, s, (const unsigned char*)fake, (const unsigned char*)label, pp,
                           label_indices, stride_h, stride_w, stride_z, H, label_index, ws, P);
    else if (dtype == 0)
        hipLaunchKernelGGL((rhlv_counts_kernel<float>), grid, dim3(256), 0, s, (const float*)fake, (const float*)label, pp, label_indices, stride_h,
                           stride_w, stride_z, H, label_index, ws, P);
    else
        hipLaunchKernelGGL((rhlv_counts_kernel<unsigned char>), grid, dim3(256), 0, s, (const unsigned char*)fake, (const unsigned char*)label, pp,
                           label_indices, stride_h, stride_w, stride_z, H, label_index, ws, P);
    HV_LAUNCH_CHECK();
    for (int i = 0; i < P.nviews; ++i) {
        if (!P.view[i].coronal && !zfast) continue;      // the lanes-along-w counts kernel left the sagittal totals
        hipLaunchKernelGGL(rhlv_tot_kernel, dim3(P.view[i].S, 2, n_pairs), dim3(256), 0, s, ws, P, i);
        HV_LAUNCH_CHECK();
    }
    return HV_OK;
}

static int rhlv_longer_view(const RhlvPlan& P) { return P.nviews > 1 && P.view[1].S > P.view[0].S ? P.view[1].S : P.view[0].S; }

// the launch sequence of the one-setting entries
static int rhlv_run(const void* fake, const void* label, const void* pairs, const float* label_indices, int n_pairs, int dtype, long long stride_h,
                    long long stride_w, long long stride_z, int H, float label_index, const RhlvPlan& P, double* out, int out_len, void* workspace,
                    hipStream_t s, const RhlvMapOuts* maps = nullptr) {
    char* ws = (char*)workspace;
    const int rc = rhlv_launch_table(fake, label, pairs, label_indices, n_pairs, dtype, stride_h, stride_w, stride_z, H, label_index, P, ws, s);
    if (rc != HV_OK) return rc;
    const int smax = rhlv_longer_view(P);
    hipLaunchKernelGGL(rhlv_range_kernel, dim3(1, P.nviews, n_pairs), dim3(64), 0, s, ws, P);
    HV_LAUNCH_CHECK();
    if (maps) hipLaunchKernelGGL(rhlv_slice_kernel<true>, dim3(smax, P.nviews, n_pairs), dim3(256), 0, s, ws, P);
    else hipLaunchKernelGGL(rhlv_slice_kernel<false>, dim3(smax, P.nviews, n_pairs), dim3(256), 0, s, ws, P);
    HV_LAUNCH_CHECK();
    hipLaunchKernelGGL(rhlv_final_kernel, dim3(1, P.nviews, n_pairs), dim3(64), 0, s, ws, P, out, out_len);
    HV_LAUNCH_CHECK();
    if (maps) {
        hipLaunchKernelGGL(rhlv_map_kernel, dim3(smax, P.nviews, n_pairs), dim3(256), 0, s, (const char*)ws, P, *maps);
        HV_LAUNCH_CHECK();
        hipLaunchKernelGGL(rhlv_profile_kernel, dim3(hv_cdiv((long long)P.W + P.Z, 256), P.nviews, n_pairs), dim3(256), 0, s, (const char*)ws, P, *maps);
        HV_LAUNCH_CHECK();
    }
    return HV_OK;
}

static bool rhlv_views_ok(int views, const hv_rhlv_view* sagittal, const hv_rhlv_view* coronal) {
    if (views < 1 || views > (HV_RHLV_SAGITTAL | HV_RHLV_CORONAL)) return false;
    if ((views & HV_RHLV_SAGITTAL) && (!sagittal || sagittal->length_divisor <= 0)) return false;
    if ((views & HV_RHLV_CORONAL) && (!coronal || coronal->length_divisor <= 0)) return false;
    return true;
}

extern "C" size_t hv_rhlv_workspace_bytes(int W, int Z) {
    if (W <= 0 || Z <= 0) return 0;
    return (size_t)rhlv_plan(W, Z, HV_RHLV_SAGITTAL, nullptr, nullptr).pair_bytes;
}

extern "C" int hv_rhlv(const void* fake, const void* label, int dtype, long long stride_h, long long stride_w, long long stride_z, int H, int W, int Z,
                       float label_index, int length_divisor, int z_lo, int z_hi, double height_threshold, double* out, void* workspace,
                       size_t workspace_bytes, void* stream) {
    if (!fake || !label || !out || H <= 0 || W <= 0 || Z <= 0 || length_divisor <= 0 || (dtype != 0 && dtype != 1)) return HV_ERR_ARG;
    if (Z > 65535) return HV_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < hv_rhlv_workspace_bytes(W, Z) || ((uintptr_t)workspace & 7)) return HV_ERR_WORKSPACE;
    const hv_rhlv_view sagittal = {length_divisor, z_lo, z_hi, height_threshold};
    return rhlv_run(fake, label, nullptr, nullptr, 1, dtype, stride_h, stride_w, stride_z, H, label_index,
                    rhlv_plan(W, Z, HV_RHLV_SAGITTAL, &sagittal, nullptr), out, 14, workspace, (hipStream_t)stream);
}

extern "C" size_t hv_rhlv_views_workspace_bytes(int W, int Z, int views, int n_pairs) {
    if (W <= 0 || Z <= 0 || n_pairs <= 0 || views < 1 || views > (HV_RHLV_SAGITTAL | HV_RHLV_CORONAL)) return 0;
    return (size_t)rhlv_plan(W, Z, views, nullptr, nullptr).pair_bytes * n_pairs;
}

extern "C" int hv_rhlv_views(const void* fake, const void* label, int dtype, long long stride_h, long long stride_w, long long stride_z, int H, int W,
                             int Z, float label_index, int views, const hv_rhlv_view* h_sagittal, const hv_rhlv_view* h_coronal, double* out,
                             void* workspace, size_t workspace_bytes, void* stream) {
    if (!fake || !label || !out || H <= 0 || W <= 0 || Z <= 0 || (dtype != 0 && dtype != 1) || !rhlv_views_ok(views, h_sagittal, h_coronal))
        return HV_ERR_ARG;
    if (Z > 65535 || W > 65535) return HV_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < hv_rhlv_views_workspace_bytes(W, Z, views, 1) || ((uintptr_t)workspace & 7)) return HV_ERR_WORKSPACE;
    return rhlv_run(fake, label, nullptr, nullptr, 1, dtype, stride_h, stride_w, stride_z, H, label_index,
                    rhlv_plan(W, Z, views, h_sagittal, h_coronal), out, 16, workspace, (hipStream_t)stream);
}

extern "C" int hv_rhlv_views_batch(const void* pairs, const float* label_indices, int n_pairs, int dtype, long long stride_h, long long stride_w,
                                   long long stride_z, int H, int W, int Z, int views, const hv_rhlv_view* h_sagittal, const hv_rhlv_view* h_coronal,
                                   double* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!pairs || !label_indices || !out || n_pairs <= 0 || H <= 0 || W <= 0 || Z <= 0 || (dtype != 0 && dtype != 1) ||
        !rhlv_views_ok(views, h_sagittal, h_coronal))
        return HV_ERR_ARG;
    if (Z > 65535 || W > 65535 || n_pairs > 65535) return HV_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < hv_rhlv_views_workspace_bytes(W, Z, views, n_pairs) || ((uintptr_t)workspace & 7)) return HV_ERR_WORKSPACE;
    return rhlv_run(nullptr, nullptr, pairs, label_indices, n_pairs, dtype, stride_h, stride_w, stride_z, H, 0.f,
                    rhlv_plan(W, Z, views, h_sagittal, h_coronal), out, 16, workspace, (hipStream_t)stream);
}

extern "C" size_t hv_rhlv_maps_workspace_bytes(int W, int Z, int views, int n_pairs) {
    if (W <= 0 || Z <= 0 || n_pairs <= 0 || views < 1 || views > (HV_RHLV_SAGITTAL | HV_RHLV_CORONAL)) return 0;
    return (size_t)rhlv_plan(W, Z, views, nullptr, nullptr, true).pair_bytes * n_pairs;
}

// the requested views' output pointers in plan order (sagittal first)
static RhlvMapOuts rhlv_map_outs(int views, const hv_rhlv_map_out* sagittal, const hv_rhlv_map_out* coronal) {
    RhlvMapOuts O = {};
    int n = 0;
    for (int bit = HV_RHLV_SAGITTAL; bit <= HV_RHLV_CORONAL; bit <<= 1) {
        if (!(views & bit)) continue;
        const hv_rhlv_map_out* a = bit == HV_RHLV_SAGITTAL ? sagittal : coronal;
        RhlvMapOut& o = O.view[n++];
        if (a) {
            o.loss = a->loss; o.hf = a->height_fake; o.hl = a->height_label; o.flags = a->flags;
            o.colp = a->column_profile; o.slicep = a->slice_profile; o.range = a->range;
        }
    }
    return O;
}

extern "C" int hv_rhlv_maps(const void* fake, const void* label, int dtype, long long stride_h, long long stride_w, long long stride_z, int H, int W,
                            int Z, float label_index, int views, const hv_rhlv_view* h_sagittal, const hv_rhlv_view* h_coronal,
                            const hv_rhlv_map_out* h_sagittal_out, const hv_rhlv_map_out* h_coronal_out, double* out, void* workspace,
                            size_t workspace_bytes, void* stream) {
    if (!fake || !label || !out || H <= 0 || W <= 0 || Z <= 0 || (dtype != 0 && dtype != 1) || !rhlv_views_ok(views, h_sagittal, h_coronal))
        return HV_ERR_ARG;
    if (Z > 65535 || W > 65535) return HV_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < hv_rhlv_maps_workspace_bytes(W, Z, views, 1) || ((uintptr_t)workspace & 7)) return HV_ERR_WORKSPACE;
    const RhlvMapOuts O = rhlv_map_outs(views, h_sagittal_out, h_coronal_out);
    return rhlv_run(fake, label, nullptr, nullptr, 1, dtype, stride_h, stride_w, stride_z, H, label_index,
                    rhlv_plan(W, Z, views, h_sagittal, h_coronal, true), out, 16, workspace, (hipStream_t)stream, &O);
}

extern "C" int hv_rhlv_maps_batch(const void* pairs, const float* label_indices, int n_pairs, int dtype, long long stride_h, long long stride_w,
                                  long long stride_z, int H, int W, int Z, int views, const hv_rhlv_view* h_sagittal, const hv_rhlv_view* h_coronal,
                                  const hv_rhlv_map_out* h_sagittal_out, const hv_rhlv_map_out* h_coronal_out, double* out, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    if (!pairs || !label_indices || !out || n_pairs <= 0 || H <= 0 || W <= 0 || Z <= 0 || (dtype != 0 && dtype != 1) ||
        !rhlv_views_ok(views, h_sagittal, h_coronal))
        return HV_ERR_ARG;
    if (Z > 65535 || W > 65535 || n_pairs > 65535) return HV_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < hv_rhlv_maps_workspace_bytes(W, Z, views, n_pairs) || ((uintptr_t)workspace & 7)) return HV_ERR_WORKSPACE;
    const RhlvMapOuts O = rhlv_map_outs(views, h_sagittal_out, h_coronal_out);
    return rhlv_run(nullptr, nullptr, pairs, label_indices, n_pairs, dtype, stride_h, stride_w, stride_z, H, 0.f,
                    rhlv_plan(W, Z, views, h_sagittal, h_coronal, true), out, 16, workspace, (hipStream_t)stream, &O);
}

// the sweep's plan: the one-setting entries' slab, then per view RhlvSweepSlice[S] and RhlvSweepRec[S][T]
static RhlvPlan rhlv_sweep_plan(int W, int Z, int views, int T, RhlvSweepPlan* Q) {
    RhlvPlan P = rhlv_plan(W, Z, views, nullptr, nullptr);
    long long off = P.pair_bytes;
    for (int i = 0; i < P.nviews; ++i) { Q->state[i] = off; off += (long long)P.view[i].S * sizeof(RhlvSweepSlice); }
    for (int i = 0; i < P.nviews; ++i) { Q->recs[i] = off; off += (long long)P.view[i].S * T * sizeof(RhlvSweepRec); }
    P.pair_bytes = off;
    return P;
}

static bool rhlv_grid_counts_ok(int n_divisors, int n_thresholds) {
    return n_divisors >= 1 && n_divisors <= HV_RHLV_MAX_DIVISORS && n_thresholds >= 1 && n_thresholds <= HV_RHLV_MAX_THRESHOLDS;
}

extern "C" size_t hv_rhlv_sweep_workspace_bytes(int W, int Z, int views, int n_pairs, int n_divisors, int n_thresholds) {
    if (W <= 0 || Z <= 0 || n_pairs <= 0 || views < 1 || views > (HV_RHLV_SAGITTAL | HV_RHLV_CORONAL) || !rhlv_grid_counts_ok(n_divisors, n_thresholds))
        return 0;
    RhlvSweepPlan Q = {};
    return (size_t)rhlv_sweep_plan(W, Z, views, n_thresholds, &Q).pair_bytes * n_pairs;
}

extern "C" int hv_rhlv_sweep(const void* pairs, const float* label_indices, int n_pairs, int dtype, long long stride_h, long long stride_w,
                             long long stride_z, int H, int W, int Z, int views, const hv_rhlv_grid* h_grid, double* out, void* workspace,
                             size_t workspace_bytes, void* stream) {
    if (!pairs || !label_indices || !out || !h_grid || n_pairs <= 0 || H <= 0 || W <= 0 || Z <= 0 || (dtype != 0 && dtype != 1) || views < 1 ||
        views > (HV_RHLV_SAGITTAL | HV_RHLV_CORONAL))
        return HV_ERR_ARG;
    if (!rhlv_grid_counts_ok(h_grid->n_divisors, h_grid->n_thresholds)) return HV_ERR_UNSUPPORTED;
    for (int d = 0; d < h_grid->n_divisors; ++d)
        if (h_grid->divisor[d] <= 0) return HV_ERR_UNSUPPORTED;
    if (Z > 65535 || W > 65535 || n_pairs > 65535 || (long long)H * (W > Z ? W : Z) > INT_MAX) return HV_ERR_UNSUPPORTED;
    const int D = h_grid->n_divisors, T = h_grid->n_thresholds;
    if (!workspace || workspace_bytes < hv_rhlv_sweep_workspace_bytes(W, Z, views, n_pairs, D, T) || ((uintptr_t)workspace & 7)) return HV_ERR_WORKSPACE;
    RhlvSweepPlan Q = {};
    const RhlvPlan P = rhlv_sweep_plan(W, Z, views, T, &Q);
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    const int rc = rhlv_launch_table(nullptr, nullptr, pairs, label_indices, n_pairs, dtype, stride_h, stride_w, stride_z, H, 0.f, P, ws, s);
    if (rc != HV_OK) return rc;
    hipLaunchKernelGGL(rhlv_sweep_slice_kernel, dim3(rhlv_longer_view(P), P.nviews, n_pairs), dim3(256), 0, s, ws, P, Q, *h_grid);
    HV_LAUNCH_CHECK();
    hipLaunchKernelGGL(rhlv_sweep_final_kernel, dim3(hv_cdiv((long long)D * T, 64), P.nviews, n_pairs), dim3(64), 0, s, (const char*)ws, P, Q, *h_grid, out);
    HV_LAUNCH_CHECK();
    return HV_OK;
}
