// Per-label 3-D shape records of V label volumes on the device: hv_shape.  For every listed label value of every
// volume: the histogram of the 256 configurations of the 2 x 2 x 2 cells of the lattice padded by one background layer (what volume, Crofton
// surface area and both Euler numbers are linear functions of: Ohser and Muecklich 2000), the voxel count, the first and second coordinate
// moments and the extents of the integer dot product d . p along the 13 directions.  The slot of a voxel is hv_label_stats' (mask, label value
// -> slot table in the kernel arguments); a voxel outside the volume has none.
//
//   shape_init_kernel     out zeroed, the extents' sentinels, the per-volume bad-label words zeroed
//   shape_count_kernel    a workgroup walks tpb tiles of 16 x 16 x 16 cells.  Per tile the 17 x 17 x 17 voxels at the cells' corners are staged in
//                         LDS as slot bytes (0xFF: none), the staging loop's fastest index on the logical axis with the smallest stride of label.
//                         A thread owns one row of 16 cells along axis 2: it reads its four rows of 17 bytes once and, per slot present in the
//                         tile, turns them into four 17-bit masks; cell k's code is two bits of each.  Runs of one code are folded in a register
//                         before they are added to the workgroup's LDS tables ([slots per pass][256] 32-bit counters, as many slots per pass as
//                         fit 64 KiB beside the rest); rows that lie wholly inside the slot (code 255 sixteen times) are added once per wave.
//                         Code 0 is not counted.  The row's own 16 voxels (corner 0 of its cells) give the moments and extents: tile-local
//                         32-bit sums and minima, folded over the wave by shuffles, moved to volume coordinates by one lane, then LDS atomics
//                         (64-bit sums, 32-bit extents).  Non-zero words leave the workgroup once: 64-bit global atomicAdd / atomicMin / atomicMax.
//   shape_final_kernel    one wave per (volume, slot): bin 0 = the cell count minus the other bins, the status word
// Only integer atomics, so the result does not depend on the order of anything; every word of out and the workspace that is read was written by
// an earlier launch of the same call.  No host synchronisation: the grids come from the shape.
#include <climits>
#include "volume_access.h"

#define SH_THREADS 256
#define SH_T 16                               // tile edge in cells
#define SH_E 17                               // staged voxels per axis
#define SH_P2 20                              // row pitch of the staging in bytes: a row is five aligned 32-bit words
#define SH_STAGE_BYTES 5792                   // 17 * 17 * 20 rounded up to 16
#define SH_MAX_PART 1024                      // workgroups per volume at most
#define SH_LDS_BYTES 65536                    // dynamic LDS a launch may ask for without an attribute
#define SH_MOM 10                             // n, sum p_a [3], sum p_a p_b [6]
#define SH_DIRS 13
#define SH_FULL 0x1FFFFu

struct ShArgs {
    HvVol lab, msk;                           // msk.p == NULL: no mask
    int V, A0, A1, A2, S;
    int ax_in, ax_mid, ax_out;                // logical axes by ascending stride of label
    int n1, n2, ntiles, tpb;                  // tiles along axes 1 and 2, tiles, tiles per workgroup
    int SP;                                   // slots per pass
    unsigned char slot[256];
};

// texture.directions(1): the 13 offsets (a, b, c) > (0, 0, 0) in lexicographic order
__device__ static const signed char sh_dir[SH_DIRS][3] = {{0, 0, 1}, {0, 1, -1}, {0, 1, 0}, {0, 1, 1}, {1, -1, -1}, {1, -1, 0}, {1, -1, 1},
                                                          {1, 0, -1}, {1, 0, 0}, {1, 0, 1}, {1, 1, -1}, {1, 1, 0}, {1, 1, 1}};

__global__ __launch_bounds__(SH_THREADS) void shape_init_kernel(long long* __restrict__ out, long long nout, u64* __restrict__ vbad, int V) {
    const long long g = (long long)blockIdx.x * SH_THREADS + threadIdx.x, step = (long long)gridDim.x * SH_THREADS;
    for (long long e = g; e < nout; e += step) {
        const int f = (int)(e % HV_SHAPE_REC);
        out[e] = (f >= HV_SHAPE_EXTENT && f < HV_SHAPE_STATUS) ? (((f - HV_SHAPE_EXTENT) & 1) ? LLONG_MIN : LLONG_MAX) : 0ll;
    }
    for (long long e = g; e < V; e += step) vbad[e] = 0ull;
}

// the 17-bit mask of the positions of a staged row (five words, the bytes past 17 are not looked at) that hold slot s
__device__ __forceinline__ unsigned sh_row_mask(const unsigned (&w)[5], unsigned s) {
    unsigned m = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int b = 0; b < 4; ++b) m |= (((w[q] >> (8 * b)) & 0xFFu) == s ? 1u : 0u) << (4 * q + b);
    m |= ((w[4] & 0xFFu) == s ? 1u : 0u) << 16;
    return m;
}

__device__ __forceinline__ int sh_wave_min(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = min(x, __shfl_xor(x, o, 64));
    return x;
}
__device__ __forceinline__ unsigned sh_wave_sum(unsigned x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += (unsigned)__shfl_xor((int)x, o, 64);
    return x;
}

// LDS: tbl [SP][256] u32 | st [17][17][SH_P2] u8 | s_mom [S][SH_MOM] u64 | s_ext [S][2 * SH_DIRS] i32 (min, max per direction) | s_present [2] u32
__global__ __launch_bounds__(SH_THREADS) void shape_count_kernel(ShArgs a, long long* __restrict__ out, u64* __restrict__ vbad) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sh_lds[];
    unsigned* tbl = (unsigned*)sh_lds;
    unsigned char* st = sh_lds + (size_t)a.SP * 1024;
    u64* s_mom = (u64*)(st + SH_STAGE_BYTES);
    int* s_ext = (int*)(s_mom + a.S * SH_MOM);
    unsigned* s_present = (unsigned*)(s_ext + a.S * 2 * SH_DIRS);
    const int tid = threadIdx.x, lane = tid & 63, v = blockIdx.y, b = blockIdx.x;
    for (int e = tid; e < a.SP * 256; e += SH_THREADS) tbl[e] = 0u;
    for (int e = tid; e < a.S * SH_MOM; e += SH_THREADS) s_mom[e] = 0ull;
    for (int e = tid; e < a.S * 2 * SH_DIRS; e += SH_THREADS) s_ext[e] = (e & 1) ? INT_MIN : INT_MAX;
    const int tile_end = min((b + 1) * a.tpb, a.ntiles);
    const int ri = tid >> 4, rj = tid & (SH_T - 1);                  // this thread's row of cells: (ri, rj, 0 .. 15)
    int bad = 0;
    for (int s0 = 0; s0 < a.S; s0 += a.SP) {
        const int ns = min(a.SP, a.S - s0);
        const u64 range = (ns == 64 ? ~0ull : ((1ull << ns) - 1ull)) << s0;
        for (int tile = b * a.tpb; tile < tile_end; ++tile) {
            // the voxel at the tile's staged index 0: cell -1 is the padding layer
            const int i0 = (tile / (a.n1 * a.n2)) * SH_T - 1, j0 = ((tile / a.n2) % a.n1) * SH_T - 1, k0 = (tile % a.n2) * SH_T - 1;
            __syncthreads();                                         // the previous tile's rows are read, the first zeroes stand
            if (tid < 2) s_present[tid] = 0u;
            __syncthreads();
            for (int e = tid; e < SH_E * SH_E * SH_E; e += SH_THREADS) {
                const int u = e % SH_E, m = (e / SH_E) % SH_E, o = e / (SH_E * SH_E);
                const int di = a.ax_in == 0 ? u : (a.ax_mid == 0 ? m : o), dj = a.ax_in == 1 ? u : (a.ax_mid == 1 ? m : o),
                          dk = a.ax_in == 2 ? u : (a.ax_mid == 2 ? m : o);
                const int i = i0 + di, j = j0 + dj, k = k0 + dk;
                int s = 0xFF;
                if (i >= 0 && i < a.A0 && j >= 0 && j < a.A1 && k >= 0 && k < a.A2) {
                    s = hv_slot(a, v, i, j, k, bad);
                    if (s != 0xFF && !(s_present[s >> 5] >> (s & 31) & 1u)) atomicOr(&s_present[s >> 5], 1u << (s & 31));
                }
                st[(di * SH_E + dj) * SH_P2 + dk] = (unsigned char)s;
            }
            __syncthreads();
            u64 pm = ((u64)s_present[0] | ((u64)s_present[1] << 32)) & range;
            if (pm == 0ull) continue;
            // rows r = 2 d0 + d1 of this thread's cells: (ri + d0, rj + d1, 0 .. 16)
            unsigned w[4][5];
            bool nothing = true;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned* row = (const unsigned*)(st + ((ri + (r >> 1)) * SH_E + rj + (r & 1)) * SH_P2);
#pragma unroll
                for (int q = 0; q < 5; ++q) w[r][q] = row[q];
                w[r][4] |= 0xFFFFFF00u;                              // the pitch's padding holds nothing
#pragma unroll
                for (int q = 0; q < 5; ++q) nothing = nothing && w[r][q] == 0xFFFFFFFFu;
            }
            if (__ballot(!nothing) == 0ull) continue;                // wave-uniform: no listed voxel near this wave's rows
            while (pm) {
                const int s = __ffsll((long long)pm) - 1;
                pm &= pm - 1;
                unsigned m0 = 0u, m1 = 0u, m2 = 0u, m3 = 0u;
                if (!nothing) {
                    m0 = sh_row_mask(w[0], (unsigned)s); m1 = sh_row_mask(w[1], (unsigned)s);
                    m2 = sh_row_mask(w[2], (unsigned)s); m3 = sh_row_mask(w[3], (unsigned)s);
                }
                unsigned* t = tbl + (s - s0) * 256;
                // rows wholly inside the slot: sixteen cells of code 255 each, one add for the wave
                const bool full = (m0 & m1 & m2 & m3) == SH_FULL;
                const u64 fb = __ballot(full);
                if (fb && lane == __ffsll((long long)fb) - 1) atomicAdd(&t[255], (unsigned)(SH_T * __popcll(fb)));
                if (!full && (m0 | m1 | m2 | m3)) {
                    unsigned rcode = 0u, rcnt = 0u;
#pragma unroll
                    for (int k = 0; k < SH_T; ++k) {
                        const unsigned code = ((m0 >> k) & 3u) | (((m1 >> k) & 3u) << 2) | (((m2 >> k) & 3u) << 4) | (((m3 >> k) & 3u) << 6);
                        if (code != rcode) {
                            if (rcode) atomicAdd(&t[rcode], rcnt);
                            rcode = code; rcnt = 0u;
                        }
                        ++rcnt;
                    }
                    if (rcode) atomicAdd(&t[rcode], rcnt);
                }
                // the row's own voxels: corner 0 of its cells (a slot is counted in one pass only, so its moments are taken once)
                const unsigned mm = m0 & 0xFFFFu;
                if (__ballot(mm != 0u) == 0ull) continue;
                unsigned cnt = (unsigned)__popc(mm), sk = 0u, skk = 0u;
#pragma unroll
                for (int k = 1; k < SH_T; ++k) {
                    const unsigned bit = (mm >> k) & 1u;
                    sk += bit * k; skk += bit * (k * k);
                }
                // tile-local sums: n, l0, l1, l2, l00, l01, l02, l11, l12, l22 (at most 4096 * 15 * 15 per tile)
                unsigned L[SH_MOM] = {cnt, cnt * ri, cnt * rj, sk, cnt * ri * ri, cnt * ri * rj, ri * sk, cnt * rj * rj, rj * sk, skk};
#pragma unroll
                for (int f = 0; f < SH_MOM; ++f) L[f] = sh_wave_sum(L[f]);
                // tile-local extents: e[2t] = min d . l, e[2t + 1] = min -(d . l)
                const int klo = mm ? __ffs((int)mm) - 1 : 0, khi = mm ? 31 - __clz((int)mm) : 0;
                int ext[2 * SH_DIRS];
#pragma unroll
                for (int d = 0; d < SH_DIRS; ++d) {
                    const int da = sh_dir[d][0], db = sh_dir[d][1], dc = sh_dir[d][2];
                    const int base = da * ri + db * rj;
                    const int lo = base + (dc > 0 ? klo : (dc < 0 ? -khi : 0)), hi = base + (dc > 0 ? khi : (dc < 0 ? -klo : 0));
                    ext[2 * d] = sh_wave_min(mm ? lo : INT_MAX);
                    ext[2 * d + 1] = sh_wave_min(mm ? -hi : INT_MAX);
                }
                if (lane == 0) {
                    const long long n = L[0], o0 = i0, o1 = j0, o2 = k0, l0 = L[1], l1 = L[2], l2 = L[3];
                    u64* mo = s_mom + s * SH_MOM;
                    atomicAdd(&mo[0], (u64)n);
                    atomicAdd(&mo[1], (u64)(n * o0 + l0));
                    atomicAdd(&mo[2], (u64)(n * o1 + l1));
                    atomicAdd(&mo[3], (u64)(n * o2 + l2));
                    atomicAdd(&mo[4], (u64)(n * o0 * o0 + 2 * o0 * l0 + (long long)L[4]));
                    atomicAdd(&mo[5], (u64)(n * o0 * o1 + o0 * l1 + o1 * l0 + (long long)L[5]));
                    atomicAdd(&mo[6], (u64)(n * o0 * o2 + o0 * l2 + o2 * l0 + (long long)L[6]));
                    atomicAdd(&mo[7], (u64)(n * o1 * o1 + 2 * o1 * l1 + (long long)L[7]));
                    atomicAdd(&mo[8], (u64)(n * o1 * o2 + o1 * l2 + o2 * l1 + (long long)L[8]));
                    atomicAdd(&mo[9], (u64)(n * o2 * o2 + 2 * o2 * l2 + (long long)L[9]));
                    int* ex = s_ext + s * 2 * SH_DIRS;
#pragma unroll
                    for (int d = 0; d < SH_DIRS; ++d) {
                        const int org = sh_dir[d][0] * i0 + sh_dir[d][1] * j0 + sh_dir[d][2] * k0;   // |d . p| < 2^31: at most 2^30 voxels
                        atomicMin(&ex[2 * d], org + ext[2 * d]);
                        atomicMax(&ex[2 * d + 1], org - ext[2 * d + 1]);
                    }
                }
            }
        }
        __syncthreads();                                             // every add of the pass has landed
        for (int e = tid; e < ns * 256; e += SH_THREADS) {
            const unsigned c = tbl[e];
            if (c == 0u) continue;
            tbl[e] = 0u;
            atomicAdd((u64*)&out[((long long)v * a.S + s0 + (e >> 8)) * HV_SHAPE_REC + (e & 255)], (u64)c);
        }
    }
    if (bad) atomicOr(&vbad[v], 1ull);
    __syncthreads();
    for (int e = tid; e < a.S * SH_MOM; e += SH_THREADS) {
        const u64 x = s_mom[e];
        if (x) atomicAdd((u64*)&out[((long long)v * a.S + e / SH_MOM) * HV_SHAPE_REC + HV_SHAPE_COUNT + e % SH_MOM], x);
    }
    for (int e = tid; e < a.S * 2 * SH_DIRS; e += SH_THREADS) {
        const int s = e / (2 * SH_DIRS), f = e % (2 * SH_DIRS);
        if (s_mom[s * SH_MOM] == 0ull) continue;
        long long* g = &out[((long long)v * a.S + s) * HV_SHAPE_REC + HV_SHAPE_EXTENT + f];
        if (f & 1) atomicMax(g, (long long)s_ext[e]);
        else atomicMin(g, (long long)s_ext[e]);
    }
}

__global__ __launch_bounds__(64) void shape_final_kernel(int S, long long cells, const u64* __restrict__ vbad, long long* __restrict__ out) {
    const long long rec = blockIdx.x;
    long long* o = out + rec * HV_SHAPE_REC;
    const int lane = threadIdx.x;
    long long sum = 0;
    for (int c = lane; c < 256; c += 64) sum += c ? o[c] : 0ll;
#pragma unroll
    for (int x = 32; x > 0; x >>= 1) sum += __shfl_xor(sum, x, 64);
    if (lane == 0) {
        o[0] = cells - sum;
        o[HV_SHAPE_STATUS] = (long long)((vbad[rec / S] ? HV_LS_BAD_LABEL : 0) | (o[HV_SHAPE_COUNT] ? 0 : HV_LS_EMPTY));
    }
}

// ------------------------------------------------------------------------------------------------ host side
static inline bool sh_sizes_ok(int V, int A0, int A1, int A2, int S) {
    return V > 0 && A0 > 0 && A1 > 0 && A2 > 0 && S >= 1 && S <= HV_LS_MAX_LABELS;
}
static inline bool sh_supported(int V, int A0, int A1, int A2) {
    if (hv_too_large(V, A0, A1, A2)) return false;
    const long long vox = (long long)A0 * A1 * A2;
    const long long m = (A0 > A1 ? (A0 > A2 ? A0 : A2) : (A1 > A2 ? A1 : A2)) - 1;
    return (unsigned __int128)vox * (unsigned __int128)m * (unsigned __int128)m < ((unsigned __int128)1 << 62);   // sum p_a p_b stays inside int64
}

extern "C" size_t hv_shape_workspace_bytes(int V, int A0, int A1, int A2, int S) {
    if (!sh_sizes_ok(V, A0, A1, A2, S) || !sh_supported(V, A0, A1, A2)) return 0;
    return hv_up16((size_t)V * 8);                                   // the per-volume bad-label words
}

extern "C" int hv_shape(const void* label, int label_dtype, long long lsv, long long ls0, long long ls1, long long ls2, const void* mask,
                        long long msv, long long ms0, long long ms1, long long ms2, int V, int A0, int A1, int A2, const int* labels, int S,
                        long long* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!label || !labels || !out || !workspace || !sh_sizes_ok(V, A0, A1, A2, S) || label_dtype < HV_DT_U8 || label_dtype > HV_DT_F64 ||
        ((uintptr_t)workspace & 15) || ((uintptr_t)out & 7))
        return HV_ERR_ARG;
    ShArgs a;
    if (!hv_slot_table(a.slot, labels, S)) return HV_ERR_ARG;
    if (!sh_supported(V, A0, A1, A2)) return HV_ERR_UNSUPPORTED;
    if (workspace_bytes < hv_up16((size_t)V * 8)) return HV_ERR_ARG;
    a.lab = hv_vol(label, label_dtype, lsv, ls0, ls1, ls2);
    a.msk = hv_vol(mask, HV_DT_U8, msv, ms0, ms1, ms2);
    a.V = V; a.A0 = A0; a.A1 = A1; a.A2 = A2; a.S = S;
    hv_axis_order(a.lab, A0, A1, A2, a.ax_in, a.ax_mid, a.ax_out);
    const int n0 = hv_cdiv((long long)A0 + 1, SH_T);                 // cells -1 .. A - 1 per axis
    a.n1 = hv_cdiv((long long)A1 + 1, SH_T); a.n2 = hv_cdiv((long long)A2 + 1, SH_T);
    const long long nt = (long long)n0 * a.n1 * a.n2;               // <= 2^30 voxels: at most 2^26 + 1 tiles
    a.ntiles = (int)nt;
    a.tpb = hv_cdiv(nt, SH_MAX_PART);
    const int P = hv_cdiv(nt, a.tpb);
    const size_t fixed = SH_STAGE_BYTES + (size_t)S * (SH_MOM * 8 + 2 * SH_DIRS * 4) + 16;
    const int fit = (int)((SH_LDS_BYTES - fixed) / 1024);            // >= 46: 64 slots leave 47 KiB
    a.SP = fit < S ? fit : S;
    const size_t lds = (size_t)a.SP * 1024 + fixed;
    hipStream_t st = (hipStream_t)stream;
    u64* vbad = (u64*)workspace;
    const long long nout = (long long)V * S * HV_SHAPE_REC;
    const long long cells = ((long long)A0 + 1) * ((long long)A1 + 1) * ((long long)A2 + 1);
    hipLaunchKernelGGL(shape_init_kernel, dim3(min(hv_cdiv(nout, SH_THREADS * 4), 2048)), dim3(SH_THREADS), 0, st, out, nout, vbad, V);
    HV_LAUNCH_CHECK();
    hipLaunchKernelGGL(shape_count_kernel, dim3(P, V), dim3(SH_THREADS), lds, st, a, out, vbad);
    HV_LAUNCH_CHECK();
    hipLaunchKernelGGL(shape_final_kernel, dim3(V * S), dim3(64), 0, st, S, cells, (const u64*)vbad, out);
    HV_LAUNCH_CHECK();
    return HV_OK;
}
