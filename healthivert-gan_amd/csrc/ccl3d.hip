// 3-D connected-component labelling of a volume on the device (hv_label3d) and the two clean-ups of a label volume built on it
// (hv_clean_components: drop small components / keep the largest; hv_fill_holes: scipy's binary_fill_holes); DESIGN.md section 8 row f10.
//
// Foreground F = {vol == value} (HV_CCL_EQ) or {vol != value} (HV_CCL_NE); connectivity c = 1, 2, 3 is generate_binary_structure(3, c): 6, 18 or
// 26 neighbours.  A component is identified by the SMALLEST raster index (i*A1 + j)*A2 + k of its voxels (the logical index, whatever the
// strides are), and the components are numbered 1..n in ascending order of it: scipy.ndimage.label's numbering.
//
// Union-find in which a parent is never larger than its child: parent[x] <= x always, a root is parent[x] == x, and links are only ever made
// by an atomic MIN on a root's word, so the root of a finished set is its smallest member.  Launches of one hv_label3d, in stream order:
//   ccl_tile_kernel     one workgroup per CC_T0 x CC_T1 x CC_T2 tile: the predicate is read through the strides, every foreground voxel is joined
//                       to its backward neighbours (3, 9 or 13 for c = 1, 2, 3) INSIDE the tile by atomicMin unions on local parents in LDS; the
//                       flattened result goes out as parent[p] = raster index of the tile-local root, -1 for background.
//   ccl_seam_kernel     one lane per voxel: the backward neighbours that lie in ANOTHER tile (across a face, an edge or a corner of the tile) are
//                       joined by lock-free unions in global memory.  Every access to parent[] in this launch is an agent-scope relaxed atomic
//                       (the XCDs' L2s are private: a plain access to a word another workgroup writes in the same launch may be stale).  A load
//                       that returns an OLDER parent is harmless: an old parent is still a member of the same set and still smaller than the
//                       child, and only the value a fetch_min RETURNS decides whether a link was made.
//   ccl_flatten_kernel  labels[p] = root of p (parent[] is read-only here), sizes[] zeroed, and the number of roots per CC_BLOCK voxels.
//   ccl_scan_kernel     one workgroup turns the per-block root counts into exclusive offsets, CC_BLOCK counts per turn of a loop; n = the total.
//   ccl_rank_kernel     parent[root] = 1 + the root's rank in raster order (only roots are written, nothing reads parent[] in this launch).
//   ccl_relabel_kernel  labels[p] = labels[p] < 0 ? 0 : parent[labels[p]], and the component sizes by integer atomic adds: one add of the
//                       popcount per wave where all its foreground lanes carry one label (the body of a vertebra), else one per lane.
//   ccl_info_kernel     one workgroup: n, the largest component (ties: the lowest label), its size, a status word, the capped size table.
// hv_clean_components adds ccl_clean_kernel (the filter); hv_fill_holes labels the complement of F with c = 1 up to the flatten step, marks
// the roots that reach one of the six faces (ccl_faces_kernel) and fills the rest (ccl_fill_kernel).
// No workgroup ever waits for another one: the phases are separated by kernel boundaries only.  Only integer atomics: the results are a pure
// function of the input, bit for bit the same on every run.  No host synchronisation, no scratch; raster indices are int32 (<= 2^30 voxels),
// element offsets into the volume 64-bit.
#include "volume_access.h"                  // hv_up16

#define CC_T0 4
#define CC_T1 8
#define CC_T2 64
#define CC_TILE (CC_T0 * CC_T1 * CC_T2)      // 2 048 voxels, 8 per lane; local parents: 8 KiB of LDS
#define CC_THREADS 256
#define CC_BLOCK 1024                       // voxels per workgroup of the raster passes = counts per turn of the scan
#define CC_SCAN_THREADS 1024

struct CcSrc { const void* p; int dt; long long s0, s1, s2; double value; int ne; };
struct CcGeo { int A0, A1, A2, n0, n1, n2; };             // n*: tiles per axis

__device__ __forceinline__ bool cc_in(const CcSrc& S, long long o) {
    bool eq;
    switch (S.dt) {
        case HV_DT_U8: eq = (double)((const uint8_t*)S.p)[o] == S.value; break;
        case HV_DT_F32: eq = (double)((const float*)S.p)[o] == S.value; break;
        default: eq = ((const double*)S.p)[o] == S.value; break;
    }
    return eq != (S.ne != 0);
}
__device__ __forceinline__ void cc_put(void* p, int dt, long long o, double v) {
    switch (dt) {
        case HV_DT_U8: ((uint8_t*)p)[o] = (uint8_t)v; break;
        case HV_DT_F32: ((float*)p)[o] = (float)v; break;
        default: ((double*)p)[o] = v; break;
    }
}
__device__ __forceinline__ void cc_copy(const void* s, long long so, void* d, long long dofs, int dt) {
    switch (dt) {
        case HV_DT_U8: ((uint8_t*)d)[dofs] = ((const uint8_t*)s)[so]; break;
        case HV_DT_F32: ((uint32_t*)d)[dofs] = ((const uint32_t*)s)[so]; break;          // bits, so that a NaN's payload survives
        default: ((unsigned long long*)d)[dofs] = ((const unsigned long long*)s)[so]; break;
    }
}

// (da, db, dc) is a backward neighbour offset of connectivity <= c: lexicographically before (0, 0, 0), at most c non-zero entries
__device__ __forceinline__ constexpr bool cc_backward(int da, int db, int dc, int c) {
    return (da < 0 || (da == 0 && (db < 0 || (db == 0 && dc < 0)))) && ((da != 0) + (db != 0) + (dc != 0) <= c);
}

// ---- tile pass: local parents in LDS, shared by the lanes of ONE workgroup (workgroup-scope relaxed atomics)
__device__ __forceinline__ int cc_lld(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int cc_lfind(int* lp, int x) {
    // terminates: a parent is never larger than its child (initially lp[x] = x, and only atomicMin writes), so x strictly decreases until
    // lp[x] == x, and x >= 0
    for (;;) {
        const int q = cc_lld(lp + x);
        if (q == x) return x;
        x = q;
    }
}
__device__ __forceinline__ void cc_lunion(int* lp, int a, int b) {
    // terminates: a and b never grow (find only descends); a turn that does not return replaces the larger root b by old < b, so a + b
    // strictly decreases from turn to turn and is >= 0
    for (;;) {
        a = cc_lfind(lp, a);
        b = cc_lfind(lp, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(lp + b, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == b) return;                      // b was a root and now hangs under a
        b = old;                                   // somebody linked b first (old < b): old's set and a's still have to meet
    }
}

__global__ __launch_bounds__(CC_THREADS) void ccl_tile_kernel(CcSrc S, CcGeo G, int conn, int* __restrict__ parent) {
    __shared__ int lp[CC_TILE];
    const int tile = blockIdx.x;
    const int t2 = tile % G.n2, t1 = (tile / G.n2) % G.n1, t0 = tile / (G.n2 * G.n1);
    const int i0 = t0 * CC_T0, j0 = t1 * CC_T1, k0 = t2 * CC_T2;
    for (int l = threadIdx.x; l < CC_TILE; l += CC_THREADS) {
        const int i = i0 + l / (CC_T1 * CC_T2), j = j0 + (l / CC_T2) % CC_T1, k = k0 + l % CC_T2;
        const bool in = i < G.A0 && j < G.A1 && k < G.A2 && cc_in(S, i * S.s0 + j * S.s1 + k * S.s2);
        lp[l] = in ? l : -1;
    }
    __syncthreads();
    for (int l = threadIdx.x; l < CC_TILE; l += CC_THREADS) {
        if (cc_lld(lp + l) < 0) continue;          // (background stays -1 and foreground never becomes negative)
        const int a = l / (CC_T1 * CC_T2), b = (l / CC_T2) % CC_T1, c = l % CC_T2;
#pragma unroll
        for (int da = -1; da <= 0; ++da)
#pragma unroll
            for (int db = -1; db <= 1; ++db)
#pragma unroll
                for (int dc = -1; dc <= 1; ++dc) {
                    if (!cc_backward(da, db, dc, 3)) continue;
                    if ((da != 0) + (db != 0) + (dc != 0) > conn) continue;
                    const int na = a + da, nb = b + db, nc = c + dc;
                    if (na < 0 || nb < 0 || nb >= CC_T1 || nc < 0 || nc >= CC_T2) continue;
                    const int q = (na * CC_T1 + nb) * CC_T2 + nc;
                    if (cc_lld(lp + q) >= 0) cc_lunion(lp, l, q);
                }
    }
    __syncthreads();
    // the local order is the raster order restricted to the tile, so the smallest local index is the smallest raster index
    for (int l = threadIdx.x; l < CC_TILE; l += CC_THREADS) {
        const int i = i0 + l / (CC_T1 * CC_T2), j = j0 + (l / CC_T2) % CC_T1, k = k0 + l % CC_T2;
        if (i >= G.A0 || j >= G.A1 || k >= G.A2) continue;
        int r = -1;
        if (lp[l] >= 0) {
            const int x = cc_lfind(lp, l);         // lp[] is no longer written
            r = ((i0 + x / (CC_T1 * CC_T2)) * G.A1 + j0 + (x / CC_T2) % CC_T1) * G.A2 + k0 + x % CC_T2;
        }
        parent[(i * G.A1 + j) * G.A2 + k] = r;
    }
}

// ---- seam pass: parents in global memory, shared by every workgroup of the launch (agent-scope relaxed atomics, nothing else)
__device__ __forceinline__ int cc_gld(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int cc_gfind(int* parent, int x) {
    // terminates: parent[x] <= x for every value the word ever held (the tile pass wrote the smallest index of a subset that contains x,
    // later writes are fetch_min), so also for a stale value; x strictly decreases until a load gives parent[x] == x, and x >= 0
    for (;;) {
        const int q = cc_gld(parent + x);
        if (q == x) return x;
        x = q;
    }
}
__device__ __forceinline__ void cc_gunion(int* parent, int a, int b) {
    // terminates: as cc_lunion -- a turn that does not return continues from old < b, a + b strictly decreases and is >= 0.  `a` may be a
    // root that a stale load still showed as one: it is a member of its set and a < b, which is all the link needs.
    for (;;) {
        a = cc_gfind(parent, a);
        b = cc_gfind(parent, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(parent + b, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == b) return;
        b = old;
    }
}

__global__ __launch_bounds__(CC_THREADS) void ccl_seam_kernel(CcGeo G, int conn, int N, int* parent) {
    const long long gp = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
    if (gp >= N) return;
    const int p = (int)gp;
    const int k = p % G.A2, j = (p / G.A2) % G.A1, i = p / (G.A2 * G.A1);
    // only voxels on the low faces of their tile, or on its high j / k faces, have a backward neighbour in another tile
    if (i % CC_T0 != 0 && j % CC_T1 != 0 && j % CC_T1 != CC_T1 - 1 && k % CC_T2 != 0 && k % CC_T2 != CC_T2 - 1) return;
    if (cc_gld(parent + p) < 0) return;
#pragma unroll
    for (int da = -1; da <= 0; ++da)
#pragma unroll
        for (int db = -1; db <= 1; ++db)
#pragma unroll
            for (int dc = -1; dc <= 1; ++dc) {
                if (!cc_backward(da, db, dc, 3)) continue;
                if ((da != 0) + (db != 0) + (dc != 0) > conn) continue;
                const int ni = i + da, nj = j + db, nk = k + dc;
                if (ni < 0 || nj < 0 || nj >= G.A1 || nk < 0 || nk >= G.A2) continue;
                if (ni / CC_T0 == i / CC_T0 && nj / CC_T1 == j / CC_T1 && nk / CC_T2 == k / CC_T2) continue;      // the tile pass joined these
                const int q = (ni * G.A1 + nj) * G.A2 + nk;
                if (cc_gld(parent + q) >= 0) cc_gunion(parent, p, q);
            }
}

// ---- raster passes: CC_BLOCK consecutive voxels per workgroup, voxel blockIdx.x * CC_BLOCK + u * CC_THREADS + threadIdx.x in turn u
__global__ __launch_bounds__(CC_THREADS) void ccl_flatten_kernel(const int* __restrict__ parent, int N, int* __restrict__ labels,
                                                                 int* __restrict__ sizes, int* __restrict__ bcount) {
    __shared__ int cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    int mine = 0;
    for (int u = 0; u < CC_BLOCK / CC_THREADS; ++u) {
        const long long gp = (long long)blockIdx.x * CC_BLOCK + u * CC_THREADS + threadIdx.x;
        if (gp >= N) break;
        const int p = (int)gp;
        int x = parent[p];
        if (x >= 0) {
            // terminates: parent[x] <= x, nothing writes parent[] in this launch; x strictly decreases to a root, x >= 0
            for (int q = parent[x]; q != x; q = parent[x]) x = q;
        }
        labels[p] = x;
        sizes[p] = 0;
        if (p == 0) sizes[N] = 0;
        mine += x == p;
    }
    if (mine) atomicAdd(&cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) bcount[blockIdx.x] = cnt;
}

// exclusive offsets of the per-block counts, in place; info[0] = the total.  nblk is a launch argument: the loop's length is known on the host.
__global__ __launch_bounds__(CC_SCAN_THREADS) void ccl_scan_kernel(int* __restrict__ bcount, int nblk, int* __restrict__ info) {
    __shared__ int wsum[CC_SCAN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int carry = 0;
    for (int base = 0; base < nblk; base += CC_SCAN_THREADS) {
        const int e = base + tid;
        const int v = e < nblk ? bcount[e] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(inc, o, 64);
            if (lane >= o) inc += y;
        }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int q = 0; q < CC_SCAN_THREADS / 64; ++q) {
            const int s = wsum[q];
            before += q < w ? s : 0;
            total += s;
        }
        if (e < nblk) bcount[e] = carry + before + inc - v;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) info[0] = carry;
}

__global__ __launch_bounds__(CC_THREADS) void ccl_rank_kernel(const int* __restrict__ labels, const int* __restrict__ boff, int N,
                                                              int* __restrict__ parent) {
    __shared__ int part[CC_BLOCK / 64];            // roots per (turn, wave), in raster order
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int before[CC_BLOCK / CC_THREADS];
    bool root[CC_BLOCK / CC_THREADS];
#pragma unroll
    for (int u = 0; u < CC_BLOCK / CC_THREADS; ++u) {
        const long long gp = (long long)blockIdx.x * CC_BLOCK + u * CC_THREADS + threadIdx.x;
        root[u] = gp < N && labels[gp < N ? gp : 0] == (int)gp;
        const unsigned long long m = __ballot(root[u]);
        before[u] = __popcll(m & ((1ULL << lane) - 1ULL));
        if (lane == 0) part[u * (CC_THREADS / 64) + w] = __popcll(m);
    }
    __syncthreads();
    const int base = boff[blockIdx.x];
#pragma unroll
    for (int u = 0; u < CC_BLOCK / CC_THREADS; ++u) {
        int pre = 0;
#pragma unroll
        for (int q = 0; q < CC_BLOCK / 64; ++q) pre += q < u * (CC_THREADS / 64) + w ? part[q] : 0;
        if (root[u]) parent[(long long)blockIdx.x * CC_BLOCK + u * CC_THREADS + threadIdx.x] = base + pre + before[u] + 1;
    }
}

__global__ __launch_bounds__(CC_THREADS) void ccl_relabel_kernel(const int* __restrict__ parent, int N, int* __restrict__ labels,
                                                                 int* __restrict__ sizes) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int u = 0; u < CC_BLOCK / CC_THREADS; ++u) {
        const long long gp = (long long)blockIdx.x * CC_BLOCK + u * CC_THREADS + threadIdx.x;
        int lab = 0;
        if (gp < N) {
            const int r = labels[gp];
            lab = r < 0 ? 0 : parent[r];
            labels[gp] = lab;
        }
        const unsigned long long fg = __ballot(lab > 0);
        if (fg == 0ULL) continue;                  // wave-uniform
        const int first = __shfl(lab, __ffsll((long long)fg) - 1, 64);
        const bool one = __ballot(lab > 0 && lab == first) == fg;
        if (one) {
            if (lane == __ffsll((long long)fg) - 1) atomicAdd(&sizes[first], __popcll(fg));
        } else if (lab > 0) {
            atomicAdd(&sizes[lab], 1);
        }
    }
}

// info[0] = n (ccl_scan_kernel).  -> table[0] n, [1] the largest label, [2] its size, [3] status; table[4 + i] = size of label i + 1.
__global__ __launch_bounds__(CC_SCAN_THREADS) void ccl_info_kernel(const int* __restrict__ sizes, const int* __restrict__ info, int cap,
                                                                   int* __restrict__ table) {
    __shared__ int bs[CC_SCAN_THREADS], bl[CC_SCAN_THREADS];
    const int n = info[0], tid = threadIdx.x;
    int best = 0, lab = 0;
    for (int i = 1 + tid; i <= n; i += CC_SCAN_THREADS) {             // ascending labels per lane: '>' keeps the lowest of equals
        const int s = sizes[i];
        if (s > best) { best = s; lab = i; }
        if (i - 1 < cap) table[4 + i - 1] = s;
    }
    for (int i = n + tid; i < cap; i += CC_SCAN_THREADS) table[4 + i] = 0;
    bs[tid] = best; bl[tid] = lab;
    __syncthreads();
    for (int h = CC_SCAN_THREADS / 2; h >= 1; h >>= 1) {
        if (tid < h) {
            const int s = bs[tid + h], l = bl[tid + h];
            if (s > bs[tid] || (s == bs[tid] && s > 0 && l < bl[tid])) { bs[tid] = s; bl[tid] = l; }
        }
        __syncthreads();
    }
    if (tid == 0) { table[0] = n; table[1] = bl[0]; table[2] = bs[0]; table[3] = n == 0 ? 1 : 0; }
}

struct CcOut { void* p; long long s0, s1, s2; int copy; };            // copy 0: out is vol itself, only the changed voxels are written

// a foreground voxel stays iff its component has >= min_size voxels and, with keep_largest, is table[1]
__global__ __launch_bounds__(CC_THREADS) void ccl_clean_kernel(CcSrc S, CcGeo G, int N, const int* __restrict__ labels,
                                                               const int* __restrict__ sizes, const int* __restrict__ table, int min_size,
                                                               int keep_largest, double fill, CcOut O) {
    const long long gp = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
    if (gp >= N) return;
    const int p = (int)gp;
    const int k = p % G.A2, j = (p / G.A2) % G.A1, i = p / (G.A2 * G.A1);
    const long long oo = i * O.s0 + j * O.s1 + k * O.s2;
    const int lab = labels[p];
    const bool drop = lab > 0 && ((min_size > 1 && sizes[lab] < min_size) || (keep_largest && lab != table[1]));
    if (drop) cc_put(O.p, S.dt, oo, fill);
    else if (O.copy) cc_copy(S.p, i * S.s0 + j * S.s1 + k * S.s2, O.p, oo, S.dt);
}

// labels[]: the roots of the COMPLEMENT's 6-connected components.  A root whose component has a voxel on a face of the volume is marked;
// every lane that marks a word stores the same 1, and nothing reads mark[] in this launch.  Lane 0 clears the four table words.
__global__ __launch_bounds__(CC_THREADS) void ccl_faces_kernel(CcGeo G, int N, const int* __restrict__ labels, int* __restrict__ mark,
                                                               int* __restrict__ table) {
    const long long gp = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
    if (gp == 0) { table[0] = 0; table[1] = 0; table[2] = 0; table[3] = 0; }
    if (gp >= N) return;
    const int p = (int)gp;
    const int k = p % G.A2, j = (p / G.A2) % G.A1, i = p / (G.A2 * G.A1);
    if (i != 0 && i != G.A0 - 1 && j != 0 && j != G.A1 - 1 && k != 0 && k != G.A2 - 1) return;
    const int r = labels[p];
    if (r >= 0) mark[r] = 1;
}

// unmarked components of the complement become `fill`; table[0] += holes, table[2] += voxels (integer adds, one per wave and word)
__global__ __launch_bounds__(CC_THREADS) void ccl_fill_kernel(CcSrc S, CcGeo G, int N, const int* __restrict__ labels,
                                                              const int* __restrict__ mark, double fill, CcOut O, int* __restrict__ table) {
    const long long gp = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
    bool hole = false, root = false;
    if (gp < N) {
        const int p = (int)gp;
        const int k = p % G.A2, j = (p / G.A2) % G.A1, i = p / (G.A2 * G.A1);
        const long long oo = i * O.s0 + j * O.s1 + k * O.s2;
        const int r = labels[p];
        hole = r >= 0 && mark[r] == 0;
        root = hole && r == p;
        if (hole) cc_put(O.p, S.dt, oo, fill);
        else if (O.copy) cc_copy(S.p, i * S.s0 + j * S.s1 + k * S.s2, O.p, oo, S.dt);
    }
    const unsigned long long mh = __ballot(hole), mr = __ballot(root);
    if ((threadIdx.x & 63) == 0) {
        if (mh) atomicAdd(&table[2], __popcll(mh));
        if (mr) atomicAdd(&table[0], __popcll(mr));
    }
}

// ------------------------------------------------------------------------------------------------ host side
static inline bool cc_dims_ok(int A0, int A1, int A2) { return A0 > 0 && A1 > 0 && A2 > 0; }
static inline bool cc_dtype_ok(int dt) { return dt == HV_DT_U8 || dt == HV_DT_F32 || dt == HV_DT_F64; }
struct CcWs { size_t parent, sizes, labels, bcount, info, total; };
static CcWs cc_layout(int A0, int A1, int A2) {
    const size_t N = (size_t)A0 * A1 * A2;
    CcWs W;
    size_t o = 0;
    W.parent = o; o += hv_up16(N * 4);
    W.sizes = o; o += hv_up16((N + 1) * 4);
    W.labels = o; o += hv_up16(N * 4);
    W.bcount = o; o += hv_up16((size_t)hv_cdiv((long long)N, CC_BLOCK) * 4);
    W.info = o; o += 16;
    W.total = o;
    return W;
}

extern "C" size_t hv_label3d_workspace_bytes(int A0, int A1, int A2) {
    if (!cc_dims_ok(A0, A1, A2)) return 0;
    return cc_layout(A0, A1, A2).total;
}

extern "C" int hv_label3d_tile(int* dims) {
    if (!dims) return HV_ERR_ARG;
    dims[0] = CC_T0; dims[1] = CC_T1; dims[2] = CC_T2;
    return HV_OK;
}

// what the three entries check alike; HV_OK, or the refusal
static int cc_check(const void* vol, int dtype, int A0, int A1, int A2, int mode, int conn, const void* table, const void* workspace,
                    size_t workspace_bytes) {
    if (!vol || !table || !workspace || !cc_dims_ok(A0, A1, A2) || !cc_dtype_ok(dtype) || (mode != HV_CCL_EQ && mode != HV_CCL_NE) || conn < 1 ||
        conn > 3 || ((uintptr_t)table & 3) || ((uintptr_t)workspace & 15))
        return HV_ERR_ARG;
    if ((long long)A0 * A1 * A2 > (1LL << 30)) return HV_ERR_UNSUPPORTED;
    if (workspace_bytes < hv_label3d_workspace_bytes(A0, A1, A2)) return HV_ERR_ARG;
    return HV_OK;
}

static CcGeo cc_geo(int A0, int A1, int A2) {
    CcGeo G;
    G.A0 = A0; G.A1 = A1; G.A2 = A2;
    G.n0 = hv_cdiv(A0, CC_T0); G.n1 = hv_cdiv(A1, CC_T1); G.n2 = hv_cdiv(A2, CC_T2);
    return G;
}

// tile pass, seam pass, flatten: labels[p] = the smallest raster index of p's component (-1: background), sizes[0..N] = 0, bcount = roots per block
static int cc_roots(const CcSrc& S, const CcGeo& G, int conn, int* parent, int* labels, int* sizes, int* bcount, hipStream_t st) {
    const int N = G.A0 * G.A1 * G.A2;
    const long long tiles = (long long)G.n0 * G.n1 * G.n2;
    hipLaunchKernelGGL(ccl_tile_kernel, dim3((unsigned)tiles), dim3(CC_THREADS), 0, st, S, G, conn, parent);
    HV_LAUNCH_CHECK();
    hipLaunchKernelGGL(ccl_seam_kernel, dim3(hv_cdiv(N, CC_THREADS)), dim3(CC_THREADS), 0, st, G, conn, N, parent);
    HV_LAUNCH_CHECK();
    hipLaunchKernelGGL(ccl_flatten_kernel, dim3(hv_cdiv(N, CC_BLOCK)), dim3(CC_THREADS), 0, st, (const int*)parent, N, labels, sizes, bcount);
    HV_LAUNCH_CHECK();
    return HV_OK;
}

// the whole labelling: labels 0 / 1..n, sizes[1..n], table
static int cc_label(const CcSrc& S, const CcGeo& G, int conn, int* labels, int* table, int cap, char* ws, const CcWs& W, hipStream_t st) {
    const int N = G.A0 * G.A1 * G.A2, nblk = hv_cdiv(N, CC_BLOCK);
    int *parent = (int*)(ws + W.parent), *sizes = (int*)(ws + W.sizes), *bcount = (int*)(ws + W.bcount), *info = (int*)(ws + W.info);
    const int e = cc_roots(S, G, conn, parent, labels, sizes, bcount, st);
    if (e != HV_OK) return e;
    hipLaunchKernelGGL(ccl_scan_kernel, dim3(1), dim3(CC_SCAN_THREADS), 0, st, bcount, nblk, info);
    HV_LAUNCH_CHECK();
    hipLaunchKernelGGL(ccl_rank_kernel, dim3(nblk), dim3(CC_THREADS), 0, st, (const int*)labels, (const int*)bcount, N, parent);
    HV_LAUNCH_CHECK();
    hipLaunchKernelGGL(ccl_relabel_kernel, dim3(nblk), dim3(CC_THREADS), 0, st, (const int*)parent, N, labels, sizes);
    HV_LAUNCH_CHECK();
    hipLaunchKernelGGL(ccl_info_kernel, dim3(1), dim3(CC_SCAN_THREADS), 0, st, (const int*)sizes, (const int*)info, cap, table);
    HV_LAUNCH_CHECK();
    return HV_OK;
}

extern "C" int hv_label3d(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, double value, int mode,
                          int connectivity, int* labels, int* table, int table_cap, void* workspace, size_t workspace_bytes, void* stream) {
    if (!labels || ((uintptr_t)labels & 3) || table_cap < 0) return HV_ERR_ARG;
    const int rc = cc_check(vol, dtype, A0, A1, A2, mode, connectivity, table, workspace, workspace_bytes);
    if (rc != HV_OK) return rc;
    CcSrc S;
    S.p = vol; S.dt = dtype; S.s0 = s0; S.s1 = s1; S.s2 = s2; S.value = value; S.ne = mode == HV_CCL_NE;
    return cc_label(S, cc_geo(A0, A1, A2), connectivity, labels, table, table_cap, (char*)workspace, cc_layout(A0, A1, A2), (hipStream_t)stream);
}

// out == vol needs equal strides (each voxel then reads and writes its own element only, and the apply launch does not read vol at all)
static bool cc_out_ok(const void* vol, long long s0, long long s1, long long s2, const void* out, long long os0, long long os1, long long os2) {
    return out && (out != vol || (os0 == s0 && os1 == s1 && os2 == s2));
}

extern "C" int hv_clean_components(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, double value,
                                   int mode, int connectivity, int min_size, int keep_largest, double fill, void* out, long long os0,
                                   long long os1, long long os2, int* table, void* workspace, size_t workspace_bytes, void* stream) {
    if (!cc_out_ok(vol, s0, s1, s2, out, os0, os1, os2) || (keep_largest != 0 && keep_largest != 1)) return HV_ERR_ARG;
    const int rc = cc_check(vol, dtype, A0, A1, A2, mode, connectivity, table, workspace, workspace_bytes);
    if (rc != HV_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const CcWs W = cc_layout(A0, A1, A2);
    const CcGeo G = cc_geo(A0, A1, A2);
    char* ws = (char*)workspace;
    int* labels = (int*)(ws + W.labels);
    CcSrc S;
    S.p = vol; S.dt = dtype; S.s0 = s0; S.s1 = s1; S.s2 = s2; S.value = value; S.ne = mode == HV_CCL_NE;
    const int e = cc_label(S, G, connectivity, labels, table, 0, ws, W, st);
    if (e != HV_OK) return e;
    CcOut O;
    O.p = out; O.s0 = os0; O.s1 = os1; O.s2 = os2; O.copy = out != vol;
    const int N = A0 * A1 * A2;
    hipLaunchKernelGGL(ccl_clean_kernel, dim3(hv_cdiv(N, CC_THREADS)), dim3(CC_THREADS), 0, st, S, G, N, (const int*)labels,
                       (const int*)(ws + W.sizes), (const int*)table, min_size, keep_largest, fill, O);
    HV_LAUNCH_CHECK();
    return HV_OK;
}

extern "C" int hv_fill_holes(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, double value, int mode,
                             double fill, void* out, long long os0, long long os1, long long os2, int* table, void* workspace,
                             size_t workspace_bytes, void* stream) {
    if (!cc_out_ok(vol, s0, s1, s2, out, os0, os1, os2)) return HV_ERR_ARG;
    const int rc = cc_check(vol, dtype, A0, A1, A2, mode, 1, table, workspace, workspace_bytes);
    if (rc != HV_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const CcWs W = cc_layout(A0, A1, A2);
    const CcGeo G = cc_geo(A0, A1, A2);
    char* ws = (char*)workspace;
    int *labels = (int*)(ws + W.labels), *mark = (int*)(ws + W.sizes);
    CcSrc S;
    S.p = vol; S.dt = dtype; S.s0 = s0; S.s1 = s1; S.s2 = s2; S.value = value; S.ne = mode != HV_CCL_NE;      // the complement
    const int e = cc_roots(S, G, 1, (int*)(ws + W.parent), labels, mark, (int*)(ws + W.bcount), st);
    if (e != HV_OK) return e;
    const int N = A0 * A1 * A2;
    hipLaunchKernelGGL(ccl_faces_kernel, dim3(hv_cdiv(N, CC_THREADS)), dim3(CC_THREADS), 0, st, G, N, (const int*)labels, mark, table);
    HV_LAUNCH_CHECK();
    CcOut O;
    O.p = out; O.s0 = os0; O.s1 = os1; O.s2 = os2; O.copy = out != vol;
    hipLaunchKernelGGL(ccl_fill_kernel, dim3(hv_cdiv(N, CC_THREADS)), dim3(CC_THREADS), 0, st, S, G, N, (const int*)labels, (const int*)mark, fill,
                       O, table);
    HV_LAUNCH_CHECK();
    return HV_OK;
}
