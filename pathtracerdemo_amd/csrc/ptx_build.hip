// ptx_build.hip -- ptx_build_blas' kernels: a mesh's BLAS built on the device as an LBVH, in the reference's
// serialisation (include/ptx.h states the tree; pathtracerdemo_amd/scene/lbvh.py is the same rule in numpy).
//
//   build_tris     one thread per triangle: its box and centre by the builder's record (ptx_tribox.h), its
//                  segment (group or gap), and the group's centre bounds by atomic max on ordered words
//                  (min and max are order-independent; a wave that lies in one group reduces first);
//   build_keys     one thread per triangle: the 30-bit code, the sort key segment << 30 | code;
//   (the sort)     hipcub::DeviceRadixSort::SortPairs, stable, the value the input position: gaps keep
//                  their place, a group its range;
//   build_tree     one thread per internal node of a group's binary radix tree over K_p = code_p 2^32 + p
//                  (Karras 2012): direction, range, split, its children's parent words;
//   build_leaves   one thread per radix node: a node of at most max_leaf triangles under a larger parent
//                  (or a root) is an emitted leaf -- its box is reduced over its triangles;
//   build_level    one launch per height, one thread per internal node: a node whose two children were
//                  finished by an EARLIER launch (their stamp is below this launch's) takes their union and
//                  1 + their emitted sizes.  Launch boundaries are the only ordering: no workgroup waits for
//                  another, nothing spins, and a node's result does not depend on which launch reached it;
//   build_roots    one thread per group: its root's emitted size (0: not finished yet) for the host's
//                  prefix sum -- the only readback before the output;
//   build_emit     one thread per radix node: an emitted node finds its depth-first index and its depth by
//                  walking its parent chain (1 per ancestor, plus the left sibling's emitted size where it is
//                  a right child) and writes its 8 words;
//   build_gather   one thread per triangle: the reordered index buffer.
//
//   build_positions   (ptx_rebuild_mesh, either builder) one thread per vertex: words 0..2 of a loaded mesh's
//                  8-word records in the geometry array to the packed positions the chains above read.
#include <hipcub/hipcub.hpp>

#include "ptx_launch.h"
#include "ptx_tribox.h"

namespace ptx {

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kSkip = 0xFFFFFFFFu;  // done[]: a slot build_level never looks at again
constexpr uint32_t kCodeBits = 30u, kCodeMask = (1u << kCodeBits) - 1u;

// f32 -> u32 with the floats' order (-0 below +0)
__device__ __forceinline__ uint32_t ordered(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unordered(uint32_t e) {
    return __uint_as_float((e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e);
}

// bit k of a 10-bit q to bit 3k
__device__ __forceinline__ uint32_t spread3(uint32_t x) {
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

// One axis' cell number: every operation in f64, rounded on its own.
__device__ __forceinline__ uint32_t cell(float c, float cmin, float cmax) {
#pragma clang fp contract(off)
    if (cmax == cmin) return 0u;
    const double num = ((double)c - (double)cmin) * 1024.0;
    const double den = (double)cmax - (double)cmin;
    return (uint32_t)fmin(floor(num / den), 1023.0);
}

// The segment of triangle t: 2g + 1 inside group g, 2g in the gap ahead of group g (2 n_groups behind the last).
__device__ __forceinline__ uint32_t segment_of(const BuildArgs &A, uint32_t t) {
    uint32_t lo = 0u, hi = A.n_groups;  // the first group whose first triangle lies past t
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (A.groups[mid].x <= t) lo = mid + 1u;
        else hi = mid;
    }
    if (lo > 0u) {
        const uint2 g = A.groups[lo - 1u];
        if (t - g.x < g.y) return 2u * (lo - 1u) + 1u;
    }
    return 2u * lo;
}

__device__ __forceinline__ uint32_t code_at(const BuildArgs &A, uint32_t p) { return (uint32_t)A.key_out[p] & kCodeMask; }

// The length of the common prefix of K_i and K_j, positions i and j = i + step of a group of n triangles that
// begins at sorted position `first`; -1 where j lies outside the group.
__device__ __forceinline__ int prefix(const BuildArgs &A, uint32_t first, int n, int i, int j) {
    if (j < 0 || j >= n) return -1;
    const uint32_t x = code_at(A, first + (uint32_t)i) ^ code_at(A, first + (uint32_t)j);
    return x ? __clz((int)x) : 32 + __clz(i ^ j);
}

__device__ __forceinline__ void box_store(float2 *dst, const float lo[3], const float hi[3]) {
    dst[0] = make_float2(lo[0], lo[1]);
    dst[1] = make_float2(lo[2], hi[0]);
    dst[2] = make_float2(hi[1], hi[2]);
}

// The triangles a radix node covers, as sorted positions [a, b], and its parent; false for a slot that is no
// node (a gap, or the last slot of a group's internal range).
__device__ __forceinline__ bool node_range(const BuildArgs &A, uint32_t id, uint32_t &a, uint32_t &b) {
    const uint32_t T = A.n_tris, p = id < T ? id : id - T;
    const uint32_t s = A.seg[p];
    if (!(s & 1u)) return false;
    if (id >= T) {
        a = b = p;
        return true;
    }
    const uint2 g = A.groups[s >> 1];
    if (p - g.x + 1u >= g.y) return false;
    const uint2 r = A.rng[id];
    a = r.x;
    b = r.y;
    return true;
}

}  // namespace

__global__ __launch_bounds__(kBlock) void build_tris(BuildArgs A) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    const bool live = t < A.n_tris;
    uint32_t s = kNone, emin[3] = {0u, 0u, 0u}, emax[3] = {0u, 0u, 0u};
    if (live) {
        float P[3][3];
        for (int v = 0; v < 3; ++v) {
            const float *p = A.pos + 3u * (size_t)A.idx[3u * (size_t)t + v];
            for (int k = 0; k < 3; ++k) P[v][k] = p[k];
        }
        float lo[3], hi[3], c[3];
        for (int k = 0; k < 3; ++k) tri_axis_bounds(P[0][k], P[1][k], P[2][k], lo[k], hi[k], c[k]);
        box_store(A.tbox + 3u * (size_t)t, lo, hi);
        for (int k = 0; k < 3; ++k) A.centre[3u * (size_t)t + k] = c[k];
        s = segment_of(A, t);
        A.seg[t] = s;
        for (int k = 0; k < 3; ++k) {
            emin[k] = ~ordered(c[k]);  // (the minimum as the maximum of the complement: both tables start at 0)
            emax[k] = ordered(c[k]);
        }
    }
    // the group's centre bounds: one atomic per wave and word where the wave lies in one group
    const uint32_t s0 = __shfl(s, 0);  // (kNone: lane 0 and with it the whole wave lies past the last triangle)
    const bool grouped = live && (s & 1u);
    if (s0 != kNone && (s0 & 1u) && __all(!live || s == s0)) {
        for (int k = 0; k < 3; ++k)
            for (int m = warpSize / 2; m > 0; m >>= 1) {
                emin[k] = max(emin[k], (uint32_t)__shfl_xor((int)emin[k], m));
                emax[k] = max(emax[k], (uint32_t)__shfl_xor((int)emax[k], m));
            }
        if ((threadIdx.x & (warpSize - 1)) == 0)
            for (int k = 0; k < 3; ++k) {
                atomicMax(A.cbound + 6u * (size_t)(s0 >> 1) + k, emin[k]);
                atomicMax(A.cbound + 6u * (size_t)(s0 >> 1) + 3u + k, emax[k]);
            }
    } else if (grouped) {
        for (int k = 0; k < 3; ++k) {
            atomicMax(A.cbound + 6u * (size_t)(s >> 1) + k, emin[k]);
            atomicMax(A.cbound + 6u * (size_t)(s >> 1) + 3u + k, emax[k]);
        }
    }
}

__global__ __launch_bounds__(kBlock) void build_keys(BuildArgs A) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= A.n_tris) return;
    const uint32_t s = A.seg[t];
    uint32_t code = 0u;
    if (s & 1u) {
        const uint32_t *cb = A.cbound + 6u * (size_t)(s >> 1);
        for (int k = 0; k < 3; ++k)
            code |= spread3(cell(A.centre[3u * (size_t)t + k], unordered(~cb[k]), unordered(cb[3 + k]))) << (2 - k);
    }
    A.key_in[t] = (unsigned long long)s << kCodeBits | code;
    A.val_in[t] = t;
}

__global__ __launch_bounds__(kBlock) void build_tree(BuildArgs A) {
    const uint32_t id = blockIdx.x * kBlock + threadIdx.x;
    if (id >= A.n_tris) return;
    const uint32_t s = A.seg[id];
    const uint2 g = (s & 1u) ? A.groups[s >> 1] : make_uint2(0u, 0u);
    const int n = (int)g.y, i = (int)(id - g.x);
    if (!(s & 1u) || i + 1 >= n) {
        A.done[id] = kSkip;
        return;
    }
    const uint32_t first = g.x;
    const int d = prefix(A, first, n, i, i + 1) - prefix(A, first, n, i, i - 1) > 0 ? 1 : -1;
    const int dmin = prefix(A, first, n, i, i - d);
    int lmax = 2;
    while (prefix(A, first, n, i, i + lmax * d) > dmin) lmax *= 2;  // (ends: past the group the prefix is -1)
    int l = 0;
    for (int u = lmax / 2; u >= 1; u /= 2)
        if (prefix(A, first, n, i, i + (l + u) * d) > dmin) l += u;
    const int j = i + l * d;
    const int dnode = prefix(A, first, n, i, j);
    int sp = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (prefix(A, first, n, i, i + (sp + t) * d) > dnode) sp += t;
    } while (t > 1);
    const int split = i + sp * d + min(d, 0);  // the last position of the left child
    const int a = min(i, j), b = max(i, j);
    const uint32_t T = A.n_tris;
    const uint32_t left = (split == a ? T : 0u) + first + (uint32_t)split;
    const uint32_t right = (split + 1 == b ? T : 0u) + first + (uint32_t)split + 1u;
    A.rng[id] = make_uint2(first + (uint32_t)a, first + (uint32_t)b);
    A.child[id] = make_uint2(left, right);
    A.parent[left] = id;
    A.parent[right] = id;
    A.done[id] = (uint32_t)(b - a + 1) > A.max_leaf ? 0u : kSkip;
}

__global__ __launch_bounds__(kBlock) void build_leaves(BuildArgs A) {
    const uint32_t id = blockIdx.x * kBlock + threadIdx.x;
    if (id >= 2u * A.n_tris) return;
    uint32_t a, b;
    if (!node_range(A, id, a, b) || b - a + 1u > A.max_leaf) return;
    const uint32_t par = A.parent[id];
    if (par != kNone) {
        const uint2 r = A.rng[par];
        if (r.y - r.x + 1u <= A.max_leaf) return;  // inside an emitted leaf
    }
    float lo[3] = {HUGE_VALF, HUGE_VALF, HUGE_VALF}, hi[3] = {-HUGE_VALF, -HUGE_VALF, -HUGE_VALF};
    for (uint32_t p = a; p <= b; ++p) {
        const float2 *bx = A.tbox + 3u * (size_t)A.val_out[p];
        const float2 u = bx[0], v = bx[1], w = bx[2];
        lo[0] = fminf(lo[0], u.x); lo[1] = fminf(lo[1], u.y); lo[2] = fminf(lo[2], v.x);
        hi[0] = fmaxf(hi[0], v.y); hi[1] = fmaxf(hi[1], w.x); hi[2] = fmaxf(hi[2], w.y);
    }
    box_store(A.nbox + 3u * (size_t)id, lo, hi);
    A.esize[id] = 1u;
    A.done[id] = 1u;
}

// `stamp` (2, 3, ...) is this launch's; a child counts as finished only with a smaller one, so a thread
// never reads what another thread of its own launch is writing.
__global__ __launch_bounds__(kBlock) void build_level(BuildArgs A, uint32_t stamp) {
    const uint32_t id = blockIdx.x * kBlock + threadIdx.x;
    if (id >= A.n_tris || A.done[id] != 0u) return;
    const uint2 c = A.child[id];
    const uint32_t dl = A.done[c.x], dr = A.done[c.y];
    if (dl == 0u || dl >= stamp || dr == 0u || dr >= stamp) return;
    const float2 *L = A.nbox + 3u * (size_t)c.x, *R = A.nbox + 3u * (size_t)c.y;
    float2 *out = A.nbox + 3u * (size_t)id;
    const float2 l0 = L[0], l1 = L[1], l2 = L[2], r0 = R[0], r1 = R[1], r2 = R[2];
    out[0] = make_float2(fminf(l0.x, r0.x), fminf(l0.y, r0.y));
    out[1] = make_float2(fminf(l1.x, r1.x), fmaxf(l1.y, r1.y));
    out[2] = make_float2(fmaxf(l2.x, r2.x), fmaxf(l2.y, r2.y));
    A.esize[id] = 1u + A.esize[c.x] + A.esize[c.y];
    A.done[id] = stamp;
}

__global__ __launch_bounds__(kBlock) void build_roots(BuildArgs A) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= A.n_groups) return;
    const uint2 r = A.groups[g];
    const uint32_t root = r.y == 1u ? A.n_tris + r.x : r.x;
    const uint32_t d = A.done[root];
    A.gsize[g] = (d != 0u && d != kSkip) ? A.esize[root] : 0u;
}

__global__ __launch_bounds__(kBlock) void build_emit(BuildArgs A) {
    const uint32_t id = blockIdx.x * kBlock + threadIdx.x;
    if (id >= 2u * A.n_tris) return;
    const uint32_t d = A.done[id];
    if (d == 0u || d == kSkip) return;  // not an emitted node
    uint32_t a, b;
    if (!node_range(A, id, a, b)) return;
    const uint32_t g = A.seg[a] >> 1;
    // the parent chain: 128 bounds the walk (a key has 62 bits)
    uint32_t index = 0u, depth = 0u;
    for (uint32_t cur = id, par = A.parent[id]; par != kNone && depth < 128u; cur = par, par = A.parent[par]) {
        const uint2 c = A.child[par];
        index += 1u + (c.y == cur ? A.esize[c.x] : 0u);
        depth += 1u;
    }
    if (index >= A.gsize[g]) return;  // (cannot happen: keeps a store inside the output whatever the tables hold)
    const size_t node = (size_t)A.goff[g] + index;
    if (node >= A.n_nodes) return;
    uint32_t w6, w7;
    if (b - a + 1u <= A.max_leaf) {
        w6 = a;
        w7 = 0xFFFF0000u | (b - a + 1u);
        atomicMax(A.max_depth, depth);
    } else {
        w6 = 8u * (index + 1u + A.esize[A.child[id].x]);
        const uint32_t x = code_at(A, a) ^ code_at(A, b);
        w7 = x ? 2u - (uint32_t)(31 - __clz((int)x)) % 3u : 0u;
    }
    const float2 *bx = A.nbox + 3u * (size_t)id;
    const float2 u = bx[0], v = bx[1], w = bx[2];
    uint4 *out = reinterpret_cast<uint4 *>(A.nodes_out + 8u * node);
    out[0] = make_uint4(__float_as_uint(u.x), __float_as_uint(u.y), __float_as_uint(v.x), __float_as_uint(v.y));
    out[1] = make_uint4(__float_as_uint(w.x), __float_as_uint(w.y), w6, w7);
}

__global__ __launch_bounds__(kBlock) void build_gather(BuildArgs A) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= A.n_tris) return;
    const uint32_t src = A.val_out[p];
    if (src >= A.n_tris) return;
    for (int k = 0; k < 3; ++k) A.idx_out[3u * (size_t)p + k] = A.idx[3u * (size_t)src + k];
}

// ptx_rebuild_mesh's way in: one thread per vertex, words 0..2 of its 8-word record to the packed positions.
__global__ __launch_bounds__(kBlock) void build_positions(const uint32_t *__restrict__ G, uint32_t vertex_word, uint32_t n_vertices,
                                                          float *__restrict__ pos) {
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= n_vertices) return;
    const uint32_t *rec = G + vertex_word + 8u * (size_t)v;
    for (int k = 0; k < 3; ++k) pos[3u * (size_t)v + k] = __uint_as_float(rec[k]);
}

static dim3 build_grid(uint32_t threads) { return dim3((threads + kBlock - 1) / kBlock); }

hipError_t launch_build_positions(const uint32_t *G, uint32_t vertex_word, uint32_t n_vertices, float *pos, hipStream_t s) {
    hipLaunchKernelGGL(build_positions, build_grid(n_vertices), dim3(kBlock), 0, s, G, vertex_word, n_vertices, pos);
    return hipGetLastError();
}

static uint32_t key_bits(const BuildArgs &A) {
    uint32_t bits = kCodeBits + 1u;
    while (bits < 64u && (2ull * A.n_groups) >> (bits - kCodeBits)) ++bits;
    return bits;
}

hipError_t build_sort_bytes(const BuildArgs &A, size_t *bytes) {
    *bytes = 0;
    return hipcub::DeviceRadixSort::SortPairs(nullptr, *bytes, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                              (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)A.n_tris, 0, (int)key_bits(A));
}

hipError_t launch_build(const BuildArgs &A, BuildStep step, uint32_t stamp, hipStream_t s) {
    const uint32_t T = A.n_tris;
    switch (step) {
    case BuildStep::Tris: hipLaunchKernelGGL(build_tris, build_grid(T), dim3(kBlock), 0, s, A); break;
    case BuildStep::Keys: hipLaunchKernelGGL(build_keys, build_grid(T), dim3(kBlock), 0, s, A); break;
    case BuildStep::Sort: {
        size_t bytes = A.sort_bytes;
        return hipcub::DeviceRadixSort::SortPairs(A.sort_temp, bytes, (const unsigned long long *)A.key_in, A.key_out,
                                                  (const uint32_t *)A.val_in, A.val_out, (int)T, 0, (int)key_bits(A), s);
    }
    case BuildStep::Tree: hipLaunchKernelGGL(build_tree, build_grid(T), dim3(kBlock), 0, s, A); break;
    case BuildStep::Leaves: hipLaunchKernelGGL(build_leaves, build_grid(2u * T), dim3(kBlock), 0, s, A); break;
    case BuildStep::Level: hipLaunchKernelGGL(build_level, build_grid(T), dim3(kBlock), 0, s, A, stamp); break;
    case BuildStep::Roots: hipLaunchKernelGGL(build_roots, build_grid(A.n_groups), dim3(kBlock), 0, s, A); break;
    case BuildStep::Emit: hipLaunchKernelGGL(build_emit, build_grid(2u * T), dim3(kBlock), 0, s, A); break;
    case BuildStep::Gather: hipLaunchKernelGGL(build_gather, build_grid(T), dim3(kBlock), 0, s, A); break;
    }
    return hipGetLastError();
}

}  // namespace ptx
