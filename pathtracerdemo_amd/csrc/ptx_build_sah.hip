// ptx_build_sah.hip -- ptx_build_blas' second builder (PTX_BLAS_SAH): the host builder's binned-SAH tree with a
// stable partition, built top-down on the device, one launch per level (include/ptx.h states the rule;
// pathtracerdemo_amd/scene/sah.py is the same rule in numpy).
//
//   sah_init     one thread per triangle: its record (ptx_tribox.h: centre and half-extent in f32) and its own
//                position as the starting order; one thread per group: the root's range;
//   sah_level    one launch per depth, one workgroup per live node.  A node's triangles are a contiguous range
//                of the current order, so the workgroup needs nobody else's data: it reduces its box and centre
//                bounds, bins its triangles into 3 x 32 bins in LDS (integer counts, f64 boxes as ordered 64-bit
//                words under atomic max), lets one lane per axis sweep the 31 candidates in f64, counts the
//                lefts by the compare, and writes its range of the next level's order -- lefts in their order,
//                then rights in theirs.  A leaf writes its range of the final order instead.  Children are two
//                consecutive node ids drawn from a counter, so ids depend on arrival order; nothing that is
//                output does (the emitted index is a function of the tree);
//   sah_size     one launch per depth in reverse, one thread per node: the size of its subtree;
//   sah_emit     one thread per node: its depth-first index by walking its parent chain, its 8 words;
//   sah_gather   one thread per triangle: the reordered index buffer.
//
// Launch boundaries are the only ordering: no workgroup waits for another and nothing spins.  The host reads
// the node counter back after every level to size the next launch.
#include "ptx_launch.h"
#include "ptx_tribox.h"

namespace ptx {

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kLeaf = 3u;  // n_link.z: 0..2 the split axis of an interior node
constexpr int kBins = 32;
constexpr int kWaves = kBlock / 64;
constexpr uint32_t kMaxDepth = 40u;
// an empty bin: the ordered word of -inf, which is also the complement of +inf's
constexpr unsigned long long kEmpty = 0x000FFFFFFFFFFFFFull;

// f64 -> u64 with the doubles' order (-0 below +0), and back
__device__ __forceinline__ unsigned long long ordered(double d) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(d);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double unordered(unsigned long long e) {
    return __longlong_as_double((long long)((e >> 63) ? (e & 0x7FFFFFFFFFFFFFFFull) : ~e));
}

// scene/bvh.py _surface_area on a box given as min and max
__device__ __forceinline__ double area(const double mn[3], const double mx[3]) {
#pragma clang fp contract(off)
    const double d0 = mx[0] - mn[0], d1 = mx[1] - mn[1], d2 = mx[2] - mn[2];
    return 2.0 * ((d0 * d1 + d1 * d2) + d2 * d0);
}

__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask) {
    return (uint32_t)__popcll(mask & ((1ull << (threadIdx.x & 63u)) - 1ull));
}

}  // namespace

__global__ __launch_bounds__(kBlock) void sah_init(SahArgs A) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t < A.n_tris) {
        float P[3][3];
        for (int v = 0; v < 3; ++v) {
            const float *p = A.pos + 3u * (size_t)A.idx[3u * (size_t)t + v];
            for (int k = 0; k < 3; ++k) P[v][k] = p[k];
        }
        float *rec = A.rec + 6u * (size_t)t;
        for (int k = 0; k < 3; ++k) tri_axis_record(P[0][k], P[1][k], P[2][k], rec[k], rec[3 + k]);
        A.order[0][t] = t;
        A.final_order[t] = t;  // (a triangle in no group keeps its place)
    }
    if (t < A.n_groups) {
        A.n_range[t] = A.groups[t];
        A.n_link[t] = make_uint4(kNone, 0u, kLeaf, t);
    }
    if (t == 0u) A.counters[0] = A.n_groups;
}

__global__ __launch_bounds__(kBlock) void sah_level(SahArgs A, uint32_t first_node, uint32_t level) {
#pragma clang fp contract(off)
    __shared__ unsigned long long bins[3][kBins][6];  // [0..2] ~ordered(tmin), [3..5] ordered(tmax): both under max
    __shared__ uint32_t bcount[3][kBins];
    __shared__ double rsa[3][kBins];  // the area of the union of bins i..31
    __shared__ double axis_cost[3];
    __shared__ int axis_cand[3];
    __shared__ float red[kWaves][12];
    __shared__ uint32_t wsum[2][kWaves];
    __shared__ uint32_t s_child;

    const uint32_t node = first_node + blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    const uint2 range = A.n_range[node];
    const uint32_t lo = range.x, count = range.y;
    const uint32_t *in = A.order[level & 1u];
    uint32_t *out = A.order[(level + 1u) & 1u];

    // the node's box (f32 min of lo, max of hi) and the bounds of its centres
    float v[12];  // cmin xyz, bmin xyz under min; cmax xyz, bmax xyz under max
    for (int k = 0; k < 6; ++k) v[k] = HUGE_VALF, v[6 + k] = -HUGE_VALF;
    for (uint32_t i = tid; i < count; i += kBlock) {
        const float *rec = A.rec + 6u * (size_t)in[lo + i];
        for (int k = 0; k < 3; ++k) {
            const float c = rec[k], h = rec[3 + k];
            v[k] = fminf(v[k], c);
            v[3 + k] = fminf(v[3 + k], (float)((double)c - (double)h));
            v[6 + k] = fmaxf(v[6 + k], c);
            v[9 + k] = fmaxf(v[9 + k], (float)((double)c + (double)h));
        }
    }
    for (int k = 0; k < 12; ++k)
        for (int m = 32; m > 0; m >>= 1) {
            const float o = __shfl_xor(v[k], m);
            v[k] = k < 6 ? fminf(v[k], o) : fmaxf(v[k], o);
        }
    if ((tid & 63u) == 0u)
        for (int k = 0; k < 12; ++k) red[wave][k] = v[k];
    for (uint32_t j = tid; j < 3u * kBins * 6u; j += kBlock) (&bins[0][0][0])[j] = kEmpty;
    if (tid < 3u * kBins) (&bcount[0][0])[tid] = 0u;
    __syncthreads();
    for (int k = 0; k < 12; ++k) {  // (every thread in the same order: the same words in all of them)
        v[k] = red[0][k];
        for (int w = 1; w < kWaves; ++w) v[k] = k < 6 ? fminf(v[k], red[w][k]) : fmaxf(v[k], red[w][k]);
    }
    const float *cmin = v, *bmin = v + 3, *cmax = v + 6, *bmax = v + 9;
    if (tid == 0u) {
        float *box = A.n_box + 6u * (size_t)node;
        for (int k = 0; k < 3; ++k) box[k] = bmin[k], box[3 + k] = bmax[k];
    }

    int axis = -1;
    double pos = 0.0;
    uint32_t n_left = 0u;
    if (count > A.max_leaf && level < kMaxDepth) {
        double bin_w[3];
        for (int a = 0; a < 3; ++a) bin_w[a] = ((double)cmax[a] - (double)cmin[a]) / (double)kBins;
        for (uint32_t i = tid; i < count; i += kBlock) {
            const float *rec = A.rec + 6u * (size_t)in[lo + i];
            unsigned long long e[6];
            double c[3];
            for (int k = 0; k < 3; ++k) {
                c[k] = (double)rec[k];
                const double h = (double)rec[3 + k];
                e[k] = ~ordered(c[k] - h);
                e[3 + k] = ordered(c[k] + h);
            }
            for (int a = 0; a < 3; ++a) {
                int b = 0;
                if (bin_w[a] > 0.0) b = (int)fmin(fmax(floor((c[a] - (double)cmin[a]) / bin_w[a]), 0.0), (double)(kBins - 1));
                atomicAdd(&bcount[a][b], 1u);
                for (int k = 0; k < 6; ++k) atomicMax(&bins[a][b][k], e[k]);
            }
        }
        __syncthreads();
        if (tid < 3u) {  // one lane per axis: candidates in ascending order, the first minimum kept
            const int a = (int)tid;
            double nmn[3], nmx[3], mn[3], mx[3];
            for (int k = 0; k < 3; ++k) nmn[k] = (double)bmin[k], nmx[k] = (double)bmax[k];
            const double root_sa = area(nmn, nmx);
            for (int k = 0; k < 3; ++k) mn[k] = HUGE_VAL, mx[k] = -HUGE_VAL;
            for (int i = kBins - 1; i >= 1; --i) {
                for (int k = 0; k < 3; ++k) {
                    mn[k] = fmin(mn[k], unordered(~bins[a][i][k]));
                    mx[k] = fmax(mx[k], unordered(bins[a][i][3 + k]));
                }
                rsa[a][i] = area(mn, mx);
            }
            for (int k = 0; k < 3; ++k) mn[k] = HUGE_VAL, mx[k] = -HUGE_VAL;
            double best = 1.25 * (double)count;
            int cand = -1;
            uint32_t lc = 0u;
            for (int i = 0; i < kBins - 1; ++i) {
                for (int k = 0; k < 3; ++k) {
                    mn[k] = fmin(mn[k], unordered(~bins[a][i][k]));
                    mx[k] = fmax(mx[k], unordered(bins[a][i][3 + k]));
                }
                lc += bcount[a][i];
                const uint32_t rc = count - lc;
                const double lp = (lc > 0u && root_sa > 0.0) ? area(mn, mx) / root_sa : 0.0;
                const double rp = (rc > 0u && root_sa > 0.0) ? rsa[a][i + 1] / root_sa : 0.0;
                const double cost = 1.0 + 1.25 * (lp * (double)lc + rp * (double)rc);
                if (cost < best) best = cost, cand = i;
            }
            axis_cost[a] = best;
            axis_cand[a] = cand;
        }
        __syncthreads();
        double best = 1.25 * (double)count;
        int cand = 0;
        for (int a = 0; a < 3; ++a)  // axis-major, strict: the first minimum of the whole sweep
            if (axis_cand[a] >= 0 && axis_cost[a] < best) best = axis_cost[a], axis = a, cand = axis_cand[a];
        if (axis >= 0) {
            const double left = axis == 0 ? (double)cmin[0] : axis == 1 ? (double)cmin[1] : (double)cmin[2];
            const double w = axis == 0 ? bin_w[0] : axis == 1 ? bin_w[1] : bin_w[2];
            pos = (double)(float)((left + w) + (double)cand * w);
            // the lefts by the compare (it can disagree with the bins on a boundary)
            uint32_t mine = 0u;
            for (uint32_t i = tid; i < count; i += kBlock) mine += (double)A.rec[6u * (size_t)in[lo + i] + axis] < pos ? 1u : 0u;
            for (int m = 32; m > 0; m >>= 1) mine += (uint32_t)__shfl_xor((int)mine, m);
            if ((tid & 63u) == 0u) wsum[0][wave] = mine;
            __syncthreads();
            for (int w2 = 0; w2 < kWaves; ++w2) n_left += wsum[0][w2];
            __syncthreads();
        }
    }
    bool split = axis >= 0 && n_left > 0u && n_left < count;
    if (split) {
        if (tid == 0u) s_child = atomicAdd(A.counters, 2u);
        __syncthreads();
        if (s_child + 2u > A.node_cap) split = false;  // (cannot happen: a leaf holds a triangle, so nodes <= 2 T - 1)
    }
    if (!split) {
        for (uint32_t i = tid; i < count; i += kBlock) A.final_order[lo + i] = in[lo + i];
        if (tid == 0u) {
            A.n_link[node].z = kLeaf;
            atomicMax(A.counters + 1, count);
        }
        return;
    }
    // the stable partition, 256 positions at a time: lefts from lo, rights from lo + n_left
    uint32_t run_l = 0u, run_r = 0u;
    for (uint32_t base = 0u; base < count; base += kBlock) {
        const uint32_t i = base + tid;
        const bool valid = i < count;
        const uint32_t t = valid ? in[lo + i] : 0u;
        const bool left = valid && (double)A.rec[6u * (size_t)t + axis] < pos;
        const unsigned long long ml = __ballot(left), mr = __ballot(valid && !left);
        if ((tid & 63u) == 0u) wsum[0][wave] = (uint32_t)__popcll(ml), wsum[1][wave] = (uint32_t)__popcll(mr);
        __syncthreads();
        uint32_t before_l = 0u, before_r = 0u, all_l = 0u, all_r = 0u;
        for (uint32_t w2 = 0; w2 < (uint32_t)kWaves; ++w2) {
            if (w2 < wave) before_l += wsum[0][w2], before_r += wsum[1][w2];
            all_l += wsum[0][w2], all_r += wsum[1][w2];
        }
        if (valid) {
            const uint32_t dst = left ? run_l + before_l + lanes_below(ml) : n_left + run_r + before_r + lanes_below(mr);
            if (dst < count) out[lo + dst] = t;  // (always: the counts are those of the same compare)
        }
        run_l += all_l;
        run_r += all_r;
        __syncthreads();
    }
    if (tid == 0u) {
        const uint32_t c = s_child;
        uint4 link = A.n_link[node];
        link.y = c;
        link.z = (uint32_t)axis;
        A.n_link[node] = link;
        A.n_range[c] = make_uint2(lo, n_left);
        A.n_range[c + 1u] = make_uint2(lo + n_left, count - n_left);
        A.n_link[c] = make_uint4(node, 0u, kLeaf, link.w);
        A.n_link[c + 1u] = make_uint4(node, 0u, kLeaf, link.w);
    }
}

__global__ __launch_bounds__(kBlock) void sah_size(SahArgs A, uint32_t first_node, uint32_t n) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint4 link = A.n_link[first_node + i];
    A.n_size[first_node + i] = link.z == kLeaf ? 1u : 1u + A.n_size[link.y] + A.n_size[link.y + 1u];
}

__global__ __launch_bounds__(kBlock) void sah_emit(SahArgs A) {
    const uint32_t id = blockIdx.x * kBlock + threadIdx.x;
    if (id >= A.n_nodes) return;
    const uint4 link = A.n_link[id];
    // the parent chain: 1 per ancestor, plus the left sibling's subtree where the chain comes up from a right child
    uint32_t index = 0u, steps = 0u;
    for (uint32_t cur = id, par = link.x; par != kNone && steps <= kMaxDepth; ++steps) {
        const uint4 up = A.n_link[par];
        index += 1u + (cur != up.y ? A.n_size[up.y] : 0u);
        cur = par;
        par = up.x;
    }
    const size_t at = (size_t)A.goff[link.w] + index;
    if (at >= A.n_nodes) return;  // (cannot happen: keeps a store inside the output whatever the tables hold)
    const uint2 range = A.n_range[id];
    uint32_t w6, w7;
    if (link.z == kLeaf) {
        w6 = range.x;
        w7 = 0xFFFF0000u | (range.y & 0xFFFFu);
    } else {
        w6 = 8u * (index + 1u + A.n_size[link.y]);
        w7 = link.z;
    }
    const float *box = A.n_box + 6u * (size_t)id;
    uint4 *dst = reinterpret_cast<uint4 *>(A.nodes_out + 8u * at);
    dst[0] = make_uint4(__float_as_uint(box[0]), __float_as_uint(box[1]), __float_as_uint(box[2]), __float_as_uint(box[3]));
    dst[1] = make_uint4(__float_as_uint(box[4]), __float_as_uint(box[5]), w6, w7);
}

__global__ __launch_bounds__(kBlock) void sah_gather(SahArgs A) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= A.n_tris) return;
    const uint32_t src = A.final_order[p];
    if (src >= A.n_tris) return;
    for (int k = 0; k < 3; ++k) A.idx_out[3u * (size_t)p + k] = A.idx[3u * (size_t)src + k];
}

hipError_t launch_sah(const SahArgs &A, SahStep step, uint32_t first_node, uint32_t n, uint32_t level, hipStream_t s) {
    const dim3 grid((n + kBlock - 1) / kBlock), block(kBlock);
    switch (step) {
    case SahStep::Init: hipLaunchKernelGGL(sah_init, grid, block, 0, s, A); break;
    case SahStep::Level: hipLaunchKernelGGL(sah_level, dim3(n), block, 0, s, A, first_node, level); break;
    case SahStep::Size: hipLaunchKernelGGL(sah_size, grid, block, 0, s, A, first_node, n); break;
    case SahStep::Emit: hipLaunchKernelGGL(sah_emit, grid, block, 0, s, A); break;
    case SahStep::Gather: hipLaunchKernelGGL(sah_gather, grid, block, 0, s, A); break;
    }
    return hipGetLastError();
}

}  // namespace ptx
