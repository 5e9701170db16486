// ptx_cost.hip -- ptx_blas_cost's kernel: the surface-area cost of one mesh's trees as the device's tables
// hold them (include/ptx.h states the rule; pathtracerdemo_amd/scene/lbvh.py sah_cost is the same in numpy).
//
//   blas_cost   one thread per child of the mesh's pairs, then one per root record.  A node's term is its
//               box's area relative to its root's -- reached through the per-pair sub-mesh table build_layout
//               keeps -- for an interior node, times 1.25 per triangle for a leaf; everything in f64 from the
//               tables' f32 boxes, each operation rounded on its own.  A workgroup adds its terms in a fixed
//               order (a shuffle tree per wave, then the waves' sums in wave order from LDS) and writes one
//               partial; the host adds the partials in index order.  No atomics: two calls give equal bits.
#include "ptx_launch.h"

namespace ptx {

namespace {

constexpr int kCostWaves = kBlock / 64;

__device__ __forceinline__ double box_area(float lx, float ly, float lz, float hx, float hy, float hz) {
#pragma clang fp contract(off)
    const double dx = (double)hx - (double)lx, dy = (double)hy - (double)ly, dz = (double)hz - (double)lz;
    return 2.0 * ((dx * dy + dy * dz) + dz * dx);
}

__device__ __forceinline__ double root_area(const SubRoot &r) { return box_area(r.x[0], r.y[0], r.z[0], r.x[1], r.y[1], r.z[1]); }

__device__ __forceinline__ double node_term(double area, double area_root, uint32_t ref) {
#pragma clang fp contract(off)
    const double rel = area_root > 0.0 ? area / area_root : 0.0;
    if (!(ref & LEAF_BIT)) return rel;
    return (rel * 1.25) * (double)((ref >> 24) & 0x7Fu);
}

__global__ __launch_bounds__(kBlock) void blas_cost(CostArgs a) {
    __shared__ double wave_sum[kCostWaves];
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    double term = 0.0;
    if (t < 2u * a.n_pairs) {
        const uint32_t p = a.pair_base + (t >> 1), c = t & 1u;
        const NodePair &q = a.nodes[p];
        const double area = box_area(q.x[c], q.y[c], q.z[c], q.x[2u + c], q.y[2u + c], q.z[2u + c]);
        term = node_term(area, root_area(a.subs[a.pair_sub[p]]), c ? q.rref : q.lref);
    } else if (t - 2u * a.n_pairs < a.n_subs) {
        const SubRoot &r = a.subs[a.sub_base + (t - 2u * a.n_pairs)];
        const double area = root_area(r);
        term = node_term(area, area, r.ref);
    }
    for (int off = 32; off > 0; off >>= 1) term += __shfl_down(term, off, 64);
    if ((threadIdx.x & 63u) == 0u) wave_sum[threadIdx.x >> 6] = term;
    __syncthreads();
    if (threadIdx.x == 0u) {
        double s = wave_sum[0];
        for (int w = 1; w < kCostWaves; ++w) s += wave_sum[w];
        a.partial[blockIdx.x] = s;
    }
}

}  // namespace

uint32_t cost_blocks(uint32_t n_pairs, uint32_t n_subs) {
    return (uint32_t)(((uint64_t)2u * n_pairs + n_subs + kBlock - 1u) / kBlock);
}

hipError_t launch_blas_cost(const CostArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(blas_cost, dim3(cost_blocks(a.n_pairs, a.n_subs)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace ptx
