// ptx_refit.hip -- ptx_update_vertices' kernels: one mesh's derived tables from its new vertex records.
//
// The topology stays (index buffer, the pairs' and roots' ref words); what follows the vertices is
// derived again on the device:
//   refit_tris    one thread per triangle: the edge-form record and the vertex / normal record, by
//                 build_layout's expressions (ptx_api.cpp), and the triangle's box by the BLAS
//                 builder's rule (scene/bvh.py _triangle_bounds + _Builder.bounds) into a scratch table;
//   refit_level   one launch per tree height, lowest first, one thread per child of a pair of that
//                 height: a leaf child reduces its triangles' boxes, an interior child takes the union
//                 of the four boxes of its own pair (a lower height: an earlier launch wrote it);
//   refit_roots   one thread per sub-mesh root: its pair's union, or its leaf's box.
// Launch boundaries are the only ordering: no workgroup waits for another.
#include "ptx_launch.h"
#include "ptx_tribox.h"

namespace ptx {

struct Box {
    float lo[3], hi[3];
};

__device__ __forceinline__ Box box_empty() {
    Box b;
    for (int k = 0; k < 3; ++k) { b.lo[k] = HUGE_VALF; b.hi[k] = -HUGE_VALF; }
    return b;
}
__device__ __forceinline__ void box_grow(Box &b, const Box &o) {
    for (int k = 0; k < 3; ++k) { b.lo[k] = fminf(b.lo[k], o.lo[k]); b.hi[k] = fmaxf(b.hi[k], o.hi[k]); }
}
__device__ __forceinline__ Box box_load(const float2 *box, uint32_t tri) {
    const float2 a = box[3u * tri], b = box[3u * tri + 1u], c = box[3u * tri + 2u];
    return Box{{a.x, a.y, b.x}, {b.y, c.x, c.y}};
}
// the box of a child or root reference: a leaf's triangles reduced, or the union of a pair's four boxes
__device__ __forceinline__ Box ref_box(const RefitMesh &m, uint32_t ref) {
    Box b = box_empty();
    if (ref & LEAF_BIT) {
        const uint32_t first = ref & LEAF_FIRST_MASK, count = (ref >> 24) & 0x7Fu;
        for (uint32_t k = 0; k < count; ++k)
            if (first + k < m.n_tris) box_grow(b, box_load(m.box, first + k));
        return b;
    }
    const NodePair &p = m.nodes[ref];
    const float *axis[3] = {p.x, p.y, p.z};
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = fminf(axis[k][0], axis[k][1]);
        b.hi[k] = fmaxf(axis[k][2], axis[k][3]);
    }
    return b;
}

__global__ __launch_bounds__(kBlock) void refit_tris(RefitMesh m) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= m.n_tris) return;
    float P[3][3], N[3][3];
    for (int v = 0; v < 3; ++v) {
        const uint32_t *rec = m.G + m.vertex + (size_t)STRIDE_VERTEX * m.G[(size_t)m.index + 3u * t + v];
        for (int k = 0; k < 3; ++k) {
            P[v][k] = __uint_as_float(rec[k]);
            N[v][k] = __uint_as_float(rec[3 + k]);
        }
    }
    const float e1[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
    const float e2[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
    float4 *tr = m.tris + 3u * (size_t)(m.tri_base + t);
    tr[0] = make_float4(P[0][0], P[0][1], P[0][2], e1[0]);
    tr[1] = make_float4(e1[1], e1[2], e2[0], e2[1]);
    tr[2] = make_float4(e2[2], 0.0f, 0.0f, 0.0f);
    float4 *tv = m.tverts + 5u * (size_t)(m.tri_base + t);
    tv[0] = make_float4(P[0][0], P[0][1], P[0][2], N[0][0]);
    tv[1] = make_float4(N[0][1], N[0][2], P[1][0], P[1][1]);
    tv[2] = make_float4(P[1][2], N[1][0], N[1][1], N[1][2]);
    tv[3] = make_float4(P[2][0], P[2][1], P[2][2], N[2][0]);
    tv[4] = make_float4(N[2][1], N[2][2], 0.0f, 0.0f);
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) tri_axis_bounds(P[0][k], P[1][k], P[2][k], lo[k], hi[k]);
    float2 *bx = m.box + 3u * (size_t)t;
    bx[0] = make_float2(lo[0], lo[1]);
    bx[1] = make_float2(lo[2], hi[0]);
    bx[2] = make_float2(hi[1], hi[2]);
}

// Thread 2i + c: child c (0 left, 1 right) of pair order[first + i].  It writes its child's slots
// {min: [c], max: [2 + c]} of the three axes; the two threads of a pair write the whole pair between
// them, neither reads a word the other writes.
__global__ __launch_bounds__(kBlock) void refit_level(RefitMesh m, uint32_t first, uint32_t n) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= 2u * n) return;
    const uint32_t c = k & 1u;
    NodePair &p = m.nodes[m.order[first + (k >> 1)]];
    const Box b = ref_box(m, c ? p.rref : p.lref);
    p.x[c] = b.lo[0]; p.x[2u + c] = b.hi[0];
    p.y[c] = b.lo[1]; p.y[2u + c] = b.hi[1];
    p.z[c] = b.lo[2]; p.z[2u + c] = b.hi[2];
}

__global__ __launch_bounds__(kBlock) void refit_roots(RefitMesh m) {
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= m.n_subs) return;
    SubRoot &r = m.subs[m.sub_base + s];
    const Box b = ref_box(m, r.ref);
    float2 *w = reinterpret_cast<float2 *>(&r);  // {x, y, z}: the ref and transmission words stay
    w[0] = make_float2(b.lo[0], b.hi[0]);
    w[1] = make_float2(b.lo[1], b.hi[1]);
    w[2] = make_float2(b.lo[2], b.hi[2]);
}

static dim3 refit_grid(uint32_t threads) { return dim3((threads + kBlock - 1) / kBlock); }

hipError_t launch_refit_tris(const RefitMesh &m, hipStream_t s) {
    if (m.n_tris == 0u) return hipSuccess;
    hipLaunchKernelGGL(refit_tris, refit_grid(m.n_tris), dim3(kBlock), 0, s, m);
    return hipGetLastError();
}
hipError_t launch_refit_level(const RefitMesh &m, uint32_t first, uint32_t n, hipStream_t s) {
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(refit_level, refit_grid(2u * n), dim3(kBlock), 0, s, m, first, n);
    return hipGetLastError();
}
hipError_t launch_refit_roots(const RefitMesh &m, hipStream_t s) {
    if (m.n_subs == 0u) return hipSuccess;
    hipLaunchKernelGGL(refit_roots, refit_grid(m.n_subs), dim3(kBlock), 0, s, m);
    return hipGetLastError();
}

}  // namespace ptx
