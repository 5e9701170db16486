// ptx_skin.hip -- ptx_skin_vertices' kernel: the bound vertices of one mesh from their bind pose, a joint
// palette and morph-target weights (include/ptx.h states the rule; scene/skin.py restates it in numpy).
//
//   skin_vertices   one thread per bound vertex.  The block first copies the palette (at most 256 x 48 B)
//                   and the target weights into LDS; a thread then reads its 48-byte bind record with three
//                   16-byte loads, adds the morph deltas (target-major tables: a wave's loads of one
//                   target are contiguous), blends its four matrices row by row from LDS and writes
//                   {P', n'.x} and {n'.y, n'.z} over words 0..5 of its vertex record.  Words 6 and 7 (uv)
//                   are not the kernel's: the record is never written whole.
// Every product and sum is rounded on its own, in the order of the rule: the arithmetic is compiled under
// fp contract(off), whatever the command line says.  ptx_update_vertices' refit chain follows on the stream.
#include "ptx_launch.h"

namespace ptx {

__global__ __launch_bounds__(kBlock) void skin_vertices(SkinArgs a) {
#pragma clang fp contract(off)
    __shared__ float4 pal[3 * kSkinMaxJoints];
    __shared__ float tw[kSkinMaxTargets];
    for (uint32_t i = threadIdx.x; i < 3u * a.n_joints; i += kBlock) pal[i] = a.palette[i];
    if (threadIdx.x < a.n_targets) tw[threadIdx.x] = a.target_weights[threadIdx.x];
    __syncthreads();
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= a.n) return;
    const float4 b0 = a.bind[3u * (size_t)v], b1 = a.bind[3u * (size_t)v + 1u], b2 = a.bind[3u * (size_t)v + 2u];
    float q[3] = {b0.x, b0.y, b0.z}, m[3] = {b0.w, b1.x, b1.y};
    const float w[4] = {b1.z, b1.w, b2.x, b2.y};
    const uint32_t j01 = __float_as_uint(b2.z), j23 = __float_as_uint(b2.w);
    // (ptx_set_skin refused indices >= n_joints; the mask keeps a read inside the LDS table regardless)
    const uint32_t j[4] = {j01 & 0xffu, (j01 >> 16) & 0xffu, j23 & 0xffu, (j23 >> 16) & 0xffu};
    for (uint32_t k = 0; k < a.n_targets; ++k) {
        const float *dp = a.target_pos + 3u * ((size_t)k * a.n + v);
        for (int c = 0; c < 3; ++c) q[c] = q[c] + tw[k] * dp[c];
        if (a.target_nrm) {
            const float *dn = a.target_nrm + 3u * ((size_t)k * a.n + v);
            for (int c = 0; c < 3; ++c) m[c] = m[c] + tw[k] * dn[c];
        }
    }
    float P[3], N[3];
    for (int r = 0; r < 3; ++r) {
        const float4 m0 = pal[3u * j[0] + r], m1 = pal[3u * j[1] + r], m2 = pal[3u * j[2] + r], m3 = pal[3u * j[3] + r];
        const float bx = ((w[0] * m0.x + w[1] * m1.x) + w[2] * m2.x) + w[3] * m3.x;
        const float by = ((w[0] * m0.y + w[1] * m1.y) + w[2] * m2.y) + w[3] * m3.y;
        const float bz = ((w[0] * m0.z + w[1] * m1.z) + w[2] * m2.z) + w[3] * m3.z;
        const float bw = ((w[0] * m0.w + w[1] * m1.w) + w[2] * m2.w) + w[3] * m3.w;
        P[r] = ((bx * q[0] + by * q[1]) + bz * q[2]) + bw;
        N[r] = (bx * m[0] + by * m[1]) + bz * m[2];
    }
    const float l = sqrtf((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]);
    if (l > 0.0f) {
        N[0] = N[0] / l;
        N[1] = N[1] / l;
        N[2] = N[2] / l;
    }
    uint32_t *rec = a.G + a.word0 + (size_t)STRIDE_VERTEX * v;  // (16-byte aligned: ptx_set_skin checked the block)
    *reinterpret_cast<float4 *>(rec) = make_float4(P[0], P[1], P[2], N[0]);
    *reinterpret_cast<float2 *>(rec + 4) = make_float2(N[1], N[2]);
}

hipError_t launch_skin_vertices(const SkinArgs &a, hipStream_t s) {
    if (a.n == 0u) return hipSuccess;
    hipLaunchKernelGGL(skin_vertices, dim3((a.n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace ptx
