// ptx_scene.cpp -- the scene arrays behind the C ABI (include/ptx.h), the MI355X traversal layout
// derived from them (ptx_device.h), and the entry points that read or edit either: upload, instance /
// material / light edits, vertex updates and skinning with their refit, the BLAS builders and the
// rebuild of a loaded mesh.  What an edit keeps and drops of the handle's cached state is stated once,
// below ("What an edit invalidates").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <unordered_map>
#include <vector>

#include "ptx_internal.h"

namespace ptx {

static inline float as_f32(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

// The instance cull's world box (Inst::wlo / whi / wpad / wscale, inst_may_hit in ptx_device.h):
// the union of the instance's sub-mesh root boxes in local space, mapped to world space through
// the inverse of M^-1 (the matrix the kernels transform rays with; M itself may differ from that
// inverse by rounding) in double precision, its 8 corners' bounds rounded outward to f32.  The
// pad covers the f32 rounding of the kernels' ray transform with >= 40x margin: 1e-5 of the
// local box's and M^-1's translation magnitudes mapped through |A^-1| (A = M^-1's linear part),
// and per ray 1e-5 * cond(A) * max|o| (wscale); inst_may_hit adds the local direction's rounding
// times the ray parameter, from the scene's largest box coordinate, pad and scale.  Never culled (wpad = -1): a projective or
// singular M^-1, non-finite values, an instance without sub-meshes.
static void inst_world_box(Inst &I, const SubRoot *roots, uint32_t nsub) {
    I.wpad = -1.0f;
    I.wscale = 0.0f;
    for (int k = 0; k < 3; ++k) I.wlo[k] = I.whi[k] = 0.0f;
    const float *m = I.minv;  // column-major: local = A * world + t
    if (nsub == 0 || m[3] != 0.0f || m[7] != 0.0f || m[11] != 0.0f || m[15] != 1.0f) return;
    double A[3][3], t[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) A[r][c] = m[4 * c + r];
        t[r] = m[12 + r];
    }
    const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                       A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
    if (!std::isfinite(det) || std::fabs(det) < 1e-30) return;
    double B[3][3];  // A^-1
    B[0][0] = (A[1][1] * A[2][2] - A[1][2] * A[2][1]) / det;
    B[0][1] = (A[0][2] * A[2][1] - A[0][1] * A[2][2]) / det;
    B[0][2] = (A[0][1] * A[1][2] - A[0][2] * A[1][1]) / det;
    B[1][0] = (A[1][2] * A[2][0] - A[1][0] * A[2][2]) / det;
    B[1][1] = (A[0][0] * A[2][2] - A[0][2] * A[2][0]) / det;
    B[1][2] = (A[0][2] * A[1][0] - A[0][0] * A[1][2]) / det;
    B[2][0] = (A[1][0] * A[2][1] - A[1][1] * A[2][0]) / det;
    B[2][1] = (A[0][1] * A[2][0] - A[0][0] * A[2][1]) / det;
    B[2][2] = (A[0][0] * A[1][1] - A[0][1] * A[1][0]) / det;
    double lo[3], hi[3];
    for (int k = 0; k < 3; ++k) { lo[k] = HUGE_VAL; hi[k] = -HUGE_VAL; }
    for (uint32_t s = 0; s < nsub; ++s) {
        const float *ax[3] = {roots[s].x, roots[s].y, roots[s].z};
        for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], (double)ax[k][0]); hi[k] = std::max(hi[k], (double)ax[k][1]); }
    }
    double lmax = 0.0, tmax = 0.0, na = 0.0, nb = 0.0;  // magnitudes, |A|inf, |A^-1|inf
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(lo[k]) || !std::isfinite(hi[k]) || lo[k] > hi[k]) return;
        lmax = std::max({lmax, std::fabs(lo[k]), std::fabs(hi[k])});
        tmax = std::max(tmax, std::fabs(t[k]));
        na = std::max(na, std::fabs(A[k][0]) + std::fabs(A[k][1]) + std::fabs(A[k][2]));
        nb = std::max(nb, std::fabs(B[k][0]) + std::fabs(B[k][1]) + std::fabs(B[k][2]));
    }
    double wlo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, whi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL}, wmax = 0.0;
    for (int c = 0; c < 8; ++c) {
        const double p[3] = {(c & 1) ? hi[0] : lo[0], (c & 2) ? hi[1] : lo[1], (c & 4) ? hi[2] : lo[2]};
        for (int r = 0; r < 3; ++r) {
            const double w = B[r][0] * (p[0] - t[0]) + B[r][1] * (p[1] - t[1]) + B[r][2] * (p[2] - t[2]);
            wlo[r] = std::min(wlo[r], w);
            whi[r] = std::max(whi[r], w);
            wmax = std::max(wmax, std::fabs(w));
        }
    }
    const double pad = 1e-5 * (1.0 + wmax) + 1e-5 * nb * (lmax + tmax);
    const double scale = 1e-5 * std::max(1.0, na * nb);
    if (!std::isfinite(pad) || !std::isfinite(scale) || !std::isfinite(wmax)) return;
    for (int k = 0; k < 3; ++k) {
        I.wlo[k] = std::nextafter((float)wlo[k], -HUGE_VALF);
        I.whi[k] = std::nextafter((float)whi[k], HUGE_VALF);
    }
    I.wpad = std::nextafter((float)pad, HUGE_VALF);
    I.wscale = std::nextafter((float)scale, HUGE_VALF);
}

// The tables that depend on the scene array's instance and material blocks, from build_layout's
// per-mesh results (h->lay_*): the instance table with the cull bounds, and the material table with the
// root records' transmission word.  build_layout derives both; ptx_update_scene only what an edit
// touched.  Nothing of the handle changes when an instance names a mesh that is not loaded.
static int layout_tables(ptx_handle *h, bool with_insts, bool with_mats) {
    const auto &S = h->scene;
    const uint32_t n_inst = h->n_inst, n_mesh = (uint32_t)h->lay_mesh_nsub.size();
    std::vector<Inst> insts;
    float cull_box = 0.0f, cull_pad = 0.0f, cull_scale = 0.0f;
    if (with_insts) {
        insts.resize(n_inst);
        for (uint32_t i = 0; i < n_inst; ++i) {
            const uint32_t *p = S.data() + STRIDE_INSTANCE * i;
            Inst &I = insts[i];
            std::memcpy(I.m, p, 64);
            std::memcpy(I.minv, p + 16, 64);
            I.mesh = p[32];
            if (I.mesh >= n_mesh) return fail(h, PTX_E_SCENE, "instance %u references mesh %u of %u", i, I.mesh, n_mesh);
            I.sub_base = h->lay_mesh_sub_base[I.mesh];
            I.nsub = h->lay_mesh_nsub[I.mesh];
            I.tri_base = h->lay_mesh_tri_base[I.mesh];
            // exactly the identity (bitwise 1 / +0, M and M^-1): the kernels' transforms of this
            // instance reduce to x + 0 (inst_point, ptx_device.h) with the same bits
            static const float kId[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
            if (!std::memcmp(I.m, kId, sizeof kId) && !std::memcmp(I.minv, kId, sizeof kId)) I.mesh |= kInstIdentity;
            inst_world_box(I, h->lay_subs.data() + I.sub_base, I.nsub);
            if (I.wpad >= 0.0f) {  // (a culled instance's coordinates are finite: inst_world_box)
                for (int k = 0; k < 3; ++k) cull_box = std::max({cull_box, std::fabs(I.wlo[k]), std::fabs(I.whi[k])});
                cull_pad = std::max(cull_pad, I.wpad);
                cull_scale = std::max(cull_scale, I.wscale);
            }
        }
    }
    if (with_mats) {
        // GetMaterial (SH/PT_1_InitPass.wgsl:285-314) per sub-mesh: material d[2] + 15*sub.  A record
        // past the scene buffer reads as zeros (WebGPU's robust buffer access would clamp or zero).
        std::vector<float> mats;  // 8 floats per sub-mesh, in SubRoot order (Scene::mats)
        for (const size_t mi : h->lay_mat_word) {
            auto word = [&](uint32_t k) { return mi + k < S.size() ? as_f32(S[mi + k]) : 0.0f; };
            const float trans = word(10);
            const bool yellow = trans > 0.0f;
            const float rec[8] = {yellow ? 1.0f : word(0), yellow ? 1.0f : word(1), yellow ? 0.0f : word(2), word(8),
                                  std::fmax(word(9), 0.01f), trans, word(11), 0.0f};
            mats.insert(mats.end(), rec, rec + 8);
        }
        if (mats.empty()) mats.resize(8, 0.0f);
        auto &subs = h->lay_subs;
        // each root record carries its sub-mesh's transmission (the Visibility restart test reads
        // it from the trace kernel's LDS root table: subs_transmission)
        if (mats.size() != 8u * subs.size()) return fail(h, PTX_E_SCENE, "material / sub-mesh tables disagree");
        for (size_t k = 0; k < subs.size(); ++k) std::memcpy(&subs[k].pad, &mats[8u * k + 5u], 4);
        if (int rc = upload(h, h->d_subs, subs.data(), subs.size() * sizeof(SubRoot))) return rc;
        h->n_subs = (uint32_t)subs.size();
        if (int rc = upload(h, h->d_mats, mats.data(), mats.size() * sizeof(float))) return rc;
    }
    if (with_insts) {
        if (int rc = upload(h, h->d_insts, insts.data(), std::max<size_t>(1, insts.size()) * sizeof(Inst))) return rc;
        h->cull_box = cull_box;
        h->cull_pad = cull_pad;
        h->cull_scale = cull_scale;
    }
    return PTX_OK;
}

// The boxes of every reachable node as the device's tables hold them now, written over words 0..5 of
// their nodes in `accel` (an array of the uploaded length): ptx_read_accel's map, lay_root_word /
// lay_pair_words, from the NodePair / SubRoot tables back to the reference's node array.
static int device_boxes_into(ptx_handle *h, uint32_t *accel) {
    const size_t n_roots = h->lay_root_word.size(), n_pairs = h->lay_pair_words.size() / 2u;
    std::vector<SubRoot> subs(n_roots);
    std::vector<NodePair> pairs(n_pairs);
    if (n_roots)
        if (int rc = read_to_host(h, subs.data(), h->d_subs.p, n_roots * sizeof(SubRoot))) return rc;
    if (n_pairs)
        if (int rc = read_to_host(h, pairs.data(), h->d_nodes.p, n_pairs * sizeof(NodePair))) return rc;
    auto put = [&](size_t w, const float *mn_mx) { std::memcpy(accel + w, mn_mx, 24); };
    for (size_t s = 0; s < n_roots; ++s) {
        const SubRoot &r = subs[s];
        const float b[6] = {r.x[0], r.y[0], r.z[0], r.x[1], r.y[1], r.z[1]};
        put(h->lay_root_word[s], b);
    }
    for (size_t p = 0; p < n_pairs; ++p) {
        const NodePair &q = pairs[p];
        const float l[6] = {q.x[0], q.y[0], q.z[0], q.x[2], q.y[2], q.z[2]};
        const float r[6] = {q.x[1], q.y[1], q.z[1], q.x[3], q.y[3], q.z[3]};
        put(h->lay_pair_words[2u * p], l);
        put(h->lay_pair_words[2u * p + 1u], r);
    }
    return PTX_OK;
}

// The host's copies of the geometry and accel arrays brought up to date with the device where a vertex
// call left them behind (ptx_handle::mesh_stale): one device-to-host copy of the vertex block per mesh
// that ptx_skin_vertices wrote, and the boxes of the refitted nodes.  build_layout reads the copies, so it
// calls this first; the tables and the lay_* maps still describe the layout being replaced.
static int sync_host_mirror(ptx_handle *h) {
    uint8_t any = 0;
    for (size_t m = 0; m < h->mesh_stale.size() && m < h->lay_mesh_vertex.size(); ++m) {
        any |= h->mesh_stale[m];
        if (!(h->mesh_stale[m] & kStaleGeometry)) continue;
        const size_t w0 = h->lay_mesh_vertex[m], n = (size_t)STRIDE_VERTEX * h->lay_mesh_nverts[m];
        if (!n || w0 + n > h->geometry.size() || h->d_geometry.bytes < (w0 + n) * 4u) continue;
        if (int rc = read_to_host(h, h->geometry.data() + w0, (const uint32_t *)h->d_geometry.p + w0, n * 4u)) return rc;
        h->mesh_stale[m] &= (uint8_t)~kStaleGeometry;
    }
    if ((any & kStaleAccel) && h->d_subs.bytes >= h->lay_root_word.size() * sizeof(SubRoot) &&
        h->d_nodes.bytes >= h->lay_pair_words.size() / 2u * sizeof(NodePair))
        if (int rc = device_boxes_into(h, h->accel.data())) return rc;
    h->mesh_stale.clear();
    return PTX_OK;
}

// ---------------------------------------------------------------- layout derivation
// Walks the reference's per-sub-mesh BLAS (three-mesh-bvh node format, GC/Structs.ts:73-80;
// read by GetBlasNode, SH/PT_01_GBufferPass.wgsl:310-322) and emits the child-pair node
// records, the edge-form triangle table and the instance table of ptx_device.h.
int build_layout(ptx_handle *h) {
    // frames in flight (either pipelined context) still read the layout being replaced
    if (int rc = quiesce(h)) return rc;
    if (!h->mesh_stale.empty())
        if (int rc = sync_host_mirror(h)) return rc;
    const uint32_t *U = h->uniform;
    const auto &S = h->scene, &G = h->geometry, &A = h->accel;
    const uint32_t off_desc = U[U_OFF_DESC], off_mat = U[U_OFF_MAT], off_index = U[U_OFF_INDEX];
    const uint32_t off_subroot = U[U_OFF_SUBROOT], off_blas = U[U_OFF_BLAS], n_inst = U[U_INST_COUNT];
    if (off_mat < off_desc || (off_mat - off_desc) % STRIDE_DESCRIPTOR)
        return fail(h, PTX_E_SCENE, "uniform offsets: descriptor block [%u,%u) is not a multiple of 6", off_desc, off_mat);
    const uint32_t n_mesh = (off_mat - off_desc) / STRIDE_DESCRIPTOR;
    if ((size_t)n_inst * STRIDE_INSTANCE > off_desc)
        return fail(h, PTX_E_SCENE, "instance count %u overlaps the descriptor block", n_inst);
    if (off_desc + (size_t)n_mesh * STRIDE_DESCRIPTOR > S.size()) return fail(h, PTX_E_SCENE, "scene buffer too short");

    std::vector<SubRoot> subs;
    std::vector<NodePair> nodes;
    std::vector<float> tris;  // 12 floats per triangle
    std::vector<size_t> mat_word;  // per sub-mesh, in SubRoot order: its material record in the scene array
    std::vector<float> tverts;  // 20 floats per triangle, triangle-table order (Scene::tverts)
    std::vector<uint32_t> mesh_sub_base(n_mesh), mesh_nsub(n_mesh), mesh_tri_base(n_mesh);
    // for ptx_update_vertices / ptx_read_accel (ptx_handle::lay_mesh_ntris ...)
    std::vector<uint32_t> mesh_ntris(n_mesh), mesh_vertex(n_mesh), mesh_nverts(n_mesh), mesh_node_base(n_mesh), mesh_nnodes(n_mesh);
    std::vector<std::vector<uint32_t>> mesh_levels(n_mesh);
    std::vector<uint32_t> order, pair_words, root_word;
    std::vector<uint32_t> pair_sub;  // per pair: its sub-mesh's SubRoot (ptx_blas_cost)
    if (A.size() > 0xffffffffull) return fail(h, PTX_E_SCENE, "accel array too long");
    uint32_t max_depth = 0;

    for (uint32_t m = 0; m < n_mesh; ++m) {
        const uint32_t *d = S.data() + off_desc + STRIDE_DESCRIPTOR * m;
        const uint32_t off_vertex = d[0], off_idx = d[1], off_root = d[3], off_b = d[4], nsub = d[5];
        mesh_sub_base[m] = (uint32_t)subs.size();
        mesh_nsub[m] = nsub;
        mesh_tri_base[m] = (uint32_t)(tris.size() / 12);
        mesh_node_base[m] = (uint32_t)nodes.size();
        mesh_vertex[m] = off_vertex;
        {   // the vertex block ends at the next larger vertex offset among the descriptors, or at the index block
            uint32_t end = off_index;
            for (uint32_t o = 0; o < n_mesh; ++o) {
                const uint32_t v = S[off_desc + STRIDE_DESCRIPTOR * o];
                if (v > off_vertex && v < end) end = v;
            }
            mesh_nverts[m] = end > off_vertex ? (end - off_vertex) / STRIDE_VERTEX : 0u;
        }
        // GetMaterial (SH/PT_1_InitPass.wgsl:285-314) per sub-mesh: material d[2] + 15*sub.  A record
        // past the scene buffer reads as zeros (WebGPU's robust buffer access would clamp or zero).
        for (uint32_t s = 0; s < nsub; ++s) mat_word.push_back((size_t)off_mat + d[2] + (size_t)STRIDE_MATERIAL * s);
        uint32_t mesh_tris = 0;
        struct Pending { uint32_t base; std::vector<uint32_t> order; };
        std::vector<Pending> per_sub;
        for (uint32_t s = 0; s < nsub; ++s) {
            size_t ri = (size_t)off_subroot + off_root + s;
            if (ri >= G.size()) return fail(h, PTX_E_SCENE, "sub-BLAS root index out of range");
            const uint32_t base = off_blas + off_b + G[ri];
            // DFS over the sub-BVH to number interior nodes
            std::unordered_map<uint32_t, uint32_t> gidx;
            std::vector<std::pair<uint32_t, uint32_t>> st{{0u, 0u}};
            std::vector<uint32_t> interior;
            while (!st.empty()) {
                auto [n, depth] = st.back();
                st.pop_back();
                size_t w = (size_t)base + 8u * n;
                if (w + 8 > A.size()) return fail(h, PTX_E_SCENE, "BLAS node %u out of range", n);
                max_depth = std::max(max_depth, depth);
                if (A[w + 7] & 0xffff0000u) {
                    uint32_t first = A[w + 6], count = A[w + 7] & 0xffffu;
                    mesh_tris = std::max(mesh_tris, first + count);
                    continue;
                }
                gidx[n] = (uint32_t)(nodes.size() + interior.size());
                interior.push_back(n);
                st.push_back({n + 1u, depth + 1});
                st.push_back({A[w + 6] / 8u, depth + 1});
                if (depth > 1000) return fail(h, PTX_E_SCENE, "BLAS too deep / cyclic");
            }
            auto ref_of = [&](uint32_t n, uint32_t &ref) -> int {
                size_t w = (size_t)base + 8u * n;
                if (A[w + 7] & 0xffff0000u) {
                    uint32_t first = A[w + 6], count = A[w + 7] & 0xffffu;
                    if (count >= 128u || first > LEAF_FIRST_MASK)
                        return fail(h, PTX_E_SCENE, "leaf (first %u, count %u) exceeds the packed ref", first, count);
                    ref = LEAF_BIT | (count << 24) | first;
                } else {
                    ref = gidx.at(n);
                }
                return PTX_OK;
            };
            SubRoot r{};
            float *axis[3] = {r.x, r.y, r.z};
            for (int k = 0; k < 3; ++k) { axis[k][0] = as_f32(A[base + k]); axis[k][1] = as_f32(A[base + 3 + k]); }
            if (int rc = ref_of(0u, r.ref)) return rc;
            subs.push_back(r);
            root_word.push_back(base);
            for (uint32_t n : interior) {
                size_t w = (size_t)base + 8u * n;
                uint32_t L = n + 1u, R = A[w + 6] / 8u;
                size_t wl = (size_t)base + 8u * L, wr = (size_t)base + 8u * R;
                NodePair np{};
                float *naxis[3] = {np.x, np.y, np.z};
                for (int k = 0; k < 3; ++k) {
                    naxis[k][0] = as_f32(A[wl + k]); naxis[k][1] = as_f32(A[wr + k]);
                    naxis[k][2] = as_f32(A[wl + 3 + k]); naxis[k][3] = as_f32(A[wr + 3 + k]);
                }
                if (int rc = ref_of(L, np.lref)) return rc;
                if (int rc = ref_of(R, np.rref)) return rc;
                nodes.push_back(np);
                pair_sub.push_back((uint32_t)subs.size() - 1u);
                pair_words.push_back((uint32_t)wl);
                pair_words.push_back((uint32_t)wr);
            }
        }
        // the mesh's pairs by height: a pair's interior children were numbered after it (the walk
        // above), so the last pair first finds every child's height known
        {
            const uint32_t nb = mesh_node_base[m], nn = (uint32_t)nodes.size() - nb;
            mesh_nnodes[m] = nn;
            std::vector<uint32_t> height(nn, 0u);
            uint32_t top = 0;
            for (uint32_t i = nn; i-- > 0;) {
                for (const uint32_t ref : {nodes[nb + i].lref, nodes[nb + i].rref}) {
                    if (ref & LEAF_BIT) continue;
                    if (ref <= nb + i || ref >= nb + nn) return fail(h, PTX_E_SCENE, "BLAS node order: a child before its parent");
                    height[i] = std::max(height[i], height[ref - nb] + 1u);
                }
                top = std::max(top, height[i]);
            }
            auto &lv = mesh_levels[m];
            lv.assign(nn ? top + 2u : 1u, 0u);
            for (uint32_t i = 0; i < nn; ++i) lv[height[i] + 1u] += 1u;
            lv[0] = (uint32_t)order.size();
            for (size_t k = 1; k < lv.size(); ++k) lv[k] += lv[k - 1];
            std::vector<uint32_t> at(lv.begin(), lv.end() - 1);
            order.resize(order.size() + nn);
            for (uint32_t i = 0; i < nn; ++i) order[at[height[i]]++] = nb + i;
        }
        mesh_ntris[m] = mesh_tris;
        // edge-form triangles in index (leaf) order, local space
        for (uint32_t prim = 0; prim < mesh_tris; ++prim) {
            size_t ii = (size_t)off_index + off_idx + 3u * prim;
            if (ii + 3 > G.size()) return fail(h, PTX_E_SCENE, "index buffer out of range");
            float P[3][3];
            for (int v = 0; v < 3; ++v) {
                size_t vi = (size_t)off_vertex + STRIDE_VERTEX * G[ii + v];
                if (vi + 3 > G.size()) return fail(h, PTX_E_SCENE, "vertex out of range");
                for (int k = 0; k < 3; ++k) P[v][k] = as_f32(G[vi + k]);
            }
            const float e1[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
            const float e2[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
            const float rec[12] = {P[0][0], P[0][1], P[0][2], e1[0], e1[1], e1[2], e2[0], e2[1], e2[2], 0, 0, 0};
            tris.insert(tris.end(), rec, rec + 12);
            float N[3][3];
            for (int v = 0; v < 3; ++v) {
                const size_t vi = (size_t)off_vertex + STRIDE_VERTEX * G[ii + v];
                if (vi + 6 > G.size()) return fail(h, PTX_E_SCENE, "vertex normal out of range");
                for (int k = 0; k < 3; ++k) N[v][k] = as_f32(G[vi + 3 + k]);
            }
            const float tv[20] = {P[0][0], P[0][1], P[0][2], N[0][0], N[0][1], N[0][2], P[1][0], P[1][1], P[1][2], N[1][0],
                                  N[1][1], N[1][2], P[2][0], P[2][1], P[2][2], N[2][0], N[2][1], N[2][2], 0.0f, 0.0f};
            tverts.insert(tverts.end(), tv, tv + 20);
        }
    }
    if (tris.empty()) tris.resize(12, 0.0f);
    if (tverts.empty()) tverts.resize(20, 0.0f);
    if (nodes.empty()) nodes.resize(1);
    if (subs.empty()) subs.resize(1);
    h->lay_subs = std::move(subs);
    h->lay_mat_word = std::move(mat_word);
    h->lay_mesh_sub_base = std::move(mesh_sub_base);
    h->lay_mesh_nsub = std::move(mesh_nsub);
    h->lay_mesh_tri_base = std::move(mesh_tri_base);
    h->lay_mesh_ntris = std::move(mesh_ntris);
    h->lay_mesh_vertex = std::move(mesh_vertex);
    h->lay_mesh_nverts = std::move(mesh_nverts);
    h->lay_mesh_node_base = std::move(mesh_node_base);
    h->lay_mesh_nnodes = std::move(mesh_nnodes);
    h->lay_mesh_levels = std::move(mesh_levels);
    h->lay_pair_words = std::move(pair_words);
    h->lay_root_word = std::move(root_word);
    if (int rc = upload(h, h->d_refit_order, order.data(), order.size() * sizeof(uint32_t))) return rc;
    if (int rc = upload(h, h->d_pair_sub, pair_sub.data(), pair_sub.size() * sizeof(uint32_t))) return rc;
    {
        uint32_t most = 1;
        for (const uint32_t t : h->lay_mesh_ntris) most = std::max(most, t);
        if (int rc = alloc_buf(h, h->d_refit_box, (size_t)most * 6u * sizeof(float))) return rc;
    }
    h->n_inst = n_inst;
    if (int rc = layout_tables(h, true, true)) return rc;
    if (int rc = upload(h, h->d_tris, tris.data(), tris.size() * sizeof(float))) return rc;
    if (int rc = upload(h, h->d_nodes, nodes.data(), nodes.size() * sizeof(NodePair))) return rc;
    if (int rc = upload(h, h->d_tverts, tverts.data(), tverts.size() * sizeof(float))) return rc;
    h->n_tris = (uint32_t)(tris.size() / 12);
    h->n_nodes = (uint32_t)nodes.size();
    h->max_depth = max_depth;
    h->stack_depth = max_depth + 2u;
    if ((size_t)h->stack_depth * kBlock * 4u > 160u * 1024u)
        return fail(h, PTX_E_SCENE, "BLAS depth %u needs more LDS than a CU has", max_depth);
    h->layout_valid = true;
    h->layout_gen += 1u;  // (the denoiser's saved triangle records lie at the previous layout's offsets)
    for (auto &c : h->ctx) c.surf_valid = false;  // the surface records name the old layout's materials
    gbuf_key_drop_all(h);  // (the G-buffers hold hits in the old layout)
    return PTX_OK;
}

static void free_skin(ptx_handle::Skin &k) {
    for (DevBuf *b : {&k.bind, &k.target_pos, &k.target_nrm, &k.pose}) free_buf(*b);
    k = ptx_handle::Skin{};
}
void drop_skins(ptx_handle *h) {
    for (auto &k : h->skins) free_skin(k);
    h->skins.clear();
}

// ---------------------------------------------------------------- what an edit invalidates
// The handle's cached state describes the arrays and tables some frame saw.  These are the rules for it; an
// entry point that changes arrays or tables lists which of them apply.

// What every call that reads or edits the derived tables asks first.
static int layout_check(ptx_handle *h, const char *what) {
    if (!h->scene_loaded || !h->frame_set || !h->layout_valid)
        return fail(h, PTX_E_INVALID, "%s: upload a scene and set a frame first", what);
    return PTX_OK;
}
// What every change of tables or shape drops: the G-buffers hold hits and materials of the old tables, and the
// surface records, PT_1's wave state and the neighbour summaries describe those.  No denoise or upsample before
// a frame or a G-buffer pass has traced them again (dn_guide would decode old hits through the new tables).
static void frames_outdated(ptx_handle *h) {
    gbuf_key_drop_all(h);
    for (auto &c : h->ctx) c.surf_valid = c.init_state_valid = c.nbr_valid = false;
    h->drawn = h->rendered = false;
}
// The handle holds no scene until the next ptx_upload_scene: a HIP error part-way through an edit left the
// device's arrays or tables between two scenes (nothing there is worth reading back: mesh_stale), or
// ptx_upload_scene replaces them.  replaced: that call's form, which has always dropped less -- it keeps
// `rendered` (a ptx_denoise right after it is accepted if a frame ever ran: a caller can see that) and the
// wave-state and summary flags of the frame contexts other than the current one.
static void scene_lost(ptx_handle *h, bool replaced = false) {
    h->scene_loaded = h->layout_valid = false;
    h->hist_valid = h->dn_hist_valid = false;
    ut_drop(h);
    h->mesh_stale.clear();
    if (!replaced) return frames_outdated(h);
    gbuf_key_drop_all(h);
    for (auto &c : h->ctx) c.surf_valid = false;
    h->cur().init_state_valid = h->cur().nbr_valid = h->drawn = false;
}
// The reuse / GI history (d_hist).  Numbering kept (instances moved, materials changed, a mesh deformed): the
// reservoirs' triangle numbers and sub-meshes still decode, but the history's surface records (d_psurf, what
// the motion pass reprojects with) were made with the old tables or shape, so it serves its frame's camera
// alone.  Numbering changed (an instance names another mesh, an index buffer was reordered): dropped -- the
// reservoirs store path vertices as (instance, triangle of its mesh, sub-mesh), and the passes would decode
// old indices through the new tables into another triangle's or mesh's records, or past the tables.
static void history_after_edit(ptx_handle *h, bool numbering_kept) {
    if (numbering_kept) h->hist_same_only = true;
    if (!numbering_kept || h->hist_moved) h->hist_valid = false;
}
// The temporal upsampler follows moved objects only on a handle that follows (ptx_upsample_follow): tracking
// with a state, the state stays, the edit is pending and the next call compares what it kept
// (upsample_follow_table); else the state is dropped.
static void upsampler_after_edit(ptx_handle *h) {
    if (h->ut_track && h->ut_valid) h->ut_pending = true;
    else ut_drop(h);
}
// A tracking consumer (the denoiser, the temporal upsampler) keeps the triangle records its last call saw: the
// first refit of a mesh since then saves them, a copy on the stream ahead of the kernel that overwrites them
// (every stream of the handle is idle: the callers' quiesce).  `snap` has d_tverts' layout, made under layout
// `track_layout`; the mesh's mark in `deformed` becomes 1 (saved) or 2 (not saved: no history).
static hipError_t snapshot_mesh(ptx_handle *h, uint32_t mesh, std::vector<uint8_t> &deformed, const DevBuf &snap,
                                uint32_t track_layout) {
    deformed.resize(h->lay_mesh_nsub.size(), 0u);
    if (deformed[mesh]) return hipSuccess;
    const size_t off = 80u * (size_t)h->lay_mesh_tri_base[mesh], nb = 80u * (size_t)h->lay_mesh_ntris[mesh];
    const bool fits = snap.p && snap.bytes == h->d_tverts.bytes && off + nb <= snap.bytes && track_layout == h->layout_gen;
    deformed[mesh] = fits ? 1u : 2u;
    if (!fits || !nb) return hipSuccess;
    return hipMemcpyAsync((char *)snap.p + off, (const char *)h->d_tverts.p + off, nb, hipMemcpyDeviceToDevice, h->cur().stream);
}

// What the vertex calls ask of handle, mesh and range alike: the records exist in the layout, and (block) their
// words lie inside the geometry arrays -- ptx_update_vertices asks that part after it has looked at its array.
static int vertex_block_check(ptx_handle *h, const char *what, uint32_t mesh, uint32_t first, uint32_t n) {
    const size_t end = (size_t)h->lay_mesh_vertex[mesh] + (size_t)STRIDE_VERTEX * ((size_t)first + n);
    if (end > h->geometry.size() || h->d_geometry.bytes < end * 4u)
        return fail(h, PTX_E_INVALID, "%s: the mesh's vertex block lies past the geometry array", what);
    return PTX_OK;
}
static int vertex_range_check(ptx_handle *h, const char *what, uint32_t mesh, uint32_t first, uint32_t n, bool block = true) {
    if (int rc = layout_check(h, what)) return rc;
    const uint32_t n_mesh = (uint32_t)h->lay_mesh_nsub.size();
    if (mesh >= n_mesh) return fail(h, PTX_E_SCENE, "%s: mesh %u of %u", what, mesh, n_mesh);
    if ((uint64_t)first + n > h->lay_mesh_nverts[mesh])
        return fail(h, PTX_E_INVALID, "%s: vertices [%u, %llu) of mesh %u, which has %u", what, first,
                    (unsigned long long)first + n, mesh, h->lay_mesh_nverts[mesh]);
    return block ? vertex_block_check(h, what, mesh, first, n) : PTX_OK;
}
// Whether the position words (0..2) of n vertex records are all finite; if not, the first that is not.
static bool positions_finite(const uint32_t *records, uint32_t n, uint32_t &vertex, uint32_t &word) {
    for (vertex = 0; vertex < n; ++vertex)
        for (word = 0; word < 3u; ++word)
            if ((records[(size_t)STRIDE_VERTEX * vertex + word] & 0x7f800000u) == 0x7f800000u) return false;
    return true;
}
static bool all_finite(const float *p, size_t n, double &max_abs) {
    for (size_t i = 0; i < n; ++i) {
        if (!std::isfinite(p[i])) return false;
        max_abs = std::max(max_abs, (double)std::fabs(p[i]));
    }
    return true;
}
}  // namespace ptx

// ptx_build_blas: host side.  One arena holds every device array of the call (BuildArgs, ptx_launch.h), the
// zeroed words first; it is freed before the call returns.  A builder names its arrays once, in a list it runs
// twice: before the allocation the list only measures (the pointers stay null), after it the list assigns.
namespace {
struct BuildArena {
    DevBuf buf;
    size_t used = 0;
    ~BuildArena() { free_buf(buf); }
    template <class T>
    void take(T *&p, size_t count) {  // the next array of the list, on a 256-byte boundary
        p = buf.p ? (T *)((char *)buf.p + used) : nullptr;
        used += (count * sizeof(T) + 255u) & ~(size_t)255u;
    }
};

// How a builder's core gets its input onto the device: the packed positions (V x 3 f32) and the index
// buffer (3T), both in the call's arena, written and waited for or enqueued on the handle's stream.
// ptx_build_blas copies the caller's host arrays in; ptx_rebuild_mesh takes them from the handle's geometry.
using BlasFill = std::function<hipError_t(float *pos, uint32_t *idx)>;

// The cores of ptx_build_blas and ptx_rebuild_mesh, after the caller's checks.  Of `d` they read the counts,
// max_leaf and the groups (host memory); positions and indices come through `fill`.  `worst` =
// sum(2 * tri_count - 1) bounds the nodes; nodes_out holds 8 * worst words.
// PTX_BLAS_SAH:
int build_blas_sah(ptx_handle *h, const char *what, const ptx_blas_desc *d, const BlasFill &fill, uint64_t worst,
                   uint32_t *nodes_out, uint32_t *indices_out, uint32_t *group_nodes_out, uint32_t *max_depth_out) {
    const uint32_t T = d->n_tris, V = d->n_vertices, G = d->n_groups;
    HIP_CHECK(h, hipSetDevice(h->device));
    const hipStream_t st = h->cur().stream;
    SahArgs A{};
    A.n_tris = T;
    A.n_groups = G;
    A.max_leaf = d->max_leaf ? d->max_leaf : 10u;
    A.node_cap = (uint32_t)worst;
    BuildArena ar;
    size_t zero_bytes = 0;
    const size_t nT = T, nV = V, nG = G, nW = worst;
    auto carve = [&] {
        ar.used = 0;
        ar.take(A.counters, 2u);
        zero_bytes = ar.used;
        ar.take(A.pos, 3u * nV), ar.take(A.idx, 3u * nT), ar.take(A.groups, nG);
        ar.take(A.rec, 6u * nT), ar.take(A.order[0], nT), ar.take(A.order[1], nT), ar.take(A.final_order, nT);
        ar.take(A.n_range, nW), ar.take(A.n_box, 6u * nW), ar.take(A.n_link, nW), ar.take(A.n_size, nW);
        ar.take(A.goff, nG);
        ar.take(A.nodes_out, 8u * nW), ar.take(A.idx_out, 3u * nT);
    };
    carve();
    if (int rc = alloc_buf(h, ar.buf, ar.used)) return rc;  // (PTX_E_NOMEM: nothing was launched)
    carve();
    hipError_t le = hipMemsetAsync(ar.buf.p, 0, zero_bytes, st);
    if (le == hipSuccess) le = fill((float *)A.pos, (uint32_t *)A.idx);
    if (le == hipSuccess) le = copy_sync(h, (void *)A.groups, d->groups, 8u * (size_t)G, hipMemcpyHostToDevice);
    auto step = [&](SahStep s, uint32_t first, uint32_t n, uint32_t level = 0u) {
        le = slot_timed(h, PTX_STAT_BUILD, st, le, [&] { return launch_sah(A, s, first, n, level, st); });
    };
    step(SahStep::Init, 0u, T);
    // One launch per depth: the node counter read back after each sizes the next.  At depth 40 every node is a
    // leaf, so 41 launches end any tree.
    constexpr uint32_t kLevels = 41u;
    std::vector<std::pair<uint32_t, uint32_t>> levels;  // {first node, nodes} per depth
    uint32_t first = 0u, live = G, counters[2] = {0u, 0u};
    while (le == hipSuccess && live > 0u && levels.size() < kLevels) {
        step(SahStep::Level, first, live, (uint32_t)levels.size());
        if (le != hipSuccess) break;
        if (int rc = read_to_host(h, counters, A.counters, sizeof counters)) return rc;
        levels.emplace_back(first, live);
        if (counters[0] < first + live || counters[0] > worst)
            return fail(h, PTX_E_HIP, "%s: %u nodes after depth %zu, the groups can need %llu", what, counters[0], levels.size() - 1u,
                        (unsigned long long)worst);
        first += live;
        live = counters[0] - first;
    }
    if (le != hipSuccess) return fail(h, PTX_E_HIP, "%s: %s", what, hipGetErrorString(le));
    if (live > 0u) return fail(h, PTX_E_HIP, "%s: the tree did not finish in %u levels", what, kLevels);
    if (counters[1] > 0xFFFFu)
        return fail(h, PTX_E_SCENE, "%s: a leaf of %u triangles cannot be serialised (the count field holds 65535)", what, counters[1]);
    for (size_t l = levels.size(); l-- > 0u;) step(SahStep::Size, levels[l].first, levels[l].second);
    if (le != hipSuccess) return fail(h, PTX_E_HIP, "%s: %s", what, hipGetErrorString(le));
    std::vector<uint32_t> gsize(G), goff(G);
    if (int rc = read_to_host(h, gsize.data(), A.n_size, 4u * (size_t)G)) return rc;  // (the roots are nodes 0 .. G - 1)
    uint64_t total = 0;
    for (uint32_t g = 0; g < G; ++g) {
        goff[g] = (uint32_t)total;
        total += gsize[g];
    }
    if (total != first) return fail(h, PTX_E_HIP, "%s: the roots hold %llu nodes of %u made", what, (unsigned long long)total, first);
    A.n_nodes = first;
    le = copy_sync(h, (void *)A.goff, goff.data(), 4u * (size_t)G, hipMemcpyHostToDevice);
    step(SahStep::Emit, 0u, A.n_nodes);
    step(SahStep::Gather, 0u, T);
    if (le != hipSuccess) return fail(h, PTX_E_HIP, "%s: %s", what, hipGetErrorString(le));
    if (int rc = read_to_host(h, nodes_out, A.nodes_out, 32u * (size_t)total)) return rc;
    if (int rc = read_to_host(h, indices_out, A.idx_out, 12u * (size_t)T)) return rc;
    *max_depth_out = (uint32_t)levels.size() - 1u;
    std::memcpy(group_nodes_out, gsize.data(), 4u * (size_t)G);
    return PTX_OK;
}

// PTX_BLAS_LBVH:
int build_blas_lbvh(ptx_handle *h, const char *what, const ptx_blas_desc *d, const BlasFill &fill, uint64_t worst,
                    uint32_t *nodes_out, uint32_t *indices_out, uint32_t *group_nodes_out, uint32_t *max_depth_out) {
    const uint32_t T = d->n_tris, V = d->n_vertices, G = d->n_groups;
    HIP_CHECK(h, hipSetDevice(h->device));
    const hipStream_t st = h->cur().stream;
    BuildArgs A{};
    A.n_tris = T;
    A.n_groups = G;
    A.max_leaf = d->max_leaf ? d->max_leaf : 10u;
    A.n_nodes = (uint32_t)worst;
    BuildArena ar;
    hipError_t le = build_sort_bytes(A, &A.sort_bytes);  // (from the counts alone: no array exists yet)
    if (le != hipSuccess) return fail(h, PTX_E_HIP, "%s: sort storage: %s", what, hipGetErrorString(le));
    size_t zero_bytes = 0;
    const size_t nT = T, nV = V, nG = G, nW = worst;
    auto carve = [&] {
        ar.used = 0;
        ar.take(A.cbound, 6u * nG), ar.take(A.done, 2u * nT), ar.take(A.max_depth, 1u);
        zero_bytes = ar.used;
        ar.take(A.parent, 2u * nT);
        ar.take(A.pos, 3u * nV), ar.take(A.idx, 3u * nT), ar.take(A.groups, nG);
        ar.take(A.tbox, 3u * nT), ar.take(A.centre, 3u * nT), ar.take(A.seg, nT);
        ar.take(A.key_in, nT), ar.take(A.key_out, nT), ar.take(A.val_in, nT), ar.take(A.val_out, nT);
        ar.take(A.rng, nT), ar.take(A.child, nT);
        ar.take(A.nbox, 6u * nT), ar.take(A.esize, 2u * nT);
        ar.take(A.gsize, nG), ar.take(A.goff, nG);
        ar.take(A.nodes_out, 8u * nW), ar.take(A.idx_out, 3u * nT);
        unsigned char *sort_temp;
        ar.take(sort_temp, A.sort_bytes), A.sort_temp = sort_temp;
    };
    carve();
    if (int rc = alloc_buf(h, ar.buf, ar.used)) return rc;
    carve();
    le = hipMemsetAsync(ar.buf.p, 0, zero_bytes, st);
    if (le == hipSuccess) le = hipMemsetAsync(A.parent, 0xFF, 8u * (size_t)T, st);
    if (le == hipSuccess) le = fill((float *)A.pos, (uint32_t *)A.idx);
    if (le == hipSuccess) le = copy_sync(h, (void *)A.groups, d->groups, 8u * (size_t)G, hipMemcpyHostToDevice);
    auto step = [&](BuildStep s, uint32_t stamp = 0u) {
        le = slot_timed(h, PTX_STAT_BUILD, st, le, [&] { return launch_build(A, s, stamp, st); });
    };
    step(BuildStep::Tris);
    step(BuildStep::Keys);
    step(BuildStep::Sort);
    step(BuildStep::Tree);
    step(BuildStep::Leaves);
    // One launch per height of the emitted tree, which the host does not know: rounds of kRound launches and a
    // readback of the roots' sizes, until every root is finished.  A key has 62 bits, which bounds a tree's height.
    constexpr uint32_t kRound = 24u, kMaxHeight = 72u;
    std::vector<uint32_t> gsize(G), goff(G);
    uint32_t stamp = 2u;
    bool finished = false;
    while (le == hipSuccess && !finished && stamp < 2u + kMaxHeight) {
        for (uint32_t k = 0; k < kRound; ++k) step(BuildStep::Level, stamp++);
        step(BuildStep::Roots);
        if (le != hipSuccess) break;
        if (int rc = read_to_host(h, gsize.data(), A.gsize, 4u * (size_t)G)) return rc;
        finished = std::find(gsize.begin(), gsize.end(), 0u) == gsize.end();
    }
    if (le != hipSuccess) return fail(h, PTX_E_HIP, "%s: %s", what, hipGetErrorString(le));
    if (!finished) return fail(h, PTX_E_HIP, "%s: the tree did not finish in %u heights", what, kMaxHeight);
    uint64_t total = 0;
    for (uint32_t g = 0; g < G; ++g) {
        goff[g] = (uint32_t)total;
        total += gsize[g];
    }
    if (total > worst) return fail(h, PTX_E_HIP, "%s: %llu nodes, more than the groups can need", what, (unsigned long long)total);
    A.n_nodes = (uint32_t)total;
    le = copy_sync(h, (void *)A.goff, goff.data(), 4u * (size_t)G, hipMemcpyHostToDevice);
    step(BuildStep::Emit);
    step(BuildStep::Gather);
    if (le != hipSuccess) return fail(h, PTX_E_HIP, "%s: %s", what, hipGetErrorString(le));
    if (int rc = read_to_host(h, nodes_out, A.nodes_out, 32u * (size_t)total)) return rc;
    if (int rc = read_to_host(h, indices_out, A.idx_out, 12u * (size_t)T)) return rc;
    if (int rc = read_to_host(h, max_depth_out, A.max_depth, 4u)) return rc;
    std::memcpy(group_nodes_out, gsize.data(), 4u * (size_t)G);
    return PTX_OK;
}

int build_blas_core(ptx_handle *h, const char *what, const ptx_blas_desc *d, const BlasFill &fill, uint64_t worst,
                    uint32_t *nodes_out, uint32_t *indices_out, uint32_t *group_nodes_out, uint32_t *max_depth_out) {
    return (d->reserved[0] == PTX_BLAS_SAH ? build_blas_sah : build_blas_lbvh)(h, what, d, fill, worst, nodes_out, indices_out,
                                                                               group_nodes_out, max_depth_out);
}
}  // namespace

extern "C" {

int ptx_upload_scene(ptx_handle *h, const uint32_t *scene, size_t n_scene, const uint32_t *geometry,
                     size_t n_geometry, const uint32_t *accel, size_t n_accel) {
    if (!h) return PTX_E_INVALID;
    HIP_CHECK(h, hipSetDevice(h->device));  // handles of one process may sit on several GPUs
    if (!scene || !geometry || (!accel && n_accel)) return fail(h, PTX_E_INVALID, "null scene array");
    if (int rc = quiesce(h)) return rc;  // frames in flight still read the old scene and layout
    h->scene.assign(scene, scene + n_scene);
    h->geometry.assign(geometry, geometry + n_geometry);
    h->accel.assign(accel ? accel : scene, accel ? accel + n_accel : scene);
    h->mesh_stale.clear();
    drop_skins(h);  // (bound to the old scene's meshes)
    if (int rc = upload(h, h->d_scene, scene, n_scene * 4u)) return rc;
    if (int rc = upload(h, h->d_geometry, geometry, n_geometry * 4u)) return rc;
    // the old scene is lost (hits in it, the histories that show it -- the denoiser's and, with its marks,
    // ptx_upsample_temporal's), and the new one is there
    scene_lost(h, /*replaced=*/true);
    h->dn_deformed.clear();  // (its marks name the old scene's meshes; without a state nothing reads them)
    h->scene_loaded = true;
    if (h->frame_set) return build_layout(h);
    return PTX_OK;
}

int ptx_update_scene(ptx_handle *h, const uint32_t *scene, size_t n_scene, uint32_t *changed_out) {
    if (!h) return PTX_E_INVALID;
    if (!scene) return fail(h, PTX_E_INVALID, "ptx_update_scene: null scene array");
    if (int rc = layout_check(h, "ptx_update_scene")) return rc;
    if (n_scene != h->scene.size())
        return fail(h, PTX_E_INVALID, "ptx_update_scene: %zu words, the uploaded array has %zu", n_scene, h->scene.size());
    // the blocks, through the uniform set on the handle: instances, (descriptors,) materials, lights + CDF
    const uint32_t *U = h->uniform;
    const size_t inst_end = (size_t)STRIDE_INSTANCE * h->n_inst, off_mat = U[U_OFF_MAT], off_light = U[U_OFF_LIGHT];
    if (inst_end > off_mat || off_mat > off_light || off_light > n_scene)
        return fail(h, PTX_E_INVALID, "ptx_update_scene: the uniform's offsets do not order the scene array's blocks");
    const size_t lo[3] = {0, off_mat, off_light}, hi[3] = {inst_end, off_light, n_scene};
    size_t first[3], last[3];  // the changed words of each block: [first, last)
    uint32_t mask = 0;
    for (int b = 0; b < 3; ++b) {
        first[b] = last[b] = hi[b];
        for (size_t w = lo[b]; w < hi[b]; ++w)
            if (scene[w] != h->scene[w]) {
                if (first[b] == hi[b]) first[b] = w;
                last[b] = w + 1;
            }
        if (first[b] != hi[b]) mask |= 1u << b;
    }
    static_assert(PTX_EDIT_INSTANCES == 1u && PTX_EDIT_MATERIALS == 2u && PTX_EDIT_LIGHTS == 4u, "block order");
    if (std::memcmp(scene + inst_end, h->scene.data() + inst_end, (off_mat - inst_end) * 4u) != 0)
        return fail(h, PTX_E_INVALID, "ptx_update_scene: the mesh descriptors differ: a new layout needs ptx_upload_scene");
    bool mesh_switched = false;  // an instance names another loaded mesh
    if (mask & PTX_EDIT_INSTANCES) {
        const uint32_t n_mesh = (uint32_t)h->lay_mesh_nsub.size();
        for (uint32_t i = 0; i < h->n_inst; ++i) {
            const uint32_t mesh = scene[STRIDE_INSTANCE * i + 32u];
            if (mesh >= n_mesh)
                return fail(h, PTX_E_SCENE, "ptx_update_scene: instance %u references mesh %u of %u", i, mesh, n_mesh);
            mesh_switched = mesh_switched || mesh != h->scene[STRIDE_INSTANCE * i + 32u];
        }
    }
    if (changed_out) *changed_out = mask;
    if (!mask) return PTX_OK;
    HIP_CHECK(h, hipSetDevice(h->device));
    if (int rc = quiesce(h)) return rc;  // frames in flight still read the scene array and the tables
    // From here on the handle changes: a HIP error part-way leaves it between the two scenes (scene_lost).
    int rc = PTX_OK;
    for (int b = 0; b < 3 && rc == PTX_OK; ++b) {
        if (!(mask & (1u << b))) continue;
        std::memcpy(h->scene.data() + first[b], scene + first[b], (last[b] - first[b]) * 4u);
        if (copy_sync(h, (uint32_t *)h->d_scene.p + first[b], scene + first[b], (last[b] - first[b]) * 4u,
                      hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(h, PTX_E_HIP, "ptx_update_scene: the copy of the changed words failed");
    }
    const bool tables = (mask & (PTX_EDIT_INSTANCES | PTX_EDIT_MATERIALS)) != 0;
    if (rc == PTX_OK && tables)
        rc = layout_tables(h, (mask & PTX_EDIT_INSTANCES) != 0, (mask & PTX_EDIT_MATERIALS) != 0);
    if (rc != PTX_OK) {
        scene_lost(h);
        return rc;
    }
    if (!tables) return PTX_OK;  // (PT_01 reads no light: everything kept stays)
    frames_outdated(h);
    history_after_edit(h, /*numbering_kept=*/!mesh_switched);
    // only an instance edit moves what the upsampler shows; ptx_denoise's temporal mode always follows
    // instances (denoise_front), so its history stays
    if (mask & PTX_EDIT_INSTANCES) upsampler_after_edit(h);
    return PTX_OK;
}

// The shared tail of ptx_update_vertices and ptx_skin_vertices, the device's vertex records of `mesh`
// being the new ones (or `le` the error that kept them from it): the refit chain, the readback of the
// mesh's root boxes, the instance table, and what the call keeps and drops.  `stale`: which of the
// host's copies the device is now ahead of (ptx_handle::mesh_stale).
static int refit_after_vertices(ptx_handle *h, uint32_t mesh, hipError_t le, uint8_t stale, const char *what) {
    const hipStream_t st = h->cur().stream;
    const uint32_t *d = h->scene.data() + h->uniform[U_OFF_DESC] + STRIDE_DESCRIPTOR * mesh;
    RefitMesh m{};
    m.G = (const uint32_t *)h->d_geometry.p;
    m.tris = (float4 *)h->d_tris.p;
    m.tverts = (float4 *)h->d_tverts.p;
    m.nodes = (NodePair *)h->d_nodes.p;
    m.subs = (SubRoot *)h->d_subs.p;
    m.box = (float2 *)h->d_refit_box.p;
    m.order = (const uint32_t *)h->d_refit_order.p;
    m.vertex = h->lay_mesh_vertex[mesh];
    m.index = h->uniform[U_OFF_INDEX] + d[1];
    m.tri_base = h->lay_mesh_tri_base[mesh];
    m.n_tris = h->lay_mesh_ntris[mesh];
    m.sub_base = h->lay_mesh_sub_base[mesh];
    m.n_subs = h->lay_mesh_nsub[mesh];
    // a tracking denoiser (include/ptx.h ptx_denoise, "Vertex motion") keeps the shape its last temporal call
    // saw; a tracking temporal upsampler (ptx_upsample_follow) the shape *its* last call saw, in a buffer of its
    // own -- a full-size handle may hold a denoiser state from another moment
    if (le == hipSuccess && h->dn_track && h->dn_hist_valid)
        le = snapshot_mesh(h, mesh, h->dn_deformed, h->d_dn_snap, h->dn_track_layout);
    if (le == hipSuccess && h->ut_track && h->ut_valid)
        le = snapshot_mesh(h, mesh, h->ut_deformed, h->d_ut_snap, h->ut_track_layout);
    le = slot_timed(h, PTX_STAT_REFIT, st, le, [&] { return launch_refit_tris(m, st); });
    const auto &lv = h->lay_mesh_levels[mesh];  // lowest height first: a pair's interior children are lower
    for (size_t k = 0; k + 1 < lv.size(); ++k)
        le = slot_timed(h, PTX_STAT_REFIT, st, le, [&] { return launch_refit_level(m, lv[k], lv[k + 1] - lv[k], st); });
    le = slot_timed(h, PTX_STAT_REFIT, st, le, [&] { return launch_refit_roots(m, st); });
    int rc = le == hipSuccess ? PTX_OK : fail(h, PTX_E_HIP, "%s: %s", what, hipGetErrorString(le));
    // the mesh's root boxes (the only readback): the instance cull boxes are made from them
    if (rc == PTX_OK && m.n_subs)
        rc = read_to_host(h, h->lay_subs.data() + m.sub_base, m.subs + m.sub_base, (size_t)m.n_subs * sizeof(SubRoot));
    if (rc == PTX_OK) rc = layout_tables(h, true, false);
    if (rc != PTX_OK) {
        scene_lost(h);
        return rc;
    }
    h->mesh_stale.resize(h->lay_mesh_nsub.size(), 0u);
    h->mesh_stale[mesh] |= stale;
    // kept and dropped as by an instance edit without a switched mesh (ptx_update_scene).  Neither the temporal
    // upsampler nor ptx_denoise's temporal mode follows vertices unless the handle is tracking (above): the
    // denoiser's history stays and is looked up as for an unchanged instance
    frames_outdated(h);
    history_after_edit(h, /*numbering_kept=*/true);
    upsampler_after_edit(h);
    return PTX_OK;
}

int ptx_update_vertices(ptx_handle *h, uint32_t mesh, uint32_t first_vertex, uint32_t n_vertices, const uint32_t *vertices) {
    if (!h) return PTX_E_INVALID;
    const char *what = "ptx_update_vertices";
    // (build_layout accepts a scene without triangles whose vertex blocks lie past the geometry array: there an
    // empty update is accepted and a bad array is refused before the block is, so the array comes between)
    if (int rc = vertex_range_check(h, what, mesh, first_vertex, n_vertices, /*block=*/false)) return rc;
    if (n_vertices == 0u) return PTX_OK;
    if (!vertices) return fail(h, PTX_E_INVALID, "%s: null vertex array", what);
    uint32_t bad_v, bad_k;
    if (!positions_finite(vertices, n_vertices, bad_v, bad_k))
        return fail(h, PTX_E_INVALID, "%s: vertex %u: position word %u is not finite", what, first_vertex + bad_v, bad_k);
    if (int rc = vertex_block_check(h, what, mesh, first_vertex, n_vertices)) return rc;
    const size_t word0 = (size_t)h->lay_mesh_vertex[mesh] + (size_t)STRIDE_VERTEX * first_vertex;
    const size_t n_words = (size_t)STRIDE_VERTEX * n_vertices;
    HIP_CHECK(h, hipSetDevice(h->device));
    if (int rc = quiesce(h)) return rc;  // frames in flight still read the geometry and the tables
    // From here on the handle changes: a HIP error part-way leaves it between the two shapes (scene_lost).
    std::memcpy(h->geometry.data() + word0, vertices, n_words * 4u);
    const hipError_t le = copy_sync(h, (uint32_t *)h->d_geometry.p + word0, vertices, n_words * 4u, hipMemcpyHostToDevice);
    return refit_after_vertices(h, mesh, le, kStaleAccel, what);
}

int ptx_read_accel(ptx_handle *h, uint32_t *accel_out, size_t n_accel) {
    if (!h) return PTX_E_INVALID;
    if (int rc = layout_check(h, "ptx_read_accel")) return rc;
    if (n_accel != h->accel.size() || (!accel_out && n_accel))
        return fail(h, PTX_E_INVALID, "ptx_read_accel: %zu words, the uploaded array has %zu", n_accel, h->accel.size());
    HIP_CHECK(h, hipSetDevice(h->device));
    if (int rc = quiesce(h)) return rc;
    if (n_accel) std::memcpy(accel_out, h->accel.data(), n_accel * 4u);
    return device_boxes_into(h, accel_out);
}

int ptx_set_skin(ptx_handle *h, const ptx_skin_desc *d) {
    if (!h) return PTX_E_INVALID;
    if (!d) return fail(h, PTX_E_INVALID, "ptx_set_skin: null descriptor");
    const char *what = "ptx_set_skin";
    if (int rc = vertex_range_check(h, what, d->mesh, d->first_vertex, d->n_vertices)) return rc;
    if (d->reserved[0] | d->reserved[1] | d->reserved[2]) return fail(h, PTX_E_INVALID, "%s: a reserved word is not zero", what);
    const uint32_t mesh = d->mesh, n = d->n_vertices;
    if (n == 0u) {  // remove the mesh's skin
        if (mesh < h->skins.size()) free_skin(h->skins[mesh]);
        return PTX_OK;
    }
    if (d->n_joints < 1u || d->n_joints > kSkinMaxJoints) return fail(h, PTX_E_INVALID, "%s: %u joints (1..256)", what, d->n_joints);
    if (d->n_targets > kSkinMaxTargets) return fail(h, PTX_E_INVALID, "%s: %u morph targets (0..8)", what, d->n_targets);
    if (!d->joints || !d->weights) return fail(h, PTX_E_INVALID, "%s: null joints or weights", what);
    if ((d->target_pos != nullptr) != (d->n_targets > 0u) || (d->target_nrm && !d->n_targets))
        return fail(h, PTX_E_INVALID, "%s: %u morph targets and a %s delta table", what, d->n_targets, d->n_targets ? "null" : "non-null");
    const size_t word0 = (size_t)h->lay_mesh_vertex[mesh] + (size_t)STRIDE_VERTEX * d->first_vertex;
    if (word0 % 4u) return fail(h, PTX_E_INVALID, "%s: the mesh's vertex block does not begin on a 16-byte boundary", what);
    for (size_t i = 0; i < 4u * (size_t)n; ++i)
        if (d->joints[i] >= d->n_joints)
            return fail(h, PTX_E_INVALID, "%s: vertex %zu: joint %u of %u", what, d->first_vertex + i / 4u, d->joints[i], d->n_joints);
    ptx_handle::Skin k;
    k.first = d->first_vertex;
    k.n = n;
    k.n_joints = d->n_joints;
    k.n_targets = d->n_targets;
    double unused = 0.0;
    if (!all_finite(d->weights, 4u * (size_t)n, unused)) return fail(h, PTX_E_INVALID, "%s: a weight is not finite", what);
    for (size_t v = 0; v < n; ++v) {
        const float *w = d->weights + 4u * v;
        k.w_max = std::max(k.w_max, (double)std::fabs(w[0]) + std::fabs(w[1]) + std::fabs(w[2]) + std::fabs(w[3]));
    }
    const size_t n_delta = 3u * (size_t)n * d->n_targets;
    if (d->n_targets && (!all_finite(d->target_pos, n_delta, k.d_max) || (d->target_nrm && !all_finite(d->target_nrm, n_delta, k.d_max))))
        return fail(h, PTX_E_INVALID, "%s: a morph delta is not finite", what);
    HIP_CHECK(h, hipSetDevice(h->device));
    // the bind pose: the caller's, or words 0..5 of the records as they are now -- on the device, where
    // ptx_skin_vertices has left the host's copy behind
    std::vector<uint32_t> now;
    if (!d->bind) {
        now.assign(h->geometry.begin() + word0, h->geometry.begin() + word0 + (size_t)STRIDE_VERTEX * n);
        if (mesh < h->mesh_stale.size() && (h->mesh_stale[mesh] & kStaleGeometry)) {
            if (int rc = quiesce(h)) return rc;
            if (int rc = read_to_host(h, now.data(), (const uint32_t *)h->d_geometry.p + word0, now.size() * 4u)) return rc;
        }
    }
    std::vector<float> rec(12u * (size_t)n);
    for (size_t v = 0; v < n; ++v) {
        float *r = rec.data() + 12u * v;
        if (d->bind) std::memcpy(r, d->bind + 6u * v, 24);
        else std::memcpy(r, now.data() + STRIDE_VERTEX * v, 24);
        std::memcpy(r + 6, d->weights + 4u * v, 16);
        const uint32_t *j = d->joints + 4u * v;
        const uint32_t packed[2] = {j[0] | j[1] << 16, j[2] | j[3] << 16};
        std::memcpy(r + 10, packed, 8);
        if (!all_finite(r, 6, k.p_max)) return fail(h, PTX_E_INVALID, "%s: vertex %zu: a bind word is not finite", what, d->first_vertex + v);
    }
    // From here on the GPU is touched, but nothing a frame reads: new tables, then the old skin's freed.
    int rc = upload(h, k.bind, rec.data(), rec.size() * sizeof(float));
    if (rc == PTX_OK && d->n_targets) rc = upload(h, k.target_pos, d->target_pos, n_delta * sizeof(float));
    if (rc == PTX_OK && d->target_nrm) rc = upload(h, k.target_nrm, d->target_nrm, n_delta * sizeof(float));
    if (rc == PTX_OK) rc = alloc_buf(h, k.pose, (12u * kSkinMaxJoints + kSkinMaxTargets) * sizeof(float));
    if (rc != PTX_OK) {
        free_skin(k);
        return rc;
    }
    if (h->skins.size() <= mesh) h->skins.resize(h->lay_mesh_nsub.size());
    free_skin(h->skins[mesh]);
    h->skins[mesh] = k;
    return PTX_OK;
}

int ptx_skin_vertices(ptx_handle *h, uint32_t mesh, const float *palette, const float *target_weights) {
    if (!h) return PTX_E_INVALID;
    const char *what = "ptx_skin_vertices";
    if (int rc = vertex_range_check(h, what, mesh, 0u, 0u)) return rc;
    if (mesh >= h->skins.size() || h->skins[mesh].n == 0u) return fail(h, PTX_E_INVALID, "%s: mesh %u has no skin", what, mesh);
    ptx_handle::Skin &k = h->skins[mesh];
    // (the layout may have been derived again since ptx_set_skin: the range is checked against this one)
    if (int rc = vertex_range_check(h, what, mesh, k.first, k.n)) return rc;
    const size_t word0 = (size_t)h->lay_mesh_vertex[mesh] + (size_t)STRIDE_VERTEX * k.first;
    if (word0 % 4u || word0 > 0xffffffffull) return fail(h, PTX_E_INVALID, "%s: the mesh's vertex block moved off a 16-byte boundary", what);
    if (!palette) return fail(h, PTX_E_INVALID, "%s: null palette", what);
    if ((target_weights != nullptr) != (k.n_targets > 0u))
        return fail(h, PTX_E_INVALID, "%s: the skin has %u morph targets and the target weights are %s", what, k.n_targets,
                    target_weights ? "given" : "null");
    double m_max = 0.0, t_sum = 0.0, unused = 0.0;
    if (!all_finite(palette, 12u * (size_t)k.n_joints, m_max)) return fail(h, PTX_E_INVALID, "%s: a palette element is not finite", what);
    if (k.n_targets && !all_finite(target_weights, k.n_targets, unused)) return fail(h, PTX_E_INVALID, "%s: a target weight is not finite", what);
    for (uint32_t t = 0; t < k.n_targets; ++t) t_sum += std::fabs((double)target_weights[t]);
    // below 2^96 every P' is finite by construction (include/ptx.h): no flag, nothing partially applied
    const double bound = 4.0 * k.w_max * m_max * (3.0 * (k.p_max + t_sum * k.d_max) + 1.0);
    if (!(bound < 0x1p96)) return fail(h, PTX_E_INVALID, "%s: the overflow bound %g is not below 2^96", what, bound);
    HIP_CHECK(h, hipSetDevice(h->device));
    if (int rc = quiesce(h)) return rc;  // frames in flight still read the geometry and the tables
    // From here on the handle changes (ptx_update_vertices: a HIP error part-way leaves it without a scene).
    const hipStream_t st = h->cur().stream;
    std::vector<float> pose(12u * (size_t)k.n_joints + k.n_targets);
    std::memcpy(pose.data(), palette, 48u * (size_t)k.n_joints);
    if (k.n_targets) std::memcpy(pose.data() + 12u * (size_t)k.n_joints, target_weights, 4u * (size_t)k.n_targets);
    hipError_t le = copy_sync(h, k.pose.p, pose.data(), pose.size() * sizeof(float), hipMemcpyHostToDevice);
    SkinArgs a{};
    a.G = (uint32_t *)h->d_geometry.p;
    a.bind = (const float4 *)k.bind.p;
    a.target_pos = (const float *)k.target_pos.p;
    a.target_nrm = (const float *)k.target_nrm.p;
    a.palette = (const float4 *)k.pose.p;
    a.target_weights = (const float *)k.pose.p + 12u * (size_t)k.n_joints;
    a.word0 = (uint32_t)word0;
    a.n = k.n;
    a.n_joints = k.n_joints;
    a.n_targets = k.n_targets;
    le = slot_timed(h, PTX_STAT_REFIT, st, le, [&] { return launch_skin_vertices(a, st); });
    return refit_after_vertices(h, mesh, le, kStaleGeometry | kStaleAccel, what);
}

int ptx_build_blas(ptx_handle *h, const ptx_blas_desc *d, uint32_t *nodes_out, size_t n_node_words, uint32_t *indices_out,
                   uint32_t *group_nodes_out, uint32_t *max_depth_out) {
    if (!h) return PTX_E_INVALID;
    const char *what = "ptx_build_blas";
    if (!d) return fail(h, PTX_E_INVALID, "%s: null descriptor", what);
    if (d->reserved[0] > PTX_BLAS_SAH) return fail(h, PTX_E_INVALID, "%s: builder %u (0 = LBVH, 1 = SAH)", what, d->reserved[0]);
    if (d->reserved[1] | d->reserved[2]) return fail(h, PTX_E_INVALID, "%s: a reserved word is not zero", what);
    const uint32_t T = d->n_tris, V = d->n_vertices, G = d->n_groups;
    if (T == 0u || T > LEAF_FIRST_MASK + 1u) return fail(h, PTX_E_INVALID, "%s: %u triangles (1..%u)", what, T, LEAF_FIRST_MASK + 1u);
    if (d->max_leaf > 64u) return fail(h, PTX_E_INVALID, "%s: max_leaf %u (0 = 10, or 1..64)", what, d->max_leaf);
    if (!d->positions || !d->indices || (!d->groups && G) || !indices_out || (!group_nodes_out && G) || !max_depth_out ||
        (!nodes_out && G))
        return fail(h, PTX_E_INVALID, "%s: null array", what);
    uint64_t worst = 0, next_free = 0;
    for (uint32_t g = 0; g < G; ++g) {
        const uint64_t first = d->groups[2u * g], count = d->groups[2u * g + 1u];
        if (count == 0u) return fail(h, PTX_E_INVALID, "%s: group %u is empty", what, g);
        if (first < next_free) return fail(h, PTX_E_INVALID, "%s: group %u begins at triangle %llu, inside or ahead of group %u", what, g,
                                           (unsigned long long)first, g - 1u);
        if (first + count > T) return fail(h, PTX_E_INVALID, "%s: group %u reaches triangle %llu of %u", what, g,
                                           (unsigned long long)(first + count), T);
        next_free = first + count;
        worst += 2u * count - 1u;
    }
    if ((uint64_t)n_node_words < 8u * worst)
        return fail(h, PTX_E_INVALID, "%s: %zu node words, the groups may need %llu", what, n_node_words, (unsigned long long)(8u * worst));
    for (size_t i = 0; i < 3u * (size_t)T; ++i)
        if (d->indices[i] >= V) return fail(h, PTX_E_INVALID, "%s: triangle %zu: index %u of %u vertices", what, i / 3u, d->indices[i], V);
    double unused = 0.0;
    if (!all_finite(d->positions, 3u * (size_t)V, unused)) return fail(h, PTX_E_INVALID, "%s: a position is not finite", what);
    if (G == 0u) {  // nothing to build: every triangle keeps its place
        std::memcpy(indices_out, d->indices, 12u * (size_t)T);
        *max_depth_out = 0u;
        return PTX_OK;
    }
    // From here on the GPU is touched, but nothing a frame reads or writes.
    const BlasFill fill = [&](float *pos, uint32_t *idx) {
        hipError_t e = copy_sync(h, pos, d->positions, 12u * (size_t)V, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = copy_sync(h, idx, d->indices, 12u * (size_t)T, hipMemcpyHostToDevice);
        return e;
    };
    return build_blas_core(h, what, d, fill, worst, nodes_out, indices_out, group_nodes_out, max_depth_out);
}

// ptx_rebuild_mesh: a loaded mesh's BLAS built again from the device's vertex records and spliced into the
// handle's arrays (include/ptx.h states the rule; scene/world.py rebuild_mesh is the same in numpy).
// Everything that can be refused is refused before the commit; the commit ends in build_layout.
int ptx_rebuild_mesh(ptx_handle *h, uint32_t mesh, uint32_t builder, uint32_t max_leaf, ptx_rebuild_info *info_out) {
    if (!h) return PTX_E_INVALID;
    const char *what = "ptx_rebuild_mesh";
    if (int rc = layout_check(h, what)) return rc;
    if (builder > PTX_BLAS_SAH) return fail(h, PTX_E_INVALID, "%s: builder %u (0 = LBVH, 1 = SAH)", what, builder);
    if (max_leaf > 64u) return fail(h, PTX_E_INVALID, "%s: max_leaf %u (0 = 10, or 1..64)", what, max_leaf);
    const uint32_t n_mesh = (uint32_t)h->lay_mesh_nsub.size();
    if (mesh >= n_mesh) return fail(h, PTX_E_SCENE, "%s: mesh %u of %u", what, mesh, n_mesh);
    HIP_CHECK(h, hipSetDevice(h->device));
    if (int rc = quiesce(h)) return rc;  // frames in flight still read the geometry and the tables
    // the host's copies first: build_layout would otherwise bring them up to date over the splice
    if (!h->mesh_stale.empty())
        if (int rc = sync_host_mirror(h)) return rc;
    const uint32_t *U = h->uniform;
    const uint32_t off_desc = U[U_OFF_DESC], off_index = U[U_OFF_INDEX], off_subroot = U[U_OFF_SUBROOT], off_blas = U[U_OFF_BLAS];
    const auto &S = h->scene, &Gm = h->geometry, &A = h->accel;
    const uint32_t *d = S.data() + off_desc + STRIDE_DESCRIPTOR * mesh;
    const uint32_t nsub = d[5], V = h->lay_mesh_nverts[mesh];
    // the mesh's blocks: each ends at the next larger start among the descriptors, or at its array's end
    size_t index0 = (size_t)off_index + d[1], index_end = off_subroot, blas0 = (size_t)off_blas + d[4], blas_end = A.size();
    for (uint32_t o = 0; o < n_mesh; ++o) {
        const uint32_t *e = S.data() + off_desc + STRIDE_DESCRIPTOR * o;
        if (o != mesh && (e[1] == d[1] || e[3] == d[3] || e[4] == d[4]))
            return fail(h, PTX_E_SCENE, "%s: mesh %u shares a block with mesh %u", what, mesh, o);
        if (e[1] > d[1]) index_end = std::min(index_end, (size_t)off_index + e[1]);
        if (e[4] > d[4]) blas_end = std::min(blas_end, (size_t)off_blas + e[4]);
    }
    if (index_end < index0 || index_end > Gm.size() || blas_end < blas0 || blas_end > A.size() ||
        (size_t)off_subroot + d[3] + nsub > Gm.size() || h->d_geometry.bytes < Gm.size() * 4u)
        return fail(h, PTX_E_SCENE, "%s: mesh %u's blocks lie past the arrays", what, mesh);
    const size_t T64 = (index_end - index0) / 3u;
    if (T64 == 0u || T64 > LEAF_FIRST_MASK + 1u || nsub == 0u)
        return fail(h, PTX_E_SCENE, "%s: mesh %u has %zu triangles in %u sub-meshes", what, mesh, T64, nsub);
    const uint32_t T = (uint32_t)T64;
    // the groups: per root the range of the leaves reachable from it (scene/world.py mesh_groups)
    std::vector<uint32_t> groups(2u * (size_t)nsub);
    uint64_t worst = 0, end_before = 0;
    for (uint32_t s = 0; s < nsub; ++s) {
        const size_t base = blas0 + Gm[(size_t)off_subroot + d[3] + s];
        uint64_t first = ~0ull, end = 0, sum = 0;
        bool empty_leaf = false;
        std::vector<uint32_t> st{0u};
        size_t visited = 0;
        while (!st.empty()) {
            const uint32_t n = st.back();
            st.pop_back();
            const size_t w = base + 8u * (size_t)n;
            if (w + 8u > blas_end || ++visited > (blas_end - blas0) / 8u)
                return fail(h, PTX_E_SCENE, "%s: mesh %u, root %u: node %u lies outside the mesh's block", what, mesh, s, n);
            if (A[w + 7] & 0xffff0000u) {
                const uint64_t lf = A[w + 6], lc = A[w + 7] & 0xffffu;
                first = std::min(first, lf);
                end = std::max(end, lf + lc);
                sum += lc;
                empty_leaf = empty_leaf || lc == 0u;
                continue;
            }
            st.push_back(A[w + 6] / 8u);
            st.push_back(n + 1u);
        }
        if (first < end_before || end > T || first >= end)
            return fail(h, PTX_E_SCENE, "%s: mesh %u, root %u covers triangles [%llu, %llu) of %u, the root before it ends at %llu", what,
                        mesh, s, (unsigned long long)first, (unsigned long long)end, T, (unsigned long long)end_before);
        if (sum != end - first || empty_leaf)
            return fail(h, PTX_E_SCENE, "%s: mesh %u, root %u: its leaves hold %llu triangles of [%llu, %llu)", what, mesh, s,
                        (unsigned long long)sum, (unsigned long long)first, (unsigned long long)end);
        groups[2u * s] = (uint32_t)first;
        groups[2u * s + 1u] = (uint32_t)(end - first);
        end_before = end;
        worst += 2u * (end - first) - 1u;
    }
    for (size_t i = 0; i < 3u * (size_t)T; ++i)
        if (Gm[index0 + i] >= V)
            return fail(h, PTX_E_SCENE, "%s: mesh %u, triangle %zu: index %u of %u vertices", what, mesh, i / 3u, Gm[index0 + i], V);
    // the positions as the host's copy holds them (it is the device's: sync_host_mirror above).  The vertex calls
    // keep them finite; an uploaded array is not looked at until here, and the builders' kernels assume it
    const size_t vertex0 = h->lay_mesh_vertex[mesh];
    if (vertex0 + (size_t)STRIDE_VERTEX * V > Gm.size())
        return fail(h, PTX_E_SCENE, "%s: mesh %u's vertex block lies past the geometry array", what, mesh);
    uint32_t bad_v, bad_k;
    if (!positions_finite(Gm.data() + vertex0, V, bad_v, bad_k))
        return fail(h, PTX_E_SCENE, "%s: mesh %u, vertex %u: position word %u is not finite", what, mesh, bad_v, bad_k);
    // the build, on the handle's stream: nothing a frame reads is written
    ptx_blas_desc bd{};
    bd.n_vertices = V;
    bd.n_tris = T;
    bd.groups = groups.data();
    bd.n_groups = nsub;
    bd.max_leaf = max_leaf;
    bd.reserved[0] = builder;
    const hipStream_t stream = h->cur().stream;
    const uint32_t *dG = (const uint32_t *)h->d_geometry.p;
    const uint32_t vertex_word = h->lay_mesh_vertex[mesh];
    const BlasFill fill = [&](float *pos, uint32_t *idx) {
        hipError_t e = slot_timed(h, PTX_STAT_BUILD, stream, hipSuccess,
                                  [&] { return launch_build_positions(dG, vertex_word, V, pos, stream); });
        if (e == hipSuccess) e = hipMemcpyAsync(idx, dG + index0, 12u * (size_t)T, hipMemcpyDeviceToDevice, stream);
        return e;
    };
    std::vector<uint32_t> nodes(8u * (size_t)worst), new_idx(3u * (size_t)T), gsize(nsub);
    uint32_t depth = 0;
    if (int rc = build_blas_core(h, what, &bd, fill, worst, nodes.data(), new_idx.data(), gsize.data(), &depth)) return rc;
    // the tree against what build_layout can hold
    uint64_t total = 0;
    for (const uint32_t g : gsize) total += g;
    if (total == 0u || total > worst) return fail(h, PTX_E_HIP, "%s: the builder returned %llu nodes", what, (unsigned long long)total);
    nodes.resize(8u * (size_t)total);
    for (size_t n = 0; n < total; ++n) {
        const uint32_t w7 = nodes[8u * n + 7u];
        if ((w7 & 0xffff0000u) && (w7 & 0xffffu) > 127u)
            return fail(h, PTX_E_SCENE, "%s: mesh %u: a leaf of %u triangles (no split exists); the layout's packed reference holds 127",
                        what, mesh, w7 & 0xffffu);
    }
    if (((size_t)depth + 2u) * kBlock * 4u > 160u * 1024u)
        return fail(h, PTX_E_SCENE, "%s: BLAS depth %u needs more LDS than a CU has", what, depth);
    const int64_t delta = (int64_t)nodes.size() - (int64_t)(blas_end - blas0);
    if ((uint64_t)((int64_t)A.size() + delta) > 0xffffffffull) return fail(h, PTX_E_SCENE, "%s: accel array too long", what);
    // From here on the handle changes: a HIP error part-way leaves it between the two trees (scene_lost).
    {
        std::vector<uint32_t> accel;
        accel.reserve((size_t)((int64_t)A.size() + delta));
        accel.insert(accel.end(), A.begin(), A.begin() + (ptrdiff_t)blas0);
        accel.insert(accel.end(), nodes.begin(), nodes.end());
        accel.insert(accel.end(), A.begin() + (ptrdiff_t)blas_end, A.end());
        h->accel = std::move(accel);
    }
    uint32_t scene_words = 0;
    if (delta != 0)
        for (uint32_t o = 0; o < n_mesh; ++o) {
            uint32_t *e = h->scene.data() + off_desc + STRIDE_DESCRIPTOR * o;
            if (e[4] > d[4]) {
                e[4] = (uint32_t)((int64_t)e[4] + delta);
                scene_words += 1u;
            }
        }
    std::memcpy(h->geometry.data() + index0, new_idx.data(), 12u * (size_t)T);
    {
        uint32_t at = 0;
        for (uint32_t s = 0; s < nsub; ++s) {
            h->geometry[(size_t)off_subroot + d[3] + s] = at;
            at += 8u * gsize[s];
        }
    }
    hipError_t le = hipSuccess;
    if (scene_words)
        le = copy_sync(h, (uint32_t *)h->d_scene.p + off_desc, h->scene.data() + off_desc, (size_t)STRIDE_DESCRIPTOR * n_mesh * 4u,
                       hipMemcpyHostToDevice);
    if (le == hipSuccess)
        le = copy_sync(h, (uint32_t *)h->d_geometry.p + index0, h->geometry.data() + index0, 12u * (size_t)T, hipMemcpyHostToDevice);
    if (le == hipSuccess)
        le = copy_sync(h, (uint32_t *)h->d_geometry.p + off_subroot + d[3], h->geometry.data() + off_subroot + d[3], 4u * (size_t)nsub,
                       hipMemcpyHostToDevice);
    int rc = le == hipSuccess ? PTX_OK : fail(h, PTX_E_HIP, "%s: %s", what, hipGetErrorString(le));
    if (rc == PTX_OK) rc = build_layout(h);
    if (rc != PTX_OK) {
        scene_lost(h);
        return rc;
    }
    // kept: the vertex records, the skins, the accumulation, the denoiser's history (keyed by instance and
    // sub-mesh; build_layout bumped layout_gen, so a snapshot in the old triangle numbering is not read).
    // dropped: what build_layout drops (G-buffers, surface records), the neighbour summaries and init state, and
    // the reuse / GI history outright, as for a switched mesh: its reservoirs name triangle numbers of the
    // index buffer that was just reordered
    frames_outdated(h);
    history_after_edit(h, /*numbering_kept=*/false);
    upsampler_after_edit(h);
    if (info_out) {
        std::memset(info_out, 0, sizeof *info_out);
        info_out->n_accel = (uint32_t)h->accel.size();
        info_out->mesh_nodes = (uint32_t)total;
        info_out->max_depth = depth;
        info_out->scene_words = scene_words;
    }
    return PTX_OK;
}

int ptx_scene_sizes(ptx_handle *h, size_t *n_scene, size_t *n_geometry, size_t *n_accel) {
    if (!h) return PTX_E_INVALID;
    if (!h->scene_loaded) return fail(h, PTX_E_INVALID, "ptx_scene_sizes: upload a scene first");
    if (n_scene) *n_scene = h->scene.size();
    if (n_geometry) *n_geometry = h->geometry.size();
    if (n_accel) *n_accel = h->accel.size();
    return PTX_OK;
}

int ptx_read_scene(ptx_handle *h, uint32_t *scene_out, size_t n_scene, uint32_t *geometry_out, size_t n_geometry,
                   uint32_t *accel_out, size_t n_accel) {
    if (!h) return PTX_E_INVALID;
    const char *what = "ptx_read_scene";
    if (int rc = layout_check(h, what)) return rc;
    const bool skip_s = !scene_out && !n_scene, skip_g = !geometry_out && !n_geometry, skip_a = !accel_out && !n_accel;
    if ((!skip_s && (!scene_out || n_scene != h->scene.size())) || (!skip_g && (!geometry_out || n_geometry != h->geometry.size())) ||
        (!skip_a && (!accel_out || n_accel != h->accel.size())))
        return fail(h, PTX_E_INVALID, "%s: (%zu, %zu, %zu) words, the handle's arrays have (%zu, %zu, %zu)", what, n_scene, n_geometry,
                    n_accel, h->scene.size(), h->geometry.size(), h->accel.size());
    HIP_CHECK(h, hipSetDevice(h->device));
    if (int rc = quiesce(h)) return rc;
    if (!skip_s) std::memcpy(scene_out, h->scene.data(), n_scene * 4u);
    if (!skip_g) {
        std::memcpy(geometry_out, h->geometry.data(), n_geometry * 4u);
        for (size_t m = 0; m < h->mesh_stale.size() && m < h->lay_mesh_vertex.size(); ++m) {  // the posed vertex blocks
            if (!(h->mesh_stale[m] & kStaleGeometry)) continue;
            const size_t w0 = h->lay_mesh_vertex[m], n = (size_t)STRIDE_VERTEX * h->lay_mesh_nverts[m];
            if (!n || w0 + n > n_geometry || h->d_geometry.bytes < (w0 + n) * 4u) continue;
            if (int rc = read_to_host(h, geometry_out + w0, (const uint32_t *)h->d_geometry.p + w0, n * 4u)) return rc;
        }
    }
    if (!skip_a) {
        std::memcpy(accel_out, h->accel.data(), n_accel * 4u);
        if (int rc = device_boxes_into(h, accel_out)) return rc;
    }
    return PTX_OK;
}

int ptx_blas_cost(ptx_handle *h, uint32_t mesh, double *cost_out) {
    if (!h) return PTX_E_INVALID;
    const char *what = "ptx_blas_cost";
    if (int rc = vertex_range_check(h, what, mesh, 0u, 0u)) return rc;
    if (!cost_out) return fail(h, PTX_E_INVALID, "%s: null cost_out", what);
    HIP_CHECK(h, hipSetDevice(h->device));
    if (int rc = quiesce(h)) return rc;
    CostArgs a{};
    a.nodes = (const NodePair *)h->d_nodes.p;
    a.subs = (const SubRoot *)h->d_subs.p;
    a.pair_sub = (const uint32_t *)h->d_pair_sub.p;
    a.pair_base = h->lay_mesh_node_base[mesh];
    a.n_pairs = h->lay_mesh_nnodes[mesh];
    a.sub_base = h->lay_mesh_sub_base[mesh];
    a.n_subs = h->lay_mesh_nsub[mesh];
    const uint32_t blocks = cost_blocks(a.n_pairs, a.n_subs);
    *cost_out = 0.0;
    if (blocks == 0u) return PTX_OK;
    const size_t pair_end = (size_t)a.pair_base + a.n_pairs;
    if ((a.n_pairs && (pair_end * sizeof(NodePair) > h->d_nodes.bytes || pair_end * 4u > h->d_pair_sub.bytes)) ||
        ((size_t)a.sub_base + a.n_subs) * sizeof(SubRoot) > h->d_subs.bytes)
        return fail(h, PTX_E_INVALID, "%s: the mesh's tables lie past the layout", what);
    DevBuf partial;
    if (int rc = alloc_buf(h, partial, (size_t)blocks * sizeof(double))) return rc;
    a.partial = (double *)partial.p;
    const hipStream_t st = h->cur().stream;
    const hipError_t le = slot_timed(h, PTX_STAT_BUILD, st, hipSuccess, [&] { return launch_blas_cost(a, st); });
    std::vector<double> sums(blocks);
    int rc = le == hipSuccess ? PTX_OK : fail(h, PTX_E_HIP, "%s: %s", what, hipGetErrorString(le));
    if (rc == PTX_OK) rc = read_to_host(h, sums.data(), partial.p, (size_t)blocks * sizeof(double));
    free_buf(partial);
    if (rc != PTX_OK) return rc;
    double total = 0.0;
    for (const double s : sums) total += s;  // in index order
    *cost_out = total;
    return PTX_OK;
}

int ptx_read_vertices(ptx_handle *h, uint32_t mesh, uint32_t first_vertex, uint32_t n_vertices, uint32_t *records_out) {
    if (!h) return PTX_E_INVALID;
    if (int rc = vertex_range_check(h, "ptx_read_vertices", mesh, first_vertex, n_vertices)) return rc;
    if (n_vertices == 0u) return PTX_OK;
    if (!records_out) return fail(h, PTX_E_INVALID, "ptx_read_vertices: null array");
    HIP_CHECK(h, hipSetDevice(h->device));
    if (int rc = quiesce(h)) return rc;
    const size_t word0 = (size_t)h->lay_mesh_vertex[mesh] + (size_t)STRIDE_VERTEX * first_vertex;
    return read_to_host(h, records_out, (const uint32_t *)h->d_geometry.p + word0, (size_t)STRIDE_VERTEX * n_vertices * 4u);
}

}  // extern "C"
