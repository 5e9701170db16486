// ptx_denoise.hip -- edge-avoiding a-trous wavelet filter of the accumulated image (ptx_denoise,
// DESIGN.md §Denoiser): guided by the primary hit of the frame context's G-buffer, variance
// estimated spatially from the image; in temporal mode the image is the frame colours integrated
// over the calls, looked up through the previous call's camera (tests/denoise_temporal_ref.py).
// All kernels one lane per pixel; the only atomics are dn_temporal's and dn_upsample_temporal_win's
// counts of clipped pixels, one add per wave that has any:
//   dn_guide     G-buffer texel -> 32-byte guide record {P.xyz, key | kDnMiss}{N.xyz, r}
//   dn_temporal  (temporal mode) history lookup + integration -> history {C.rgb, n}, moments {m1, m2};
//                dn_temporal_verts: the same for a call that follows deformed meshes (tests/denoise_follow_ref.py)
//   dn_variance  7x7 guide-weighted luminance moments -> working image {r, g, b, v}; <true>: on the
//                history, the integrated moments' variance where n >= 4
//   dn_atrous    one iteration at step 2^i on the working image (ping-pong); steps 1, 2, 4 stage
//                the 16x16 tile and its apron in LDS, steps >= 8 gather their taps directly
//   dn_upsample  (ptx_upsample) a denoised image of 1/S the size, written at full size under the
//                full-size guide records; the tile's footprint in the small image staged in LDS;
//                dn_upsample_win (ptx_upsample_bands): a band of it from a window of the small image
//   dn_upsample_temporal  (ptx_upsample_temporal) the same inputs, the small image rendered through one
//                phase of the S x S block: the own sample and the interpolated estimate integrated with
//                the previous call's history {H.rgb, n}, gathered like dn_temporal's
//                dn_upsample_temporal_win (ptx_upsample_temporal_bands): a band of it from a window of the small
//                image and the rows of the previous state the band holds
// Every kernel but dn_guide addresses a row window (DnWin): a W x rows image that is the whole
// frame, or a band with the halo rows ptx_denoise_bands brought from its neighbours, filtered as if
// it were the whole image; a launch computes rows [c0, c1) of it.
// Arithmetic is the definition's, operation by operation (tests/denoise_ref.py restates it in
// numpy and the outputs are compared bit for bit): f32, no contraction, sums in tap order, a
// skipped tap leaves every sum untouched.
#include "ptx_wave_common.h"

namespace ptx {

constexpr uint32_t kDnMiss = 0xFFFFFFFFu;  // guide key word of a pixel without a primary hit (a key has bit 31 clear)
constexpr int kDnTile = 16;                // a workgroup's pixels: 16 x 16, thread t -> (t & 15, t >> 4)
static_assert(kDnTile * kDnTile == kBlock, "one lane per pixel of the tile");

// ---------------------------------------------------------------- guide records
__device__ __forceinline__ void dn_guide_px(const Scene &sc, uint4 g, float4 *__restrict__ guide, size_t pix,
                                            float sigma_plane) {
    if (!(g.x & 0x80000000u)) {
        guide[2u * pix] = make_float4(0.0f, 0.0f, 0.0f, asf(kDnMiss));
        guide[2u * pix + 1u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const Surface X = get_surface(sc, gdecode(g));
    const f3 cam = mk(asf(sc.U[U_CAMPOS]), asf(sc.U[U_CAMPOS + 1]), asf(sc.U[U_CAMPOS + 2]));
    const float r = sigma_plane * length(X.pos - cam);
    guide[2u * pix] = make_float4(X.pos.x, X.pos.y, X.pos.z, asf(g.x & 0x7fffffffu));
    guide[2u * pix + 1u] = make_float4(X.nrm.x, X.nrm.y, X.nrm.z, r);
}
// The band's own rows, read through the Scene's tiling: `gbuf` and `guide` start at the band's first row.
__global__ __launch_bounds__(kBlock) void dn_guide(const Scene sc, const uint4 *__restrict__ gbuf,
                                                   float4 *__restrict__ guide, float sigma_plane) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    uint32_t x, y;
    if (p >= padded_pixels(sc) || !tile_xy(sc, p, x, y)) return;
    const size_t pix = (size_t)(y - sc.row_begin) * sc.width + x;
    dn_guide_px(sc, gbuf[pix], guide, pix, sigma_plane);
}
// A window's halo rows, from the neighbours' texels: `texels` holds the `top` rows above the band,
// then the rows below it; texel row r is window row r (r < top) or r + skip (skip = the band's rows).
__global__ __launch_bounds__(kBlock) void dn_guide_halo(const Scene sc, const uint4 *__restrict__ texels, uint32_t rows,
                                                        uint32_t top, uint32_t skip, float4 *__restrict__ guide,
                                                        float sigma_plane) {
    const uint32_t x = blockIdx.x * kDnTile + (threadIdx.x & 15u), r = blockIdx.y * kDnTile + (threadIdx.x >> 4);
    if (x >= sc.width || r >= rows) return;
    const uint32_t y = r < top ? r : r + skip;
    dn_guide_px(sc, texels[(size_t)r * sc.width + x], guide, (size_t)y * sc.width + x, sigma_plane);
}

// ---------------------------------------------------------------- row window
// (DnWin and DnImage: ptx_launch.h)  A window's pixel (x, y) is element y * W + x of every buffer a
// kernel is given; rows outside [0, rows) are outside the image: never a tap.
// The pixel of a filter input whose own rows and halo rows lie in two buffers.
__device__ __forceinline__ float4 dn_load(const DnImage &I, uint32_t W, uint32_t x, uint32_t y) {
    if (y >= I.o0 && y < I.o1) return I.own[(size_t)(y - I.o0) * W + x];
    return I.halo[(size_t)(y < I.o0 ? y : y - (I.o1 - I.o0)) * W + x];
}

// ---------------------------------------------------------------- shared arithmetic
// Guide weight of a tap with the centre's key (the caller skips every other tap).
__device__ __forceinline__ float dn_gamma(f3 Pp, f3 Np, float rp, f3 Pq, f3 Nq) {
    float wn = fmaxf(0.0f, dot(Np, Nq));
#pragma unroll
    for (int k = 0; k < 7; ++k) wn = wn * wn;
    const float wd = fmaxf(0.0f, 1.0f - __builtin_fabsf(dot(Np, Pq - Pp)) / rp);
    return wn * wd;
}
__device__ __forceinline__ f3 rgb(float4 c) { return mk(c.x, c.y, c.z); }

// A tile's staging area: the 16x16 pixels and an apron of A pixels on every side.
template <int A>
struct DnTile {
    static constexpr int N = kDnTile + 2 * A, E = N * N;
    // entry of pixel (tx + dx, ty + dy) of the tile (|dx|, |dy| <= A)
    static __device__ __forceinline__ int at(int tx, int ty, int dx, int dy) { return (ty + A + dy) * N + (tx + A + dx); }
};
// Fill the staging area from global memory; pixels outside the window become misses (never a tap).
// img(x, y): the input's pixel.
template <int A, bool WITH_CV, bool WITH_LUM, class Img>
__device__ __forceinline__ void dn_stage(uint32_t W, const DnWin &win, const float4 *__restrict__ guide, Img img,
                                         float4 *g0, float4 *g1, float4 *cv, float *lum) {
    using T = DnTile<A>;
    const int x0 = (int)blockIdx.x * kDnTile - A, y0 = (int)(win.c0 + blockIdx.y * kDnTile) - A;
    for (int e = (int)threadIdx.x; e < T::E; e += kBlock) {
        const int gx = x0 + e % T::N, gy = y0 + e / T::N;
        float4 a = make_float4(0.0f, 0.0f, 0.0f, asf(kDnMiss)), b = make_float4(0.0f, 0.0f, 0.0f, 0.0f), c = b;
        if (gx >= 0 && gy >= 0 && gx < (int)W && gy < (int)win.rows) {
            const size_t q = (size_t)gy * W + (size_t)gx;
            a = guide[2u * q];
            b = guide[2u * q + 1u];
            c = img((uint32_t)gx, (uint32_t)gy);
        }
        g0[e] = a;
        g1[e] = b;
        if (WITH_CV) cv[e] = c;
        if (WITH_LUM) lum[e] = luminance(rgb(c));
    }
    __syncthreads();
}

// ---------------------------------------------------------------- temporal integration
// The previous temporal call as dn_temporal sees it.  mode: 0 no history (the first call, or after a
// reset), 1 the camera words are that call's (the history of pixel p is at p), 2 reproject through vp.
struct DnHistory {
    float vp[16];  // that call's VP (mat4_inverse of its uniform words 4..19)
    float alpha_min;
    uint32_t mode;
    // the rows of the frame that call's state covers (a band: its window then), [y0, y0 + rows):
    // pguide, phist and pmom start at row y0
    uint32_t y0, rows;
};
constexpr float kDnNMax = 255.0f;    // the history length saturates here
constexpr float kDnNMoments = 4.0f;  // from this length on the variance comes from the integrated moments

// inst_point / inst_point_t for a kept instance record (DnPrev::mesh carries kInstIdentity as Inst::mesh does).
__device__ __forceinline__ f3 dn_prev_point(bool identity, const float *m, f3 p) {
    if (identity && finite3(p)) return f3{p.x + 0.0f, p.y + 0.0f, p.z + 0.0f};
    return xform_point(m, p);
}
__device__ __forceinline__ f3 dn_prev_point_t(bool identity, const float *m, f3 p) {
    if (identity && finite3(p)) return f3{p.x + 0.0f, p.y + 0.0f, p.z + 0.0f};
    return xform_point_t(m, p);
}

// History lookup and integration of one pixel: reads this frame's guide record and colour and up to
// four previous guide / history / moment records, writes the new history {C.rgb, n} and moments
// {m1, m2}.  Pixels are projected in the W x H frame's coordinates (the window's row 0 is its row
// win.y0); `frame` and `accum` start at row c0 of the window (the band's own rows: what a launch
// computes).  A candidate inside the frame but outside the rows the previous state covers is not
// taken (as if n' = 0 there), and a pixel with such a candidate counts in *clip.
// The four taps' records are gathered directly, all issued ahead of the tests: under
// camera motion a tile's footprint in the previous frame is a shifted, nearly rigid tile, so
// neighbouring lanes' taps share cache lines, but its extent is not bounded.
// OBJ (a call that finds an instance changed since the previous one: denoise_front's table, one DnObj
// per instance, a hit pixel's is obj[key >> 16]; past n_obj: flag 0): flag 0 as without the table;
// flag 2 no lookup (n = 1); flag 1 the instance moved rigidly -- the hit point and normal go through
// D = M_prev * Minv_cur to where they were at the previous call, Q and Nq (not renormalised), Q is
// always reprojected through vp, the same camera or not, and the taps are tested against Q and Nq.
// VERTS (a call that finds a mesh deformed since the previous one, "Vertex motion"): flag 3 -- Q and Nq are
// get_surface's position and normalised normal of the pixel's G-buffer texel `g` (gbuf starts at row c0 of
// the window, like frame) on the previous call's geometry: the triangle record saved before the refit
// (snap: Scene::tverts' layout and indices) under that call's instance matrices (prev[inst]); then as flag 1.
template <bool OBJ, bool VERTS>
__device__ __forceinline__ void dn_temporal_px(uint32_t W, uint32_t H, const DnWin &win, const DnHistory &Hs,
                                               const float4 *__restrict__ guide, const float4 *__restrict__ frame,
                                               const float4 *__restrict__ accum, const float4 *__restrict__ pguide,
                                               const float4 *__restrict__ phist, const float2 *__restrict__ pmom,
                                               float4 *__restrict__ hist, float2 *__restrict__ mom,
                                               unsigned long long *__restrict__ clip,
                                               const DnObj *__restrict__ obj, uint32_t n_obj,
                                               const uint4 *__restrict__ gbuf, const DnPrev *__restrict__ prev,
                                               const float4 *__restrict__ snap) {
    const uint32_t x = blockIdx.x * kDnTile + (threadIdx.x & 15u), y = win.c0 + blockIdx.y * kDnTile + (threadIdx.x >> 4);
    if (x >= W || y >= win.c1) return;
    const size_t pix = (size_t)y * W + x, own = (size_t)(y - win.c0) * W + x;
    const float4 a = guide[2u * pix];
    const uint32_t key = asu(a.w);
    if (key == kDnMiss) {  // no primary hit: the accumulated colour, never a tap (n = 0)
        const float4 c = accum[own];
        hist[pix] = make_float4(c.x, c.y, c.z, 0.0f);
        mom[pix] = make_float2(0.0f, 0.0f);
        return;
    }
    const float4 b = guide[2u * pix + 1u];
    uint4 g = make_uint4(0u, 0u, 0u, 0u);
    if (VERTS) g = gbuf[own];  // (issued with the guide and colour loads: the snapshot record's address hangs on it)
    const f3 F = rgb(frame[own]), Pp = rgb(a), Np = rgb(b);
    const float l = luminance(F);
    f3 C = F;
    float m1 = l, m2 = l * l, n = 1.0f;
    uint32_t flag = 0u;
    f3 Q = Pp, Nq = Np;  // the point and normal the previous call saw
    if (OBJ) {
        const uint32_t inst = key >> 16;
        if (Hs.mode != 0u && inst < n_obj) flag = obj[inst].flag;
        if (VERTS && flag == 3u) {
            const DnPrev &I = prev[inst];
            const float4 *q = snap + 5u * (size_t)(I.tri_base + g.y);
            const float4 ta = q[0], tb = q[1], tc = q[2], td = q[3], te = q[4];  // (tri_verts' record)
            const bool id = (I.mesh & kInstIdentity) != 0u;
            const f3 p0 = dn_prev_point(id, I.m, mk(ta.x, ta.y, ta.z)), n0 = dn_prev_point_t(id, I.minv, mk(ta.w, tb.x, tb.y));
            const f3 p1 = dn_prev_point(id, I.m, mk(tb.z, tb.w, tc.x)), n1 = dn_prev_point_t(id, I.minv, mk(tc.y, tc.z, tc.w));
            const f3 p2 = dn_prev_point(id, I.m, mk(td.x, td.y, td.z)), n2 = dn_prev_point_t(id, I.minv, mk(td.w, te.x, te.y));
            const float bu = asf(g.z), bv = asf(g.w), bw = 1.0f - bu - bv;
            Nq = normalize((n0 * bu + n1 * bv) + n2 * bw);
            Q = (p0 * bu + p1 * bv) + p2 * bw;
        }
        if (flag == 1u) {
            const float *d = obj[inst].d;
            Q.x = ((d[0] * Pp.x + d[4] * Pp.y) + d[8] * Pp.z) + d[12];
            Q.y = ((d[1] * Pp.x + d[5] * Pp.y) + d[9] * Pp.z) + d[13];
            Q.z = ((d[2] * Pp.x + d[6] * Pp.y) + d[10] * Pp.z) + d[14];
            Nq.x = (d[0] * Np.x + d[4] * Np.y) + d[8] * Np.z;
            Nq.y = (d[1] * Np.x + d[5] * Np.y) + d[9] * Np.z;
            Nq.z = (d[2] * Np.x + d[6] * Np.y) + d[10] * Np.z;
        }
    }
    if (Hs.mode != 0u && !(OBJ && flag == 2u)) {
        // candidate taps k = 2 j + i (j outer): pixel, bilinear weight, inside the image
        size_t q[4];
        float w[4];
        bool in[4], clipped = false;
        // this pixel in the previous state (a band's own rows are always covered)
        const size_t pc = (size_t)(win.y0 + y - Hs.y0) * W + x;
        if (Hs.mode == 1u && !(OBJ && flag == 1u) && !(VERTS && flag == 3u)) {
#pragma unroll
            for (int k = 0; k < 4; ++k) { q[k] = pc; w[k] = 1.0f; in[k] = k == 0; }
        } else {
            const float *vp = Hs.vp;
            const float cx = ((vp[0] * Q.x + vp[4] * Q.y) + vp[8] * Q.z) + vp[12];
            const float cy = ((vp[1] * Q.x + vp[5] * Q.y) + vp[9] * Q.z) + vp[13];
            const float cw = ((vp[3] * Q.x + vp[7] * Q.y) + vp[11] * Q.z) + vp[15];
            const float fx = ((cx / cw + 1.0f) * 0.5f) * (float)W - 0.5f, fy = ((cy / cw + 1.0f) * 0.5f) * (float)H - 0.5f;
            const float x0 = __builtin_floorf(fx), y0 = __builtin_floorf(fy);
            const float ax = fx - x0, ay = fy - y0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = k & 1, j = k >> 1;
                const float qx = x0 + (float)i, qy = y0 + (float)j;
                // (a NaN or infinite projection compares false: outside)
                in[k] = cw > 0.0f && qx >= 0.0f && qx < (float)W && qy >= 0.0f && qy < (float)H;
                const uint32_t ry = (uint32_t)(in[k] ? (int)qy : (int)Hs.y0) - Hs.y0;  // (below y0: wraps past rows)
                if (in[k] && ry >= Hs.rows) {
                    clipped = true;
                    in[k] = false;
                }
                q[k] = in[k] ? (size_t)ry * W + (size_t)(int)qx : pc;  // (an outside tap loads the centre, unused)
                w[k] = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
            }
            const unsigned long long cm = __ballot(clipped);  // (over the wave's lanes that look a history up)
            if (clipped && __lane_id() == (uint32_t)__ffsll((long long)cm) - 1u) atomicAdd(clip, (unsigned long long)__popcll(cm));
        }
        float4 qa[4], qb[4], qh[4];
        float2 qm[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            qa[k] = pguide[2u * q[k]];
            qb[k] = pguide[2u * q[k] + 1u];
            qh[k] = phist[q[k]];
            qm[k] = pmom[q[k]];
        }
        float sw = 0.0f, s1 = 0.0f, s2 = 0.0f, nh = __builtin_inff();
        f3 sC = mk(0.0f, 0.0f, 0.0f);
        bool any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!in[k] || asu(qa[k].w) != key || !(qh[k].w >= 1.0f)) continue;
            if (!(dot(Nq, rgb(qb[k])) >= 0.9f)) continue;
            if (!(__builtin_fabsf(dot(Nq, rgb(qa[k]) - Q)) <= b.w)) continue;
            sw += w[k];
            sC = sC + rgb(qh[k]) * w[k];
            s1 += w[k] * qm[k].x;
            s2 += w[k] * qm[k].y;
            nh = fminf(nh, qh[k].w);
            any = true;
        }
        if (any && sw > 0.0f) {
            n = fminf(nh + 1.0f, kDnNMax);
            const float al = fmaxf(1.0f / n, Hs.alpha_min);
            C = mix3(sC / sw, F, al);
            m1 = mixf(s1 / sw, l, al);
            m2 = mixf(s2 / sw, l * l, al);
        }
    }
    hist[pix] = make_float4(C.x, C.y, C.z, n);
    mom[pix] = make_float2(m1, m2);
}
template <bool OBJ>
__global__ __launch_bounds__(kBlock) void dn_temporal(uint32_t W, uint32_t H, const DnWin win, const DnHistory Hs,
                                                      const float4 *__restrict__ guide, const float4 *__restrict__ frame,
                                                      const float4 *__restrict__ accum, const float4 *__restrict__ pguide,
                                                      const float4 *__restrict__ phist, const float2 *__restrict__ pmom,
                                                      float4 *__restrict__ hist, float2 *__restrict__ mom,
                                                      unsigned long long *__restrict__ clip,
                                                      const DnObj *__restrict__ obj, uint32_t n_obj) {
    dn_temporal_px<OBJ, false>(W, H, win, Hs, guide, frame, accum, pguide, phist, pmom, hist, mom, clip, obj, n_obj, nullptr,
                               nullptr, nullptr);
}
// The instance that follows vertices: also the pixel's G-buffer texel (16 B) and, on a flag-3 pixel, the
// previous call's instance record (DnPrev) and the 80-byte snapshot record.
__global__ __launch_bounds__(kBlock) void dn_temporal_verts(uint32_t W, uint32_t H, const DnWin win, const DnHistory Hs,
                                                            const float4 *__restrict__ guide, const float4 *__restrict__ frame,
                                                            const float4 *__restrict__ accum, const float4 *__restrict__ pguide,
                                                            const float4 *__restrict__ phist, const float2 *__restrict__ pmom,
                                                            float4 *__restrict__ hist, float2 *__restrict__ mom,
                                                            unsigned long long *__restrict__ clip,
                                                            const DnObj *__restrict__ obj, uint32_t n_obj,
                                                            const uint4 *__restrict__ gbuf, const DnPrev *__restrict__ prev,
                                                            const float4 *__restrict__ snap) {
    dn_temporal_px<true, true>(W, H, win, Hs, guide, frame, accum, pguide, phist, pmom, hist, mom, clip, obj, n_obj, gbuf, prev,
                               snap);
}

// ---------------------------------------------------------------- variance pass
// The 7x7 guide-weighted luminance moments of a hit pixel of the staged tile.
__device__ __forceinline__ float dn_var7(const float4 *g0, const float4 *g1, const float *lum, int tx, int ty, float4 a,
                                         float4 b) {
    using T = DnTile<3>;
    const uint32_t key = asu(a.w);
    const f3 Pp = rgb(a), Np = rgb(b);
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int dy = -3; dy <= 3; ++dy) {
#pragma unroll
        for (int dx = -3; dx <= 3; ++dx) {
            const int e = T::at(tx, ty, dx, dy);
            const float4 qa = g0[e];
            if (asu(qa.w) != key) continue;
            const float gm = dn_gamma(Pp, Np, b.w, rgb(qa), rgb(g1[e]));
            const float lq = lum[e];
            s0 += gm;
            s1 += gm * lq;
            s2 += gm * (lq * lq);
        }
    }
    const float m = s1 / s0;
    return fmaxf(0.0f, s2 / s0 - m * m);
}
// MOMENTS (temporal mode): `img` is the new history {C.rgb, n}; where n >= kDnNMoments the variance
// is the integrated moments', and the 7x7 sums run only elsewhere.
// The input is a DnImage: the accumulation's halo rows lie in a buffer of their own (the history is
// one buffer: o0 = 0, o1 = rows).
template <bool MOMENTS>
__global__ __launch_bounds__(kBlock) void dn_variance(uint32_t W, const DnWin win, const DnImage img,
                                                      const float2 *__restrict__ mom, const float4 *__restrict__ guide,
                                                      float4 *__restrict__ out) {
    using T = DnTile<3>;
    __shared__ float4 g0[T::E], g1[T::E];
    __shared__ float lum[T::E];
    dn_stage<3, false, true>(W, win, guide, [&](uint32_t qx, uint32_t qy) { return dn_load(img, W, qx, qy); }, g0, g1,
                             nullptr, lum);
    const int tx = (int)(threadIdx.x & 15u), ty = (int)(threadIdx.x >> 4);
    const uint32_t x = blockIdx.x * kDnTile + (uint32_t)tx, y = win.c0 + blockIdx.y * kDnTile + (uint32_t)ty;
    if (x >= W || y >= win.c1) return;
    const size_t pix = (size_t)y * W + x;
    const float4 c = dn_load(img, W, x, y);
    const float4 a = g0[T::at(tx, ty, 0, 0)], b = g1[T::at(tx, ty, 0, 0)];
    float v = 0.0f;
    if (asu(a.w) != kDnMiss) {
        if (MOMENTS && c.w >= kDnNMoments) {
            const float2 m = mom[pix];
            v = fmaxf(0.0f, m.y - m.x * m.x);
        } else {
            v = dn_var7(g0, g1, lum, tx, ty, a, b);
        }
    }
    out[pix] = make_float4(c.x, c.y, c.z, v);
}

// ---------------------------------------------------------------- a-trous iteration
struct DnSums { float sw; f3 sc; float sv; };
__device__ __forceinline__ void dn_tap(DnSums &S, float h, f3 Pp, f3 Np, float rp, float lp, float dp, float4 qa,
                                       float4 qb, float4 qc) {
    const float gm = dn_gamma(Pp, Np, rp, rgb(qa), rgb(qb));
    const float t = fmaxf(0.0f, 1.0f - (__builtin_fabsf(lp - luminance(rgb(qc))) / dp) / 4.0f);
    const float wl = (t * t) * (t * t);
    const float w = (h * gm) * wl;
    S.sw += w;
    S.sc = S.sc + rgb(qc) * w;
    S.sv += (w * w) * qc.w;
}
__device__ __forceinline__ float dn_b(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }
__device__ __forceinline__ float dn_w3(int d) { return d == 0 ? 0.5f : 0.25f; }

// Steps 1, 2, 4: the tile and its apron of 2 * STEP pixels in LDS (48 B per entry: 19 / 27 / 48 KiB).
template <int STEP>
__global__ __launch_bounds__(kBlock) void dn_atrous_tiled(uint32_t W, const DnWin win, const float4 *__restrict__ in,
                                                          const float4 *__restrict__ guide, float4 *__restrict__ out,
                                                          float sigma_lum, uint32_t last) {
    using T = DnTile<2 * STEP>;
    __shared__ float4 g0[T::E], g1[T::E], cv[T::E];
    dn_stage<2 * STEP, true, false>(W, win, guide, [&](uint32_t qx, uint32_t qy) { return in[(size_t)qy * W + qx]; }, g0,
                                    g1, cv, nullptr);
    const int tx = (int)(threadIdx.x & 15u), ty = (int)(threadIdx.x >> 4);
    const uint32_t x = blockIdx.x * kDnTile + (uint32_t)tx, y = win.c0 + blockIdx.y * kDnTile + (uint32_t)ty;
    if (x >= W || y >= win.c1) return;
    const int ec = T::at(tx, ty, 0, 0);
    const float4 a = g0[ec], b = g1[ec], c = cv[ec];
    const uint32_t key = asu(a.w);
    float4 o = make_float4(c.x, c.y, c.z, 0.0f);
    if (key != kDnMiss) {
        float vb = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int e = T::at(tx, ty, dx, dy);
                if (asu(g0[e].w) == key) vb += (dn_w3(dy) * dn_w3(dx)) * cv[e].w;
            }
        const float dp = sigma_lum * __builtin_sqrtf(vb) + 1e-6f;
        const float lp = luminance(rgb(c));
        const f3 Pp = rgb(a), Np = rgb(b);
        DnSums S{0.0f, mk(0.0f, 0.0f, 0.0f), 0.0f};
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int e = T::at(tx, ty, STEP * dx, STEP * dy);
                const float4 qa = g0[e];
                if (asu(qa.w) != key) continue;
                dn_tap(S, dn_b(dy) * dn_b(dx), Pp, Np, b.w, lp, dp, qa, g1[e], cv[e]);
            }
        }
        const f3 cn = S.sc / S.sw;
        o = make_float4(cn.x, cn.y, cn.z, S.sv / (S.sw * S.sw));
    }
    if (last) o.w = 1.0f;
    out[(size_t)y * W + x] = o;
}

// Steps >= 8: a pixel's taps share no cache line with its neighbours' -- gathered directly, one
// tap row's 15 loads issued together ahead of that row's weight chains.
__global__ __launch_bounds__(kBlock) void dn_atrous_gather(uint32_t W, const DnWin win, int step,
                                                           const float4 *__restrict__ in, const float4 *__restrict__ guide,
                                                           float4 *__restrict__ out, float sigma_lum, uint32_t last) {
    const int x = (int)(blockIdx.x * kDnTile + (threadIdx.x & 15u)), y = (int)(win.c0 + blockIdx.y * kDnTile + (threadIdx.x >> 4));
    const int H = (int)win.rows;
    if (x >= (int)W || y >= (int)win.c1) return;
    const size_t pix = (size_t)y * W + (size_t)x;
    const float4 a = guide[2u * pix], b = guide[2u * pix + 1u], c = in[pix];
    const uint32_t key = asu(a.w);
    float4 o = make_float4(c.x, c.y, c.z, 0.0f);
    if (key != kDnMiss) {
        float vb = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = x + dx, qy = y + dy;
                const bool inside = qx >= 0 && qy >= 0 && qx < (int)W && qy < H;
                const size_t q = inside ? (size_t)qy * W + (size_t)qx : pix;
                const uint32_t kq = asu(guide[2u * q].w);
                const float vq = in[q].w;
                if (inside && kq == key) vb += (dn_w3(dy) * dn_w3(dx)) * vq;
            }
        const float dp = sigma_lum * __builtin_sqrtf(vb) + 1e-6f;
        const float lp = luminance(rgb(c));
        const f3 Pp = rgb(a), Np = rgb(b);
        DnSums S{0.0f, mk(0.0f, 0.0f, 0.0f), 0.0f};
        for (int dy = -2; dy <= 2; ++dy) {
            const int qy = y + step * dy;
            const bool row_in = qy >= 0 && qy < H;
            float4 qa[5], qb[5], qc[5];
            bool ok[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const int qx = x + step * (k - 2);
                ok[k] = row_in && qx >= 0 && qx < (int)W;
                const size_t q = ok[k] ? (size_t)qy * W + (size_t)qx : pix;  // (an outside tap loads the centre, unused)
                qa[k] = guide[2u * q];
                qb[k] = guide[2u * q + 1u];
                qc[k] = in[q];
            }
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                if (!ok[k] || asu(qa[k].w) != key) continue;
                dn_tap(S, dn_b(dy) * dn_b(k - 2), Pp, Np, b.w, lp, dp, qa[k], qb[k], qc[k]);
            }
        }
        const f3 cn = S.sc / S.sw;
        o = make_float4(cn.x, cn.y, cn.z, S.sv / (S.sw * S.sw));
    }
    if (last) o.w = 1.0f;
    out[pix] = o;
}

// ---------------------------------------------------------------- guided upsampling (ptx_upsample)
// A w x h image `lc` with the guide records `lg` of its denoise, written at S times the size under
// the full-size guide records `hg` (Upsampling; tests/upsample_ref.py).  Pixel
// (x, y) sits at f = (x + 0.5) / S - 0.5 of the small image, x0 = floor(f): stage 1 weighs the four
// pixels (x0 + i, y0 + j) with the pixel's key bilinearly and by dn_gamma, stage 2 (no weight
// there) averages the 16 of (x0 - 1 .. x0 + 2)^2 with its key, stage 3 (none either) takes pixel
// (x / S, y / S).  A tile's x0 spans at most 16 / S + 1 columns, so every candidate of its pixels
// lies in the kUpN x kUpN window staged from (x0 - 1, y0 - 1) of the tile's first pixel.
constexpr int kUpN = 12;
constexpr uint32_t kUpOutside = 0xFFFFFFFEu;  // staged key of an entry outside the image: no pixel's key (bit 31), not a miss
// WIN (ptx_upsample_bands): the small image is a row window (UpWin, ptx_launch.h) whose colours lie in
// two buffers, and the full-size rows are a band's.  Every position -- fx, x0, ax, fy, y0, ay, stage
// 3's y / S -- is the frame's (at S = 3, (float(y) + 0.5f) / 3.0f of a window-relative y rounds
// differently: tests/upsample_bands_ref.py); the window's offsets enter addresses only.  A row of
// the frame outside the window is staged like a row outside the frame: with 2 halo rows no pixel of
// the band has a candidate there.  Without WIN the code is the whole image's, `win` unread.
template <int S, bool WIN>
__device__ __forceinline__ void dn_upsample_tile(uint32_t W, uint32_t H, uint32_t w, uint32_t h, const UpWin &win,
                                                 const float4 *__restrict__ hg, const float4 *__restrict__ lg,
                                                 const float4 *__restrict__ lc, const float4 *__restrict__ lhalo,
                                                 float4 *__restrict__ out, float4 *g0, float4 *g1, float4 *cv) {
    static_assert(S >= 2 && S <= 4 && (kDnTile + S - 2) / S + 4 <= kUpN, "the window holds a tile's candidates");
    const int tx = (int)(threadIdx.x & 15u), ty = (int)(threadIdx.x >> 4);
    // the tile's first pixel in the frame; hg and out start at row Y0 of it
    const uint32_t Y0 = WIN ? win.Y0 : 0u, Y1 = WIN ? win.Y1 : H;
    const uint32_t bx = blockIdx.x * kDnTile, by = Y0 + blockIdx.y * kDnTile;
    const int ox = (int)__builtin_floorf(((float)bx + 0.5f) / (float)S - 0.5f) - 1;
    const int oy = (int)__builtin_floorf(((float)by + 0.5f) / (float)S - 0.5f) - 1;
    if (threadIdx.x < (uint32_t)(kUpN * kUpN)) {
        const int e = (int)threadIdx.x, gx = ox + e % kUpN, gy = oy + e / kUpN;
        float4 a = make_float4(0.0f, 0.0f, 0.0f, asf(kUpOutside)), b = make_float4(0.0f, 0.0f, 0.0f, 0.0f), c = b;
        if (WIN) {
            // lg starts at the window's row 0 (row win.y0 of the small frame); the window's rows [o0, o1)
            // are lc's, the rows above and then the rows below them lhalo's
            const int wy = gy - (int)win.y0;
            if (gx >= 0 && gy >= 0 && gx < (int)w && gy < (int)h && wy >= 0 && wy < (int)win.rows) {
                const size_t q = (size_t)wy * w + (size_t)gx;
                a = lg[2u * q];
                b = lg[2u * q + 1u];
                c = dn_load(DnImage{lc, lhalo, win.o0, win.o1}, w, (uint32_t)gx, (uint32_t)wy);
            }
        } else if (gx >= 0 && gy >= 0 && gx < (int)w && gy < (int)h) {
            const size_t q = (size_t)gy * w + (size_t)gx;
            a = lg[2u * q];
            b = lg[2u * q + 1u];
            c = lc[q];
        }
        g0[e] = a;
        g1[e] = b;
        cv[e] = c;
    }
    __syncthreads();
    const uint32_t x = bx + (uint32_t)tx, y = by + (uint32_t)ty;
    if (x >= W || y >= Y1) return;
    const size_t pix = (size_t)(y - Y0) * W + x;
    const float4 a = hg[2u * pix], b = hg[2u * pix + 1u];
    const uint32_t key = asu(a.w);
    const f3 Pp = rgb(a), Np = rgb(b);
    const float fx = ((float)x + 0.5f) / (float)S - 0.5f, fy = ((float)y + 0.5f) / (float)S - 0.5f;
    const float x0 = __builtin_floorf(fx), y0 = __builtin_floorf(fy);
    const float ax = fx - x0, ay = fy - y0;
    // (x0, y0) in the window: 1 .. kUpN - 3 by the bound above (clamped: no LDS index depends on it holding)
    const int lx = min(max((int)x0 - ox, 1), kUpN - 3), ly = min(max((int)y0 - oy, 1), kUpN - 3);
    f3 o;
    float sw = 0.0f;
    f3 sc = mk(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = (ly + j) * kUpN + (lx + i);
            const float4 qa = g0[e];
            if (asu(qa.w) != key) continue;
            const float bw = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
            const float gm = key == kDnMiss ? 1.0f : dn_gamma(Pp, Np, b.w, rgb(qa), rgb(g1[e]));
            const float wt = bw * gm;
            sw += wt;
            sc = sc + rgb(cv[e]) * wt;
        }
    if (sw > 0.0f) {
        o = sc / sw;
    } else {
        uint32_t n = 0u;
        sc = mk(0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int j = -1; j < 3; ++j)
#pragma unroll
            for (int i = -1; i < 3; ++i) {
                const int e = (ly + j) * kUpN + (lx + i);
                if (asu(g0[e].w) != key) continue;
                n += 1u;
                sc = sc + rgb(cv[e]);
            }
        if (n > 0u) o = sc / (float)n;
        else o = rgb(cv[min(max((int)(y / (uint32_t)S) - oy, 0), kUpN - 1) * kUpN + min(max((int)(x / (uint32_t)S) - ox, 0), kUpN - 1)]);
    }
    out[pix] = make_float4(o.x, o.y, o.z, 1.0f);
}
template <int S>
__global__ __launch_bounds__(kBlock) void dn_upsample(uint32_t W, uint32_t H, uint32_t w, uint32_t h,
                                                      const float4 *__restrict__ hg, const float4 *__restrict__ lg,
                                                      const float4 *__restrict__ lc, float4 *__restrict__ out) {
    __shared__ float4 g0[kUpN * kUpN], g1[kUpN * kUpN], cv[kUpN * kUpN];
    dn_upsample_tile<S, false>(W, H, w, h, UpWin{}, hg, lg, lc, nullptr, out, g0, g1, cv);
}
// A band of the full-size frame (rows [win.Y0, win.Y1), where hg and out start) from a window of the small one.
template <int S>
__global__ __launch_bounds__(kBlock) void dn_upsample_win(uint32_t W, uint32_t H, uint32_t w, uint32_t h, const UpWin win,
                                                          const float4 *__restrict__ hg, const float4 *__restrict__ lg,
                                                          const float4 *__restrict__ lc, const float4 *__restrict__ lhalo,
                                                          float4 *__restrict__ out) {
    __shared__ float4 g0[kUpN * kUpN], g1[kUpN * kUpN], cv[kUpN * kUpN];
    dn_upsample_tile<S, true>(W, H, w, h, win, hg, lg, lc, lhalo, out, g0, g1, cv);
}

// ---------------------------------------------------------------- temporal upsampling (ptx_upsample_temporal)
// The small image was rendered through phase (px, py): its pixel (i, j) looked through full-size pixel
// (S i + px, S j + py) (ptx_phase_uniform).  Per full-size pixel: the current estimate u -- dn_upsample's
// stages 1 and 2 at fx = float(x - px) / S, stage 3 the nearest small pixel --, the pixel's own sample d
// where the phase's grid has one with its key, and the history {H, n} of the previous call, looked up as
// dn_temporal looks its history up (a tap counts with any n' >= 0; a pixel without a hit looks only at
// itself, and only under the same camera); then the table of DESIGN.md §4.5, Temporal upsampling
// (tests/upsample_temporal_ref.py).  16 consecutive x - px have at most (16 + S - 2) / S + 1 values of
// x0 = floor((x - px) / S), and every candidate lies in x0 - 1 .. x0 + 2: the staged window is
// kN x kN from (x0 - 1, y0 - 1) of the tile's first pixel, kN = (16 + S - 2) / S + 4 (12, 9, 8).
struct UpHistory {
    float vp[16];  // the previous call's VP (mat4_inverse of the full-size uniform words 4..19 it saw)
    float alpha_min, alpha_fill;
    uint32_t mode;  // 0 no history, 1 that call's camera words are this one's, 2 reproject through vp
    uint32_t px, py;
};
__device__ __forceinline__ int up_floor_div(int a, int s) { return a >= 0 ? a / s : -((-a + s - 1) / s); }

// WIN (ptx_upsample_temporal_bands): rows [win.up.Y0, win.up.Y1) of the frame -- hg, hist and out start
// at row Y0 -- from a row window of the small frame (UpWin, as dn_upsample_tile<S, true>) and the rows
// [win.hy0, win.hy0 + win.hrows) of the previous state, where pguide and phist start.  Every position
// is the frame's: fx, x0, ax, fy, y0, ay, the grid test (y - py) mod S, stage 3's clamp against h, the
// reprojection's H; the offsets enter addresses only.
//   The small rows: for full-size row y, y0 = floor((y - py) / S).  A band of small rows [b0, b1) has
// y in [S b0, S b1): the smallest y0 is floor((S b0 - py) / S) = b0 - 1 for py > 0 (b0 for py = 0), the
// largest floor((S b1 - 1 - py) / S) = b1 - 1 since 0 <= S - 1 - py < S.  Stage 2 reaches y0 - 1 .. y0 + 2,
// stage 3 y0 or y0 + 1: rows b0 - 2 .. b1 + 1, two of either neighbour for every phase.  A pixel on the
// phase's grid has (y - py) a multiple of S that is >= S b0 - (S - 1), so >= S b0: its own sample's row
// (y - py) / S is one of b0 .. b1 - 1, the band's own.  A row of the frame outside the window is staged
// like a row outside the frame; no pixel of the band has a candidate there.
//   The history: a tap inside the frame whose row is not one of the state's hrows rows is not taken (as
// if its n' were below 0), dn_temporal's test with its unsigned row wrap, and a pixel with such a tap
// counts in *win.clip: one ballot and one add of its popcount per wave.  Only mode 2 with a primary
// hit and cw > 0 has taps off the pixel itself, so nothing else clips.
// Without WIN the code is the whole image's, `win` and `lhalo` unread.
// FOLLOW (a call of a following handle that finds an instance changed or a mesh deformed since the previous
// one, ptx_upsample_follow; tests/upsample_follow_ref.py): 0 the code above, `fo` unread.  1: a hit pixel's
// lookup goes by its instance's flag, fo.obj[key >> 16] (past fo.n_obj: 0), as dn_temporal<true>'s does -- flag 0
// as without the table; flag 2 no tap; flag 1 Q = D P and Nq = D N (dn_temporal_px's element order, not
// renormalised), Q always projected through vp, in mode 1 too, and the taps tested against Q and Nq with this
// pixel's r.  2: also flag 3, Q and Nq from the snapshot's triangle record under the previous call's instance
// matrices at the barycentrics of this pixel's G-buffer texel (fo.verts.gbuf starts at row Y0, like hg), by
// dn_temporal_px<true, true>'s expressions; then as flag 1.  A flag-1 or flag-3 pixel has taps off itself in
// mode 1 as well, so with a table a band's pixels can clip in either mode.
template <int S, bool WIN, int FOLLOW>
__device__ __forceinline__ void dn_upsample_temporal_tile(uint32_t W, uint32_t H, uint32_t w, uint32_t h, const UpHistory &Hs,
                                                          const UtWin &win, const UtFollow &fo, const float4 *__restrict__ hg,
                                                          const float4 *__restrict__ lg, const float4 *__restrict__ lc,
                                                          const float4 *__restrict__ lhalo, const float4 *__restrict__ pguide,
                                                          const float4 *__restrict__ phist, float4 *__restrict__ hist,
                                                          float4 *__restrict__ out, float4 *g0, float4 *g1, float4 *cv) {
    static_assert(S >= 2 && S <= 4, "scales 2, 3, 4");
    constexpr int kN = (kDnTile + S - 2) / S + 4;
    static_assert(kN * kN <= kBlock, "one lane per staged entry");
    const int tx = (int)(threadIdx.x & 15u), ty = (int)(threadIdx.x >> 4);
    // the tile's first pixel in the frame
    const uint32_t Y0 = WIN ? win.up.Y0 : 0u, Y1 = WIN ? win.up.Y1 : H;
    const uint32_t bx = blockIdx.x * kDnTile, by = Y0 + blockIdx.y * kDnTile;
    const uint32_t x = bx + (uint32_t)tx, y = by + (uint32_t)ty;
    const bool live = x < W && y < Y1;
    const size_t pix = live ? (size_t)(y - Y0) * W + x : 0u;  // (a lane outside the image loads pixel 0, unused)
    // this pixel in the previous state (a band's own rows are always covered)
    const size_t pc = WIN ? (size_t)((live ? y : Y0) - win.hy0) * W + (live ? x : 0u) : pix;
    const float4 a = hg[2u * pix], b = hg[2u * pix + 1u];
    const uint32_t key = asu(a.w);
    const f3 Pp = rgb(a), Np = rgb(b);
    // ---- where the previous call saw this pixel's point: Q, Nq (the flag, the texel and the snapshot record
    // are issued with the guide loads)
    uint32_t flag = 0u;
    f3 Q = Pp, Nq = Np;
    if (FOLLOW) {
        uint4 g = make_uint4(0u, 0u, 0u, 0u);
        if (FOLLOW == 2) g = fo.verts.gbuf[pix];
        const uint32_t inst = key >> 16;
        if (Hs.mode != 0u && key != kDnMiss && inst < fo.n_obj) flag = fo.obj[inst].flag;
        if (FOLLOW == 2 && flag == 3u) {
            const DnPrev &I = fo.verts.prev[inst];
            // (clamped: a G-buffer the host wrote may name any triangle; the handle's own never reaches the bound)
            const float4 *t = fo.verts.snap + 5u * (size_t)min(I.tri_base + g.y, fo.n_snap - 1u);
            const float4 ta = t[0], tb = t[1], tc = t[2], td = t[3], te = t[4];  // (tri_verts' record)
            const bool id = (I.mesh & kInstIdentity) != 0u;
            const f3 p0 = dn_prev_point(id, I.m, mk(ta.x, ta.y, ta.z)), n0 = dn_prev_point_t(id, I.minv, mk(ta.w, tb.x, tb.y));
            const f3 p1 = dn_prev_point(id, I.m, mk(tb.z, tb.w, tc.x)), n1 = dn_prev_point_t(id, I.minv, mk(tc.y, tc.z, tc.w));
            const f3 p2 = dn_prev_point(id, I.m, mk(td.x, td.y, td.z)), n2 = dn_prev_point_t(id, I.minv, mk(td.w, te.x, te.y));
            const float bu = asf(g.z), bv = asf(g.w), bw = 1.0f - bu - bv;
            Nq = normalize((n0 * bu + n1 * bv) + n2 * bw);
            Q = (p0 * bu + p1 * bv) + p2 * bw;
        }
        if (flag == 1u) {
            const float *d = fo.obj[inst].d;
            Q.x = ((d[0] * Pp.x + d[4] * Pp.y) + d[8] * Pp.z) + d[12];
            Q.y = ((d[1] * Pp.x + d[5] * Pp.y) + d[9] * Pp.z) + d[13];
            Q.z = ((d[2] * Pp.x + d[6] * Pp.y) + d[10] * Pp.z) + d[14];
            Nq.x = (d[0] * Np.x + d[4] * Np.y) + d[8] * Np.z;
            Nq.y = (d[1] * Np.x + d[5] * Np.y) + d[9] * Np.z;
            Nq.z = (d[2] * Np.x + d[6] * Np.y) + d[10] * Np.z;
        }
    }
    // ---- the history's taps k = 2 j + i (j outer), all loads issued ahead of the staging and the tests
    size_t q[4];
    float wq[4];
    bool in[4], clipped = false;
    float4 qa[4], qb[4], qh[4];
    const bool moved = FOLLOW && (flag == 1u || flag == 3u);  // (followed: through vp under the same camera too)
    if (Hs.mode == 1u && !moved) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { q[k] = pc; wq[k] = 1.0f; in[k] = k == 0 && !(FOLLOW && flag == 2u); }
    } else if (Hs.mode != 0u) {
        const float *vp = Hs.vp;
        const float cx = ((vp[0] * Q.x + vp[4] * Q.y) + vp[8] * Q.z) + vp[12];
        const float cy = ((vp[1] * Q.x + vp[5] * Q.y) + vp[9] * Q.z) + vp[13];
        const float cw = ((vp[3] * Q.x + vp[7] * Q.y) + vp[11] * Q.z) + vp[15];
        const float hx = ((cx / cw + 1.0f) * 0.5f) * (float)W - 0.5f, hy = ((cy / cw + 1.0f) * 0.5f) * (float)H - 0.5f;
        const float hx0 = __builtin_floorf(hx), hy0 = __builtin_floorf(hy);
        const float bx1 = hx - hx0, by1 = hy - hy0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = k & 1, j = k >> 1;
            const float qx = hx0 + (float)i, qy = hy0 + (float)j;
            // (a NaN or infinite projection compares false: outside)
            in[k] = key != kDnMiss && !(FOLLOW && flag == 2u) && cw > 0.0f && qx >= 0.0f && qx < (float)W && qy >= 0.0f &&
                    qy < (float)H;
            if (WIN) {
                const uint32_t ry = (uint32_t)(in[k] ? (int)qy : (int)win.hy0) - win.hy0;  // (below hy0: wraps past hrows)
                if (live && in[k] && ry >= win.hrows) clipped = true;
                in[k] = in[k] && ry < win.hrows;
                q[k] = in[k] ? (size_t)ry * W + (size_t)(int)qx : pc;
            } else {
                q[k] = in[k] ? (size_t)(int)qy * W + (size_t)(int)qx : pix;  // (an outside tap loads the centre, unused)
            }
            wq[k] = (i ? bx1 : 1.0f - bx1) * (j ? by1 : 1.0f - by1);
        }
    }
    if (Hs.mode != 0u) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            qa[k] = pguide[2u * q[k]];
            qb[k] = pguide[2u * q[k] + 1u];
            qh[k] = phist[q[k]];
        }
    }
    if (WIN && (Hs.mode == 2u || (FOLLOW && Hs.mode != 0u))) {  // (wave-uniform: every lane of the wave votes)
        const unsigned long long cm = __ballot(clipped);
        if (clipped && __lane_id() == (uint32_t)__ffsll((long long)cm) - 1u) atomicAdd(win.clip, (unsigned long long)__popcll(cm));
    }
    // ---- the tile's footprint in the small image
    const int ox = up_floor_div((int)bx - (int)Hs.px, S) - 1, oy = up_floor_div((int)by - (int)Hs.py, S) - 1;
    if (threadIdx.x < (uint32_t)(kN * kN)) {
        const int e = (int)threadIdx.x, gx = ox + e % kN, gy = oy + e / kN;
        float4 sa = make_float4(0.0f, 0.0f, 0.0f, asf(kUpOutside)), sb = make_float4(0.0f, 0.0f, 0.0f, 0.0f), sc4 = sb;
        if (WIN) {
            // lg starts at the window's row 0 (row win.up.y0 of the small frame); the window's rows [o0, o1)
            // are lc's, the rows above and then the rows below them lhalo's
            const int wy = gy - (int)win.up.y0;
            if (gx >= 0 && gy >= 0 && gx < (int)w && gy < (int)h && wy >= 0 && wy < (int)win.up.rows) {
                const size_t lq = (size_t)wy * w + (size_t)gx;
                sa = lg[2u * lq];
                sb = lg[2u * lq + 1u];
                sc4 = dn_load(DnImage{lc, lhalo, win.up.o0, win.up.o1}, w, (uint32_t)gx, (uint32_t)wy);
            }
        } else if (gx >= 0 && gy >= 0 && gx < (int)w && gy < (int)h) {
            const size_t lq = (size_t)gy * w + (size_t)gx;
            sa = lg[2u * lq];
            sb = lg[2u * lq + 1u];
            sc4 = lc[lq];
        }
        g0[e] = sa;
        g1[e] = sb;
        cv[e] = sc4;
    }
    __syncthreads();
    if (!live) return;
    // ---- the current estimate u
    const int dxi = (int)x - (int)Hs.px, dyi = (int)y - (int)Hs.py;
    const float fx = (float)dxi / (float)S, fy = (float)dyi / (float)S;
    const float x0 = __builtin_floorf(fx), y0 = __builtin_floorf(fy);
    const float ax = fx - x0, ay = fy - y0;
    // (x0, y0) in the window: 1 .. kN - 3 by the bound above (clamped: no LDS index depends on it holding)
    const int lx = min(max((int)x0 - ox, 1), kN - 3), ly = min(max((int)y0 - oy, 1), kN - 3);
    f3 u;
    float sw = 0.0f;
    f3 sc = mk(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = (ly + j) * kN + (lx + i);
            const float4 ga = g0[e];
            if (asu(ga.w) != key) continue;
            const float bw = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
            const float gm = key == kDnMiss ? 1.0f : dn_gamma(Pp, Np, b.w, rgb(ga), rgb(g1[e]));
            const float wt = bw * gm;
            sw += wt;
            sc = sc + rgb(cv[e]) * wt;
        }
    if (sw > 0.0f) {
        u = sc / sw;
    } else {
        uint32_t cnt = 0u;
        sc = mk(0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int j = -1; j < 3; ++j)
#pragma unroll
            for (int i = -1; i < 3; ++i) {
                const int e = (ly + j) * kN + (lx + i);
                if (asu(g0[e].w) != key) continue;
                cnt += 1u;
                sc = sc + rgb(cv[e]);
            }
        if (cnt > 0u) {
            u = sc / (float)cnt;
        } else {
            const int nx = min(max((int)x0 + (ax >= 0.5f ? 1 : 0), 0), (int)w - 1);
            const int ny = min(max((int)y0 + (ay >= 0.5f ? 1 : 0), 0), (int)h - 1);
            u = rgb(cv[min(max(ny - oy, 0), kN - 1) * kN + min(max(nx - ox, 0), kN - 1)]);
        }
    }
    // ---- the own sample: on the phase's grid x0 is the small pixel that looked through this one
    const int es = ly * kN + lx;
    const bool sampled = dxi >= 0 && dyi >= 0 && dxi % S == 0 && dyi % S == 0 && asu(g0[es].w) == key;
    const f3 d = rgb(cv[es]);
    // ---- the history
    float hw = 0.0f, nh = __builtin_inff();
    f3 hC = mk(0.0f, 0.0f, 0.0f);
    bool any = false;
    if (Hs.mode != 0u) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!in[k] || asu(qa[k].w) != key || !(qh[k].w >= 0.0f)) continue;
            if (key != kDnMiss) {
                if (!(dot(Nq, rgb(qb[k])) >= 0.9f)) continue;
                if (!(__builtin_fabsf(dot(Nq, rgb(qa[k]) - Q)) <= b.w)) continue;
            }
            hw += wq[k];
            hC = hC + rgb(qh[k]) * wq[k];
            nh = fminf(nh, qh[k].w);
            any = true;
        }
    }
    const bool have = any && hw > 0.0f;
    // ---- integration
    f3 Hn;
    float n;
    if (sampled && have) {
        n = fminf(nh + 1.0f, kDnNMax);
        Hn = mix3(hC / hw, d, fmaxf(1.0f / n, Hs.alpha_min));
    } else if (sampled) {
        Hn = d;
        n = 1.0f;
    } else if (have && nh >= 1.0f) {
        Hn = mix3(hC / hw, u, Hs.alpha_fill);
        n = nh;
    } else {
        Hn = u;
        n = 0.0f;
    }
    out[pix] = make_float4(Hn.x, Hn.y, Hn.z, 1.0f);
    hist[pix] = make_float4(Hn.x, Hn.y, Hn.z, n);
}
template <int S, int FOLLOW>
__global__ __launch_bounds__(kBlock) void dn_upsample_temporal(uint32_t W, uint32_t H, uint32_t w, uint32_t h, const UpHistory Hs,
                                                               const UtFollow fo, const float4 *__restrict__ hg,
                                                               const float4 *__restrict__ lg, const float4 *__restrict__ lc,
                                                               const float4 *__restrict__ pguide,
                                                               const float4 *__restrict__ phist, float4 *__restrict__ hist,
                                                               float4 *__restrict__ out) {
    constexpr int kN = (kDnTile + S - 2) / S + 4;
    __shared__ float4 g0[kN * kN], g1[kN * kN], cv[kN * kN];
    dn_upsample_temporal_tile<S, false, FOLLOW>(W, H, w, h, Hs, UtWin{}, fo, hg, lg, lc, nullptr, pguide, phist, hist, out, g0, g1,
                                                cv);
}
// A band of the full-size frame from a window of the small one and the covered rows of the previous state.
template <int S, int FOLLOW>
__global__ __launch_bounds__(kBlock) void dn_upsample_temporal_win(uint32_t W, uint32_t H, uint32_t w, uint32_t h,
                                                                   const UpHistory Hs, const UtWin win, const UtFollow fo,
                                                                   const float4 *__restrict__ hg, const float4 *__restrict__ lg,
                                                                   const float4 *__restrict__ lc, const float4 *__restrict__ lhalo,
                                                                   const float4 *__restrict__ pguide,
                                                                   const float4 *__restrict__ phist, float4 *__restrict__ hist,
                                                                   float4 *__restrict__ out) {
    constexpr int kN = (kDnTile + S - 2) / S + 4;
    __shared__ float4 g0[kN * kN], g1[kN * kN], cv[kN * kN];
    dn_upsample_temporal_tile<S, true, FOLLOW>(W, H, w, h, Hs, win, fo, hg, lg, lc, lhalo, pguide, phist, hist, out, g0, g1, cv);
}

// ---------------------------------------------------------------- launches
static dim3 dn_grid(uint32_t W, const DnWin &win) {
    return dim3((W + kDnTile - 1) / kDnTile, (win.c1 - win.c0 + kDnTile - 1) / kDnTile);
}

hipError_t launch_denoise_guide(const Scene &sc, const uint4 *gbuf, float4 *guide, float sigma_plane, hipStream_t s) {
    const uint32_t tiles = ((sc.width + 7u) / 8u) * ((sc.row_end - sc.row_begin + 7u) / 8u);
    hipLaunchKernelGGL(dn_guide, dim3((tiles * 64u + kBlock - 1) / kBlock), dim3(kBlock), 0, s, sc, gbuf, guide, sigma_plane);
    return hipGetLastError();
}
hipError_t launch_denoise_guide_halo(const Scene &sc, const uint4 *texels, uint32_t top, uint32_t bottom, float4 *guide,
                                     float sigma_plane, hipStream_t s) {
    const uint32_t rows = top + bottom;
    hipLaunchKernelGGL(dn_guide_halo, dim3((sc.width + kDnTile - 1) / kDnTile, (rows + kDnTile - 1) / kDnTile), dim3(kBlock), 0,
                       s, sc, texels, rows, top, sc.row_end - sc.row_begin, guide, sigma_plane);
    return hipGetLastError();
}
hipError_t launch_denoise_variance(uint32_t W, const DnWin &win, const DnImage &img, const float4 *guide, float4 *out,
                                   hipStream_t s) {
    hipLaunchKernelGGL(dn_variance<false>, dn_grid(W, win), dim3(kBlock), 0, s, W, win, img, (const float2 *)nullptr, guide, out);
    return hipGetLastError();
}
hipError_t launch_denoise_temporal(uint32_t W, uint32_t H, const DnWin &win, const float *vp_prev, float alpha_min,
                                   uint32_t mode, uint32_t prev_y0, uint32_t prev_rows, const float4 *guide,
                                   const float4 *frame, const float4 *accum, const float4 *pguide, const float4 *phist,
                                   const float2 *pmom, float4 *hist, float2 *mom, unsigned long long *clip,
                                   const DnObj *obj, uint32_t n_obj, const DnVerts &verts, hipStream_t s) {
    DnHistory Hs{};
    for (int i = 0; i < 16; ++i) Hs.vp[i] = vp_prev[i];
    Hs.alpha_min = alpha_min;
    Hs.mode = mode;
    Hs.y0 = prev_y0;
    Hs.rows = prev_rows;
    if (verts.snap) {
        if (!obj || !verts.gbuf || !verts.prev) return hipErrorInvalidValue;  // (flag 3 lives in obj)
        hipLaunchKernelGGL(dn_temporal_verts, dn_grid(W, win), dim3(kBlock), 0, s, W, H, win, Hs, guide, frame, accum, pguide,
                           phist, pmom, hist, mom, clip, obj, n_obj, verts.gbuf, verts.prev, verts.snap);
    } else if (obj)
        hipLaunchKernelGGL(dn_temporal<true>, dn_grid(W, win), dim3(kBlock), 0, s, W, H, win, Hs, guide, frame, accum, pguide,
                           phist, pmom, hist, mom, clip, obj, n_obj);
    else
        hipLaunchKernelGGL(dn_temporal<false>, dn_grid(W, win), dim3(kBlock), 0, s, W, H, win, Hs, guide, frame, accum, pguide,
                           phist, pmom, hist, mom, clip, (const DnObj *)nullptr, 0u);
    return hipGetLastError();
}
hipError_t launch_denoise_variance_moments(uint32_t W, const DnWin &win, const float4 *hist, const float2 *mom,
                                           const float4 *guide, float4 *out, hipStream_t s) {
    const DnImage img{hist, nullptr, 0u, win.rows};
    hipLaunchKernelGGL(dn_variance<true>, dn_grid(W, win), dim3(kBlock), 0, s, W, win, img, mom, guide, out);
    return hipGetLastError();
}
hipError_t launch_denoise_atrous(uint32_t W, const DnWin &win, uint32_t step, const float4 *in, const float4 *guide,
                                 float4 *out, float sigma_lum, bool last, hipStream_t s) {
    const dim3 g = dn_grid(W, win), bl(kBlock);
    const uint32_t l = last ? 1u : 0u;
    if (step == 1u) hipLaunchKernelGGL(dn_atrous_tiled<1>, g, bl, 0, s, W, win, in, guide, out, sigma_lum, l);
    else if (step == 2u) hipLaunchKernelGGL(dn_atrous_tiled<2>, g, bl, 0, s, W, win, in, guide, out, sigma_lum, l);
    else if (step == 4u) hipLaunchKernelGGL(dn_atrous_tiled<4>, g, bl, 0, s, W, win, in, guide, out, sigma_lum, l);
    else hipLaunchKernelGGL(dn_atrous_gather, g, bl, 0, s, W, win, (int)step, in, guide, out, sigma_lum, l);
    return hipGetLastError();
}

hipError_t launch_denoise_upsample(uint32_t s, uint32_t W, uint32_t H, const float4 *guide_hi, const float4 *guide_lo,
                                   const float4 *color_lo, float4 *out, hipStream_t st) {
    const dim3 g((W + kDnTile - 1) / kDnTile, (H + kDnTile - 1) / kDnTile), bl(kBlock);
    const uint32_t w = W / s, h = H / s;
    if (s == 2u) hipLaunchKernelGGL(dn_upsample<2>, g, bl, 0, st, W, H, w, h, guide_hi, guide_lo, color_lo, out);
    else if (s == 3u) hipLaunchKernelGGL(dn_upsample<3>, g, bl, 0, st, W, H, w, h, guide_hi, guide_lo, color_lo, out);
    else if (s == 4u) hipLaunchKernelGGL(dn_upsample<4>, g, bl, 0, st, W, H, w, h, guide_hi, guide_lo, color_lo, out);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
// FOLLOW by what the call carries: no table the unchanged instantiation, a table dn_temporal<true>'s rule,
// a snapshot beside it dn_temporal_verts' too.
static int ut_follow_kind(const UtFollow &fo) {
    if (!fo.obj) return fo.verts.snap || fo.verts.gbuf || fo.verts.prev ? -1 : 0;
    if (!fo.verts.snap) return 1;
    return fo.verts.gbuf && fo.verts.prev && fo.n_snap ? 2 : -1;  // (flag 3 lives in obj)
}
template <int S>
static void ut_launch(int kind, dim3 g, dim3 bl, hipStream_t st, uint32_t W, uint32_t H, uint32_t w, uint32_t h, const UpHistory &Hs,
                      const UtFollow &fo, const float4 *hg, const float4 *lg, const float4 *lc, const float4 *pg, const float4 *ph,
                      float4 *hist, float4 *out) {
    if (kind == 0) hipLaunchKernelGGL((dn_upsample_temporal<S, 0>), g, bl, 0, st, W, H, w, h, Hs, fo, hg, lg, lc, pg, ph, hist, out);
    else if (kind == 1) hipLaunchKernelGGL((dn_upsample_temporal<S, 1>), g, bl, 0, st, W, H, w, h, Hs, fo, hg, lg, lc, pg, ph, hist, out);
    else hipLaunchKernelGGL((dn_upsample_temporal<S, 2>), g, bl, 0, st, W, H, w, h, Hs, fo, hg, lg, lc, pg, ph, hist, out);
}
template <int S>
static void ut_launch_win(int kind, dim3 g, dim3 bl, hipStream_t st, uint32_t W, uint32_t H, uint32_t w, uint32_t h,
                          const UpHistory &Hs, const UtWin &win, const UtFollow &fo, const float4 *hg, const float4 *lg,
                          const float4 *lc, const float4 *lh, const float4 *pg, const float4 *ph, float4 *hist, float4 *out) {
    if (kind == 0) hipLaunchKernelGGL((dn_upsample_temporal_win<S, 0>), g, bl, 0, st, W, H, w, h, Hs, win, fo, hg, lg, lc, lh, pg, ph, hist, out);
    else if (kind == 1) hipLaunchKernelGGL((dn_upsample_temporal_win<S, 1>), g, bl, 0, st, W, H, w, h, Hs, win, fo, hg, lg, lc, lh, pg, ph, hist, out);
    else hipLaunchKernelGGL((dn_upsample_temporal_win<S, 2>), g, bl, 0, st, W, H, w, h, Hs, win, fo, hg, lg, lc, lh, pg, ph, hist, out);
}
hipError_t launch_denoise_upsample_temporal(uint32_t s, uint32_t W, uint32_t H, uint32_t px, uint32_t py, float alpha_min,
                                            float alpha_fill, uint32_t mode, const float *vp_prev, const UtFollow &fo,
                                            const float4 *guide_hi, const float4 *guide_lo, const float4 *color_lo,
                                            const float4 *guide_prev, const float4 *hist_prev, float4 *hist, float4 *out,
                                            hipStream_t st) {
    const dim3 g((W + kDnTile - 1) / kDnTile, (H + kDnTile - 1) / kDnTile), bl(kBlock);
    const uint32_t w = W / s, h = H / s;
    const int kind = ut_follow_kind(fo);
    if (px >= s || py >= s || W != s * w || H != s * h || kind < 0) return hipErrorInvalidValue;  // (the staged window's bound)
    UpHistory Hs{};
    for (int i = 0; i < 16; ++i) Hs.vp[i] = vp_prev[i];
    Hs.alpha_min = alpha_min;
    Hs.alpha_fill = alpha_fill;
    Hs.mode = mode;
    Hs.px = px;
    Hs.py = py;
    if (s == 2u) ut_launch<2>(kind, g, bl, st, W, H, w, h, Hs, fo, guide_hi, guide_lo, color_lo, guide_prev, hist_prev, hist, out);
    else if (s == 3u) ut_launch<3>(kind, g, bl, st, W, H, w, h, Hs, fo, guide_hi, guide_lo, color_lo, guide_prev, hist_prev, hist, out);
    else if (s == 4u) ut_launch<4>(kind, g, bl, st, W, H, w, h, Hs, fo, guide_hi, guide_lo, color_lo, guide_prev, hist_prev, hist, out);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
hipError_t launch_denoise_upsample_temporal_win(uint32_t s, uint32_t W, uint32_t H, uint32_t px, uint32_t py, float alpha_min,
                                                float alpha_fill, uint32_t mode, const float *vp_prev, const UtWin &win,
                                                const UtFollow &fo, const float4 *guide_hi, const float4 *guide_lo,
                                                const float4 *color_lo, const float4 *halo_lo, const float4 *guide_prev,
                                                const float4 *hist_prev, float4 *hist, float4 *out, hipStream_t st) {
    const dim3 g((W + kDnTile - 1) / kDnTile, (win.up.Y1 - win.up.Y0 + kDnTile - 1) / kDnTile), bl(kBlock);
    const uint32_t w = W / s, h = H / s;
    const int kind = ut_follow_kind(fo);
    if (px >= s || py >= s || W != s * w || H != s * h || kind < 0) return hipErrorInvalidValue;  // (the staged window's bound)
    // the rows the kernel addresses: the band's own inside the covered rows, the window's own rows inside the window
    if (win.up.Y0 >= win.up.Y1 || win.up.Y1 > H || win.hy0 > win.up.Y0 || win.hy0 + win.hrows < win.up.Y1 || !win.clip ||
        win.up.o0 > win.up.o1 || win.up.o1 > win.up.rows)
        return hipErrorInvalidValue;
    UpHistory Hs{};
    for (int i = 0; i < 16; ++i) Hs.vp[i] = vp_prev[i];
    Hs.alpha_min = alpha_min;
    Hs.alpha_fill = alpha_fill;
    Hs.mode = mode;
    Hs.px = px;
    Hs.py = py;
    if (s == 2u) ut_launch_win<2>(kind, g, bl, st, W, H, w, h, Hs, win, fo, guide_hi, guide_lo, color_lo, halo_lo, guide_prev, hist_prev, hist, out);
    else if (s == 3u) ut_launch_win<3>(kind, g, bl, st, W, H, w, h, Hs, win, fo, guide_hi, guide_lo, color_lo, halo_lo, guide_prev, hist_prev, hist, out);
    else if (s == 4u) ut_launch_win<4>(kind, g, bl, st, W, H, w, h, Hs, win, fo, guide_hi, guide_lo, color_lo, halo_lo, guide_prev, hist_prev, hist, out);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
hipError_t launch_denoise_upsample_win(uint32_t s, uint32_t W, uint32_t H, const UpWin &win, const float4 *guide_hi,
                                       const float4 *guide_lo, const float4 *color_lo, const float4 *halo_lo, float4 *out,
                                       hipStream_t st) {
    const dim3 g((W + kDnTile - 1) / kDnTile, (win.Y1 - win.Y0 + kDnTile - 1) / kDnTile), bl(kBlock);
    const uint32_t w = W / s, h = H / s;
    if (s == 2u) hipLaunchKernelGGL(dn_upsample_win<2>, g, bl, 0, st, W, H, w, h, win, guide_hi, guide_lo, color_lo, halo_lo, out);
    else if (s == 3u) hipLaunchKernelGGL(dn_upsample_win<3>, g, bl, 0, st, W, H, w, h, win, guide_hi, guide_lo, color_lo, halo_lo, out);
    else if (s == 4u) hipLaunchKernelGGL(dn_upsample_win<4>, g, bl, 0, st, W, H, w, h, win, guide_hi, guide_lo, color_lo, halo_lo, out);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace ptx
