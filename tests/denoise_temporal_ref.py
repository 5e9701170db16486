"""numpy f32 restatement of the denoiser's temporal mode (include/ptx.h ptx_denoise, temporal = 1;
DESIGN.md §Denoiser, "Temporal mode").

Test infrastructure only: the checker of dn_temporal / dn_variance_t in
pathtracerdemo_amd/csrc/ptx_denoise.hip, whose history and output must equal this one bit for bit.
The guides, the 7x7 variance and the a-trous iterations are tests/denoise_ref.py's; what is stated
here is the history lookup (same pixel, or bilinear through the previous call's VP), the
integration and the choice of the variance.  One elementwise numpy operation per rounding, taps in
the definition's order (j outer), a skipped tap leaves every sum as it was.
"""
from __future__ import annotations

import numpy as np

import denoise_ref as D

f32 = np.float32
DEFAULT_ALPHA_MIN = 0.05
N_MAX = 255
N_MOMENTS = 4  # from this history length on the variance comes from the integrated moments


def mat4_inverse(m):
    """The f32 inverse of a column-major f32 matrix: cofactors in double, one rounding to f32
    (include/ptx.h: "VP' of the previous call"); zeros when singular."""
    m = [float(v) for v in np.asarray(m, np.float32)]
    inv = [0.0] * 16
    inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10]
    inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10]
    inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9]
    inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9]
    inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10]
    inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10]
    inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9]
    inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9]
    inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6]
    inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6]
    inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5]
    inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5]
    inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6]
    inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6]
    inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5]
    inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5]
    det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12]
    return np.array([v / det if det != 0.0 else 0.0 for v in inv], np.float64).astype(np.float32)


def mixf(a, b, t):
    return a * (f32(1) - t) + b * t


class _State:
    def __init__(self, G, camera, C, m1, m2, n):
        self.G, self.camera, self.C, self.m1, self.m2, self.n = G, camera, C, m1, m2, n
        self.vp = mat4_inverse(camera[:16].view(np.float32))


class TemporalDenoiser:
    """The state a handle keeps from one temporal call to the next, and the call itself."""

    def __init__(self):
        self.state = None
        self.taps = None  # of the last temporal call: (H, W) number of taken taps, -1 where no lookup ran
        self.same_pixel = False  # the last temporal call used the same-pixel rule

    def reset(self):
        """ptx_upload_scene / ptx_reset_accumulation: the next call sees no history."""
        self.state = None

    @property
    def history(self):
        """PTX_BUF_DENOISE_HISTORY: (H, W, 4) f32 {C.rgb, n}."""
        s = self.state
        return np.concatenate([s.C, s.n[..., None]], -1).astype(np.float32)

    @property
    def moments(self):
        return self.state.m1, self.state.m2

    # -------------------------------------------------------------- history lookup
    def _candidates(self, G, camera):
        """[(inside, qx, qy, w)] per candidate tap, and the pixels a lookup runs for."""
        H, W = G.key.shape
        s = self.state
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        if np.array_equal(camera, s.camera):
            self.same_pixel = True
            return [(np.ones((H, W), bool), xs, ys, np.ones((H, W), np.float32))], G.hit
        self.same_pixel = False
        vp, P = s.vp, G.P
        cx = ((vp[0] * P[..., 0] + vp[4] * P[..., 1]) + vp[8] * P[..., 2]) + vp[12]
        cy = ((vp[1] * P[..., 0] + vp[5] * P[..., 1]) + vp[9] * P[..., 2]) + vp[13]
        cw = ((vp[3] * P[..., 0] + vp[7] * P[..., 1]) + vp[11] * P[..., 2]) + vp[15]
        fx = ((cx / cw + f32(1)) * f32(0.5)) * f32(W) - f32(0.5)
        fy = ((cy / cw + f32(1)) * f32(0.5)) * f32(H) - f32(0.5)
        x0, y0 = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0, fy - y0
        out = []
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + f32(i), y0 + f32(j)
                inside = (qx >= 0) & (qx < f32(W)) & (qy >= 0) & (qy < f32(H))  # (NaN: outside)
                w = (ax if i else f32(1) - ax) * (ay if j else f32(1) - ay)
                qxi = np.where(inside, qx, 0).astype(np.int64)
                qyi = np.where(inside, qy, 0).astype(np.int64)
                out.append((inside, qxi, qyi, w.astype(np.float32)))
        return out, G.hit & (cw > 0)

    def _lookup(self, G, camera):
        """(has history, C_h, m1_h, m2_h, n_h) per pixel."""
        H, W = G.key.shape
        s = self.state
        sw = np.zeros((H, W), np.float32)
        sC = np.zeros((H, W, 3), np.float32)
        s1 = np.zeros((H, W), np.float32)
        s2 = np.zeros((H, W), np.float32)
        nh = np.full((H, W), np.inf, np.float32)
        taken_any = np.zeros((H, W), bool)
        cands, runs = self._candidates(G, camera)
        self.taps = np.where(runs, 0, -1)
        for inside, qx, qy, w in cands:
            kq, nq = s.G.key[qy, qx], s.n[qy, qx]
            ok = runs & inside & (kq == G.key) & (nq >= 1)
            ok &= D.dot3(G.N, s.G.N[qy, qx]) >= f32(0.9)
            ok &= np.abs(D.dot3(G.N, s.G.P[qy, qx] - G.P)) <= G.r
            sw = np.where(ok, sw + w, sw)
            sC = np.where(ok[..., None], sC + w[..., None] * s.C[qy, qx], sC)
            s1 = np.where(ok, s1 + w * s.m1[qy, qx], s1)
            s2 = np.where(ok, s2 + w * s.m2[qy, qx], s2)
            nh = np.where(ok, np.minimum(nh, nq), nh)
            taken_any |= ok
            self.taps = self.taps + ok
        have = taken_any & (sw > 0)
        return have, sC / sw[..., None], s1 / sw, s2 / sw, nh

    # -------------------------------------------------------------- the call
    def denoise(self, frame_color, accum, G, uniform, iterations=0, sigma_lum=0.0, alpha_min=0.0, temporal=True):
        """(H, W, 4) f32 denoised image of one call.  G: this frame's guides (they carry sigma_plane);
        frame_color: PTX_BUF_FRAME_COLOR; accum: PTX_BUF_ACCUM (the colour of pixels without a hit)."""
        if not temporal:
            return D.denoise(accum, G, iterations, sigma_lum)  # (neither reads nor writes the state)
        n_it = iterations or D.DEFAULT_ITERATIONS
        sl = sigma_lum or D.DEFAULT_SIGMA_LUM
        am = f32(alpha_min or DEFAULT_ALPHA_MIN)
        assert 1 <= n_it <= 6 and np.isfinite(am) and 0 < am <= 1
        camera = np.ascontiguousarray(np.asarray(uniform, np.uint32)[4:23]).copy()
        hit = G.hit
        H, W = hit.shape
        with np.errstate(all="ignore"):
            F = np.ascontiguousarray(np.asarray(frame_color, np.float32)[..., :3])
            l = D.luminance(F)
            C, m1, m2, n = F.copy(), l, l * l, np.ones((H, W), np.float32)
            if self.state is not None:
                have, Ch, m1h, m2h, nh = self._lookup(G, camera)
                nn = np.minimum(nh + f32(1), f32(N_MAX))
                a = np.fmax(f32(1) / nn, am)
                C = np.where(have[..., None], mixf(Ch, F, a[..., None]), C)
                m1 = np.where(have, mixf(m1h, l, a), m1)
                m2 = np.where(have, mixf(m2h, l * l, a), m2)
                n = np.where(have, nn, n)
            else:
                self.taps = np.full((H, W), -1)
                self.same_pixel = False
            acc = np.asarray(accum, np.float32)[..., :3]
            C = np.where(hit[..., None], C, acc).astype(np.float32)
            m1 = np.where(hit, m1, f32(0)).astype(np.float32)
            m2 = np.where(hit, m2, f32(0)).astype(np.float32)
            n = np.where(hit, n, f32(0)).astype(np.float32)
            self.state = _State(G, camera, C, m1, m2, n)
            v = np.where(n >= N_MOMENTS, np.fmax(f32(0), m2 - m1 * m1), D.variance(C, G))
            v = np.where(hit, v, f32(0)).astype(np.float32)
            c = C
            for i in range(n_it):
                c, v = D.atrous(c, v, G, 1 << i, sl)
        out = np.ones((H, W, 4), np.float32)
        out[..., :3] = c
        return out
