"""numpy f32 restatement of the temporal upsampling (include/ptx.h ptx_phase_uniform and
ptx_upsample_temporal, DESIGN.md §4.5 "Temporal upsampling").

Test infrastructure only: the checker of ptx_phase_uniform (pathtracerdemo_amd/csrc/ptx_api.cpp) and of
dn_upsample_temporal (pathtracerdemo_amd/csrc/ptx_denoise.hip), whose outputs must equal these bit for
bit.  Built on tests/denoise_ref.py's Guides and tests/denoise_temporal_ref.py's mat4_inverse and mixf.
Vectorised over the full-size image, one elementwise numpy operation per rounding, candidates in the
definition's order (j outer), a skipped candidate leaves every sum as it was (np.where, not a zero
weight).

Details the prose definition leaves open, pinned here (DESIGN.md repeats them):
  * ptx_phase_uniform: when dx and dy are both zero the sixteen matrix words are copied (t + 0 * c0
    would turn a -0 into +0); otherwise every component of the translation column is
    (t + dx * c0) + dy * c1, zero factors included.
  * a pixel without a primary hit (key MISS) goes through the same table as any other: it is sampled
    when lo's pixel of its phase is a miss too, its guide weight in stages 1 and 2 is ptx_upsample's (1),
    and its history is the same pixel's when the camera words are equal and that pixel was a miss (no
    normal or plane test: a miss has neither); under a moved camera it has no history.
  * a hit pixel's same-pixel tap passes the same four tests as a reprojected one (key, n' >= 0,
    normals, plane): a host may have rewritten the G-buffer between the calls.
  * history exists when at least one tap was taken and the taken weights sum to more than 0.
  * alpha_min: 0 selects DEFAULT_ALPHA_MIN, otherwise finite and in (0, 1].  alpha_fill: any negative
    finite value selects DEFAULT_ALPHA_FILL, otherwise in [0, 1] (0 keeps a sampled history as it is).
  * n is stored as an f32; alpha = fmax(1 / n, alpha_min) with n = fmin(n_h + 1, 255).
"""
from __future__ import annotations

import numpy as np

import denoise_ref as D
import denoise_temporal_ref as T

f32 = np.float32
MISS = D.MISS
DEFAULT_ALPHA_MIN = 0.02
DEFAULT_ALPHA_FILL = 0.05
N_MAX = 255


# ---------------------------------------------------------------- the phase helper
def phase_uniform(hi_uniform, s, px, py):
    """The uniform of the W/s x H/s frame whose pixel (i, j) looks through hi's pixel (s i + px, s j + py)."""
    u = np.array(hi_uniform, np.uint32).copy()
    assert u.shape == (33,) and s in (2, 3, 4) and 0 <= px < s and 0 <= py < s
    W, H = int(u[0]), int(u[1])
    assert W > 0 and H > 0 and W % s == 0 and H % s == 0
    u[0], u[1] = W // s, H // s
    dx = f32(2 * px - (s - 1)) / f32(W)
    dy = f32(2 * py - (s - 1)) / f32(H)
    if dx != 0 or dy != 0:
        m = u[4:20].view(np.float32)
        with np.errstate(all="ignore"):
            t = (m[12:16] + dx * m[0:4]) + dy * m[4:8]
        u[16:20] = t.astype(np.float32).view(np.uint32)
    return u


# ---------------------------------------------------------------- the current estimate
def positions(n_hi, s, p):
    """Per full-size coordinate x: (x0, ax) of f = float(x - p) / float(s) in the small image."""
    f = (np.arange(n_hi, dtype=np.int64) - p).astype(np.float32) / f32(s)
    x0 = np.floor(f)
    return x0.astype(np.int64), (f - x0).astype(np.float32)


def _gather(a, qy, qx):
    h, w = a.shape[:2]
    return a[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)]


def estimate(c, G_lo, G_hi, s, px, py):
    """(u (H, W, 3), stage (H, W) in {1, 2, 3}): ptx_upsample's stages 1 and 2 at the phase's
    positions, stage 3 the nearest pixel of lo."""
    with np.errstate(all="ignore"):
        h, w = G_lo.key.shape
        H, W = G_hi.key.shape
        x0, ax = positions(W, s, px)
        y0, ay = positions(H, s, py)
        X0, Y0 = np.broadcast_to(x0[None, :], (H, W)), np.broadcast_to(y0[:, None], (H, W))
        AX, AY = np.broadcast_to(ax[None, :], (H, W)), np.broadcast_to(ay[:, None], (H, W))
        Kp, Pp, Np, rp = G_hi.key, G_hi.P, G_hi.N, G_hi.r
        miss = Kp == MISS
        sw = np.zeros((H, W), np.float32)
        sc = np.zeros((H, W, 3), np.float32)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = X0 + i, Y0 + j
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                ok = inside & (_gather(G_lo.key, qy, qx) == Kp)
                b = (AX if i else f32(1) - AX) * (AY if j else f32(1) - AY)
                Pq, Nq = _gather(G_lo.P, qy, qx), _gather(G_lo.N, qy, qx)
                wn = np.fmax(f32(0), D.dot3(Np, Nq))
                for _ in range(7):
                    wn = wn * wn
                wd = np.fmax(f32(0), f32(1) - np.abs(D.dot3(Np, Pq - Pp)) / rp)
                gm = np.where(miss, f32(1), wn * wd).astype(np.float32)
                wt = b * gm
                sw = np.where(ok, sw + wt, sw)
                sc = np.where(ok[..., None], sc + wt[..., None] * _gather(c, qy, qx), sc)
        one = sw > 0  # (a NaN sum compares false)
        out1 = sc / sw[..., None]
        n = np.zeros((H, W), np.int64)
        sc = np.zeros((H, W, 3), np.float32)
        for j in range(4):
            for i in range(4):
                qx, qy = X0 - 1 + i, Y0 - 1 + j
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                ok = inside & (_gather(G_lo.key, qy, qx) == Kp)
                n = np.where(ok, n + 1, n)
                sc = np.where(ok[..., None], sc + _gather(c, qy, qx), sc)
        two = ~one & (n > 0)
        out2 = sc / n.astype(np.float32)[..., None]
        out3 = c[np.clip(Y0 + (AY >= f32(0.5)), 0, h - 1), np.clip(X0 + (AX >= f32(0.5)), 0, w - 1)]
        stage = np.where(one, 1, np.where(two, 2, 3)).astype(np.int32)
        u = np.where(one[..., None], out1, np.where(two[..., None], out2, out3)).astype(np.float32)
    return u, stage


def own_sample(c, G_lo, G_hi, s, px, py):
    """(on the phase's grid (H, W), sampled (H, W), d (H, W, 3)): lo's pixel that looked through each hi pixel."""
    H, W = G_hi.key.shape
    dx, dy = np.arange(W, dtype=np.int64) - px, np.arange(H, dtype=np.int64) - py
    grid = ((dx % s) == 0)[None, :] & ((dy % s) == 0)[:, None]
    qx, qy = np.broadcast_to((dx // s)[None, :], (H, W)), np.broadcast_to((dy // s)[:, None], (H, W))
    sampled = grid & (_gather(G_lo.key, qy, qx) == G_hi.key)
    return grid, sampled, _gather(c, qy, qx)


# ---------------------------------------------------------------- the call and its state
class _State:
    def __init__(self, G, camera, Hc, n):
        self.G, self.camera, self.H, self.n = G, camera, Hc, n
        self.vp = T.mat4_inverse(camera[:16].view(np.float32))


class TemporalUpsampler:
    """The state the full-size handle keeps from one ptx_upsample_temporal to the next, and the call."""

    def __init__(self):
        self.state = None
        self.info = {}  # of the last call: stage, grid, sampled, have, taps (-1: no lookup ran), same_pixel, case

    def reset(self):
        """Everything that drops the state: the next call is a first call."""
        self.state = None

    @property
    def history(self):
        """PTX_BUF_UPSAMPLE_HISTORY: (H, W, 4) f32 {H.rgb, n}."""
        return np.concatenate([self.state.H, self.state.n[..., None]], -1).astype(np.float32)

    def _lookup(self, G, camera):
        """(has history, H_h, n_h, taps, same pixel) per pixel: dn_temporal's rule on the full-size state, a
        tap counting with any n' >= 0."""
        H, W = G.key.shape
        st = self.state
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        same = np.array_equal(camera, st.camera)
        if same:
            cands, runs = [(np.ones((H, W), bool), xs, ys, np.ones((H, W), np.float32))], np.ones((H, W), bool)
        else:
            vp, P = st.vp, G.P
            cx = ((vp[0] * P[..., 0] + vp[4] * P[..., 1]) + vp[8] * P[..., 2]) + vp[12]
            cy = ((vp[1] * P[..., 0] + vp[5] * P[..., 1]) + vp[9] * P[..., 2]) + vp[13]
            cw = ((vp[3] * P[..., 0] + vp[7] * P[..., 1]) + vp[11] * P[..., 2]) + vp[15]
            fx = ((cx / cw + f32(1)) * f32(0.5)) * f32(W) - f32(0.5)
            fy = ((cy / cw + f32(1)) * f32(0.5)) * f32(H) - f32(0.5)
            x0, y0 = np.floor(fx), np.floor(fy)
            ax, ay = fx - x0, fy - y0
            cands = []
            for j in (0, 1):
                for i in (0, 1):
                    qx, qy = x0 + f32(i), y0 + f32(j)
                    inside = (qx >= 0) & (qx < f32(W)) & (qy >= 0) & (qy < f32(H))  # (NaN: outside)
                    w = (ax if i else f32(1) - ax) * (ay if j else f32(1) - ay)
                    cands.append((inside, np.where(inside, qx, 0).astype(np.int64), np.where(inside, qy, 0).astype(np.int64),
                                  w.astype(np.float32)))
            runs = G.hit & (cw > 0)
        sw = np.zeros((H, W), np.float32)
        sC = np.zeros((H, W, 3), np.float32)
        nh = np.full((H, W), np.inf, np.float32)
        taps = np.where(runs, 0, -1)
        any_ = np.zeros((H, W), bool)
        for inside, qx, qy, w in cands:
            nq = st.n[qy, qx]
            ok = runs & inside & (st.G.key[qy, qx] == G.key) & (nq >= 0)
            geo = (D.dot3(G.N, st.G.N[qy, qx]) >= f32(0.9)) & (np.abs(D.dot3(G.N, st.G.P[qy, qx] - G.P)) <= G.r)
            ok &= ~G.hit | geo
            sw = np.where(ok, sw + w, sw)
            sC = np.where(ok[..., None], sC + st.H[qy, qx] * w[..., None], sC)
            nh = np.where(ok, np.minimum(nh, nq), nh)
            any_ |= ok
            taps = taps + ok
        return any_ & (sw > 0), sC / sw[..., None], nh, taps, same

    def upsample(self, lo_rgb, G_lo, G_hi, hi_uniform, s, px, py, alpha_min=0.0, alpha_fill=-1.0):
        """(H, W, 4) f32 {H.rgb, 1}: PTX_BUF_DENOISED of one call.  lo_rgb: lo's denoised image (h, w, >= 3),
        rendered through phase_uniform(hi_uniform, s, px, py); G_lo: the guides of that denoise; G_hi: the
        full-size guides (they carry sigma_plane)."""
        c = np.ascontiguousarray(np.asarray(lo_rgb, np.float32)[..., :3])
        h, w = G_lo.key.shape
        H, W = G_hi.key.shape
        assert s in (2, 3, 4) and (H, W) == (s * h, s * w) and c.shape[:2] == (h, w) and 0 <= px < s and 0 <= py < s
        am = f32(alpha_min or DEFAULT_ALPHA_MIN)
        af = f32(DEFAULT_ALPHA_FILL if alpha_fill < 0 else alpha_fill)
        assert np.isfinite(am) and 0 < am <= 1 and np.isfinite(af) and 0 <= af <= 1
        camera = np.ascontiguousarray(np.asarray(hi_uniform, np.uint32)[4:23]).copy()
        with np.errstate(all="ignore"):
            u, stage = estimate(c, G_lo, G_hi, s, px, py)
            grid, sampled, d = own_sample(c, G_lo, G_hi, s, px, py)
            if self.state is not None:
                have, Hh, nh, taps, same = self._lookup(G_hi, camera)
            else:
                have, Hh, nh = np.zeros((H, W), bool), np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32)
                taps, same = np.full((H, W), -1), False
            nn = np.minimum(nh + f32(1), f32(N_MAX))
            a = np.fmax(f32(1) / nn, am)
            case = np.where(sampled, np.where(have, 0, 1), np.where(have & (nh >= 1), 2, 3))
            Hn = np.where((case == 0)[..., None], T.mixf(Hh, d, a[..., None]),
                          np.where((case == 1)[..., None], d,
                                   np.where((case == 2)[..., None], T.mixf(Hh, u, af), u))).astype(np.float32)
            n = np.where(case == 0, nn, np.where(case == 1, f32(1), np.where(case == 2, nh, f32(0)))).astype(np.float32)
        self.state = _State(G_hi, camera, Hn, n)
        self.info = dict(stage=stage, grid=grid, sampled=sampled, have=have, taps=taps, same_pixel=same, case=case)
        out = np.ones((H, W, 4), np.float32)
        out[..., :3] = Hn
        return out
