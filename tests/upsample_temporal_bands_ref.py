"""numpy restatement of ptx_upsample_temporal_bands (include/ptx.h, DESIGN.md §4.5 "Temporal upsampling,
bands"), built on tests/upsample_temporal_ref.py's TemporalUpsampler.

Test infrastructure only: the checker of dn_upsample_temporal_win (pathtracerdemo_amd/csrc/ptx_denoise.hip)
and of the call's exchange, whose outputs must equal these bit for bit.

A band's result is the whole-frame definition evaluated on the previous state with the taps outside
the band's covered rows removed.  So this keeps the frame's assembled previous state and a validity
flag per band, and for band i runs TemporalUpsampler on a copy of that state whose n is -1 (a tap
fails the n' >= 0 test, the first thing after the key) outside rows [Y0 - min(T, Y0), Y1 + min(T, H - Y1))
and in the rows of bands without a state; a band without a state of its own runs a first call.  It keeps
band i's rows.  Every position is the frame's by construction: nothing is evaluated band-relative.

Clipped pixels (PTX_COUNTER_UPSAMPLE_CLIP) are counted from the candidates themselves: a pixel of the
band whose lookup reprojects (the camera words differ, a primary hit, cw > 0) and that has at least one
candidate inside the image but outside the covered rows.  The same-pixel rule never clips.

history_rows is taken as given: the call's minimum band height (T rows per full-size band) is the
caller's to respect, so the restatement can be compared with the whole image at T >= H.
"""
from __future__ import annotations

import numpy as np

import upsample_temporal_ref as UT

f32 = np.float32


def candidate_rows(G, st):
    """(runs (H, W), [(inside (H, W), row (H, W))] x 4): the reprojected candidates of TemporalUpsampler._lookup
    under a camera that differs from the state's, operation by operation."""
    H, W = G.key.shape
    with np.errstate(all="ignore"):
        vp, P = st.vp, G.P
        cx = ((vp[0] * P[..., 0] + vp[4] * P[..., 1]) + vp[8] * P[..., 2]) + vp[12]
        cy = ((vp[1] * P[..., 0] + vp[5] * P[..., 1]) + vp[9] * P[..., 2]) + vp[13]
        cw = ((vp[3] * P[..., 0] + vp[7] * P[..., 1]) + vp[11] * P[..., 2]) + vp[15]
        fx = ((cx / cw + f32(1)) * f32(0.5)) * f32(W) - f32(0.5)
        fy = ((cy / cw + f32(1)) * f32(0.5)) * f32(H) - f32(0.5)
        x0, y0 = np.floor(fx), np.floor(fy)
        out = []
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + f32(i), y0 + f32(j)
                inside = (qx >= 0) & (qx < f32(W)) & (qy >= 0) & (qy < f32(H))
                out.append((inside, np.where(inside, qy, 0).astype(np.int64)))
        return G.hit & (cw > 0), out


class BandTemporalUpsampler:
    """The states the full-size bands keep from one ptx_upsample_temporal_bands to the next, and the call.
    bounds: the full-size bands' rows [0, Y1, ..., H]; history_rows: T of every call (0 = 32)."""

    def __init__(self, bounds, history_rows=0):
        self.bounds = [int(b) for b in bounds]
        self.T = int(history_rows) or 32
        self.n_bands = len(self.bounds) - 1
        self.state = None  # the frame's assembled previous state (rows of bands without one: unspecified)
        self.valid = [False] * self.n_bands
        self.clips = [0] * self.n_bands      # of the last call, per band
        self.halo_taps = [0] * self.n_bands  # taps taken from rows the exchange brought, per band
        self.clip_mask = None                # the clipped pixels of the last call (H, W) bool
        self.info = {}                       # of the last call, assembled from the bands' rows

    def reset(self):
        self.valid = [False] * self.n_bands

    def drop(self, i):
        """Band i's state alone is dropped: it starts without history, its neighbours find no taps in its rows."""
        self.valid[i] = False

    @property
    def history(self):
        return np.concatenate([self.state.H, self.state.n[..., None]], -1).astype(np.float32)

    def covered(self, i):
        H = self.bounds[-1]
        Y0, Y1 = self.bounds[i], self.bounds[i + 1]
        return Y0 - min(self.T, Y0), Y1 + min(self.T, H - Y1)

    def _masked(self, keep_rows):
        """The previous state with n = -1 outside the rows keep_rows (H,) bool and in bands without a state."""
        st = self.state
        keep = keep_rows.copy()
        for k in range(self.n_bands):
            if not self.valid[k]:
                keep[self.bounds[k]:self.bounds[k + 1]] = False
        n = np.where(keep[:, None], st.n, f32(-1)).astype(np.float32)
        return UT._State(st.G, st.camera, st.H, n)

    def upsample(self, lo_rgb, G_lo, G_hi, hi_uniform, s, px, py, alpha_min=0.0, alpha_fill=-1.0):
        """(H, W, 4) f32 {H.rgb, 1}: the bands' PTX_BUF_DENOISED in band order, of one call."""
        H, W = G_hi.key.shape
        assert H == self.bounds[-1]
        camera = np.ascontiguousarray(np.asarray(hi_uniform, np.uint32)[4:23]).copy()
        out = np.ones((H, W, 4), np.float32)
        Hn, n = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32)
        info = {}
        rows = np.arange(H)
        self.clip_mask = np.zeros((H, W), bool)
        for i in range(self.n_bands):
            Y0, Y1 = self.bounds[i], self.bounds[i + 1]
            lo_c, hi_c = self.covered(i)
            t = UT.TemporalUpsampler()
            self.clips[i] = self.halo_taps[i] = 0
            if self.state is not None and self.valid[i]:
                t.state = self._masked((rows >= lo_c) & (rows < hi_c))
                if not np.array_equal(camera, self.state.camera):
                    runs, cands = candidate_rows(G_hi, self.state)
                    clip = np.zeros((H, W), bool)
                    for inside, qy in cands:
                        clip |= runs & inside & ((qy < lo_c) | (qy >= hi_c))
                    self.clips[i] = int(clip[Y0:Y1].sum())
                    self.clip_mask[Y0:Y1] = clip[Y0:Y1]
                # the taps the own rows alone would give: the others came from halo rows
                t_own = UT.TemporalUpsampler()
                t_own.state = self._masked((rows >= Y0) & (rows < Y1))
                t_own.upsample(lo_rgb, G_lo, G_hi, hi_uniform, s, px, py, alpha_min, alpha_fill)
                own_taps = np.maximum(t_own.info["taps"][Y0:Y1], 0).sum()
            o = t.upsample(lo_rgb, G_lo, G_hi, hi_uniform, s, px, py, alpha_min, alpha_fill)
            if t.info["taps"].max() >= 0 and self.valid[i] and self.state is not None:
                self.halo_taps[i] = int(np.maximum(t.info["taps"][Y0:Y1], 0).sum() - own_taps)
            out[Y0:Y1] = o[Y0:Y1]
            Hn[Y0:Y1], n[Y0:Y1] = t.state.H[Y0:Y1], t.state.n[Y0:Y1]
            for k, v in t.info.items():
                if isinstance(v, np.ndarray):
                    info.setdefault(k, np.zeros_like(v))[Y0:Y1] = v[Y0:Y1]
                else:
                    info.setdefault(k, []).append(v)
        self.state = UT._State(G_hi, camera, Hn, n)
        self.valid = [True] * self.n_bands
        self.info = info
        return out
