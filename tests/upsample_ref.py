"""numpy f32 restatement of the guided upsampling (include/ptx.h ptx_upsample, DESIGN.md §4.5 Upsampling).

Test infrastructure only: the checker of dn_upsample in pathtracerdemo_amd/csrc/ptx_denoise.hip, whose
output must equal this one bit for bit.  Built on tests/denoise_ref.py: the guides are its Guides (of
the small image's denoise and of the full-size G-buffer), the guide weight is its _gamma's arithmetic
with the centre taken from the full-size guides.  Vectorised over the full-size image, one elementwise
numpy operation per rounding, candidates in the definition's order, a skipped candidate leaves every
sum as it was (np.where, not a zero weight).
"""
from __future__ import annotations

import numpy as np

import denoise_ref as D

f32 = np.float32
MISS = D.MISS


def positions(n_hi, s):
    """Per full-size coordinate: (x0, ax) of f = (x + 0.5) / s - 0.5 in the small image."""
    f = (np.arange(n_hi, dtype=np.float32) + f32(0.5)) / f32(s) - f32(0.5)
    x0 = np.floor(f)
    return x0.astype(np.int64), (f - x0).astype(np.float32)


def _gather(a, qy, qx, inside):
    """a[qy, qx] where inside (clamped indices elsewhere: never used)."""
    h, w = a.shape[:2]
    return a[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)]


def upsample(lo_rgb, G_lo, G_hi, s):
    """(image (H, W, 4) f32 with alpha 1, stage (H, W) in {1, 2, 3}) of the small image lo_rgb
    (h, w, >= 3) with guides G_lo, at the size of the guides G_hi = s times that."""
    c = np.ascontiguousarray(np.asarray(lo_rgb, np.float32)[..., :3])
    h, w = G_lo.key.shape
    H, W = G_hi.key.shape
    assert s in (2, 3, 4) and (H, W) == (s * h, s * w) and c.shape[:2] == (h, w)
    x0, ax = positions(W, s)
    y0, ay = positions(H, s)
    X0, Y0 = np.broadcast_to(x0[None, :], (H, W)), np.broadcast_to(y0[:, None], (H, W))
    AX, AY = np.broadcast_to(ax[None, :], (H, W)), np.broadcast_to(ay[:, None], (H, W))
    Kp, Pp, Np, rp = G_hi.key, G_hi.P, G_hi.N, G_hi.r
    miss = Kp == MISS
    with np.errstate(all="ignore"):
        # stage 1: guided bilinear
        sw = np.zeros((H, W), np.float32)
        sc = np.zeros((H, W, 3), np.float32)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = X0 + i, Y0 + j
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                ok = inside & (_gather(G_lo.key, qy, qx, inside) == Kp)
                b = (AX if i else f32(1) - AX) * (AY if j else f32(1) - AY)
                Pq, Nq = _gather(G_lo.P, qy, qx, inside), _gather(G_lo.N, qy, qx, inside)
                wn = np.fmax(f32(0), D.dot3(Np, Nq))
                for _ in range(7):
                    wn = wn * wn
                wd = np.fmax(f32(0), f32(1) - np.abs(D.dot3(Np, Pq - Pp)) / rp)
                gm = np.where(miss, f32(1), wn * wd).astype(np.float32)
                wt = b * gm
                sw = np.where(ok, sw + wt, sw)
                sc = np.where(ok[..., None], sc + wt[..., None] * _gather(c, qy, qx, inside), sc)
        one = sw > 0  # (a NaN sum compares false)
        out1 = sc / sw[..., None]
        # stage 2: same-key average
        n = np.zeros((H, W), np.int64)
        sc = np.zeros((H, W, 3), np.float32)
        for j in range(4):
            for i in range(4):
                qx, qy = X0 - 1 + i, Y0 - 1 + j
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                ok = inside & (_gather(G_lo.key, qy, qx, inside) == Kp)
                n = np.where(ok, n + 1, n)
                sc = np.where(ok[..., None], sc + _gather(c, qy, qx, inside), sc)
        two = ~one & (n > 0)
        out2 = sc / n.astype(np.float32)[..., None]
        # stage 3: nearest
        out3 = c[(np.arange(H) // s)[:, None], (np.arange(W) // s)[None, :]]
    stage = np.where(one, 1, np.where(two, 2, 3)).astype(np.int32)
    img = np.ones((H, W, 4), np.float32)
    img[..., :3] = np.where(one[..., None], out1, np.where(two[..., None], out2, out3))
    return img, stage


def replicate(lo, s):
    """Pixel replication of an (h, w, k) image: what a host shows without the guides."""
    return np.repeat(np.repeat(np.asarray(lo), s, axis=0), s, axis=1)
