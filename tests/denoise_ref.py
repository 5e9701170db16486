"""numpy f32 restatement of the denoiser (include/ptx.h ptx_denoise).

Test infrastructure only: the checker of pathtracerdemo_amd/csrc/ptx_denoise.hip, whose output
must equal this one bit for bit.  Vectorised over the image, one elementwise numpy operation per
rounding, taps in the definition's order, a skipped tap leaves every sum as it was (np.where, not
a zero weight).  The guides come from tests/wgsl_ref.py's GetSurface on the G-buffer words -- the
per-pixel restatement of the reference shader -- so nothing here shares get_surface with the kernels.
"""
from __future__ import annotations

import numpy as np

import wgsl_ref as R

f32 = np.float32
MISS = np.uint32(0xFFFFFFFF)  # key of a pixel without a primary hit, and of every pixel outside the image
DEFAULT_ITERATIONS, DEFAULT_SIGMA_LUM, DEFAULT_SIGMA_PLANE = 5, 4.0, 0.02
B5 = [f32(1 / 16), f32(1 / 4), f32(3 / 8), f32(1 / 4), f32(1 / 16)]
W3 = [f32(1 / 4), f32(1 / 2), f32(1 / 4)]


class Guides:
    """Per pixel: key (instance | sub-mesh, MISS without a hit), P, N (H, W, 3) and r = sigma_plane * |P - camera|."""

    def __init__(self, key, P, N, r):
        self.key = np.ascontiguousarray(key, np.uint32)
        self.P = np.ascontiguousarray(P, np.float32)
        self.N = np.ascontiguousarray(N, np.float32)
        self.r = np.ascontiguousarray(r, np.float32)

    @property
    def hit(self):
        return self.key != MISS


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def guides_from_surfaces(key, P, N, camera, sigma_plane=DEFAULT_SIGMA_PLANE):
    """Guides of given surfaces (synthetic guide sets): r from the camera position."""
    P = np.asarray(P, np.float32)
    d = P - np.asarray(camera, np.float32)
    return Guides(key, P, N, f32(sigma_plane) * np.sqrt(dot3(d, d)))


def guides_from_gbuffer(uniform, scene, geometry, accel, gbuffer, sigma_plane=DEFAULT_SIGMA_PLANE):
    """Guides of a rendered frame: GetSurface (tests/wgsl_ref.py) of every G-buffer texel with a hit."""
    sc = R.Scene(uniform, scene, geometry, accel)
    g = np.asarray(gbuffer, np.uint32)
    H, W = g.shape[:2]
    key = np.where(g[..., 0] >> 31 == 1, g[..., 0] & np.uint32(0x7FFFFFFF), MISS).astype(np.uint32)
    P = np.zeros((H, W, 3), np.float32)
    N = np.zeros((H, W, 3), np.float32)
    gf = g.view(np.float32)
    for y, x in zip(*np.nonzero(key != MISS)):
        w = g[y, x]
        s = R.GetSurface(sc, (int(w[0] >> 16) & 0x7FFF, int(w[0]) & 0xFFFF, int(w[1]), gf[y, x, 2], gf[y, x, 3]))
        P[y, x] = s["pos"]
        N[y, x] = s["n"]
    cam = np.asarray(uniform, np.uint32)[20:23].view(np.float32)
    G = guides_from_surfaces(key, P, N, cam, sigma_plane)
    G.r[key == MISS] = 0
    return G


class _Taps:
    """Neighbour views of per-pixel arrays: at(a, ox, oy)[y, x] = a[y + oy, x + ox], `fill` outside."""

    def __init__(self, H, W, reach):
        self.H, self.W, self.R = H, W, reach
        self._pad = {}

    def at(self, a, ox, oy, fill=0):
        k = id(a)
        if k not in self._pad:
            width = [(self.R, self.R), (self.R, self.R)] + [(0, 0)] * (a.ndim - 2)
            self._pad[k] = (a, np.pad(a, width, constant_values=fill))  # (keeps `a` alive: ids are not reused)
        p = self._pad[k][1]
        return p[self.R + oy:self.R + oy + self.H, self.R + ox:self.R + ox + self.W]


def _gamma(G, T, ox, oy):
    """(tap taken, guide weight) of tap q = p + (ox, oy) for every centre p."""
    kq = T.at(G.key, ox, oy, fill=MISS)
    ok = (G.key != MISS) & (kq == G.key)  # outside, a miss, or another key: skipped
    wn = np.fmax(f32(0), dot3(G.N, T.at(G.N, ox, oy)))
    for _ in range(7):
        wn = wn * wn
    wd = np.fmax(f32(0), f32(1) - np.abs(dot3(G.N, T.at(G.P, ox, oy) - G.P)) / G.r)
    return ok, wn * wd


def luminance(c):
    return (c[..., 0] * f32(0.2126) + c[..., 1] * f32(0.7152)) + c[..., 2] * f32(0.0722)


def variance(c, G):
    """The variance pass: 7x7 guide-weighted luminance moments, v = max(0, E[l^2] - E[l]^2)."""
    H, W = G.key.shape
    T = _Taps(H, W, 3)
    lum = luminance(c)
    s0 = np.zeros((H, W), np.float32)
    s1 = np.zeros((H, W), np.float32)
    s2 = np.zeros((H, W), np.float32)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            ok, gm = _gamma(G, T, dx, dy)
            lq = T.at(lum, dx, dy)
            s0 = np.where(ok, s0 + gm, s0)
            s1 = np.where(ok, s1 + gm * lq, s1)
            s2 = np.where(ok, s2 + gm * (lq * lq), s2)
    m = s1 / s0
    v = np.fmax(f32(0), s2 / s0 - m * m)
    return np.where(G.hit, v, f32(0)).astype(np.float32)


def atrous(c, v, G, step, sigma_lum):
    """One iteration at `step` on the pair (c, v)."""
    H, W = G.key.shape
    T = _Taps(H, W, max(2 * step, 1))
    hit = G.hit
    vb = np.zeros((H, W), np.float32)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            ok = hit & (T.at(G.key, dx, dy, fill=MISS) == G.key)  # the variance, too, stays inside the key
            vb = np.where(ok, vb + (W3[dy + 1] * W3[dx + 1]) * T.at(v, dx, dy), vb)
    dp = f32(sigma_lum) * np.sqrt(vb) + f32(1e-6)
    lum = luminance(c)
    sw = np.zeros((H, W), np.float32)
    sc = np.zeros((H, W, 3), np.float32)
    sv = np.zeros((H, W), np.float32)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ok, gm = _gamma(G, T, step * dx, step * dy)
            h = B5[dy + 2] * B5[dx + 2]
            t = np.fmax(f32(0), f32(1) - (np.abs(lum - T.at(lum, step * dx, step * dy)) / dp) / f32(4))
            wl = (t * t) * (t * t)
            w = (h * gm) * wl
            sw = np.where(ok, sw + w, sw)
            sc = np.where(ok[..., None], sc + w[..., None] * T.at(c, step * dx, step * dy), sc)
            sv = np.where(ok, sv + (w * w) * T.at(v, step * dx, step * dy), sv)
    cn = sc / sw[..., None]
    vn = sv / (sw * sw)
    return (np.where(hit[..., None], cn, c).astype(np.float32), np.where(hit, vn, f32(0)).astype(np.float32))


def denoise(accum, G, iterations=0, sigma_lum=0.0):
    """(H, W, 4) f32: rgb after the last iteration, alpha 1; the guides carry sigma_plane."""
    n = iterations or DEFAULT_ITERATIONS
    sl = sigma_lum or DEFAULT_SIGMA_LUM
    assert 1 <= n <= 6
    with np.errstate(all="ignore"):
        c = np.ascontiguousarray(np.asarray(accum, np.float32)[..., :3])
        v = variance(c, G)
        for i in range(n):
            c, v = atrous(c, v, G, 1 << i, sl)
    out = np.ones(c.shape[:2] + (4,), np.float32)
    out[..., :3] = c
    return out


def denoise_frame(accum, uniform, cs, gbuffer, iterations=0, sigma_lum=0.0, sigma_plane=0.0):
    """The denoised image of a rendered frame of compiled scene `cs`."""
    G = guides_from_gbuffer(uniform, cs.scene, cs.geometry, cs.accel, gbuffer, sigma_plane or DEFAULT_SIGMA_PLANE)
    return denoise(accum, G, iterations, sigma_lum)
