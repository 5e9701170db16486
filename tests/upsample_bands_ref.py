"""numpy f32 restatement of the guided upsampling of a band (include/ptx.h ptx_upsample_bands, DESIGN.md
§4.5 Upsampling, Bands).

Test infrastructure only: tests/upsample_ref.py's upsample applied to a ROW WINDOW of the small image
-- a band's rows [b0, b1) and `halo` rows of its neighbours on either side, where the frame has them --
as if the window were the whole image, with the row positions (y0, ay) taken from the frame's rows.
dn_upsample_win in pathtracerdemo_amd/csrc/ptx_denoise.hip does the same with halo = 2.
upsample_ref is wrapped, not edited: while it runs on a window its positions() answers the row axis
(its second call) from frame coordinates.
"""
from __future__ import annotations

import contextlib

import numpy as np

import denoise_ref as D
import upsample_ref as U

f32 = np.float32
HALO = 2  # rows of each neighbour a band reads: y0 - 1 .. y0 + 2 with y0 = b0 - 1 .. b1 - 1


def rows(G, a, b):
    """The guides of rows [a, b)."""
    return D.Guides(G.key[a:b], G.P[a:b], G.N[a:b], G.r[a:b])


def frame_row_positions(Y0, n_hi, s, w0):
    """(y0, ay) of the full-size rows Y0 .. Y0 + n_hi of the frame, y0 as a row of the window that
    starts at the small frame's row w0: the position is the frame's, the offset only addresses."""
    f = (np.arange(Y0, Y0 + n_hi, dtype=np.float32) + f32(0.5)) / f32(s) - f32(0.5)
    y0 = np.floor(f)
    return y0.astype(np.int64) - w0, (f - y0).astype(np.float32)


@contextlib.contextmanager
def _rows_from_frame(Y0, w0):
    """upsample_ref.upsample asks positions(W, s), then positions(H, s): the second answer is the frame's."""
    plain, calls = U.positions, []

    def positions(n_hi, s):
        calls.append(n_hi)
        return plain(n_hi, s) if len(calls) == 1 else frame_row_positions(Y0, n_hi, s, w0)

    U.positions = positions
    try:
        yield
    finally:
        U.positions = plain
    assert len(calls) == 2


def upsample_band(lo_rgb, G_lo, G_hi, s, b0, b1, halo=HALO, window_relative=False):
    """(image (s * (b1 - b0), W, 4), stage) of the full-size rows [s * b0, s * b1): the small frame's
    window [b0 - halo, b1 + halo) clipped to the frame, upsampled as if it were the whole image.
    window_relative: positions from the window's own row numbers (what the kernel must not do)."""
    h = G_lo.key.shape[0]
    w0, w1 = max(0, b0 - halo), min(h, b1 + halo)
    c = np.asarray(lo_rgb, np.float32)[w0:w1]
    Gl, Gh = rows(G_lo, w0, w1), rows(G_hi, s * w0, s * w1)
    if window_relative:
        img, stage = U.upsample(c, Gl, Gh, s)
    else:
        with _rows_from_frame(s * w0, w0):
            img, stage = U.upsample(c, Gl, Gh, s)
    a = s * (b0 - w0)
    return img[a:a + s * (b1 - b0)], stage[a:a + s * (b1 - b0)]


def upsample_bands(lo_rgb, G_lo, G_hi, s, cuts, halo=HALO, window_relative=False):
    """Every band's rows in order: the bands are [0, cuts[0]), [cuts[0], cuts[1]), ..., [cuts[-1], h)."""
    bounds = [0] + list(cuts) + [G_lo.key.shape[0]]
    parts = [upsample_band(lo_rgb, G_lo, G_hi, s, a, b, halo, window_relative) for a, b in zip(bounds, bounds[1:])]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
