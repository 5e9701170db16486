"""The guided upsampling's numpy restatement (tests/upsample_ref.py) on the CPU: the C ABI's new
surface, the properties the definition in DESIGN.md §4.5 (Upsampling) promises, and what it buys on
this renderer's output: a denoised 48x36 image written at 96x72 under the full-size G-buffer against
the same image pixel-replicated.  dn_upsample is compared with the same restatement bit for bit in
tests/test_gpu_upsample.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import denoise_ref as D
import upsample_ref as U
from helpers import rel_l2, uniform_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the ABI's new surface
def test_header_declares_the_upsampler_and_the_binding_mirrors_it():
    from pathtracerdemo_amd import _native as N
    txt = open(os.path.join(ROOT, "include", "ptx.h")).read()
    assert re.search(r"^int ptx_upsample\(ptx_handle \*hi, ptx_handle \*lo, const ptx_upsample_params \*p", txt, re.M)
    assert re.search(r"float sigma_plane;.*\n\s*uint32_t reserved\[7\];.*\n\} ptx_upsample_params;", txt)
    defs = {k: int(v) for k, v in re.findall(r"^#define\s+(PTX_\w+)\s+(\d+)\b", txt, re.M)}
    assert defs["PTX_ABI_VERSION"] == N.PTX_ABI_VERSION == 5
    assert "ptx_upsample" in N.EXPORTED
    assert ctypes.sizeof(N.PtxUpsampleParams) == 32
    assert [f[0] for f in N.PtxUpsampleParams._fields_] == ["sigma_plane", "reserved"]
    lib = N.load()
    assert lib.ptx_abi_version() == 5
    assert lib.ptx_upsample(None, None, None) == -1


# ------------------------------------------------------------------ properties on synthetic guides
def ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def one_plane(w, h, s):
    """Every pixel of both sizes on one plane facing the camera, one key, equal normals: gamma = 1
    (N.N = 1 exactly, the plane distance 0 exactly)."""
    def guides(ww, hh):
        P = np.zeros((hh, ww, 3), np.float32)
        P[..., 0], P[..., 1] = np.meshgrid(np.arange(ww, dtype=np.float32), np.arange(hh, dtype=np.float32))
        N = np.zeros((hh, ww, 3), np.float32)
        N[..., 2] = 1
        return D.guides_from_surfaces(np.full((hh, ww), 5, np.uint32), P, N, (0.0, 0.0, 9.0))
    return guides(w, h), guides(s * w, s * h)


def plain_bilinear(c, s):
    """Bilinear interpolation at the definition's positions with its expressions and order, taps
    outside the image skipped."""
    h, w = c.shape[:2]
    x0, ax = U.positions(s * w, s)
    y0, ay = U.positions(s * h, s)
    sw = np.zeros((s * h, s * w), np.float32)
    sc = np.zeros((s * h, s * w, 3), np.float32)
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = (x0 + i)[None, :], (y0 + j)[:, None]
            ok = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            b = ((ax if i else np.float32(1) - ax)[None, :] * (ay if j else np.float32(1) - ay)[:, None]) * np.float32(1)
            t = c[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)]
            sw = np.where(ok, sw + b, sw)
            sc = np.where(ok[..., None], sc + b[..., None] * t, sc)
    return sc / sw[..., None]


@pytest.mark.parametrize("s", [2, 3, 4])
def test_one_plane_is_plain_bilinear(s):
    w, h = 13, 9
    Gl, Gh = one_plane(w, h, s)
    rng = np.random.default_rng(5)
    c = rng.gamma(0.6, 0.5, (h, w, 3)).astype(np.float32)
    out, stage = U.upsample(c, Gl, Gh, s)
    assert (stage == 1).all() and (out[..., 3] == 1).all()
    np.testing.assert_array_equal(out[..., :3].view(np.uint32), plain_bilinear(c, s).view(np.uint32))
    c[...] = np.array([0.31, 0.62, 0.17], np.float32)
    out, _ = U.upsample(c, Gl, Gh, s)
    want = np.broadcast_to(c[0, 0], out[..., :3].shape).copy()
    assert ulps(out[..., :3].copy(), want).max() <= 1


def walls(w, h, s):
    """A wall in three keys (vertical stripes, the middle one a single small pixel wide) under a
    band of sky; full-size keys follow the small ones except a full-size stripe one pixel wide that
    no small pixel owns (stage 3) and one whose small neighbours lie two small pixels away (stage 2)."""
    def guides(ww, hh, k):
        xs, ys = np.meshgrid(np.arange(ww, dtype=np.float32), np.arange(hh, dtype=np.float32))
        P = np.stack([(xs + np.float32(0.5)) * np.float32(0.1 / k), (ys + np.float32(0.5)) * np.float32(0.1 / k),
                      np.zeros_like(xs)], -1).astype(np.float32)
        n = np.array([-0.08, 0.0, 1.0], np.float32)
        N = np.broadcast_to(n / np.sqrt((n * n).sum(dtype=np.float32)), P.shape).astype(np.float32)
        return P, N
    kl = np.where(np.arange(w) < w // 2, 1, 2)[None, :].repeat(h, 0).astype(np.uint32)
    kl[:, w // 2] = 3
    kl[:2] = D.MISS
    kh = U.replicate(kl, s).copy()
    kh[s * 2:, 1] = 9                     # a key no small pixel has: nearest
    kh[s * 2:, s * (w // 2 + 2)] = 3      # key 3 seen again where the 2x2 has none of it but the 4x4 has
    Pl, Nl = guides(w, h, 1)
    Ph, Nh = guides(s * w, s * h, s)
    cam = (1.0, 0.7, 4.0)
    return D.guides_from_surfaces(kl, Pl, Nl, cam), D.guides_from_surfaces(kh, Ph, Nh, cam)


@pytest.mark.parametrize("s", [2, 3, 4])
def test_other_keys_do_not_leak(s):
    w, h = 14, 10
    Gl, Gh = walls(w, h, s)
    rng = np.random.default_rng(11)
    c = rng.gamma(0.6, 0.5, (h, w, 3)).astype(np.float32)
    base, stage = U.upsample(c, Gl, Gh, s)
    assert all((stage == k).any() for k in (1, 2, 3)), np.bincount(stage.ravel())
    assert np.isfinite(base).all()
    for key in (1, 3, D.MISS):
        other = c.copy()
        sel = Gl.key != key
        other[sel] = rng.uniform(0, 1e6, (int(sel.sum()), 3)).astype(np.float32)
        moved, stage2 = U.upsample(other, Gl, Gh, s)
        np.testing.assert_array_equal(stage2, stage)
        mine = (Gh.key == key) & (stage < 3)
        assert mine.any()
        np.testing.assert_array_equal(moved[mine].view(np.uint32), base[mine].view(np.uint32))
        assert (moved[Gh.key != key] != base[Gh.key != key]).any()


# ------------------------------------------------------------------ quality on oracle frames
w, h, S = 48, 36, 2
FRAMES = (1, 4)
#        scene, reuse pipeline, frames of the long accumulation, asserted bounds at frames 1 and 4:
# halfway between the measured ratio and 1 (tests/test_denoise_temporal_ref.py's convention)
# measured: C1 0.928 / 0.800, C3 0.734 / 0.741
CASES = [("scene1", False, 512, (0.964, 0.900)), ("scene3", True, 256, (0.867, 0.871))]


@pytest.fixture(scope="module", params=CASES, ids=["c1_restir", "c3_reuse"])
def frames(request, oracle_mod):
    scene, reuse, n_long, bounds = request.param
    cs = request.getfixturevalue(scene)
    O = oracle_mod

    def run(fr, f):
        fr.set_frame_index(f)
        fr.run_reuse_frame(threads=8) if reuse else fr.run(O.PASS_RESTIR, threads=8)

    hi = O.Frame(uniform_for(cs, S * w, S * h), cs.scene, cs.geometry, cs.accel)
    first = None
    for f in range(1, n_long + 1):
        run(hi, f)
        if f == 1:
            first = hi.accum.copy()
    G_hi = D.guides_from_gbuffer(hi.uniform, cs.scene, cs.geometry, cs.accel, hi.gbuffer)
    lo = O.Frame(uniform_for(cs, w, h), cs.scene, cs.geometry, cs.accel)
    assert (np.asarray(lo.uniform)[4:23] == np.asarray(hi.uniform)[4:23]).all()
    snaps = {}
    for f in range(1, max(FRAMES) + 1):
        run(lo, f)
        if f in FRAMES:
            snaps[f] = lo.accum.copy()
    G_lo = D.guides_from_gbuffer(lo.uniform, cs.scene, cs.geometry, cs.accel, lo.gbuffer)
    return snaps, G_lo, G_hi, hi.accum.copy(), first, bounds


def test_guided_upsample_beats_pixel_replication(frames):
    """Relative L2 against the long 96x72 accumulation of the guided upsample of the denoised 48x36
    image / that of its pixel replication.  Measured: C1 0.928 / 0.800, C3 0.734 / 0.741 (frames 1 / 4); asserted: halfway to 1.
    Not asserted: against the full-size spatial denoise of frame 1, what the host gives up, the guided
    upsample of frame 1 has 0.99 (C1) and 1.90 (C3) times the error."""
    snaps, G_lo, G_hi, truth, first, bounds = frames
    assert G_hi.hit.any() and not G_hi.hit.all() and len(np.unique(G_hi.key)) > 2
    full = rel_l2(D.denoise(first, G_hi)[..., :3], truth[..., :3])
    for f, bound in zip(FRAMES, bounds):
        den = D.denoise(snaps[f], G_lo)
        up, stage = U.upsample(den, G_lo, G_hi, S)
        e_up = rel_l2(up[..., :3], truth[..., :3])
        e_rep = rel_l2(U.replicate(den, S)[..., :3], truth[..., :3])
        print(f"frames {f}: guided {e_up:.4f} replicated {e_rep:.4f} ratio {e_up / e_rep:.3f}; full-size denoise of "
              f"frame 1 {full:.4f} (guided / full {e_up / full:.3f}); stages {np.bincount(stage.ravel(), minlength=4)[1:].tolist()}")
        assert e_up <= bound * e_rep, (f, e_up, e_rep)
