"""ptx_denoise_bands on the GPU: a frame split into row bands denoises itself after one exchange of
2^(iterations + 1) halo rows (peer copies between the handles of one process here; their
communicators in tests/loopback_denoise_bands.py).  The bar: every band's rows of the result equal
one whole-image handle's ptx_denoise bit for bit -- which tests/test_gpu_denoise*.py pin to the numpy
restatement -- in spatial and temporal mode; where a band's temporal state does not reach (the clip
rule) the band equals the restatement with the previous history zeroed outside its window; nothing
else of a handle changes, and what the call refuses it refuses before touching the GPU."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_ref as D
import denoise_temporal_ref as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "loopback", "libptx_loopback_rccl.so")
ALT = dict(sigma_lum=1.0, sigma_plane=0.005)  # (tests/test_gpu_denoise.py's alternate sigmas)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want, what):
    bad = np.any(bits(got) != bits(want), axis=-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[:4].tolist()}"


def make(cs, W, H, pipeline, a=0, b=0, **kw):
    from pathtracerdemo_amd.renderer import Renderer
    if pipeline in ("reuse", "gi"):
        kw.setdefault("reuse_radius", 12)
    r = Renderer(W, H, device=0, pipeline=pipeline, row_begin=a, row_end=b, **kw)
    r.Initialize(cs)
    return r


def split(cs, W, H, pipeline, cuts, **kw):
    bounds = [0] + list(cuts) + [H]
    return [make(cs, W, H, pipeline, a, b, **kw) for a, b in zip(bounds, bounds[1:])]


def frame(one, bands, yaw=None, pitch=None, reset=False):
    """The next frame on the whole-image handle (if any) and on the bands."""
    from pathtracerdemo_amd.renderer import Renderer
    for r in ([one] if one is not None else []) + list(bands):
        if yaw is not None:
            r.GetCamera().set_yaw(yaw)
        if pitch is not None:
            r.GetCamera().set_pitch(pitch)
        if reset:
            r.ResetFrameCount()
        r.Update()
    if one is not None:
        one.Render()
    if bands and bands[0].pipeline in ("reuse", "gi"):
        Renderer.render_bands(bands)
    else:
        for b in bands:
            b.Render()


def gathered(bands, name):
    return np.concatenate([getattr(b, name)() for b in bands])


def close(*rs):
    for r in rs:
        r.close()


# ------------------------------------------------------------------ spatial mode
def test_small_split_equals_one_handle_and_the_restatement(scene1):
    """72x80 as bands of 17, 33 and 30 rows, one frame: 1, 2 and 3 iterations (halos of 4, 8, 16 rows)
    equal the whole-image handle and the numpy restatement; 4 iterations need 32 rows of every band."""
    from pathtracerdemo_amd import _native as native
    from pathtracerdemo_amd.renderer import Renderer
    W, H = 72, 80
    one, bands = make(scene1, W, H, "restir"), split(scene1, W, H, "restir", [17, 50])
    frame(one, bands)
    same(gathered(bands, "read_image"), one.read_image(), "accumulation")
    G = D.guides_from_gbuffer(one.uniform, scene1.scene, scene1.geometry, scene1.accel, one.read_gbuffer())
    assert G.hit.any() and not G.hit.all()
    out = np.zeros((H, W, 4), np.float32)
    for n in (1, 2, 3):
        one.Denoise(iterations=n)
        Renderer.denoise_bands(bands, out, iterations=n)
        same(out, one.read_denoised(), f"{n} iterations, against one handle")
        same(out, D.denoise(one.read_image(), G, iterations=n), f"{n} iterations, against the restatement")
        same(gathered(bands, "read_denoised"), out, f"{n} iterations, read_denoised per band")
    with pytest.raises(native.PtxError, match=r"band 0 has 17 rows.*32 rows"):
        Renderer.denoise_bands(bands, iterations=4)
    same(gathered(bands, "read_denoised"), out, "a refused call leaves the result")
    close(one, *bands)


@pytest.mark.parametrize("pipeline,W,H,cuts,calls", [
    ("reuse", 64, 200, [66, 133], [{}, ALT]),
    ("reuse", 48, 260, [130], [dict(iterations=6)]),
    ("gi", 64, 200, [66, 133], [{}]),
], ids=["reuse_default_reach", "reuse_maximum_reach", "gi_default_reach"])
def test_default_and_maximum_reach_equal_one_handle(scene3, pipeline, W, H, cuts, calls):
    from pathtracerdemo_amd.renderer import Renderer
    one, bands = make(scene3, W, H, pipeline), split(scene3, W, H, pipeline, cuts)
    for _ in range(2):
        frame(one, bands)
    same(gathered(bands, "read_image"), one.read_image(), "accumulation")
    hit = one.read_gbuffer()[..., 0] >> 31 == 1
    assert hit.any() and not hit.all()
    out = np.zeros((H, W, 4), np.float32)
    for params in calls:
        one.Denoise(**params)
        Renderer.denoise_bands(bands, out, **params)
        same(out, one.read_denoised(), f"{params}")
        assert (out[hit][:, :3] != one.read_image()[hit][:, :3]).any()
    close(one, *bands)


def test_one_whole_image_handle_is_ptx_denoise(scene1):
    from pathtracerdemo_amd import _native as native
    from pathtracerdemo_amd.renderer import Renderer
    a, b = make(scene1, 70, 45, "restir"), make(scene1, 70, 45, "restir")
    frame(None, [a, b])
    before = b.stats()
    a.Denoise(iterations=4)
    Renderer.denoise_bands([b], iterations=4)
    same(b.read_denoised(), a.read_denoised(), "n = 1")
    s = b.stats()
    assert s["kernel_launches"][native.PTX_STAT_DENOISE] == 2 + 4
    assert s["device_bytes"] - before["device_bytes"] == 70 * 45 * 64
    close(a, b)


# ------------------------------------------------------------------ nothing else changes
@pytest.mark.parametrize("temporal", [False, True], ids=["spatial", "temporal"])
def test_nothing_else_changes_and_the_call_is_ordered(scene3, temporal):
    """A 3-band set that never denoises, read after each of 3 frames, against sets that denoise after
    every frame with the next frame enqueued at once, nothing synchronised in between, read after
    frame K = 1, 2, 3: the same accumulation, history reservoirs and G-buffer.  And the denoised
    image of frame 1 is frame 1's when frames 2 and 3 were enqueued right behind the call."""
    from pathtracerdemo_amd.renderer import Renderer
    W, H, cuts = 64, 200, [66, 133]
    names = ("read_image", "read_history", "read_gbuffer")
    twin = split(scene3, W, H, "reuse", cuts, frame_color=True)
    want = []
    for _ in range(3):
        frame(None, twin)
        want.append([gathered(twin, n) for n in names])
    close(*twin)
    first = None
    for K in (1, 2, 3):
        bands = split(scene3, W, H, "reuse", cuts, frame_color=True)
        for _ in range(K):
            frame(None, bands)
            Renderer.denoise_bands(bands, temporal=temporal)
        for n, w in zip(names, want[K - 1]):
            same(gathered(bands, n), w, f"after {K} frames: {n}")
        if K == 1:
            first = gathered(bands, "read_denoised")
            assert (first[..., :3] != want[0][0][..., :3]).any()
        close(*bands)
    bands = split(scene3, W, H, "reuse", cuts, frame_color=True)
    frame(None, bands)
    Renderer.denoise_bands(bands, temporal=temporal)
    frame(None, bands)
    frame(None, bands)
    same(gathered(bands, "read_denoised"), first, "frame 1's denoised image behind frames 2 and 3")
    for n, w in zip(names, want[2]):
        same(gathered(bands, n), w, f"frames 2 and 3 behind the call: {n}")
    close(*bands)


# ------------------------------------------------------------------ temporal mode
def test_temporal_without_clips_equals_one_handle(scene3):
    """Four temporal calls, the camera yawing 1.5 degrees and the frame count restarting before each:
    denoised image and history equal the whole-image temporal handle's, no band clips, and the
    history is in use."""
    from pathtracerdemo_amd.renderer import Renderer
    W, H = 64, 200
    one = make(scene3, W, H, "reuse", frame_color=True)
    bands = split(scene3, W, H, "reuse", [66, 133], frame_color=True)
    out = np.zeros((H, W, 4), np.float32)
    for call in range(4):
        frame(one, bands, yaw=1.5 * call, reset=True)
        one.Denoise(temporal=True)
        Renderer.denoise_bands(bands, out, temporal=True)
        same(out, one.read_denoised(), f"call {call + 1}: denoised")
        same(gathered(bands, "read_denoise_history"), one.read_denoise_history(), f"call {call + 1}: history")
    assert [b.denoise_clips() for b in bands] == [0, 0, 0]
    hist = one.read_denoise_history()
    hit = hist[..., 3] > 0
    assert hit.any() and hist[hit][:, 3].mean() > 1.5, "the history must be in use"
    close(one, *bands)


def test_temporal_clip_rule(scene1):
    """72x80 as bands of 17, 33 and 30 rows, 1 iteration: a band's state covers 4 halo rows.  After a
    12 degree pitch some history lies further away: those candidates are not taken, the pixels are
    counted, and each band's new history equals the restatement's second call with the first call's
    n zeroed outside that band's window.  A still camera never clips (the same-pixel rule)."""
    from pathtracerdemo_amd.renderer import Renderer
    W, H, cuts = 72, 80, [17, 50]
    bounds = [0] + cuts + [H]
    bands = split(scene1, W, H, "restir", cuts, frame_color=True)
    t = T.TemporalDenoiser()

    def guides():
        return D.guides_from_gbuffer(bands[0].uniform, scene1.scene, scene1.geometry, scene1.accel, gathered(bands, "read_gbuffer"))

    frame(None, bands)
    t.denoise(gathered(bands, "read_frame_color"), gathered(bands, "read_image"), guides(), bands[0].uniform, iterations=1)
    Renderer.denoise_bands(bands, iterations=1, temporal=True)
    same(gathered(bands, "read_denoise_history"), t.history, "call 1: history")
    frame(None, bands)  # (a still camera: the history of pixel p is at p)
    t.denoise(gathered(bands, "read_frame_color"), gathered(bands, "read_image"), guides(), bands[0].uniform, iterations=1)
    Renderer.denoise_bands(bands, iterations=1, temporal=True)
    same(gathered(bands, "read_denoise_history"), t.history, "call 2 (still camera): history")
    assert [b.denoise_clips() for b in bands] == [0, 0, 0]
    frame(None, bands, pitch=12.0, reset=True)
    G, F, A = guides(), gathered(bands, "read_frame_color"), gathered(bands, "read_image")
    Renderer.denoise_bands(bands, iterations=1, temporal=True)
    clips = [b.denoise_clips() for b in bands]
    assert max(clips) > 0, clips
    for k, b in enumerate(bands):
        tb = copy.deepcopy(t)
        lo, hi = max(0, bounds[k] - 4), min(H, bounds[k + 1] + 4)
        tb.state.n[:lo] = 0
        tb.state.n[hi:] = 0
        tb.denoise(F, A, G, b.uniform, iterations=1)
        same(b.read_denoise_history(), tb.history[bounds[k]:bounds[k + 1]], f"band {k}: history under the clip rule")
        assert (tb.history[bounds[k]:bounds[k + 1], :, 3] > 1).any()
    close(*bands)


# ------------------------------------------------------------------ refusals
def _bands(cs, rows, pipelines=("restir",) * 3, widths=(72,) * 3, flags=(True,) * 3, render=(True,) * 3):
    out = []
    for (a, b), p, w, fc, rn in zip(rows, pipelines, widths, flags, render):
        r = make(cs, w, 80, p, a, b, frame_color=fc)
        if rn:
            r.Update()
            r.Render()
        out.append(r)
    return out


ROWS = [(0, 17), (17, 50), (50, 80)]
REFUSALS = {
    "size": (dict(widths=(72, 64, 72)), {}, "differs in size or pipeline"),
    "pipeline": (dict(pipelines=("restir", "mcpt", "restir")), {}, "differs in size or pipeline"),
    "gap": (dict(rows=[(0, 17), (20, 50), (50, 80)]), {}, "does not start where"),
    "not_covering": (dict(rows=ROWS[:2]), {}, "cover rows"),
    "mcpt": (dict(pipelines=("mcpt",) * 3), {}, "TEST_MCPT"),
    "not_rendered": (dict(render=(True, True, False)), {}, "nothing rendered"),
    "iterations_7": ({}, dict(iterations=7), "iterations"),
    "sigma_nan": ({}, dict(sigma_lum=float("nan")), "sigma_lum"),
    "sigma_plane_negative": ({}, dict(sigma_plane=-0.5), "sigma_plane"),
    "temporal_2": ({}, dict(temporal=2), "temporal 2"),
    "alpha_above_1": ({}, dict(temporal=True, alpha_min=1.5), "alpha_min"),
    "temporal_without_the_flag": (dict(flags=(True, False, True)), dict(temporal=True), "PTX_FLAG_FRAME_COLOR"),
    "small_band": ({}, dict(iterations=4), r"band 0 has 17 rows.*32 rows"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_leave_the_handles_rendering(scene1, case):
    from pathtracerdemo_amd import _native as native
    from pathtracerdemo_amd.renderer import Renderer
    kw, call, message = REFUSALS[case]
    kw = dict(kw)
    rows = kw.pop("rows", ROWS)
    bands, twins = _bands(scene1, rows, **kw), _bands(scene1, rows, **kw)
    with pytest.raises(native.PtxError, match=message):
        Renderer.denoise_bands(bands, **dict(dict(iterations=1), **call))
    for b in bands:
        with pytest.raises(native.PtxError):
            b.read_denoised()  # (refused before anything was allocated)
    for r in bands + twins:
        r.Update()
        r.Render()
    same(gathered([b for b in bands if b.width == 72], "read_image"),
         gathered([b for b in twins if b.width == 72], "read_image"), "the next frame")
    if case in ("iterations_7", "sigma_nan", "temporal_2", "small_band", "not_rendered"):  # and now the call goes through
        Renderer.denoise_bands(bands, iterations=1)
        assert np.isfinite(gathered(bands, "read_denoised")).all()
    close(*bands, *twins)


# ------------------------------------------------------------------ communicators
def test_loopback_communicator_bands_denoise():
    """tests/loopback_denoise_bands.py in a child process (the communicator library is chosen once
    per process): three bands of 64x200 over the loopback communicator, as three rank-form calls
    from three host threads and through the n = 3 branch; spatial and two temporal calls each."""
    assert os.path.exists(STUB), "build it: make -C tests/loopback (or __graft_entry__.build())"
    env = dict(os.environ, PTX_RCCL_LIB=STUB, LOOPBACK_TIMEOUT_MS="3000", PTX_AB="COMM_TIMEOUT_S=10")
    p = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "loopback_denoise_bands.py")], env=env,
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert [c["form"] for c in out["calls"]] == ["rank"] * 3 + ["bands"] * 3
    assert [c["temporal"] for c in out["calls"]] == [False, True, True] * 2
    for c in out["calls"]:
        assert c["denoised"] == 0 and c["history"] == 0, c
        assert all(g > 0 for g in c["halo_bytes_grew"]), c
    assert out["clips"] == [0, 0, 0] and out["mean_n"] > 1.5
    assert out["refused_small_band"]
