"""PTX_FLAG_FRAME_COLOR and ptx_denoise's temporal mode on the GPU (dn_temporal and
dn_variance<true> of pathtracerdemo_amd/csrc/ptx_denoise.hip) against the numpy restatement
(tests/denoise_temporal_ref.py), bit for bit: the frame-colour tap in every pipeline, camera
sequences that take every path of the history lookup, images smaller than the filter's reach, the
order behind pipelined frames, that nothing else changes, the resets, the spatial call on the same
handle, the refusals, the statistics and the render pass."""
import ctypes

import numpy as np
import pytest

import denoise_ref as D
import denoise_temporal_ref as T

pytestmark = pytest.mark.gpu
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make(pipeline, W, H, cs, frames=0, frame_color=True, **kw):
    from pathtracerdemo_amd.renderer import Renderer
    r = Renderer(W, H, device=0, pipeline=pipeline, frame_color=frame_color, **kw)
    r.Initialize(cs)
    for _ in range(frames):
        r.Update()
        r.Render()
    return r


_guides = {}


def guides_of(r, cs):
    """The restatement's guides of the frame last rendered (computed once per distinct frame: the
    sequences below render the same frames for every parameter set)."""
    gb = r.read_gbuffer()
    key = (id(cs), r.uniform[:23].tobytes(), gb.tobytes())
    if key not in _guides:
        _guides[key] = D.guides_from_gbuffer(r.uniform, cs.scene, cs.geometry, cs.accel, gb)
    return _guides[key]


def step(r, yaw=None, reset=False):
    if yaw is not None:
        r.GetCamera().set_yaw(yaw)
    if reset:
        r.ResetFrameCount()  # (the engine does on every camera move)
    r.Update()
    r.Render()


def check_call(r, t, cs, what, **params):
    """One temporal Denoise on the handle and in the restatement, fed what the handle holds."""
    G = guides_of(r, cs)
    want = t.denoise(r.read_frame_color(), r.read_image(), G, r.uniform, **params)
    r.Denoise(temporal=True, **params)
    for name, got, exp in (("history", r.read_denoise_history(), t.history), ("denoised", r.read_denoised(), want)):
        bad = bits(got) != bits(exp)
        assert not bad.any(), f"{what}: {name}: {int(bad.any(-1).sum())} pixels differ, first at {np.argwhere(bad.any(-1))[:4].tolist()}"
    return G


# ------------------------------------------------------------------ the tap
@pytest.mark.parametrize("W,H", [(70, 45), (24, 17)])
@pytest.mark.parametrize("pipeline", ["restir", "reuse", "gi", "mcpt"])
def test_frame_color_is_what_the_accumulation_mixed_in(scene3, pipeline, W, H):
    """Frames 1..4: mixf(previous accumulation, frame colour, 1 / (F + 1)) is the new accumulation bit
    for bit (at every pixel with a primary hit; TEST_MCPT: at every pixel); a twin without the flag
    holds the same accumulation, reservoirs and G-buffer and W * H * 16 bytes less."""
    r, twin = make(pipeline, W, H, scene3), make(pipeline, W, H, scene3, frame_color=False)
    prev = r.read_image()
    assert (prev == 0).all()
    for f in range(1, 5):
        for x in (r, twin):
            step(x)
        acc, c, gb = r.read_image(), r.read_frame_color(), r.read_gbuffer()
        t = f32(1) / f32(f + 1)
        want = prev[..., :3] * (f32(1) - t) + c[..., :3] * t
        hit = np.ones((H, W), bool) if pipeline == "mcpt" else gb[..., 0] >> 31 == 1
        assert hit.any() and (pipeline == "mcpt" or not hit.all())
        np.testing.assert_array_equal(bits(acc[..., :3][hit]), bits(want[hit]), f"frame {f}")
        assert (c[hit][:, 3] == 1).all() and (c[hit][:, :3] != acc[hit][:, :3]).any()
        names = ["read_image", "read_gbuffer", "read_reservoir"] + (["read_history"] if pipeline in ("reuse", "gi") else [])
        for name in names:
            np.testing.assert_array_equal(bits(getattr(r, name)()), bits(getattr(twin, name)()), f"frame {f}: {name}")
        prev = acc
    assert r.stats()["device_bytes"] - twin.stats()["device_bytes"] == W * H * 16
    from pathtracerdemo_amd import _native as native
    with pytest.raises(native.PtxError):
        twin.read_frame_color()
    r.close()
    twin.close()


# ------------------------------------------------------------------ bit-exact sequences
YAW = 1.5
#        yaw, ResetFrameCount first
SEQUENCE = [(0.0, False), (0.0, False), (YAW, True), (2 * YAW, True), (3 * YAW, True), (3 * YAW, False),
            (150.0, True), (150.0, False)]


@pytest.mark.parametrize("params", [{}, dict(alpha_min=0.2)], ids=["defaults", "alpha_min0.2"])
@pytest.mark.parametrize("iterations", [1, 5, 6])
@pytest.mark.parametrize("pipeline,scene,W,H", [("reuse", "scene3", 96, 72), ("restir", "scene1", 70, 45),
                                                ("gi", "scene3", 48, 32)])
def test_sequence_bit_exact_against_the_restatement(request, pipeline, scene, W, H, iterations, params):
    """Eight frames -- two still, three with a small yaw (ResetFrameCount before each, as the engine
    does), one still, a jump to a camera that sees mostly other surfaces, one still -- with a temporal
    Denoise after each: the denoised image and the history equal the restatement's after every call."""
    cs = request.getfixturevalue(scene)
    r, t = make(pipeline, W, H, cs), T.TemporalDenoiser()
    seen = dict(same=0, partial=0, mixed_history=0, mixed_n=0, misses=0)
    for f, (yaw, reset) in enumerate(SEQUENCE, start=1):
        step(r, yaw, reset)
        G = check_call(r, t, cs, f"frame {f}", iterations=iterations, **params)
        n, hit = t.history[..., 3], G.hit
        assert t.same_pixel == (f in (2, 6, 8))
        seen["same"] += t.same_pixel
        seen["partial"] += (not t.same_pixel) and bool(((t.taps >= 1) & (t.taps <= 3)).any())
        seen["mixed_history"] += bool((n[hit] == 1).any() and (n[hit] > 1).any())
        seen["mixed_n"] += bool((n[hit] >= 4).any() and ((n[hit] < 4)).any())
        seen["misses"] += bool((~hit).any())
    assert all(seen.values()), seen
    r.close()


@pytest.mark.parametrize("W,H", [(24, 17), (8, 8)])
def test_images_smaller_than_the_filters_reach(scene1, W, H):
    r, t = make("restir", W, H, scene1), T.TemporalDenoiser()
    for f, yaw in enumerate((0.0, 2.0, 4.0), start=1):
        step(r, yaw, reset=f > 1)
        G = check_call(r, t, scene1, f"frame {f}")
        assert G.hit.any()
    assert (t.history[..., 3] > 1).any()
    r.close()


# ------------------------------------------------------------------ order, side effects, resets
def test_temporal_denoise_shows_the_frame_it_followed(scene3):
    """Temporal Denoise behind frames 1 and 2, then frames 3 and 4 enqueued at once (the pipelined
    reuse handle runs them on alternating streams): denoised image and history are frame 2's."""
    W, H = 96, 72
    out = []
    for extra in (0, 2):
        r = make("reuse", W, H, scene3)
        for _ in range(2):
            step(r)
            r.Denoise(temporal=True)
        for _ in range(extra):
            step(r)
        out.append((r.read_denoised(), r.read_denoise_history()))
        r.close()
    np.testing.assert_array_equal(bits(out[1][0]), bits(out[0][0]))
    np.testing.assert_array_equal(bits(out[1][1]), bits(out[0][1]))
    assert (out[0][1][..., 3] == 2).any()


def test_nothing_else_changes(scene3):
    """A reuse handle that denoises temporally after each of 3 frames (the camera moves before the
    third) against one that never does: the same accumulation, history reservoirs and G-buffer."""
    a, b = make("reuse", 64, 48, scene3), make("reuse", 64, 48, scene3)
    for f in range(3):
        for r in (a, b):
            step(r, 2.0 if f == 2 else 0.0)
        a.Denoise(temporal=True)
        for name in ("read_image", "read_history", "read_gbuffer", "read_frame_color"):
            np.testing.assert_array_equal(bits(getattr(a, name)()), bits(getattr(b, name)()), f"frame {f + 1}: {name}")
    a.close()
    b.close()


@pytest.mark.parametrize("how", ["reset_accumulation", "upload_scene"])
def test_resets_drop_the_history(scene3, how):
    """After ptx_reset_accumulation or ptx_upload_scene the next temporal call is a fresh handle's
    first: n = 1 and C = the frame's colour at every pixel with a hit."""
    W, H = 48, 32
    r = make("reuse", W, H, scene3)
    for _ in range(2):
        step(r)
        r.Denoise(temporal=True)
    assert (r.read_denoise_history()[..., 3] == 2).any()
    cs = scene3
    if how == "reset_accumulation":
        r.reset_accumulation()
    else:
        r._call("ptx_upload_scene", r._h, cs.scene.ctypes.data, len(cs.scene), cs.geometry.ctypes.data, len(cs.geometry),
                cs.accel.ctypes.data if len(cs.accel) else None, len(cs.accel))
    step(r)  # (the same camera: only the reset can have dropped the history)
    r.Denoise(temporal=True)
    h, c, hit = r.read_denoise_history(), r.read_frame_color(), r.read_gbuffer()[..., 0] >> 31 == 1
    assert hit.any() and (h[hit][:, 3] == 1).all() and (h[~hit][:, 3] == 0).all()
    np.testing.assert_array_equal(bits(h[hit][:, :3]), bits(c[hit][:, :3]))
    # and equal to a fresh handle's first call fed the same frame: the restatement without state
    t = T.TemporalDenoiser()
    want = t.denoise(c, r.read_image(), guides_of(r, cs), r.uniform)
    np.testing.assert_array_equal(bits(r.read_denoised()), bits(want))
    step(r)
    r.Denoise(temporal=True)
    assert (r.read_denoise_history()[hit][:, 3] == 2).all()
    r.close()


def test_spatial_call_on_a_frame_color_handle(scene1):
    """temporal=False is today's filter bit for bit and leaves the history as it was; the temporal
    call after it continues from the call before it."""
    r, t = make("restir", 24, 17, scene1), T.TemporalDenoiser()
    step(r)
    check_call(r, t, scene1, "frame 1")
    step(r, 2.0, reset=True)
    hist = r.read_denoise_history()
    r.Denoise(temporal=False, alpha_min=float("nan"))  # (alpha_min is read in temporal mode only)
    want = D.denoise(r.read_image(), guides_of(r, scene1))
    np.testing.assert_array_equal(bits(r.read_denoised()), bits(want))
    np.testing.assert_array_equal(bits(r.read_denoise_history()), bits(hist))
    check_call(r, t, scene1, "frame 2")
    assert (t.history[..., 3] == 2).any()
    r.close()


# ------------------------------------------------------------------ refusals
REFUSALS = {
    "no_flag": (dict(pipeline="reuse", frame_color=False), dict(temporal=True)),
    "alpha_nan": (dict(pipeline="reuse"), dict(temporal=True, alpha_min=float("nan"))),
    "alpha_negative": (dict(pipeline="reuse"), dict(temporal=True, alpha_min=-0.25)),
    "alpha_above_1": (dict(pipeline="reuse"), dict(temporal=True, alpha_min=1.5)),
    "temporal_2": (dict(pipeline="reuse"), dict(temporal=2)),
    "band": (dict(pipeline="restir", row_begin=16, row_end=48), dict(temporal=True)),
    "mcpt": (dict(pipeline="mcpt"), dict(temporal=True)),
    "before_any_render": (dict(pipeline="reuse"), dict(temporal=True)),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_leave_the_handle_rendering(scene3, case):
    from pathtracerdemo_amd import _native as native
    kw, call = REFUSALS[case]
    first = 0 if case == "before_any_render" else 1
    r, twin = make(W=64, H=48, cs=scene3, frames=first, **kw), make(W=64, H=48, cs=scene3, frames=first, **kw)
    with pytest.raises(native.PtxError):
        r.Denoise(**call)
    with pytest.raises(native.PtxError):
        r.read_denoise_history()
    for x in (r, twin):
        step(x)
    np.testing.assert_array_equal(bits(r.read_image()), bits(twin.read_image()))
    if kw.get("frame_color", True):
        np.testing.assert_array_equal(bits(r.read_frame_color()), bits(twin.read_frame_color()))
    if case in ("before_any_render", "temporal_2", "alpha_nan"):  # and now the call goes through
        r.Denoise(temporal=True)
        assert np.isfinite(r.read_denoised()).all() and (r.read_denoise_history()[..., 3] == 1).any()
    r.close()
    twin.close()


def test_the_new_buffers_are_read_only(scene1):
    from pathtracerdemo_amd import _native as native
    r = make("restir", 24, 17, scene1, 1)
    r.Denoise(temporal=True)
    c, h = r.read_frame_color(), r.read_denoise_history()
    for which, arr in ((native.PTX_BUF_FRAME_COLOR, c), (native.PTX_BUF_DENOISE_HISTORY, h)):
        with pytest.raises(native.PtxError):
            r.write_buffer(which, np.zeros_like(arr))
        ptr, nbytes = ctypes.c_void_p(), ctypes.c_size_t()
        r._call("ptx_device_pointer", r._h, which, ctypes.byref(ptr), ctypes.byref(nbytes))
        assert ptr.value and nbytes.value == 24 * 17 * 16
    np.testing.assert_array_equal(bits(r.read_frame_color()), bits(c))
    np.testing.assert_array_equal(bits(r.read_denoise_history()), bits(h))
    r.close()


# ------------------------------------------------------------------ statistics, present
@pytest.mark.parametrize("timed", [False, True])
def test_stats_count_the_temporal_calls_launches(scene1, timed):
    from pathtracerdemo_amd import _native as native
    W, H = 70, 45
    r = make("restir", W, H, scene1, 1, time_launches=timed)
    before = r.stats()
    r.Denoise(iterations=4, temporal=True)
    r.synchronize()
    s = r.stats()
    assert s["kernel_launches"][native.PTX_STAT_DENOISE] == 3 + 4  # guide, dn_temporal, variance, 4 iterations
    assert (s["kernel_ms_total"][native.PTX_STAT_DENOISE] > 0) == timed
    # the spatial filter's 64 bytes per pixel and the temporal state's 80: guide records, 2 x (history + moments)
    assert s["device_bytes"] - before["device_bytes"] == W * H * (64 + 80)
    step(r)
    r.Denoise(iterations=4, temporal=True)
    r.synchronize()
    s2 = r.stats()
    assert s2["device_bytes"] == s["device_bytes"]
    assert s2["kernel_launches"][native.PTX_STAT_DENOISE] == 2 * (3 + 4)
    r.close()


def test_present_shows_the_temporal_result(scene1, oracle_mod):
    r = make("restir", 70, 45, scene1)
    for yaw in (0.0, 0.0, 2.0):
        step(r, yaw, reset=yaw > 0)
        r.Denoise(temporal=True)
    den = r.read_denoised()
    assert (den != r.read_image()).any()
    r.set_present_source("denoised")
    for cw, ch, bgra in [(70, 45, False), (200, 150, True)]:
        np.testing.assert_array_equal(r.Present(cw, ch, bgra=bgra), oracle_mod.present(den, cw, ch, bgra))
    r.close()
