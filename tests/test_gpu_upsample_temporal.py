"""ptx_upsample_temporal on the GPU (dn_upsample_temporal in pathtracerdemo_amd/csrc/ptx_denoise.hip)
against its numpy restatement (tests/upsample_temporal_ref.py), bit for bit in PTX_BUF_DENOISED and
PTX_BUF_UPSAMPLE_HISTORY: every scale, image sizes whose tiles are cut at both edges, s^2 + 1 calls
that cycle the phases under a camera at rest and then one yaw, a small handle denoised spatially and
temporally; that the state lives as long as include/ptx.h says, that the call changes nothing else, is
ordered against the small handle's later work, feeds the render pass, and is refused where it is not
defined.

The reference is computed from what the handles hold: the small handle's denoised image and G-buffer,
the full-size handle's G-buffer and uniform."""
import ctypes

import numpy as np
import pytest

import denoise_ref as D
import upsample_temporal_ref as UT

pytestmark = pytest.mark.gpu


def cycle(s):
    """s^2 + 1 phases: every phase once (the diagonal first), then the first again."""
    ph = [(px, py) for py in range(s) for px in range(s)]
    ph = sorted(ph, key=lambda p: (p[0] != p[1], p))
    return ph + ph[:1]


def make_hi(W, H, cs, pipeline="restir", **kw):
    from pathtracerdemo_amd import _native as N
    from pathtracerdemo_amd.renderer import Renderer
    hi = Renderer(W, H, device=0, pipeline=pipeline, **kw)
    hi.Initialize(cs)
    hi.Update()
    hi.run_pass(N.PTX_PASS_GBUFFER)
    return hi


def make_lo(w, h, cs, pipeline="restir", **kw):
    from pathtracerdemo_amd.renderer import Renderer
    lo = Renderer(w, h, device=0, pipeline=pipeline, **kw)
    lo.Initialize(cs)
    return lo


def frame(lo, hi, s, px, py, temporal=False):
    """One small frame through phase (px, py) of hi's current frame, denoised."""
    lo.set_phase_of(hi, s, px, py)
    lo.Render()
    lo.Denoise(temporal=temporal)


def guides_of(r, cs, sigma_plane=0.0):
    return D.guides_from_gbuffer(r.uniform, cs.scene, cs.geometry, cs.accel, r.read_gbuffer(), sigma_plane or D.DEFAULT_SIGMA_PLANE)


def bits_equal(got, want, what=""):
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.any(-1).sum())} pixels differ, first at {np.argwhere(bad.any(-1))[:4].tolist()}"


def check_call(hi, t, want, what):
    bits_equal(hi.read_denoised(), want, what + ": PTX_BUF_DENOISED")
    bits_equal(hi.read_upsample_history(), t.history, what + ": PTX_BUF_UPSAMPLE_HISTORY")


CASES = [  # s, lo size, pipeline, scene, lo's denoise temporal, sigma_plane, alpha_min, alpha_fill
    (2, 12, 8, "restir", "scene3", False, 0.0, 0.0, -1.0),
    (2, 11, 7, "reuse", "scene3", True, 0.005, 0.0, 0.0),
    (3, 12, 8, "reuse", "scene3", True, 0.0, 0.5, 0.3),
    (3, 11, 7, "restir", "scene1", False, 0.005, 0.0, 0.0),
    (4, 12, 8, "gi", "scene3", False, 0.0, 0.0, 0.0),
    (4, 11, 7, "restir", "scene3", False, 0.005, 0.0, 0.3),
    (2, 2, 2, "restir", "scene3", False, 0.0, 0.0, -1.0),  # the 4 x 4 full-size image: smaller than a tile
]


@pytest.mark.parametrize("s,w,h,pipeline,scene,temporal,sigma_plane,alpha_min,alpha_fill", CASES)
def test_bit_exact_against_the_restatement(request, s, w, h, pipeline, scene, temporal, sigma_plane, alpha_min, alpha_fill):
    from pathtracerdemo_amd import _native as N
    cs = request.getfixturevalue(scene)
    hi = make_hi(s * w, s * h, cs)
    lo = make_lo(w, h, cs, pipeline, frame_color=temporal)
    t = UT.TemporalUpsampler()
    G_hi = guides_of(hi, cs, sigma_plane)
    cases = set()
    phases = cycle(s)
    for k, (px, py) in enumerate(phases):
        if k == len(phases) - 1:  # one yaw: the reprojecting branch
            hi.camera.set_yaw(1.5)
            hi.Update()
            hi.run_pass(N.PTX_PASS_GBUFFER)
            G_hi = guides_of(hi, cs, sigma_plane)
        frame(lo, hi, s, px, py, temporal)
        hi.UpsampleTemporal(lo, px, py, sigma_plane=sigma_plane, alpha_min=alpha_min, alpha_fill=alpha_fill)
        want = t.upsample(lo.read_denoised(), guides_of(lo, cs), G_hi, hi.uniform, s, px, py, alpha_min, alpha_fill)
        check_call(hi, t, want, f"call {k + 1}, phase ({px}, {py})")
        assert t.info["same_pixel"] == (0 < k < len(phases) - 1)
        cases |= set(np.unique(t.info["case"]).tolist())
    assert not t.info["same_pixel"] and t.info["have"].any(), "the last call looked its history up through the previous camera"
    assert cases == {0, 1, 2, 3}, cases
    n = t.history[..., 3]
    assert n.max() >= 1 and (hi.read_denoised()[..., 3] == 1).all()
    hi.close()
    lo.close()


def test_a_host_written_gbuffer_reaches_every_branch(scene3):
    """The full-size G-buffer rewritten by the host after its pass: texels permuted among pixels (other
    keys and misses where lo sees something else) and one column given a far texel (a feature one pixel
    wide that no small pixel owns).  Stages 2 and 3 and "on the phase's grid, key differs" are all reached."""
    from pathtracerdemo_amd import _native as N
    s, w, h = 3, 12, 8
    hi = make_hi(s * w, s * h, scene3)
    lo = make_lo(w, h, scene3)
    rng = np.random.default_rng(3)
    g = hi.read_gbuffer().reshape(-1, 4).copy()
    idx = rng.choice(len(g), 120, replace=False)
    g[idx] = g[np.roll(idx, 1)]
    g = g.reshape(s * h, s * w, 4)
    g[:, 7] = g[s * h - 1, s * w - 1]
    g[2:5, 20:23] = 0  # misses
    hi.write_buffer(N.PTX_BUF_GBUFFER, g)
    G_hi = guides_of(hi, scene3)
    t = UT.TemporalUpsampler()
    stages, off_key = set(), False
    for k, (px, py) in enumerate(cycle(s)[:4]):
        frame(lo, hi, s, px, py)
        hi.UpsampleTemporal(lo, px, py, alpha_fill=0.3)
        want = t.upsample(lo.read_denoised(), guides_of(lo, scene3), G_hi, hi.uniform, s, px, py, alpha_fill=0.3)
        check_call(hi, t, want, f"call {k + 1}")
        stages |= set(np.unique(t.info["stage"]).tolist())
        off_key |= bool((t.info["grid"] & ~t.info["sampled"]).any())
    assert stages == {1, 2, 3} and off_key, (stages, off_key)
    assert not G_hi.hit.all() and len(np.unique(G_hi.key)) > 2
    np.testing.assert_array_equal(hi.read_gbuffer(), g)
    hi.close()
    lo.close()


DROPS = ["upload", "reset", "upsample", "upsample_bands", "denoise", "denoise_bands"]


@pytest.mark.parametrize("drop", DROPS + ["set_frame"])
def test_state_lifetime(scene3, drop):
    """Each of the listed calls on the full-size handle drops the state: the next call equals a first call.
    ptx_set_frame alone (another frame index) does not.  s = 3 at the centred phase, whose small camera is
    the full-size one: the same small handle also serves ptx_upsample."""
    from pathtracerdemo_amd import _native as N
    from pathtracerdemo_amd.renderer import Renderer
    s, w, h, px, py = 3, 8, 6, 1, 1
    hi = make_hi(s * w, s * h, scene3)
    lo = make_lo(w, h, scene3)
    frame(lo, hi, s, px, py)
    hi.UpsampleTemporal(lo, px, py)
    first, first_hist = hi.read_denoised(), hi.read_upsample_history()
    assert set(np.unique(first_hist[..., 3])) == {0.0, 1.0}
    u = hi.uniform.copy()
    if drop == "upload":
        hi.Initialize(scene3)
        hi.set_uniform(u)
        hi.run_pass(N.PTX_PASS_GBUFFER)
    elif drop == "reset":
        hi.reset_accumulation()
    elif drop == "upsample":
        hi.Upsample(lo)
    elif drop == "upsample_bands":
        Renderer.upsample_bands([hi], [lo])
    elif drop == "denoise":
        hi.Denoise()
    elif drop == "denoise_bands":
        Renderer.denoise_bands([hi])
    else:
        u[23] += 5
        hi.set_uniform(u)
    hi.UpsampleTemporal(lo, px, py)
    if drop == "set_frame":
        n = hi.read_upsample_history()[..., 3]
        assert (n[first_hist[..., 3] == 1] == 2).all() and (n[first_hist[..., 3] == 0] == 0).all()
    else:
        bits_equal(hi.read_denoised(), first, drop)
        bits_equal(hi.read_upsample_history(), first_hist, drop)
    hi.close()
    lo.close()


@pytest.mark.parametrize("timed", [False, True])
def test_nothing_else_changes(scene3, timed):
    """Across a call: lo's accumulation, G-buffer, reservoirs, history reservoirs, denoiser state and output
    and hi's G-buffer and accumulation keep their bits; two launches; once, 112 bytes per full-size pixel
    (the output and two sets of guide records and history)."""
    from pathtracerdemo_amd import _native as N
    s, w, h = 2, 11, 7
    hi = make_hi(s * w, s * h, scene3, time_launches=timed)
    lo = make_lo(w, h, scene3, "reuse", frame_color=True)
    names_lo = ("read_image", "read_gbuffer", "read_reservoir", "read_history", "read_denoise_history", "read_denoised",
                "read_frame_color")
    for k, (px, py) in enumerate(cycle(s)[:3]):
        frame(lo, hi, s, px, py, temporal=True)
        kept = [(r, name, getattr(r, name)()) for r, names in ((lo, names_lo), (hi, ("read_gbuffer", "read_image"))) for name in names]
        before = hi.stats()
        hi.UpsampleTemporal(lo, px, py)
        hi.synchronize()
        after = hi.stats()
        for r, name, want in kept:
            np.testing.assert_array_equal(getattr(r, name)().view(np.uint32), want.view(np.uint32), f"call {k + 1}: {name}")
        assert after["kernel_launches"][N.PTX_STAT_DENOISE] - before["kernel_launches"][N.PTX_STAT_DENOISE] == 2
        assert (after["kernel_ms_total"][N.PTX_STAT_DENOISE] > before["kernel_ms_total"][N.PTX_STAT_DENOISE]) == timed
        assert after["device_bytes"] - before["device_bytes"] == (hi.width * hi.height * 112 if k == 0 else 0)
    hi.close()
    lo.close()


def test_the_small_handles_next_work_waits(scene3):
    """Denoise(), UpsampleTemporal(), then at once two more frames and a Denoise() of the (pipelined) small
    handle, no synchronize; and Denoise(), a frame, UpsampleTemporal(), Denoise(): the full-size image is
    made of the denoise the call followed."""
    s, w, h = 3, 12, 8
    hi = make_hi(s * w, s * h, scene3)
    G_hi = guides_of(hi, scene3)
    twin, lo = make_lo(w, h, scene3, "reuse"), make_lo(w, h, scene3, "reuse")
    t = UT.TemporalUpsampler()
    # the twin runs the same frames and is read at every step
    frame(twin, hi, s, 0, 0)
    den0, G0 = twin.read_denoised(), guides_of(twin, scene3)
    frame(lo, hi, s, 0, 0)
    hi.UpsampleTemporal(lo, 0, 0)
    for _ in range(2):
        lo.Render()
    lo.Denoise()
    check_call(hi, t, t.upsample(den0, G0, G_hi, hi.uniform, s, 0, 0), "frames behind the call")
    assert (lo.read_denoised() != den0).any()
    # a frame between the denoise and the call: the pipelined handle has moved to its next context's stream
    frame(lo, hi, s, 2, 1)
    den1, G1 = lo.read_denoised(), guides_of(lo, scene3)
    lo.synchronize(), hi.synchronize()
    lo.Denoise()  # (the same image again, enqueued)
    lo.Render()
    hi.UpsampleTemporal(lo, 2, 1)
    lo.Denoise()
    lo.Render()
    lo.Denoise()
    check_call(hi, t, t.upsample(den1, G1, G_hi, hi.uniform, s, 2, 1), "a frame between the denoise and the call")
    for r in (hi, lo, twin):
        r.close()


def test_present_shows_the_result(scene1, oracle_mod):
    from pathtracerdemo_amd import _native as N
    s = 2
    hi = make_hi(44, 28, scene1)
    lo = make_lo(22, 14, scene1)
    frame(lo, hi, s, 1, 0)
    with pytest.raises(N.PtxError):
        hi.set_present_source("denoised")  # nothing upsampled yet
    with pytest.raises(N.PtxError):
        hi.read_upsample_history()
    hi.UpsampleTemporal(lo, 1, 0)
    up = hi.read_denoised()
    assert (up[..., 3] == 1).all() and np.isfinite(up).all()
    hi.set_present_source("denoised")
    for cw, ch, bgra in [(44, 28, False), (200, 150, True)]:
        np.testing.assert_array_equal(hi.Present(cw, ch, bgra=bgra), oracle_mod.present(up, cw, ch, bgra))
    # and the result is no source of a plain upsample
    big = make_hi(88, 56, scene1)
    with pytest.raises(N.PtxError) as e:
        big.Upsample(hi)
    assert "ptx_upsample_temporal's output" in str(e.value)
    for r in (big, hi, lo):
        r.close()


def test_refusals(scene1, scene3):
    """Every refusal returns PTX_E_INVALID with its message before any GPU work: PTX_STAT_DENOISE and the
    buffers of both handles stay as they were."""
    from pathtracerdemo_amd import _native as N
    from pathtracerdemo_amd.renderer import Renderer
    lib = N.load()
    s, w, h = 2, 12, 8
    hi = make_hi(s * w, s * h, scene3)
    lo = make_lo(w, h, scene3)
    frame(lo, hi, s, 1, 0)
    hi.UpsampleTemporal(lo, 1, 0)
    hi.synchronize()
    kept = [(r, name, getattr(r, name)()) for r in (lo, hi) for name in ("read_image", "read_gbuffer", "read_denoised")]
    kept.append((hi, "read_upsample_history", hi.read_upsample_history()))
    launches = hi.stats()["kernel_launches"][N.PTX_STAT_DENOISE]
    assert lib.ptx_upsample_temporal(None, lo._h, None) == -1 and lib.ptx_upsample_temporal(hi._h, None, None) == -1

    def refused(big, small, needle, px=1, py=0, **kw):
        with pytest.raises(N.PtxError) as e:
            big.UpsampleTemporal(small, px, py, **kw)
        assert "(-1)" in str(e.value) and needle in str(e.value), str(e.value)

    refused(hi, hi, "one handle")
    for bad in (-0.5, float("nan"), float("inf")):
        refused(hi, lo, "sigma_plane", sigma_plane=bad)
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        refused(hi, lo, "alpha_min", alpha_min=bad)
    for bad in (1.5, float("nan"), float("inf"), float("-inf")):
        refused(hi, lo, "alpha_fill", alpha_fill=bad)
    for k in range(3):
        p = N.PtxUpsampleTemporalParams(px=1, py=0, alpha_fill=-1.0)
        p.reserved[k] = 1
        assert lib.ptx_upsample_temporal(hi._h, lo._h, ctypes.byref(p)) == -1 and b"reserved" in lib.ptx_last_error(hi._h)
    refused(hi, lo, "phase", px=2, py=0)
    refused(hi, lo, "phase", px=0, py=2)
    # lo was rendered through phase (1, 0): every other phase, and NULL parameters (phase (0, 0)), name the camera
    for px, py in ((0, 0), (1, 1), (0, 1)):
        refused(hi, lo, "camera", px=px, py=py)
    assert lib.ptx_upsample_temporal(hi._h, lo._h, None) == -1 and b"camera" in lib.ptx_last_error(hi._h)
    # the unshifted uniform at s = 2: ptx_upsample's camera is no phase's
    plain = make_lo(w, h, scene3)
    plain.Update()
    plain.Render()
    plain.Denoise()
    assert (plain.uniform[4:23] == hi.uniform[4:23]).all()
    for px, py in ((0, 0), (1, 0), (0, 1), (1, 1)):
        refused(hi, plain, "camera", px=px, py=py)
    plain.close()

    def other(W, H, cs=scene3, pipeline="restir", gbuffer=True, yaw=0.0, **kw):
        r = Renderer(W, H, device=0, pipeline=pipeline, **kw)
        r.Initialize(cs)
        r.camera.set_yaw(yaw)
        r.Update()
        if gbuffer:
            r.run_pass(N.PTX_PASS_MCPT if pipeline == "mcpt" else N.PTX_PASS_GBUFFER)
        return r

    cases = [(dict(W=2 * w, H=2 * h, row_begin=8, row_end=16), "bands are not supported"), (dict(W=2 * w, H=2 * h, pipeline="mcpt"), "TEST_MCPT"),
             (dict(W=2 * w, H=2 * h, gbuffer=False), "G-buffer"), (dict(W=30, H=20), "times"), (dict(W=5 * w, H=5 * h), "times"),
             (dict(W=2 * w, H=3 * h), "times"), (dict(W=w, H=h), "times"), (dict(W=2 * w, H=2 * h, yaw=2.0), "camera"),
             (dict(W=2 * w, H=2 * h, cs=scene1), "triangles")]
    for kw, needle in cases:
        r = other(**kw)
        refused(r, lo, needle)
        r.close()
    r = Renderer(2 * w, 2 * h, device=0)  # no scene at all
    refused(r, lo, "G-buffer")
    r.close()
    # the small side: a band, TEST_MCPT, nothing denoised
    for kw, needle in [(dict(row_begin=2, row_end=6), "bands are not supported"), (dict(pipeline="mcpt"), "TEST_MCPT"), (dict(), "denoised")]:
        r = make_lo(w, h, scene3, **kw)
        r.set_phase_of(hi, s, 1, 0)
        r.run_pass(N.PTX_PASS_MCPT if kw.get("pipeline") == "mcpt" else N.PTX_PASS_GBUFFER)
        refused(hi, r, needle)
        r.close()
    hi.synchronize()
    assert hi.stats()["kernel_launches"][N.PTX_STAT_DENOISE] == launches
    for r, name, want in kept:
        np.testing.assert_array_equal(getattr(r, name)().view(np.uint32), want.view(np.uint32), name)
    hi.UpsampleTemporal(lo, 1, 0)  # and the pair still works
    assert hi.stats()["kernel_launches"][N.PTX_STAT_DENOISE] == launches + 2
    hi.close()
    lo.close()
