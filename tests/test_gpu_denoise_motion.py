"""Object motion in the temporal denoiser on the GPU (dn_temporal<true> of
pathtracerdemo_amd/csrc/ptx_denoise.hip) against the numpy restatement (tests/denoise_motion_ref.py),
bit for bit: a chair moved, turned under a camera yaw and rescaled between temporal Denoise calls, a
light edit that leaves the lookup alone, the unchanged path without edits, two bands, and the temporal
upsampler, which does not follow objects and starts over after an instance edit."""
import numpy as np
import pytest

import denoise_motion_ref as M
import denoise_ref as D
import denoise_temporal_ref as T
import scene_edits as E

pytestmark = pytest.mark.gpu
W, H = 96, 72


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make(cs=None, w=W, h=H, **kw):
    from pathtracerdemo_amd.renderer import Renderer
    r = Renderer(w, h, device=0, pipeline="reuse", frame_color=True, **kw)
    r.Initialize(cs or E.base())
    return r


_guides = {}


def guides_of(r):
    cs, gb = r.compiled, r.read_gbuffer()
    key = (cs.scene.tobytes(), r.uniform[:23].tobytes(), gb.tobytes())
    if key not in _guides:
        _guides[key] = D.guides_from_gbuffer(r.uniform, cs.scene, cs.geometry, cs.accel, gb)
    return _guides[key]


def step(r, scene=None, yaw=None):
    mask = r.UpdateScene(E.compose(**scene)) if scene is not None else 0
    if yaw is not None:
        r.GetCamera().set_yaw(yaw)
    if mask or yaw is not None:
        r.ResetFrameCount()  # (as the engine does on a camera move)
    r.Update()
    r.Render()
    return mask


def check_call(r, t, what, **params):
    """One temporal Denoise on the handle and in the restatement, fed what the handle holds."""
    G = guides_of(r)
    kw = dict(insts=E.instance_block(r.compiled)) if isinstance(t, M.MotionDenoiser) else {}
    want = t.denoise(r.read_frame_color(), r.read_image(), G, r.uniform, **kw, **params)
    r.Denoise(temporal=True, **params)
    for name, got, exp in (("history", r.read_denoise_history(), t.history), ("denoised", r.read_denoised(), want)):
        bad = bits(got) != bits(exp)
        assert not bad.any(), f"{what}: {name}: {int(bad.any(-1).sum())} pixels differ, first at {np.argwhere(bad.any(-1))[:4].tolist()}"
    return G


def chair_of(G):
    return G.hit & (G.key >> np.uint32(16) == E.CHAIR)


#             scene after the step                 yaw    flags of the call
MAIN = [
    ("still",   None,                              None,  None),
    ("still",   None,                              None,  None),
    ("E_move",  dict(chair="move"),                None,  [0, 0, 1]),
    ("E_turn",  dict(chair="turn"),                1.5,   [0, 0, 1]),
    ("still",   None,                              None,  None),
    ("E_scale", dict(chair="scale"),               None,  [0, 0, 2]),
    ("E_light", dict(chair="scale", light=1),      None,  None),
]


def test_main_sequence_bit_exact_against_the_restatement():
    r, t = make(), M.MotionDenoiser()
    n_before = None
    for f, (what, scene, yaw, flags) in enumerate(MAIN, start=1):
        step(r, scene, yaw)
        G = check_call(r, t, f"call {f} ({what})")
        assert (t.flags.tolist() if t.flags is not None else None) == flags, what
        n, chair, hit = t.history[..., 3], chair_of(G), G.hit
        assert chair.sum() > 100
        if what in ("E_move", "E_turn"):
            assert (n[chair] > 1).any(), f"{what}: no chair pixel found its history"
            assert (t.taps[chair] >= 1).sum() >= 0.45 * chair.sum()
        if what == "E_scale":
            assert (n[chair] == 1).all() and (n[hit & ~chair] > 1).any()
        if what == "E_light":  # the same camera, no instance differs: every hit pixel's history grows
            assert t.same_pixel and (n[hit] == np.minimum(n_before[hit] + 1, 255)).all()
        n_before = n
    r.close()


def test_without_edits_the_unchanged_kernel_runs():
    """Still and moved cameras and a light edit, no instance edit: the bits are TemporalDenoiser's, and
    every temporal call launches what it launched before (guide, dn_temporal, variance, iterations)."""
    from pathtracerdemo_amd import _native as native
    r, t = make(), T.TemporalDenoiser()
    for f, (scene, yaw) in enumerate([(None, None), (None, None), (None, 1.5), (dict(light=1), None), (None, 3.0)], start=1):
        step(r, scene, yaw)
        before = r.stats()["kernel_launches"][native.PTX_STAT_DENOISE]
        check_call(r, t, f"call {f}", iterations=2)
        assert r.stats()["kernel_launches"][native.PTX_STAT_DENOISE] - before == 3 + 2
    assert (t.history[..., 3] > 2).any()
    r.close()


def test_an_edited_call_launches_no_more():
    from pathtracerdemo_amd import _native as native
    r = make()
    for scene in (None, dict(chair="move")):
        step(r, scene)
        before = r.stats()["kernel_launches"][native.PTX_STAT_DENOISE]
        r.Denoise(temporal=True, iterations=2)
        assert r.stats()["kernel_launches"][native.PTX_STAT_DENOISE] - before == 3 + 2
    r.close()


def test_two_bands_equal_the_whole_image():
    from pathtracerdemo_amd.renderer import Renderer
    one = make()
    bands = [make(row_begin=a, row_end=b) for a, b in ((0, 40), (40, H))]
    for f, scene in enumerate((None, None, dict(chair="move"), None), start=1):
        step(one, scene)
        one.Denoise(temporal=True, iterations=3)
        for x in bands:
            if scene is not None:
                x.UpdateScene(E.compose(**scene))
                x.ResetFrameCount()
            x.Update()
        Renderer.render_bands(bands)
        out = np.zeros((H, W, 4), np.float32)
        Renderer.denoise_bands(bands, out, temporal=True, iterations=3)
        assert sum(x.denoise_clips() for x in bands) == 0
        np.testing.assert_array_equal(bits(np.concatenate([x.read_denoise_history() for x in bands])),
                                      bits(one.read_denoise_history()), f"history, call {f}")
        np.testing.assert_array_equal(bits(out), bits(one.read_denoised()), f"denoised, call {f}")
    G = guides_of(one)
    assert (one.read_denoise_history()[..., 3][chair_of(G)] > 2).any()  # the chair kept its history over the move
    for x in [one] + bands:
        x.close()


def test_temporal_upsampler_starts_over_after_an_instance_edit_only():
    """An UpsampleTemporal pair: E_light on both leaves hi's history growing; E_move on hi makes its next
    call a first call (n <= 1 everywhere)."""
    s = 2
    hi, lo = make(w=W, h=H), make(w=W // s, h=H // s)

    def call(phase):
        px, py = phase % s, phase // s % s
        hi.Update()
        hi.run_pass(0)  # PTX_PASS_GBUFFER: the full-size guides
        lo.set_phase_of(hi, s, px, py)
        lo.Render()
        lo.Denoise(temporal=True, iterations=2)
        hi.UpsampleTemporal(lo, px, py)
        return hi.read_upsample_history()[..., 3]

    for k in range(5):
        n = call(k)
    assert n.max() >= 2
    for x in (hi, lo):
        assert x.UpdateScene(E.compose(light=1)) == 4
    n2 = call(5)
    assert n2.max() >= n.max() and (n2 > 1).any(), "a light edit must keep the upsampler's history"
    for x in (hi, lo):
        assert x.UpdateScene(E.compose(chair="move", light=1)) == 1
    n3 = call(6)
    assert n3.max() <= 1, "an instance edit must drop the upsampler's history"
    for k in range(7, 11):  # (phase (0, 1) of call 6 comes round again at call 10)
        n4 = call(k)
    assert n4.max() >= 2, "the history builds again"
    hi.close()
    lo.close()


def test_denoise_and_upsample_wait_for_a_frame_after_an_instance_or_material_edit():
    """Between an instance or material edit and the next frame the G-buffer on the handle is the old
    tables': the denoiser and the upsamplers refuse; a light edit changes nothing of that."""
    from pathtracerdemo_amd import _native as native
    s = 2
    hi, lo = make(w=W, h=H), make(w=W // s, h=H // s)
    hi.Update()
    hi.run_pass(native.PTX_PASS_GBUFFER)
    lo.set_phase_of(hi, s, 0, 0)
    lo.Render()
    lo.Denoise(temporal=True, iterations=2)
    hi.UpsampleTemporal(lo, 0, 0)
    for x in (hi, lo):
        assert x.UpdateScene(E.compose(light=1)) == 4
    lo.Denoise(temporal=True, iterations=2)
    hi.UpsampleTemporal(lo, 0, 0)
    for scene, mask in ((dict(chair="move", light=1), 1), (dict(chair="move", light=1, mat=True), 2)):
        for x in (hi, lo):
            assert x.UpdateScene(E.compose(**scene)) == mask
        for call in (lambda: lo.Denoise(temporal=True), lambda: lo.Denoise(), lambda: hi.UpsampleTemporal(lo, 0, 0),
                     lambda: hi.Upsample(lo)):
            with pytest.raises(native.PtxError):
                call()
        hi.Update()
        hi.run_pass(native.PTX_PASS_GBUFFER)
        lo.set_phase_of(hi, s, 0, 0)
        with pytest.raises(native.PtxError):  # (lo has not rendered yet)
            lo.Denoise(temporal=True, iterations=2)
        lo.Render()
        lo.Denoise(temporal=True, iterations=2)
        hi.UpsampleTemporal(lo, 0, 0)
    assert np.isfinite(hi.read_denoised()).all()
    hi.close()
    lo.close()
