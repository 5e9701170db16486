"""Vertex motion in the temporal denoiser on the GPU (dn_temporal_verts of pathtracerdemo_amd/csrc/ptx_denoise.hip,
ptx_denoise_params.reserved[2]) against the numpy restatement (tests/denoise_follow_ref.py), bit for bit: the
chair posed through its skin, bent, moved and rescaled between temporal Denoise calls (tests/follow_edits.py),
the room bent, two bands, the unchanged default, and what the snapshot costs and when it is dropped."""
import ctypes
import dataclasses

import numpy as np
import pytest

import denoise_follow_ref as F
import denoise_motion_ref as M
import denoise_ref as D
import follow_edits as FE
import scene_edits as E
import skin_edits as S
import vertex_edits as V

pytestmark = pytest.mark.gpu
W, H = 96, 72


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make(w=W, h=H, skin=True, **kw):
    from pathtracerdemo_amd.renderer import Renderer
    r = Renderer(w, h, device=0, pipeline="reuse", frame_color=True, **kw)
    r.Initialize(E.base())
    r.Update()  # (the skin wants a frame set)
    if skin:
        S.set_skin(r, FE.CHAIR_MESH, 3)
    return r


_guides = {}


def guides_of(r):
    cs, gb = r.compiled, r.read_gbuffer()
    key = (cs.scene.tobytes(), cs.geometry.tobytes(), r.uniform[:23].tobytes(), gb.tobytes())
    if key not in _guides:
        _guides[key] = D.guides_from_gbuffer(r.uniform, cs.scene, cs.geometry, cs.accel, gb)
    return _guides[key]


def step(r, calls=(), chair=None, light=0, yaw=None):
    """One frame after the step's vertex calls, scene edit and yaw; returns the meshes deformed."""
    for c in calls:
        FE.apply(r, c)
    mask = 0
    if chair is not None:
        mask = r.UpdateScene(dataclasses.replace(r.compiled, scene=E.compose(chair=chair, light=light).scene))
    if yaw is not None:
        r.GetCamera().set_yaw(yaw)
    if mask or yaw is not None or calls:
        r.ResetFrameCount()  # (as the engine does on a camera move)
    r.Update()
    r.Render()
    return (FE.CHAIR_MESH,) if calls else ()


def check_call(r, t, what, deformed=(), follow=True, **params):
    """One temporal Denoise on the handle and in the restatement, fed what the handle holds."""
    G, cs = guides_of(r), r.compiled
    kw = dict(insts=E.instance_block(cs))
    if isinstance(t, F.FollowDenoiser):
        kw.update(follow=follow, scene=cs.scene, geometry=cs.geometry, accel=cs.accel, gbuffer=r.read_gbuffer(), deformed=deformed)
    want = t.denoise(r.read_frame_color(), r.read_image(), G, r.uniform, **kw, **params)
    denoise(r, follow, **params)
    for name, got, exp in (("history", r.read_denoise_history(), t.history), ("denoised", r.read_denoised(), want)):
        bad = bits(got) != bits(exp)
        assert not bad.any(), f"{what}: {name}: {int(bad.any(-1).sum())} pixels differ, first at {np.argwhere(bad.any(-1))[:4].tolist()}"
    return G


def denoise(r, follow, **params):
    """A temporal Denoise that follows vertices or does not (Renderer.follow_vertices: reserved[2] of the call)."""
    r.follow_vertices = follow
    r.Denoise(temporal=True, **params)


def flags_of(t):
    return t.flags.tolist() if t.flags is not None else None


def test_main_sequence_bit_exact_against_the_restatement():
    """Every step of follow_edits.MAIN, a following Denoise after each: history and output are the restatement's
    bits, the flags are the table's, the posed steps find the chair's history (the share of
    tests/test_denoise_follow_ref.py on the GPU's own G-buffer) and its length grows past 2 across them."""
    r, t = make(), F.FollowDenoiser()
    for f, (what, calls, chair, light, yaw, flags) in enumerate(FE.MAIN, start=1):
        deformed = step(r, calls, chair, light, yaw)
        G = check_call(r, t, f"call {f} ({what})", deformed, iterations=2)
        assert flags_of(t) == flags, what
        n, ch = t.history[..., 3], FE.chair_of(G)
        assert ch.sum() > 100
        if what in FE.POSED:
            share = (t.taps[ch] >= 1).sum() / ch.sum()
            print(f"{what}: {int(ch.sum())} chair pixels, share with a tap {share:.2f}, longest history {n[ch].max():.0f}")
            assert share >= 0.45, what
            assert (n[ch] > 2).any(), f"{what}: no chair pixel kept a history over the poses"
    r.close()


def test_default_is_unchanged():
    """The same sequence without follow_vertices: MotionDenoiser's bits, today's not-following lookup."""
    r, t = make(), M.MotionDenoiser()
    for f, (what, calls, chair, light, yaw, flags) in enumerate(FE.MAIN, start=1):
        step(r, calls, chair, light, yaw)
        check_call(r, t, f"call {f} ({what})", follow=False, iterations=2)
    r.close()


def test_without_a_vertex_update_following_is_the_same_call():
    """Still, a yaw, an instance move: a following handle gives the not-following handle's bits, and both launch
    guide, dn_temporal, variance and the iterations."""
    from pathtracerdemo_amd import _native as native
    a, b = make(), make()
    for f, (chair, yaw) in enumerate([(None, None), (None, None), (None, FE.YAW), ("move", None)], start=1):
        for r, follow in ((a, True), (b, False)):
            step(r, (), chair, 0, yaw)
            before = r.stats()["kernel_launches"][native.PTX_STAT_DENOISE]
            denoise(r, follow, iterations=2)
            assert r.stats()["kernel_launches"][native.PTX_STAT_DENOISE] - before == 3 + 2
        np.testing.assert_array_equal(bits(a.read_denoise_history()), bits(b.read_denoise_history()), f"history, call {f}")
        np.testing.assert_array_equal(bits(a.read_denoised()), bits(b.read_denoised()), f"denoised, call {f}")
    assert (a.read_denoise_history()[..., 3] > 2).any()
    a.close()
    b.close()


def test_snapshot_costs_a_copy_and_one_buffer():
    """An update on a tracking handle launches what it launches on any handle (the save is a copy), a following
    call with a deformed mesh launches 3 + iterations, and device_bytes grows once, by 80 B per triangle."""
    from pathtracerdemo_amd import _native as native
    a, b = make(), make()
    for r in (a, b):
        step(r)
        r.Denoise(temporal=True, iterations=2)
    s0 = a.stats()
    denoise(a, True, iterations=2)
    b.Denoise(temporal=True, iterations=2)
    assert a.stats()["device_bytes"] - s0["device_bytes"] == 80 * s0["triangles"]
    assert b.stats()["device_bytes"] == s0["device_bytes"]
    refit = []
    for r in (a, b):
        before = r.stats()["kernel_launches"][native.PTX_STAT_REFIT]
        step(r, (("pose", FE.POSE_A),))
        refit.append(r.stats()["kernel_launches"][native.PTX_STAT_REFIT] - before)
    assert refit[0] == refit[1] > 0
    s1 = a.stats()
    denoise(a, True, iterations=2)
    assert a.stats()["kernel_launches"][native.PTX_STAT_DENOISE] - s1["kernel_launches"][native.PTX_STAT_DENOISE] == 3 + 2
    grown = a.stats()["device_bytes"]  # (with the table of the first call that finds something changed, as ever)
    for k in range(2):
        step(a, (("pose", FE.POSE_B if k else FE.POSE_HALF),))
        denoise(a, True, iterations=2)
    assert a.stats()["device_bytes"] == grown
    a.close()
    b.close()


def test_room_bent_most_of_the_frame_follows():
    r, t = make(skin=False), F.FollowDenoiser()
    for f in range(2):
        step(r)
        check_call(r, t, f"call {f + 1} (still)", iterations=2)
    r.UpdateVertices(FE.ROOM_MESH, V.bend(FE.ROOM_MESH))
    r.ResetFrameCount()
    r.Update()
    r.Render()
    G = check_call(r, t, "call 3 (room bent)", (FE.ROOM_MESH,), iterations=2)
    pf, _ = t.pixel_flags(G)
    # most of what the frame shows: the room is more than half of the pixels with a primary hit (a third of the
    # frame looks out of the window and has none, so half of W * H is not the room's to reach)
    assert flags_of(t) == [3, 0, 0] and (pf == 3).sum() > 0.5 * G.hit.sum()
    assert (t.history[..., 3][pf == 3] == 3).any()
    r.close()


def test_two_bands_equal_the_whole_image():
    from pathtracerdemo_amd.renderer import Renderer
    one = make()
    bands = [make(row_begin=a, row_end=b) for a, b in ((0, 40), (40, H))]
    for f, calls in enumerate(((), (("pose", FE.POSE_A),), (("pose", FE.POSE_B),)), start=1):
        step(one, calls)
        denoise(one, True, iterations=3)
        for x in bands:
            for c in calls:
                FE.apply(x, c)
            if calls:
                x.ResetFrameCount()
            x.Update()
        Renderer.render_bands(bands)
        out = np.zeros((H, W, 4), np.float32)
        for x in bands:
            x.follow_vertices = True
        Renderer.denoise_bands(bands, out, temporal=True, iterations=3)
        assert sum(x.denoise_clips() for x in bands) == 0
        np.testing.assert_array_equal(bits(np.concatenate([x.read_denoise_history() for x in bands])),
                                      bits(one.read_denoise_history()), f"history, call {f}")
        np.testing.assert_array_equal(bits(out), bits(one.read_denoised()), f"denoised, call {f}")
    ch = FE.chair_of(guides_of(one))
    assert (one.read_denoise_history()[..., 3][ch] > 2).any()  # the chair kept its history over the poses
    for x in [one] + bands:
        x.close()


def test_a_dropped_state_drops_the_marks():
    """After ptx_reset_accumulation, and after Initialize again, a following call is a first call: n <= 1
    everywhere, whatever was marked and saved before."""
    r = make()
    for _ in range(2):
        step(r)
        denoise(r, True, iterations=2)
    step(r, (("pose", FE.POSE_A),))
    r.reset_accumulation()
    r.Update()
    r.Render()
    denoise(r, True, iterations=2)
    assert r.read_denoise_history()[..., 3].max() <= 1
    step(r, (("pose", FE.POSE_B),))
    denoise(r, True, iterations=2)
    assert r.read_denoise_history()[..., 3].max() == 2
    step(r, (("pose", FE.POSE_A),))
    r.Initialize(E.base())
    r.Update()
    r.Render()
    denoise(r, True, iterations=2)
    assert r.read_denoise_history()[..., 3].max() <= 1
    assert np.isfinite(r.read_denoised()).all()
    r.close()


def test_reserved_2_out_of_range_is_refused():
    from pathtracerdemo_amd import _native as native
    r = make(skin=False)
    step(r)
    with pytest.raises(native.PtxError):
        denoise(r, 2)
    p = native.PtxDenoiseParams()
    p.reserved[2] = 2  # (refused without the temporal mode too: only 1 is ignored there)
    assert r._lib.ptx_denoise(r._h, ctypes.byref(p)) == native.PTX_E_INVALID
    r.follow_vertices = True
    r.Denoise()
    r.close()
