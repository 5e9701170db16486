"""The restatement of following in the temporal upsampler (tests/upsample_follow_ref.py) on the oracle's
G-buffers, hi 96x72 and lo 48x36 (s = 2) through ptx_phase_uniform's uniform, scene_edits' chair moved and
turned: no GPU.  What it pins is what tests/test_gpu_upsample_follow.py compares the kernel against: that with
no edit it is TemporalUpsampler, that with the switch off it is TemporalUpsampler reset at the edit, that
following finds the moved chair's history where the unfollowed lookup on the kept state does not; and the C
ABI's new entry point."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import denoise_ref as D
import scene_edits as E
import upsample_follow_ref as UF
import upsample_temporal_ref as UT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, S = 96, 72, 2
CYCLE = [(0, 0), (1, 1), (1, 0), (0, 1)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def uniform_of(cs, yaw=0.0):
    from pathtracerdemo_amd.scene.camera import Camera
    c = Camera(W, H)
    c.set_location(0, 0, 6)
    c.set_yaw(yaw)
    c.set_pitch(0)
    return cs.uniform(W, H, c.view_projection_inverse(), c.location, 1)


_frames = {}


def frames(oracle_mod, name, yaw, phase):
    """(cs, hi uniform, hi G-buffer, hi guides, lo guides) of the oracle's G-buffer passes of one (edit, yaw, phase)."""
    key = (name, yaw, phase)
    if key not in _frames:
        cs = E.base() if name == "base" else E.edited(name)
        if (name, yaw) not in _frames:
            u = uniform_of(cs, yaw)
            f = oracle_mod.Frame(u, cs.scene, cs.geometry, cs.accel)
            f.run(oracle_mod.PASS_GBUFFER)
            gb = np.array(f.gbuffer, np.uint32)
            _frames[(name, yaw)] = (u, gb, D.guides_from_gbuffer(u, cs.scene, cs.geometry, cs.accel, gb))
        u, gb, G = _frames[(name, yaw)]
        ul = UT.phase_uniform(u, S, *phase)
        fl = oracle_mod.Frame(ul, cs.scene, cs.geometry, cs.accel)
        fl.run(oracle_mod.PASS_GBUFFER)
        _frames[key] = (cs, u, gb, G, D.guides_from_gbuffer(ul, cs.scene, cs.geometry, cs.accel, fl.gbuffer))
    return _frames[key]


def colours(seed):
    return np.random.default_rng(seed).random((H // S, W // S, 4), dtype=np.float32)


def follow_call(t, fr, colour, phase, **kw):
    cs, u, gb, G, Gl = fr
    return t.upsample(colour, Gl, G, u, S, *phase, insts=E.instance_block(cs), scene=cs.scene, geometry=cs.geometry,
                      accel=cs.accel, gbuffer=gb, **kw)


def plain_call(t, fr, colour, phase):
    cs, u, gb, G, Gl = fr
    return t.upsample(colour, Gl, G, u, S, *phase)


def chair_of(G):
    return G.hit & (G.key >> np.uint32(16) == E.CHAIR)


# ------------------------------------------------------------------ the ABI's new surface
def test_header_declares_the_switch_and_the_binding_mirrors_it():
    from pathtracerdemo_amd import _native as N
    from pathtracerdemo_amd.renderer import Renderer
    txt = open(os.path.join(ROOT, "include", "ptx.h")).read()
    assert re.search(r"^int ptx_upsample_follow\(ptx_handle \*hi, uint32_t follow\);", txt, re.M)
    defs = {k: int(v) for k, v in re.findall(r"^#define\s+(PTX_\w+)\s+(\d+)\b", txt, re.M)}
    assert defs["PTX_ABI_VERSION"] == N.PTX_ABI_VERSION == 5
    assert "ptx_upsample_follow" in N.EXPORTED
    assert ctypes.sizeof(N.PtxUpsampleTemporalParams) == 32  # (the switch is no parameter: the struct is unchanged)
    lib = N.load()
    assert lib.ptx_abi_version() == 5
    assert lib.ptx_upsample_follow.argtypes == [ctypes.c_void_p, ctypes.c_uint32]
    assert lib.ptx_upsample_follow(None, 0) == N.PTX_E_INVALID == lib.ptx_upsample_follow(None, 1)
    assert list(inspect.signature(Renderer.set_upsample_follow).parameters)[1:] == ["on"]
    assert isinstance(Renderer.upsample_follow, property) and Renderer.upsample_follow.fset is None


# ------------------------------------------------------------------ the restatement
def test_no_edit_is_temporal_upsampler(oracle_mod):
    """Still calls, a yaw and a light edit, following: TemporalUpsampler's bits, taps included, and no table."""
    f, t = UF.FollowUpsampler(), UT.TemporalUpsampler()
    for k, (name, yaw) in enumerate([("base", 0.0), ("base", 0.0), ("base", 0.0), ("light", 1.5), ("light", 1.5)]):
        ph = CYCLE[k % 4]
        fr, c = frames(oracle_mod, name, yaw, ph), colours(k)
        a, b = follow_call(f, fr, c, ph), plain_call(t, fr, c, ph)
        np.testing.assert_array_equal(bits(a), bits(b))
        np.testing.assert_array_equal(bits(f.history), bits(t.history))
        np.testing.assert_array_equal(f.taps, t.info["taps"])
        assert f.flags is None
    assert (t.history[..., 3] > 1).any()


def test_switch_off_is_temporal_upsampler_reset_at_the_edit(oracle_mod):
    f, t = UF.FollowUpsampler(), UT.TemporalUpsampler()
    for k, name in enumerate(["base", "base", "move", "move", "turn"]):
        ph = CYCLE[k % 4]
        fr, c = frames(oracle_mod, name, 0.0, ph), colours(10 + k)
        if k in (2, 4):
            t.reset()
        a, b = follow_call(f, fr, c, ph, follow=False), plain_call(t, fr, c, ph)
        np.testing.assert_array_equal(bits(a), bits(b))
        np.testing.assert_array_equal(bits(f.history), bits(t.history))
        assert f.flags is None
        if k in (2, 4):
            assert f.history[..., 3].max() <= 1
    # the switch takes effect after a call made while it is on: an edit before that call still drops the state
    fr = frames(oracle_mod, "base", 0.0, CYCLE[1])
    follow_call(f, fr, colours(20), CYCLE[1], follow=True)
    assert f.flags is None and f.history[..., 3].max() <= 1
    fr = frames(oracle_mod, "move", 0.0, CYCLE[2])
    follow_call(f, fr, colours(21), CYCLE[2], follow=True)
    assert f.flags.tolist() == [0, 0, 1]
    # switching off between the edit and the call: a first call
    f.set_follow(False)
    fr = frames(oracle_mod, "base", 0.0, CYCLE[3])
    follow_call(f, fr, colours(22), CYCLE[3], follow=True)
    assert f.flags is None and f.history[..., 3].max() <= 1


@pytest.mark.parametrize("name,yaw", [("move", 0.0), ("turn", 1.5)])
def test_following_the_instance_finds_the_chairs_history(oracle_mod, name, yaw):
    """The share of chair pixels that take at least one tap after the edit: at least 0.45 following, and at
    least 3 times what the unfollowed lookup finds on the kept state -- the denoiser's bounds on the same
    G-buffers (tests/test_scene_edit_inputs.py: 131 / 218 and 98 / 163 there).  The upsampler applies the same
    key, normal and plane tests with the weaker n' >= 0, so it cannot fall below them.  Measured here: E_move 218
    chair pixels, 131 following, 2 unfollowed; E_turn with yaw 1.5: 163, 98, 16."""
    f, t = UF.FollowUpsampler(), UT.TemporalUpsampler()
    for k in range(2):
        fr, c = frames(oracle_mod, "base", 0.0, CYCLE[k]), colours(30 + k)
        follow_call(f, fr, c, CYCLE[k])
        plain_call(t, fr, c, CYCLE[k])
    fr, c = frames(oracle_mod, name, yaw, CYCLE[2]), colours(32)
    follow_call(f, fr, c, CYCLE[2])
    plain_call(t, fr, c, CYCLE[2])  # (the state kept across the edit, looked up as if nothing had moved)
    assert f.flags.tolist() == [0, 0, 1]
    G = fr[3]
    chair = chair_of(G)
    n, follow, kept = int(chair.sum()), int((f.taps[chair] >= 1).sum()), int((t.info["taps"][chair] >= 1).sum())
    print(f"{name}: {n} chair pixels, {follow} with a tap following the instance, {kept} with the unfollowed lookup")
    assert n > 100
    assert follow >= 0.45 * n and follow >= 3 * kept
    assert (f.history[..., 3][chair] > 1).any()
    # everything that is not the chair looks its history up as before
    np.testing.assert_array_equal(f.taps[~chair], t.info["taps"][~chair])
    np.testing.assert_array_equal(bits(f.history[~chair]), bits(t.history[~chair]))


def test_a_rescaled_instance_starts_over_alone(oracle_mod):
    f = UF.FollowUpsampler()
    for k in range(4):
        follow_call(f, frames(oracle_mod, "base", 0.0, CYCLE[k]), colours(40 + k), CYCLE[k])
    fr = frames(oracle_mod, "scale", 0.0, CYCLE[0])  # (the first phase again: its pixels are sampled a second time)
    follow_call(f, fr, colours(44), CYCLE[0])
    assert f.flags.tolist() == [0, 0, 2]
    G = fr[3]
    chair, n = chair_of(G), f.history[..., 3]
    assert chair.any() and (n[chair] <= 1).all() and (f.taps[chair] == -1).all()
    assert (n[G.hit & ~chair] > 1).any()
