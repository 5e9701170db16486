"""The restatement of vertex motion in the temporal denoiser (tests/denoise_follow_ref.py) on the oracle's
G-buffers, 96x72, scene_edits.base() with the chair posed by skin_edits and bent by vertex_edits
(tests/follow_edits.py): no GPU.  What it pins is what tests/test_gpu_denoise_follow.py compares the kernel
against: that following is MotionDenoiser while nothing is deformed, that it finds the chair's history over
the posed steps where today's lookup does not, and the flags of a deformed instance that is also rescaled or
switched."""
import dataclasses

import numpy as np

import denoise_follow_ref as F
import denoise_motion_ref as M
import denoise_ref as D
import follow_edits as FE
import scene_edits as E

W, H = 96, 72


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def uniform_of(cs, yaw=None):
    from pathtracerdemo_amd.scene.camera import Camera
    c = Camera(W, H)
    c.set_location(0, 0, 6)
    c.set_yaw(yaw or 0.0)
    c.set_pitch(0)
    return cs.uniform(W, H, c.view_projection_inverse(), c.location, 1)


_frames = {}


def frame(oracle_mod, call=None, chair="base", light=0, yaw=None):
    """(cs, uniform, G-buffer, guides) of the oracle's frame of one shape, scene and camera, computed once."""
    key = (call, chair, light, yaw)
    if key not in _frames:
        cs = FE.compiled(call, chair, light)
        u = uniform_of(cs, yaw)
        f = oracle_mod.Frame(u, cs.scene, cs.geometry, cs.accel)
        f.run(oracle_mod.PASS_GBUFFER)
        gb = np.array(f.gbuffer, np.uint32)
        _frames[key] = (cs, u, gb, D.guides_from_gbuffer(u, cs.scene, cs.geometry, cs.accel, gb))
    return _frames[key]


def colours(seed):
    return np.random.default_rng(seed).random((H, W, 4), dtype=np.float32)


def follow_call(t, fr, colour, deformed=(), follow=True, **kw):
    cs, u, gb, G = fr
    return t.denoise(colour, colour, G, u, insts=E.instance_block(cs), follow=follow, scene=cs.scene, geometry=cs.geometry,
                     accel=cs.accel, gbuffer=gb, deformed=deformed, **kw)


def test_nothing_deformed_is_motion_denoiser(oracle_mod):
    """(a) A still call, a yaw and an instance move, following but with no mesh deformed: MotionDenoiser's bits."""
    f, m = F.FollowDenoiser(), M.MotionDenoiser()
    for k, (chair, yaw, flags) in enumerate([("base", None, None), ("base", None, None), ("base", FE.YAW, None),
                                             ("move", FE.YAW, [0, 0, 1])]):
        fr = frame(oracle_mod, None, chair, 0, yaw)
        cs, u, gb, G = fr
        c = colours(k)
        a = follow_call(f, fr, c, iterations=2)
        b = m.denoise(c, c, G, u, insts=E.instance_block(cs), iterations=2)
        np.testing.assert_array_equal(bits(a), bits(b))
        np.testing.assert_array_equal(bits(f.history), bits(m.history))
        np.testing.assert_array_equal(f.taps, m.taps)
        assert (f.flags.tolist() if f.flags is not None else None) == flags
    assert (f.history[..., 3] > 2).any()


def test_following_finds_the_posed_chairs_history(oracle_mod):
    """(b) tests/test_gpu_denoise_follow.py's main sequence on the oracle's G-buffers.  In every posed call the
    following restatement takes at least one tap on >= 0.45 of the chair's hit pixels (the share
    tests/test_gpu_denoise_motion.py asks of a moved chair), and the not-following restatement, fed the same
    inputs, ends with another n on chair pixels: the GPU test cannot pass on a denoiser that does not follow.
      The poses are skin_edits' POSE_A = 1.0 and POSE_B = -0.6 as they are (and 0.5 for the first of the two
    poses of one step); nothing had to shrink.  Measured here, chair pixels / with a tap following / with a tap
    not following: pose_a 152 / 124 / 64, pose_b_yaw 171 / 140 / 89, two_poses 281 / 232 / 74 (a share of
    0.82-0.83 following), and the steps with a bend: bend 177 / 135 / 80, bend_move 231 / 151 / 141, bend_scale
    302 / 251 / 0 (not following, a rescaled instance starts over)."""
    f, m = F.FollowDenoiser(), M.MotionDenoiser()
    shape, diff = None, 0
    for k, (name, calls, chair, light, yaw_step, flags) in enumerate(FE.MAIN):
        yaw = yaw_step if yaw_step is not None else (yaw if k else None)
        shape = calls[-1] if calls else shape
        fr = frame(oracle_mod, shape, chair, light, yaw)
        cs, u, gb, G = fr
        c = colours(100 + k)
        follow_call(f, fr, c, deformed=(FE.CHAIR_MESH,) if calls else (), iterations=1)
        m.denoise(c, c, G, u, insts=E.instance_block(cs), iterations=1)
        assert (f.flags.tolist() if f.flags is not None else None) == flags, name
        ch = FE.chair_of(G)
        n, fol, tod = int(ch.sum()), int((f.taps[ch] >= 1).sum()), int((m.taps[ch] >= 1).sum())
        print(f"{name}: {n} chair pixels, {fol} with a tap following the vertices, {tod} not following")
        assert n > 100
        if name in FE.POSED:
            assert fol >= 0.45 * n, name
        # everything that is not the chair looks its history up as before
        np.testing.assert_array_equal(bits(f.history[~ch]), bits(m.history[~ch]))
        diff += int((f.history[..., 3][ch] != m.history[..., 3][ch]).sum())
    assert (f.history[..., 3][ch] != m.history[..., 3][ch]).any(), "the sequence does not tell following from not following"
    assert diff > 0 and (f.history[..., 3][ch] > 2).any()


def test_deformed_and_rescaled_follows_and_a_switched_mesh_does_not(oracle_mod):
    """(c) flag 3 needs no rigidity; another mesh word is flag 2, deformed or not."""
    f = F.FollowDenoiser()
    base = frame(oracle_mod, None)
    follow_call(f, base, colours(1), iterations=1)
    follow_call(f, base, colours(2), iterations=1)
    fr = frame(oracle_mod, ("bend", 1.0), "scale")
    follow_call(f, fr, colours(3), deformed=(FE.CHAIR_MESH,), iterations=1)
    assert f.flags.tolist() == [0, 0, 3]
    ch = FE.chair_of(fr[3])
    assert (f.taps[ch] >= 1).sum() >= 0.45 * ch.sum() and (f.history[..., 3][ch] == 3).any()
    # the chair's instance switched to the window's mesh while the chair's mesh was deformed
    cs = E.compose(chair="window")
    u = uniform_of(cs)
    fo = oracle_mod.Frame(u, cs.scene, fr[0].geometry, fr[0].accel)
    fo.run(oracle_mod.PASS_GBUFFER)
    gb = np.array(fo.gbuffer, np.uint32)
    sw = (dataclasses.replace(fr[0], scene=cs.scene), u, gb, D.guides_from_gbuffer(u, cs.scene, fr[0].geometry, fr[0].accel, gb))
    follow_call(f, sw, colours(4), deformed=(FE.CHAIR_MESH,), iterations=1)
    assert f.flags.tolist() == [0, 0, 2]
    assert (f.history[..., 3][FE.chair_of(sw[3])] == 1).all()
    # a call that does not follow ends the tracking: the next following call has nothing to look up by
    follow_call(f, sw, colours(5), follow=False, iterations=1)
    follow_call(f, sw, colours(6), deformed=(FE.CHAIR_MESH,), iterations=1)
    assert f.flags is None
