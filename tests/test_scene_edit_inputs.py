"""What ptx_update_scene's tests are built on, checked without a GPU: the edits of c3_interior_32
(tests/scene_edits.py) keep the layout and touch only their block of the scene array, and the numpy
restatement of object motion in the temporal denoiser (tests/denoise_motion_ref.py) is the old
restatement while nothing moves, follows a moved chair where the old lookup loses it, and gives up on
a rescaled one."""
import numpy as np
import pytest

import denoise_motion_ref as M
import denoise_ref as D
import denoise_temporal_ref as T
import scene_edits as E

W, H = 96, 72


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------ the edits
@pytest.mark.parametrize("name", E.EDITS)
def test_edit_keeps_the_layout(name):
    b, cs = E.base(), E.edited(name)
    assert len(cs.scene) == len(b.scene) == 950
    assert cs.offsets == b.offsets and cs.instance_count == b.instance_count == 3 and cs.light_count == b.light_count == 32
    np.testing.assert_array_equal(cs.geometry, b.geometry)
    np.testing.assert_array_equal(cs.accel, b.accel)
    o = b.offsets
    np.testing.assert_array_equal(cs.scene[o["mesh_descriptor"]:o["material"]], b.scene[o["mesh_descriptor"]:o["material"]])


@pytest.mark.parametrize("name,blocks,lo,hi,count", [
    ("move", {"instances"}, 78, 96, 4), ("turn", {"instances"}, 66, 96, None), ("scale", {"instances"}, 66, 97, None),
    ("light", {"lights"}, 358, 916, 32), ("mat", {"materials"}, 117, 119, None),
    ("light_mat", {"lights", "materials"}, 117, 916, None)])
def test_edit_changes_its_block_only(name, blocks, lo, hi, count):
    cs = E.edited(name)
    w = E.changed_words(cs)
    assert len(w) and {E.block_of(cs, int(x)) for x in w} == blocks
    assert lo <= w.min() and w.max() <= hi
    if count is not None:
        assert len(w) == count and (w.min(), w.max()) == (lo, hi)
    if name == "light":  # the intensities alone (word 16 of each light): the CDF of halved lights is the same
        assert ((w - cs.offsets["light"]) % 18 == 16).all()
    if blocks == {"instances"}:  # the chair alone
        assert (w // 33 == E.CHAIR).all()


def test_uniform_is_the_same_for_every_edit():
    cam = np.eye(4, dtype=np.float32).reshape(16)
    u = E.base().uniform(W, H, cam, (0, 0, 6), 1)
    for name in E.EDITS:
        np.testing.assert_array_equal(E.edited(name).uniform(W, H, cam, (0, 0, 6), 1), u)


# ------------------------------------------------------------------ the restatement
def uniform_of(cs, yaw=0.0):
    from pathtracerdemo_amd.scene.camera import Camera
    c = Camera(W, H)
    c.set_location(0, 0, 6)
    c.set_yaw(yaw)
    c.set_pitch(0)
    return cs.uniform(W, H, c.view_projection_inverse(), c.location, 1)


_guides = {}


def guides(oracle_mod, name, yaw=0.0):
    """The guides of the oracle's G-buffer of one (edit, yaw), computed once."""
    if (name, yaw) not in _guides:
        cs = E.base() if name == "base" else E.edited(name)
        u = uniform_of(cs, yaw)
        f = oracle_mod.Frame(u, cs.scene, cs.geometry, cs.accel)
        f.run(oracle_mod.PASS_GBUFFER)
        _guides[(name, yaw)] = (cs, u, D.guides_from_gbuffer(u, cs.scene, cs.geometry, cs.accel, f.gbuffer))
    return _guides[(name, yaw)]


def colours(seed):
    return np.random.default_rng(seed).random((H, W, 4), dtype=np.float32)


def test_no_instance_differs_is_the_old_restatement(oracle_mod):
    """Still camera, moved camera, a light edit: MotionDenoiser equals TemporalDenoiser bit for bit."""
    m, t = M.MotionDenoiser(), T.TemporalDenoiser()
    for f, (name, yaw) in enumerate([("base", 0.0), ("base", 0.0), ("light", 1.5), ("light", 1.5)]):
        cs, u, G = guides(oracle_mod, name, yaw)
        F = colours(f)
        a = m.denoise(F, F, G, u, insts=E.instance_block(cs), iterations=2)
        b = t.denoise(F, F, G, u, iterations=2)
        np.testing.assert_array_equal(bits(a), bits(b))
        np.testing.assert_array_equal(bits(m.history), bits(t.history))
        np.testing.assert_array_equal(m.taps, t.taps)
        assert m.flags is None
    assert (t.history[..., 3] > 2).any()


@pytest.mark.parametrize("name,yaw", [("move", 0.0), ("turn", 1.5)])
def test_following_the_instance_finds_the_chairs_history(oracle_mod, name, yaw):
    """The share of chair pixels that take at least one tap (every hit pixel of the previous call has
    n = 1, so the n >= 1 test passes wherever the key matches): at least 45 % following the instance,
    and at least 3 times today's lookup.  Measured here: E_move 218 chair pixels, 131 following, 2 with
    today's lookup (the camera stands still, so today's lookup is the same-pixel rule; reprojecting P
    through the unchanged camera instead, which the denoiser never does at rest, would give 11); E_turn
    with yaw 1.5: 163, 98, 16."""
    b, u0, G0 = guides(oracle_mod, "base")
    cs, u1, G1 = guides(oracle_mod, name, yaw)
    Z = np.zeros((H, W, 4), np.float32)
    m, t = M.MotionDenoiser(), T.TemporalDenoiser()
    m.denoise(Z, Z, G0, u0, insts=E.instance_block(b), iterations=1)
    t.denoise(Z, Z, G0, u0, iterations=1)
    m.denoise(Z, Z, G1, u1, insts=E.instance_block(cs), iterations=1)
    t.denoise(Z, Z, G1, u1, iterations=1)
    assert m.flags.tolist() == [0, 0, 1]
    chair = G1.hit & (G1.key >> np.uint32(16) == E.CHAIR)
    n, follow, today = int(chair.sum()), int((m.taps[chair] >= 1).sum()), int((t.taps[chair] >= 1).sum())
    print(f"{name}: {n} chair pixels, {follow} with a tap following the instance, {today} with today's lookup")
    assert n > 100
    assert follow >= 0.45 * n and follow >= 3 * today
    # everything that is not the chair looks its history up as before
    np.testing.assert_array_equal(m.taps[~chair], t.taps[~chair])
    np.testing.assert_array_equal(bits(m.history[~chair]), bits(t.history[~chair]))


def test_a_rescaled_instance_starts_over(oracle_mod):
    b, u0, G0 = guides(oracle_mod, "base")
    cs, u1, G1 = guides(oracle_mod, "scale")
    F = colours(7)
    m = M.MotionDenoiser()
    m.denoise(F, F, G0, u0, insts=E.instance_block(b), iterations=1)
    m.denoise(F, F, G0, u0, insts=E.instance_block(b), iterations=1)
    m.denoise(F, F, G1, u1, insts=E.instance_block(cs), iterations=1)
    assert m.flags.tolist() == [0, 0, 2]
    chair = G1.hit & (G1.key >> np.uint32(16) == E.CHAIR)
    assert chair.any() and (m.history[chair][:, 3] == 1).all() and (m.taps[chair] == -1).all()
    np.testing.assert_array_equal(bits(m.history[chair][:, :3]), bits(F[chair][:, :3]))
    assert (m.history[G1.hit & ~chair][:, 3] == 3).any()


def test_object_table_flags():
    b = E.instance_block(E.base())
    same = M.object_table(b, b)
    assert same[0].tolist() == [0, 0, 0] and not same[1].any()
    flags, Dm = M.object_table(b, E.instance_block(E.edited("turn")))
    assert flags.tolist() == [0, 0, 1]
    d = Dm[E.CHAIR].reshape(4, 4).T.astype(np.float64)  # (column-major -> rows)
    np.testing.assert_allclose(d[:3, :3] @ d[:3, :3].T, np.eye(3), atol=1e-5)
    np.testing.assert_array_equal(d[3], [0, 0, 0, 1])
    other = E.instance_block(E.edited("move")).copy()
    other[33 * E.CHAIR + 32] = 0  # another mesh: never followed
    assert M.object_table(b, other)[0].tolist() == [0, 0, 2]
    nan = E.instance_block(E.edited("move")).copy()
    nan[33 * E.CHAIR + 16] = np.float32(np.nan).view(np.uint32)
    assert M.object_table(b, nan)[0].tolist() == [0, 0, 2]
