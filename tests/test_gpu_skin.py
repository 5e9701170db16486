"""ptx_set_skin / ptx_skin_vertices / ptx_read_vertices on the GPU: a mesh of c3_interior_32 skinned and morphed
on the device (tests/skin_edits.py).  read_vertices and read_accel equal the numpy rule and the Python refit
(scene/world.py skin_mesh) BIT FOR BIT; every frame of an animated sequence equals the CPU oracle on those
arrays in all four pipelines, the reuse history surviving; counters and memory; every refusal of both calls,
each leaving the handle rendering the unedited oracle frame; the host mirror across a changed layout key;
ptx_update_vertices over a skinned range; two bands against the whole image."""
import ctypes

import numpy as np
import pytest

import scene_edits as E
import skin_edits as S
import vertex_edits as V
from helpers import uniform_for
from test_gpu_scene_edit import W, H, assert_same, make, tick

pytestmark = pytest.mark.gpu
CHAIR, ROOM = S.CHAIR_MESH, S.ROOM_MESH


def assert_tables(r, want, what):
    """The device's records of every mesh, the accel array and the renderer's compiled arrays against `want`."""
    for mesh in range(3):
        got = r.read_vertices(mesh)
        bad = (got != S.block(want, mesh)).any(axis=1)
        assert bad.sum() == 0, f"{what}: {bad.sum()} records of mesh {mesh} differ, first {np.nonzero(bad)[0][:8].tolist()}"
    got = r.read_accel()
    assert int((got != want.accel).sum()) == 0, f"{what}: {int((got != want.accel).sum())} accel words differ"
    np.testing.assert_array_equal(r.compiled.geometry, want.geometry)
    np.testing.assert_array_equal(r.compiled.accel, want.accel)


# ------------------------------------------------------------------ the tables
#         mesh   joints scale      morph range
CASES = {
    "j3": (CHAIR, 3, S.POSE_A, 0, None),
    "j32": (CHAIR, 32, S.POSE_A, 0, None),
    "j1": (CHAIR, 1, S.POSE_A, 0, None),
    "morph_only": (CHAIR, 3, 0.0, 1, None),
    "skin_morph": (CHAIR, 3, S.POSE_A, 1, None),
    "skin_morph_normals": (CHAIR, 32, S.POSE_B, 2, None),
    "sub_range": (CHAIR, 3, S.POSE_A, 0, S.PARTIAL),
    "room": (ROOM, 3, S.POSE_A, 2, None),
}


@pytest.mark.parametrize("case", list(CASES))
def test_read_vertices_and_read_accel_are_the_python_rule(case):
    mesh, joints, scale, morph, rng = CASES[case]
    b = E.base()
    r = make("restir")
    r.Update()
    S.set_skin(r, mesh, joints, morph, rng)
    assert_tables(r, b, f"{case}: after SetSkin alone")
    S.pose(r, mesh, joints, scale, morph)
    want = S.compiled(mesh, joints, scale, morph, rng)
    assert_tables(r, want, case)
    rec, rec0 = r.read_vertices(mesh), S.block(b, mesh)
    np.testing.assert_array_equal(rec[:, 6:8], rec0[:, 6:8])  # the uv words are not the kernel's
    lo, hi = rng or (0, len(rec))
    np.testing.assert_array_equal(rec[:lo], rec0[:lo])
    np.testing.assert_array_equal(rec[hi:], rec0[hi:])
    assert (rec[lo:hi, 0:3] != rec0[lo:hi, 0:3]).any(axis=1).sum() > (hi - lo) // 2
    np.testing.assert_array_equal(r.read_vertices(mesh, lo + 3, 5), rec[lo + 3:lo + 8])
    assert r.compiled.scene is b.scene
    r.close()


def test_the_room_then_the_chair_on_one_handle():
    r = make("restir")
    r.Update()
    S.set_skin(r, ROOM, 3)
    S.set_skin(r, CHAIR, 32, 2)
    S.pose(r, ROOM, 3, S.POSE_A)
    room = S.compiled(ROOM, 3, S.POSE_A)
    assert_tables(r, room, "the room")
    S.pose(r, CHAIR, 32, S.POSE_B, 2)
    both = S.compiled(CHAIR, 32, S.POSE_B, 2, base=room, tag="room")
    assert_tables(r, both, "the room, then the chair")
    # a second SetSkin replaces the chair's skin; the bind pose is the caller's, not the posed records
    S.set_skin(r, CHAIR, 3)
    S.pose(r, CHAIR, 3, S.POSE_A)
    assert_tables(r, S.compiled(CHAIR, 3, S.POSE_A, base=room, tag="room"), "the chair's second skin")
    r.close()


def test_identity_palette_with_one_hot_weights_gives_the_uploaded_arrays_back():
    b = E.base()
    r = make("restir")
    r.Update()
    n = len(S.block(b, CHAIR))
    joints = np.zeros((n, 4), np.uint32)
    joints[:, 1:] = (1, 2, 0)  # (other joints at weight 0)
    one_hot = np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1))
    r.SetSkin(CHAIR, joints, one_hot)  # (bind = NULL: the records as the handle holds them)
    turn = S.palette(CHAIR, 3, S.POSE_A)
    turn[0] = turn[2]
    r.SkinVertices(CHAIR, turn)
    posed = r.read_vertices(CHAIR)
    assert (r.read_accel() != b.accel).any() and (posed[:, 0:3] != S.block(b, CHAIR)[:, 0:3]).any(axis=1).sum() > n // 2
    r.SkinVertices(CHAIR, S.palette(CHAIR, 3, 0.0))
    np.testing.assert_array_equal(r.read_accel(), b.accel)
    rec, rec0 = r.read_vertices(CHAIR), S.block(b, CHAIR)
    np.testing.assert_array_equal(rec[:, 0:3], rec0[:, 0:3])
    np.testing.assert_array_equal(rec[:, 6:8], rec0[:, 6:8])
    # (the normals are normalised again: the rule's bits, an ulp or two from the uploaded ones)
    assert np.abs(rec[:, 3:6].view(np.float32).astype(np.float64) - rec0[:, 3:6].view(np.float32)).max() < 3 * 2.0 ** -24
    np.testing.assert_array_equal(r.compiled.accel, b.accel)
    # bind = NULL after a pose binds the posed records (read from the device: the host's copy is behind)
    r.SkinVertices(CHAIR, turn)
    np.testing.assert_array_equal(r.read_vertices(CHAIR), posed)
    r.SetSkin(CHAIR, joints, one_hot)
    r.SkinVertices(CHAIR, S.palette(CHAIR, 3, 0.0))
    np.testing.assert_array_equal(r.read_vertices(CHAIR)[:, 0:3], posed[:, 0:3])
    r.close()


# ------------------------------------------------------------------ frames
#            pose (palette scale; None: no call)  yaw   the oracle's history is dropped
SEQUENCE = [(None,                                0.0,  False),  # the bind pose as uploaded
            (S.POSE_A,                            0.0,  False),
            (S.POSE_A,                            0.0,  False),  # the same pose, skinned again
            (S.POSE_B,                            0.0,  False),
            (0.0,                                 3.0,  True)]   # the bind pose through the identity palette + yaw 3


def oracle_step(O, fr, pipeline, cs, uniform, drop):
    fr.geometry = np.ascontiguousarray(cs.geometry, dtype=np.uint32)
    fr.accel = np.ascontiguousarray(cs.accel, dtype=np.uint32)
    fr.set_camera(uniform)
    fr.set_frame_index(int(uniform[23]))
    if drop:
        fr.hist_valid = False
    if pipeline == "reuse":
        fr.run_reuse_frame(threads=8)
    elif pipeline == "gi":
        fr.run_gi_frame(threads=8)
    else:
        fr.run(O.PASS_RESTIR if pipeline == "restir" else O.PASS_MCPT, threads=8)


def compare(r, fr, pipeline, what):
    assert_same(r.read_image(), fr.accum, f"accumulation, {what}")
    if pipeline != "mcpt":
        assert_same(r.read_gbuffer(), fr.gbuffer, f"G-buffer, {what}")
    if pipeline == "restir":
        assert_same(r.read_reservoir(), fr.reservoir, f"reservoirs, {what}")
    if pipeline == "reuse":
        assert_same(r.read_reservoir(), fr.reservoir, f"temporal output, {what}")
        assert_same(r.read_history(), fr.res_hist, f"spatial output, {what}")
    if pipeline == "gi":
        assert_same(r.read_reservoir(), fr.gi_res, f"GI temporal output, {what}")
        assert_same(r.read_history(), fr.gi_hist, f"GI spatial output, {what}")


@pytest.mark.parametrize("pipeline", ["reuse", "gi", "restir", "mcpt"])
def test_skin_sequence_bit_exact_against_the_oracle(oracle_mod, pipeline):
    O = oracle_mod
    b = E.base()
    r = make(pipeline)
    fr = O.Frame(uniform_for(b, W, H, 1), b.scene, b.geometry, b.accel)
    used_after_skin = 0
    for f, (scale, yaw, drop) in enumerate(SEQUENCE, start=1):
        if f == 2:
            S.set_skin(r, CHAIR, 3, 2)
        if scale is not None:
            S.pose(r, CHAIR, 3, scale, 2)
        cs = b if scale is None else S.compiled(CHAIR, 3, scale, 2)
        tick(r, yaw)
        oracle_step(O, fr, pipeline, cs, r.uniform, drop)
        compare(r, fr, pipeline, f"frame {f} (pose {scale})")
        if pipeline == "reuse" and scale is not None and not drop:
            used_after_skin += int((fr.reservoir[..., 29] > 1).sum())
    assert np.isfinite(fr.accum).all()
    assert pipeline != "reuse" or used_after_skin > 0, "the reuse history must survive the skin call"
    r.close()


# ------------------------------------------------------------------ counters, memory, SetSkin alone
def test_launches_and_memory():
    from pathtracerdemo_amd import _native as native
    slot = native.PTX_STAT_REFIT
    r = make("restir", time_launches=True)
    r.Update()
    s0 = r.stats()
    r.UpdateVertices(CHAIR, V.bend())
    s1 = r.stats()
    refit = s1["kernel_launches"][slot] - s0["kernel_launches"][slot]
    sk = S.skin(CHAIR, 32, 2)
    S.set_skin(r, CHAIR, 32, 2)
    s2 = r.stats()
    n = len(sk.bind)
    tables = 48 * n + 2 * (2 * n * 12) + (256 * 12 + 8) * 4  # bind records, two delta tables of two targets, a call's pose
    assert s2["device_bytes"] - s1["device_bytes"] == tables
    assert s2["kernel_launches"][slot] == s1["kernel_launches"][slot], "SetSkin launches nothing"
    S.pose(r, CHAIR, 32, S.POSE_A, 2)
    s3 = r.stats()
    assert s3["kernel_launches"][slot] - s2["kernel_launches"][slot] == refit + 1
    assert s3["kernel_ms_total"][slot] > s2["kernel_ms_total"][slot]
    assert s3["device_bytes"] == s2["device_bytes"], "SkinVertices allocates nothing"
    # n_vertices == 0 removes the skin and gives its memory back; the upload drops every skin
    r.SetSkin(CHAIR, np.zeros((0, 4), np.uint32), np.zeros((0, 4), np.float32))
    assert r.stats()["device_bytes"] == s1["device_bytes"]
    with pytest.raises(ValueError):
        S.pose(r, CHAIR, 32, S.POSE_A, 2)
    pal = S.palette(CHAIR, 32)
    assert native.load().ptx_skin_vertices(r._h, CHAIR, pal.ctypes.data, None) == native.PTX_E_INVALID  # no skin
    S.set_skin(r, CHAIR, 3)
    r.Initialize(E.base())
    r.Update()
    assert native.load().ptx_skin_vertices(r._h, CHAIR, pal.ctypes.data, None) == native.PTX_E_INVALID
    r.close()


def test_set_skin_alone_changes_no_frame_and_keeps_the_history():
    r, twin = make("reuse"), make("reuse")
    for x in (r, twin):
        tick(x)
        tick(x)
    S.set_skin(r, CHAIR, 32, 2)
    for yaw in (0.0, 1.5):  # (a still frame, then a moved one: the history is still reprojected)
        for x in (r, twin):
            tick(x, yaw)
        for name in ("read_image", "read_gbuffer", "read_reservoir", "read_history"):
            assert_same(getattr(r, name)(), getattr(twin, name)(), f"{name}, yaw {yaw}")
        assert (r.read_reservoir()[..., 29] > 1).any(), "the history is used"
    r.close()
    twin.close()


# ------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def unedited(oracle_mod):
    """The oracle's reuse frames of the unedited scene: two still frames, a third, then yaw 1.5 (made once;
    the refusal tests compare their frames 3 and 4 with it)."""
    b = E.base()
    probe = make("reuse")
    fr = oracle_mod.Frame(uniform_for(b, W, H, 1), b.scene, b.geometry, b.accel)
    frames = []
    for yaw in (0.0, 0.0, 0.0, 1.5):
        probe.GetCamera().set_yaw(yaw)
        probe.Update()
        oracle_step(oracle_mod, fr, "reuse", b, probe.uniform, False)
        frames.append({k: np.array(getattr(fr, k)) for k in ("accum", "gbuffer", "reservoir", "res_hist")})
    probe.close()
    return frames


def assert_unedited(r, unedited, what):
    """r has rendered two frames: the next two are the unedited scene's, history and all."""
    for f, yaw in ((2, 0.0), (3, 1.5)):
        tick(r, yaw)
        want = unedited[f]
        assert_same(r.read_image(), want["accum"], f"{what}: accumulation, frame {f + 1}")
        assert_same(r.read_gbuffer(), want["gbuffer"], f"{what}: G-buffer, frame {f + 1}")
        assert_same(r.read_reservoir(), want["reservoir"], f"{what}: temporal output, frame {f + 1}")
        assert_same(r.read_history(), want["res_hist"], f"{what}: spatial output, frame {f + 1}")
    np.testing.assert_array_equal(r.read_accel(), E.base().accel)
    np.testing.assert_array_equal(r.read_vertices(CHAIR), S.block(E.base(), CHAIR))


def _desc(native, keep, **over):
    """A valid descriptor of the chair's 3-joint skin with two targets and normal deltas, fields replaced by
    `over` (arrays are kept alive in `keep`; a value None is a null pointer)."""
    sk = S.skin(CHAIR, 3, 2)
    arrays = dict(joints=sk.joints, weights=sk.weights, bind=sk.bind, target_pos=sk.target_pos, target_nrm=sk.target_nrm)
    fields = dict(mesh=CHAIR, first_vertex=0, n_vertices=len(sk.bind), n_joints=3, n_targets=2)
    reserved = over.pop("reserved", None)
    for k, v in over.items():
        if k in arrays:
            arrays[k] = v
        else:
            fields[k] = v
    for k, a in arrays.items():
        if a is not None:
            a = np.ascontiguousarray(a)
            keep.append(a)
            fields[k] = a.ctypes.data
    d = native.PtxSkinDesc(**fields)
    if reserved is not None:
        d.reserved[reserved] = 1
    return d


def _poked(a, index, value):
    a = np.array(a)
    a[index] = value
    return a


def _set_skin_refusals():
    sk = S.skin(CHAIR, 3, 2)
    n = len(sk.bind)
    return {
        "mesh_not_loaded": (dict(mesh=3), -3),
        "range_past_the_block": (dict(first_vertex=1), -1),
        "first_wraps": (dict(first_vertex=0xFFFFFFFF, n_vertices=2), -1),
        "range_past_a_middle_mesh": (dict(mesh=1, first_vertex=30, n_vertices=3), -1),
        "no_joints": (dict(n_joints=0), -1),
        "too_many_joints": (dict(n_joints=257), -1),
        "too_many_targets": (dict(n_targets=9), -1),
        "joint_index_past_the_count": (dict(joints=_poked(sk.joints, (n - 1, 3), 3)), -1),
        "nan_weight": (dict(weights=_poked(sk.weights, (17, 2), np.nan)), -1),
        "inf_bind_word": (dict(bind=_poked(sk.bind, (n - 1, 5), -np.inf)), -1),
        "nan_position_delta": (dict(target_pos=_poked(sk.target_pos, (1, 99, 0), np.nan)), -1),
        "inf_normal_delta": (dict(target_nrm=_poked(sk.target_nrm, (0, 0, 2), np.inf)), -1),
        "null_joints": (dict(joints=None), -1),
        "null_weights": (dict(weights=None), -1),
        "targets_without_deltas": (dict(target_pos=None, target_nrm=None), -1),
        "deltas_without_targets": (dict(n_targets=0, target_nrm=None), -1),
        "normal_deltas_without_targets": (dict(n_targets=0, target_pos=None), -1),
        "reserved_word": (dict(reserved=1), -1),
    }


SET_SKIN_REFUSALS = ["null_descriptor", "mesh_not_loaded", "range_past_the_block", "first_wraps", "range_past_a_middle_mesh",
                     "no_joints", "too_many_joints", "too_many_targets", "joint_index_past_the_count", "nan_weight",
                     "inf_bind_word", "nan_position_delta", "inf_normal_delta", "null_joints", "null_weights",
                     "targets_without_deltas", "deltas_without_targets", "normal_deltas_without_targets", "reserved_word"]


@pytest.mark.parametrize("case", SET_SKIN_REFUSALS)
def test_set_skin_refusals_leave_the_unedited_frame(unedited, case):
    from pathtracerdemo_amd import _native as native
    lib = native.load()
    r = make("reuse")
    tick(r)
    tick(r)
    keep = []
    S.set_skin(r, CHAIR, 3)  # (a refused call leaves the skin that was bound)
    if case == "null_descriptor":
        assert lib.ptx_set_skin(r._h, None) == native.PTX_E_INVALID
    else:
        over, code = _set_skin_refusals()[case]
        assert lib.ptx_set_skin(r._h, ctypes.byref(_desc(native, keep, **over))) == code
    assert_unedited(r, unedited, case)
    S.pose(r, CHAIR, 3, S.POSE_A)  # the skin bound before the refusal is still the mesh's
    np.testing.assert_array_equal(r.compiled.accel, S.compiled(CHAIR, 3, S.POSE_A).accel)
    r.close()


def _skin_vertices_refusals():
    pal = S.palette(CHAIR, 3)
    return {
        "mesh_not_loaded": (3, pal, S.TW, -3),
        "mesh_without_a_skin": (ROOM, pal, S.TW, -1),
        "null_palette": (CHAIR, None, S.TW, -1),
        "nan_palette": (CHAIR, _poked(pal, (2, 11), np.nan), S.TW, -1),
        "inf_palette": (CHAIR, _poked(pal, (0, 0), np.inf), S.TW, -1),
        "null_target_weights": (CHAIR, pal, None, -1),
        "nan_target_weight": (CHAIR, pal, _poked(S.TW, 1, np.nan), -1),
        "the_overflow_bound": (CHAIR, _poked(pal, (1, 3), 2.0 ** 100), S.TW, -1),
    }


@pytest.mark.parametrize("case", ["mesh_not_loaded", "mesh_without_a_skin", "null_palette", "nan_palette", "inf_palette",
                                  "null_target_weights", "nan_target_weight", "the_overflow_bound",
                                  "target_weights_without_targets"])
def test_skin_vertices_refusals_leave_the_unedited_frame(unedited, case):
    from pathtracerdemo_amd import _native as native
    from pathtracerdemo_amd.scene.skin import BOUND, overflow_bound
    lib = native.load()
    r = make("reuse")
    tick(r)
    tick(r)
    if case == "target_weights_without_targets":
        S.set_skin(r, CHAIR, 3, 0)
        mesh, pal, tw, code = CHAIR, S.palette(CHAIR, 3), S.TW, -1
    else:
        S.set_skin(r, CHAIR, 3, 2)
        mesh, pal, tw, code = _skin_vertices_refusals()[case]
    if case == "the_overflow_bound":
        sk = S.skin(CHAIR, 3, 2)
        assert not overflow_bound(sk.bind, sk.weights, pal, sk.target_pos, sk.target_nrm, tw) < BOUND
    assert lib.ptx_skin_vertices(r._h, mesh, None if pal is None else pal.ctypes.data,
                                 None if tw is None else tw.ctypes.data) == code
    assert r.stats()["kernel_launches"][native.PTX_STAT_REFIT] == 0
    assert_unedited(r, unedited, case)
    # after a refused SkinVertices a valid call still works
    morph = 0 if case == "target_weights_without_targets" else 2
    S.pose(r, CHAIR, 3, S.POSE_A, morph)
    assert_tables(r, S.compiled(CHAIR, 3, S.POSE_A, morph), f"{case}: the valid call after it")
    r.close()


def test_refused_without_handle_scene_or_frame_and_read_vertices():
    from pathtracerdemo_amd import _native as native
    from pathtracerdemo_amd.renderer import Renderer
    lib = native.load()
    keep = []
    pal = S.palette(CHAIR, 3)
    out = np.zeros((16, 8), np.uint32)
    r = Renderer(W, H, device=0, pipeline="reuse")

    def all_three(handle):
        return (lib.ptx_set_skin(handle, ctypes.byref(_desc(native, keep))),
                lib.ptx_skin_vertices(handle, CHAIR, pal.ctypes.data, S.TW.ctypes.data),
                lib.ptx_read_vertices(handle, CHAIR, 0, 16, out.ctypes.data))
    assert all_three(None) == (-1, -1, -1)   # a null handle
    assert all_three(r._h) == (-1, -1, -1)   # no scene
    r.Initialize(E.base())
    assert all_three(r._h) == (-1, -1, -1)   # no frame set: no layout
    with pytest.raises(ValueError):
        S.set_skin(r, CHAIR, 3)
    r.Update()
    # ptx_read_vertices: ptx_read_accel's preconditions, ptx_update_vertices' range rules
    n = len(S.block(E.base(), CHAIR))
    assert lib.ptx_read_vertices(r._h, 3, 0, 16, out.ctypes.data) == -3  # PTX_E_SCENE
    assert lib.ptx_read_vertices(r._h, CHAIR, n - 15, 16, out.ctypes.data) == native.PTX_E_INVALID
    assert lib.ptx_read_vertices(r._h, CHAIR, 0xFFFFFFFF, 2, out.ctypes.data) == native.PTX_E_INVALID
    assert lib.ptx_read_vertices(r._h, 1, 30, 3, out.ctypes.data) == native.PTX_E_INVALID
    assert lib.ptx_read_vertices(r._h, CHAIR, 0, 16, None) == native.PTX_E_INVALID
    assert lib.ptx_read_vertices(r._h, CHAIR, n, 0, None) == native.PTX_OK
    assert lib.ptx_read_vertices(r._h, CHAIR, n - 16, 16, out.ctypes.data) == native.PTX_OK
    np.testing.assert_array_equal(out, S.block(E.base(), CHAIR)[n - 16:])
    # the Renderer's own argument checks
    sk = S.skin(CHAIR, 3)
    with pytest.raises(ValueError):
        r.SetSkin(CHAIR, sk.joints, sk.weights[:-1])
    with pytest.raises(ValueError):
        r.SetSkin(CHAIR, sk.joints, sk.weights, sk.bind[:-1])
    with pytest.raises(ValueError):
        r.SkinVertices(CHAIR, pal)
    S.set_skin(r, CHAIR, 3)
    with pytest.raises(ValueError):
        r.SkinVertices(CHAIR, pal[:2])
    with pytest.raises(ValueError):
        r.SkinVertices(CHAIR, pal, S.TW)
    assert r.compiled is E.base()
    r.close()


# ------------------------------------------------------------------ the host mirror
def test_a_changed_layout_key_derives_the_layout_from_the_skinned_arrays(oracle_mod):
    """ptx_skin_vertices leaves the handle's host copy of the geometry (and of the refitted boxes) behind the
    device; a frame with another layout key (here: one instance fewer), and then the scene's own key
    again, derive the layout from the host copies twice -- which must be the skinned arrays by then."""
    from pathtracerdemo_amd import _native as native
    r = make("restir")
    r.Update()
    S.set_skin(r, CHAIR, 32, 2)
    S.pose(r, CHAIR, 32, S.POSE_A, 2)
    want = S.compiled(CHAIR, 32, S.POSE_A, 2)
    other = np.array(r.uniform, dtype=np.uint32)
    assert other[31] > 1
    other[31] -= 1
    assert native.load().ptx_set_frame(r._h, other.ctypes.data) == native.PTX_OK
    r.ResetFrameCount()
    tick(r)
    assert_tables(r, want, "after the layout was derived again")
    fr = oracle_mod.Frame(uniform_for(want, W, H, 1), want.scene, want.geometry, want.accel)
    oracle_step(oracle_mod, fr, "restir", want, r.uniform, False)
    compare(r, fr, "restir", "the frame after the changed layout key")
    stale = oracle_mod.Frame(uniform_for(want, W, H, 1), want.scene, E.base().geometry, E.base().accel)
    oracle_step(oracle_mod, stale, "restir", E.base(), r.uniform, False)
    assert (stale.gbuffer != fr.gbuffer).any(), "the pose must show in the frame"
    # the skin outlives the new layout
    S.pose(r, CHAIR, 32, S.POSE_B, 2)
    assert_tables(r, S.compiled(CHAIR, 32, S.POSE_B, 2), "pose B after the new layout")
    r.close()


def test_update_vertices_over_a_skinned_range_then_the_skin_again():
    r = make("restir")
    r.Update()
    S.set_skin(r, CHAIR, 3, 1)
    S.pose(r, CHAIR, 3, S.POSE_A, 1)
    first = (r.read_vertices(CHAIR), r.read_accel())
    r.UpdateVertices(CHAIR, V.bend())
    np.testing.assert_array_equal(r.read_vertices(CHAIR)[:, 0:3].view(np.float32), V.bend())
    assert (r.read_accel() != first[1]).any()
    S.pose(r, CHAIR, 3, S.POSE_A, 1)  # the bind tables are separate: the range is overwritten
    np.testing.assert_array_equal(r.read_vertices(CHAIR), first[0])
    np.testing.assert_array_equal(r.read_accel(), first[1])
    assert_tables(r, S.compiled(CHAIR, 3, S.POSE_A, 1), "the skin again")
    r.close()


# ------------------------------------------------------------------ bands
def test_two_bands_equal_the_whole_image():
    from pathtracerdemo_amd.renderer import Renderer
    R = 12  # (a band holds at least reuse_radius rows)
    one = make("reuse", reuse_radius=R)
    bands = [make("reuse", reuse_radius=R, row_begin=a, row_end=b) for a, b in ((0, 14), (14, H))]
    for f, (scale, yaw) in enumerate([(None, 0.0), (None, 0.0), (S.POSE_A, 0.0), (S.POSE_A, 0.0), (S.POSE_B, 1.5)], start=1):
        for x in [one] + bands:
            if f == 3:
                S.set_skin(x, CHAIR, 3, 2)
            if scale is not None:
                S.pose(x, CHAIR, 3, scale, 2)
            x.GetCamera().set_yaw(yaw)
            x.Update()
        one.Render()
        img = np.zeros((H, W, 4), np.float32)
        Renderer.render_bands(bands, img)
        assert_same(np.concatenate([x.read_gbuffer() for x in bands]), one.read_gbuffer(), f"G-buffer, frame {f}")
        assert_same(np.concatenate([x.read_reservoir() for x in bands]), one.read_reservoir(), f"temporal output, frame {f}")
        assert_same(np.concatenate([x.read_history() for x in bands]), one.read_history(), f"spatial output, frame {f}")
        assert_same(img, one.read_image(), f"radiance, frame {f}")
    for x in bands:
        np.testing.assert_array_equal(x.read_accel(), one.read_accel())
        np.testing.assert_array_equal(x.read_vertices(CHAIR), one.read_vertices(CHAIR))
    for x in [one] + bands:
        x.close()
