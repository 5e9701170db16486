"""ptx_rebuild_mesh / ptx_read_scene / ptx_blas_cost on the GPU: a loaded mesh of c3_interior_32 rebuilt in place
after a pose far from its bind pose (tests/rebuild_cases.py).  The handle's arrays equal the numpy rule
(scene/world.py rebuild_mesh) -- scene and geometry BIT FOR BIT, accel after fold_zero; frames equal those of a
fresh handle that uploaded the rebuilt handle's own arrays, and the CPU oracle on them; the reuse history is
dropped, skins and the denoiser's history survive; the cost against the numpy rule; every refusal, each
leaving the handle rendering the unedited frame; two bands against the whole image; counters and memory."""
import ctypes
import dataclasses

import numpy as np
import pytest

import lbvh_cases as L
import rebuild_cases as RC
import scene_edits as E
import skin_edits as S
from helpers import uniform_for
from pathtracerdemo_amd.scene import world as Wd
from test_gpu_scene_edit import W, H, assert_same, make, tick

pytestmark = pytest.mark.gpu
CHAIR, WINDOW, ROOM = RC.CHAIR, RC.WINDOW, RC.ROOM
READS = ("read_image", "read_gbuffer", "read_reservoir", "read_history")


def pose8(r):
    """The chair's 32-joint skin bound and posed at scale 8."""
    S.set_skin(r, CHAIR, RC.JOINTS)
    r.SkinVertices(CHAIR, RC.palette8())


def assert_arrays(got, want, what):
    scene, geometry, accel = got
    np.testing.assert_array_equal(scene, want.scene, f"{what}: scene")
    np.testing.assert_array_equal(geometry, want.geometry, f"{what}: geometry")
    assert len(accel) == len(want.accel), f"{what}: accel length {len(accel)}, want {len(want.accel)}"
    bad = np.nonzero(L.fold_zero(accel) != L.fold_zero(want.accel))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} accel words differ, first {bad[:8].tolist()}"


def same_frames(a, b, what, reads=READS):
    for name in reads:
        assert_same(getattr(a, name)(), getattr(b, name)(), f"{what}: {name}")


# ------------------------------------------------------------------ 1. arrays
@pytest.mark.parametrize("case", ["chair_sah", "room_lbvh"])
def test_arrays_are_the_python_rule(case):
    r = make("restir")
    r.Update()
    if case == "chair_sah":
        pose8(r)
        np.testing.assert_array_equal(r.compiled.geometry, RC.posed().geometry)
        mesh, builder, want, before = CHAIR, "sah", RC.rebuilt("sah"), RC.posed()
    else:
        S.set_skin(r, ROOM, 3)
        S.pose(r, ROOM, 3, S.POSE_A)
        mesh, builder, want, before = ROOM, "lbvh", RC.room_rebuilt(), RC.room_posed()
    info = r.RebuildMesh(mesh, builder)
    assert_arrays(r.read_scene(), want, case)
    c = r.compiled
    assert_arrays((c.scene, c.geometry, c.accel), want, f"{case}: compiled")
    assert c.max_bvh_depth == want.max_bvh_depth and c.offsets == want.offsets
    roots = Wd.mesh_blocks(want, mesh)["roots"]
    assert info == dict(n_accel=len(want.accel), mesh_nodes=RC.node_count(want, mesh),
                        max_depth=max(Wd._root_leaves(want.accel[s:e])[2] for s, e in roots),
                        scene_words=int((want.scene != before.scene).sum()))
    assert info["scene_words"] == (2 if case == "room_lbvh" else 0)
    assert (len(want.accel) != len(before.accel)) or case == "chair_sah"
    np.testing.assert_array_equal(r.read_accel(), r.compiled.accel)
    first = [a.copy() for a in r.read_scene()]
    assert r.RebuildMesh(mesh, builder) == dict(info, scene_words=0)  # (the same length again: no descriptor moves)
    for a, b in zip(r.read_scene(), first):
        np.testing.assert_array_equal(a, b, "a second rebuild returns the same bytes")
    r.close()


# ------------------------------------------------------------------ 2. frames
def oracle_frame(O, cs, pipeline, uniform):
    fr = O.Frame(uniform, cs.scene, cs.geometry, cs.accel)
    fr.set_frame_index(int(uniform[23]))
    if pipeline == "reuse":
        fr.run_reuse_frame(threads=8)
    elif pipeline == "gi":
        fr.run_gi_frame(threads=8)
    else:
        fr.run(O.PASS_RESTIR if pipeline == "restir" else O.PASS_MCPT, threads=8)
    return fr


@pytest.mark.parametrize("pipeline", ["restir", "reuse", "gi", "mcpt"])
def test_frames_equal_a_fresh_handle_with_the_rebuilt_arrays(oracle_mod, pipeline):
    r = make(pipeline)
    tick(r)
    pose8(r)
    r.RebuildMesh(CHAIR, "sah")
    r.reset_accumulation()
    r.ResetFrameCount()
    fresh = make(pipeline, cs=r.compiled)
    for f in (1, 2):
        tick(r)
        tick(fresh)
        assert np.array_equal(r.uniform, fresh.uniform)
        # (mcpt keeps an accumulation alone; restir has no spatial output)
        same_frames(r, fresh, f"{pipeline}, frame {f}", {"mcpt": READS[:1], "restir": READS[:3]}.get(pipeline, READS))
        if pipeline == "restir" and f == 1:
            fr = oracle_frame(oracle_mod, r.compiled, pipeline, r.uniform)
            assert_same(r.read_image(), fr.accum, "accumulation against the oracle")
            assert_same(r.read_gbuffer(), fr.gbuffer, "G-buffer against the oracle")
            assert_same(r.read_reservoir(), fr.reservoir, "reservoirs against the oracle")
            stale = oracle_frame(oracle_mod, E.base(), pipeline, r.uniform)
            assert (stale.gbuffer != fr.gbuffer).any(), "the pose must show in the frame"
    r.close()
    fresh.close()


# ------------------------------------------------------------------ 3. the reuse history is dropped
@pytest.mark.parametrize("pipeline", ["reuse", "gi"])
def test_the_reuse_history_is_dropped(pipeline):
    r = make(pipeline)
    tick(r)
    tick(r)
    if pipeline == "reuse":
        assert (r.read_reservoir()[..., 29] > 1).any(), "a history is in use before the rebuild"
    pose8(r)
    r.RebuildMesh(CHAIR, "sah")
    tick(r)  # frame 3: the same camera, no reset
    fresh = make(pipeline, cs=r.compiled)
    fresh.frame_count = 2
    tick(fresh)
    assert np.array_equal(r.uniform, fresh.uniform)
    assert_same(r.read_history(), fresh.read_history(), "the spatial output of the frame after the rebuild")
    assert_same(r.read_reservoir(), fresh.read_reservoir(), "its temporal output")
    r.close()
    fresh.close()


# ------------------------------------------------------------------ 4. skins survive
def test_skins_survive():
    r = make("restir")
    r.Update()
    pose8(r)
    r.RebuildMesh(CHAIR, "sah")
    S.pose(r, CHAIR, RC.JOINTS, S.POSE_B)  # no SetSkin in between
    want = Wd.skin_mesh(RC.rebuilt("sah"), CHAIR, RC.chair_skin(), S.palette(CHAIR, RC.JOINTS, S.POSE_B))
    np.testing.assert_array_equal(r.read_vertices(CHAIR), S.block(want, CHAIR))
    got = r.read_accel()
    assert int((L.fold_zero(got) != L.fold_zero(want.accel)).sum()) == 0, "the refit on the new topology"
    assert_arrays(r.read_scene(), want, "read_scene after the pose")
    np.testing.assert_array_equal(r.compiled.geometry, want.geometry)
    r.close()


# ------------------------------------------------------------------ 5. the denoiser's history survives
def test_the_denoiser_history_survives():
    from pathtracerdemo_amd import _native as native
    r = make("reuse", frame_color=True)
    tick(r)
    r.Denoise(temporal=True, iterations=2)
    g0 = r.read_gbuffer()
    assert r.read_denoise_history()[..., 3].max() == 1
    r.RebuildMesh(CHAIR, "sah")  # the undeformed chair
    p = native.PtxDenoiseParams()
    p.reserved[0] = 1
    assert r._lib.ptx_denoise(r._h, ctypes.byref(p)) == native.PTX_E_INVALID, "no frame has run since the rebuild"
    tick(r)
    r.Denoise(temporal=True, iterations=2)
    g1 = r.read_gbuffer()
    n = r.read_denoise_history()[..., 3]
    hit = (g0[..., 0] >> 31 == 1) & (g1[..., 0] >> 31 == 1)
    kept = hit & (g0[..., 0] == g1[..., 0])
    print(f"{int(hit.sum())} hit pixels, {int(kept.sum())} with the same key word, n == 2 on {int((n[kept] == 2).sum())}")
    assert (n[kept] == 2).all()
    assert 2 * int(kept.sum()) >= int(hit.sum()) > 0
    r.close()


# ------------------------------------------------------------------ 6. cost
def assert_cost(r, cs, what):
    out = {}
    for mesh in range(3):
        got, want = r.blas_cost(mesh), Wd.mesh_cost(cs, mesh)
        nodes = RC.node_count(cs, mesh)
        print(f"{what}: mesh {mesh}: {got!r} against {want!r}, {nodes} nodes, |diff| / want = {abs(got - want) / want:.3e}")
        assert abs(got - want) <= nodes * 2.0 ** -52 * want, f"{what}: mesh {mesh}: {got!r} against {want!r}"
        assert r.blas_cost(mesh) == got, "two calls give equal bits"
        out[mesh] = got
    return out


def test_cost_is_the_python_rule():
    r = make("restir")
    r.Update()
    assert_cost(r, E.base(), "at upload")
    pose8(r)
    before = assert_cost(r, r.compiled, "after the scale-8 refit")[CHAIR]
    assert abs(before - Wd.mesh_cost(RC.posed(), CHAIR)) <= 3525 * 2.0 ** -52 * before
    r.RebuildMesh(CHAIR, "sah")
    after = assert_cost(r, r.compiled, "after the rebuild")[CHAIR]
    assert after <= 0.85 * before
    r.close()


# ------------------------------------------------------------------ 7. refusals
def refused(r, code, mesh=CHAIR, builder=1, max_leaf=0):
    from pathtracerdemo_amd import _native as native
    info = native.PtxRebuildInfo()
    assert r._lib.ptx_rebuild_mesh(r._h, mesh, builder, max_leaf, ctypes.byref(info)) == code
    return r._lib.ptx_last_error(r._h).decode()


def twins(cs=None):
    """Two reuse handles of one scene after two frames each: the refused call goes to the first."""
    pair = make("reuse", cs=cs), make("reuse", cs=cs)
    for x in pair:
        tick(x)
        tick(x)
    return pair


def assert_unedited(r, twin, what):
    """The next two frames, history and all, are those of the handle that never saw the call."""
    for yaw in (0.0, 1.5):
        tick(r, yaw)
        tick(twin, yaw)
        same_frames(r, twin, f"{what}, yaw {yaw}")
    for a, b in zip(r.read_scene(), twin.read_scene()):
        np.testing.assert_array_equal(a, b)
    assert (r.read_reservoir()[..., 29] > 1).any(), "the history was kept"
    r.close()
    twin.close()


def test_refused_parameters_leave_the_unedited_frame():
    from pathtracerdemo_amd import _native as native
    from pathtracerdemo_amd.renderer import Renderer
    lib = native.load()
    assert lib.ptx_rebuild_mesh(None, CHAIR, 1, 0, None) == native.PTX_E_INVALID
    bare = Renderer(W, H, device=0, pipeline="reuse")
    sizes = [ctypes.c_size_t(7) for _ in range(3)]
    cost = ctypes.c_double(0.0)
    assert lib.ptx_rebuild_mesh(bare._h, CHAIR, 1, 0, None) == native.PTX_E_INVALID  # no scene
    assert lib.ptx_scene_sizes(bare._h, *[ctypes.byref(k) for k in sizes]) == native.PTX_E_INVALID
    assert lib.ptx_blas_cost(bare._h, CHAIR, ctypes.byref(cost)) == native.PTX_E_INVALID
    bare.Initialize(E.base())
    assert lib.ptx_rebuild_mesh(bare._h, CHAIR, 1, 0, None) == native.PTX_E_INVALID  # no frame set: no layout
    assert lib.ptx_read_scene(bare._h, None, 0, None, 0, None, 0) == native.PTX_E_INVALID
    assert lib.ptx_scene_sizes(bare._h, *[ctypes.byref(k) for k in sizes]) == native.PTX_OK
    assert [int(k.value) for k in sizes] == [len(E.base().scene), len(E.base().geometry), len(E.base().accel)]
    with pytest.raises(ValueError):
        bare.RebuildMesh(CHAIR)
    bare.close()
    r, twin = twins()
    refused(r, native.PTX_E_INVALID, builder=2)
    refused(r, native.PTX_E_INVALID, max_leaf=65)
    assert "mesh 3" in refused(r, native.PTX_E_SCENE, mesh=3)
    with pytest.raises(ValueError):
        r.RebuildMesh(CHAIR, "median")
    assert lib.ptx_blas_cost(r._h, 3, ctypes.byref(cost)) == native.PTX_E_SCENE
    assert lib.ptx_blas_cost(r._h, CHAIR, None) == native.PTX_E_INVALID
    n = len(E.base().accel)
    out = np.zeros(n + 1, np.uint32)
    assert lib.ptx_read_scene(r._h, None, 0, None, 0, out.ctypes.data, n + 1) == native.PTX_E_INVALID  # a wrong length
    assert lib.ptx_read_scene(r._h, None, 0, None, 0, None, n) == native.PTX_E_INVALID
    assert lib.ptx_read_scene(r._h, None, 0, None, 0, out.ctypes.data, n) == native.PTX_OK  # NULL with 0 is skipped
    np.testing.assert_array_equal(out[:n], E.base().accel)
    assert r.stats()["kernel_launches"][native.PTX_STAT_BUILD] == 0
    assert_unedited(r, twin, "refused parameters")


def _broken(case):
    """C3 with arrays ptx_upload_scene accepts and ptx_rebuild_mesh(chair) must refuse."""
    base = E.base()
    o = base.offsets
    b = Wd.mesh_blocks(base, CHAIR)
    scene, geometry, accel = base.scene.copy(), base.geometry.copy(), base.accel.copy()
    s1, e1 = b["roots"][1]
    leaf = next(w for w in range(s1, e1, 8) if accel[w + 7] & 0xFFFF0000)
    if case == "roots_overlap":        # a leaf of root 1 names triangles of root 0
        accel[leaf + 6] = 0
    elif case == "leaves_do_not_tile":  # a hole in root 1's range
        assert (accel[leaf + 7] & 0xFFFF) > 1
        accel[leaf + 7] -= 1
    elif case == "index_past_the_vertices":
        n_vert = (b["vertex_end"] - b["vertex"]) // Wd.STRIDE_VERTEX
        geometry[b["index"] + 3 * 12400 + 1] = n_vert  # (a triangle of root 1: the word lies in the index block)
    elif case == "shared_blas":        # the window traces the chair's first root
        scene[o["mesh_descriptor"] + 6 * WINDOW + 4] = scene[o["mesh_descriptor"] + 6 * CHAIR + 4]
    return dataclasses.replace(base, scene=scene, geometry=geometry, accel=accel)


@pytest.mark.parametrize("case", ["roots_overlap", "leaves_do_not_tile", "index_past_the_vertices", "shared_blas"])
def test_refused_scenes_leave_the_unedited_frame(case):
    from pathtracerdemo_amd import _native as native
    cs = _broken(case)
    with pytest.raises(ValueError):
        Wd.rebuild_mesh(cs, CHAIR, "sah")
    r, twin = twins(cs)
    msg = refused(r, native.PTX_E_SCENE)
    print(f"{case}: {msg}")
    assert "ptx_rebuild_mesh" in msg
    assert r.stats()["kernel_launches"][native.PTX_STAT_BUILD] == 0, "refused before anything is launched"
    assert_unedited(r, twin, case)


def test_the_oversized_leaf_is_refused_for_sah_and_split_by_lbvh():
    from pathtracerdemo_amd import _native as native
    from pathtracerdemo_amd.scene.lbvh import build_blas_lbvh
    cs, idx = L.one_instance_scene("f_random", build_blas_lbvh)
    pair = make("reuse", cs=cs), make("reuse", cs=cs)
    corner = np.array([[0.25, 0.5, 1.0], [1.25, 0.5, 1.0], [0.25, 1.5, 2.0]], np.float32)
    pos = np.zeros((len(idx), 3), np.float32)
    pos[idx.reshape(-1, 3)] = corner  # every triangle has its own three vertices: all onto the same three points
    for x in pair:
        tick(x)
        x.UpdateVertices(0, pos)
        tick(x)
    r, twin = pair
    msg = refused(r, native.PTX_E_SCENE, mesh=0, builder=native.PTX_BLAS_SAH)
    assert "leaf of 1000 triangles" in msg, msg
    with pytest.raises(native.PtxError):
        r.RebuildMesh(0, "sah")
    for a, b in zip(r.read_scene(), twin.read_scene()):
        np.testing.assert_array_equal(a, b)
    tick(r)
    tick(twin)
    same_frames(r, twin, "after the refused SAH rebuild")
    info = r.RebuildMesh(0, "lbvh")  # identical codes split by position
    want = Wd.rebuild_mesh(twin.compiled, 0, "lbvh")
    assert_arrays(r.read_scene(), want, "the LBVH rebuild of identical triangles")
    leaves = want.accel.reshape(-1, 8)
    assert (leaves[leaves[:, 7] >> 16 == 0xFFFF, 7] & 0xFFFF).max() <= 10 and info["mesh_nodes"] == len(leaves)
    r.close()
    twin.close()


# ------------------------------------------------------------------ 8. bands
def test_two_bands_equal_the_whole_image():
    from pathtracerdemo_amd.renderer import Renderer
    R = 12  # (a band holds at least reuse_radius rows)
    one = make("reuse", reuse_radius=R)
    bands = [make("reuse", reuse_radius=R, row_begin=a, row_end=b) for a, b in ((0, 14), (14, H))]
    for f in range(1, 6):
        for x in [one] + bands:
            if f == 3:
                pose8(x)
                x.RebuildMesh(CHAIR, "sah")
            x.GetCamera().set_yaw(1.5 if f == 5 else 0.0)
            x.Update()
        one.Render()
        img = np.zeros((H, W, 4), np.float32)
        Renderer.render_bands(bands, img)
        assert_same(np.concatenate([x.read_gbuffer() for x in bands]), one.read_gbuffer(), f"G-buffer, frame {f}")
        assert_same(np.concatenate([x.read_reservoir() for x in bands]), one.read_reservoir(), f"temporal output, frame {f}")
        assert_same(np.concatenate([x.read_history() for x in bands]), one.read_history(), f"spatial output, frame {f}")
        assert_same(img, one.read_image(), f"radiance, frame {f}")
    for x in bands:
        for a, b in zip(x.read_scene(), one.read_scene()):
            np.testing.assert_array_equal(a, b)
    for x in [one] + bands:
        x.close()


# ------------------------------------------------------------------ 9. stats
def test_launches_and_memory():
    from pathtracerdemo_amd import _native as native
    slot = native.PTX_STAT_BUILD
    r = make("restir", time_launches=True)
    r.Update()
    pose8(r)
    b = Wd.mesh_blocks(r.compiled, CHAIR)
    rec = S.block(r.compiled, CHAIR)
    s0 = r.stats()
    r.build_blas(rec[:, 0:3].copy().view(np.float32), r.compiled.geometry[b["index"]:b["index_end"]], RC.CHAIR_GROUPS, builder="sah")
    s1 = r.stats()
    builder = s1["kernel_launches"][slot] - s0["kernel_launches"][slot]
    assert builder > 0
    info = r.RebuildMesh(CHAIR, "sah")
    s2 = r.stats()
    assert s2["kernel_launches"][slot] - s1["kernel_launches"][slot] == builder + 1, "the builder's launches, plus one"
    assert s2["kernel_ms_total"][slot] > s1["kernel_ms_total"][slot]
    for k in range(16):
        assert k == slot or s2["kernel_launches"][k] == s0["kernel_launches"][k]
    # the layout's tables: 64 B per pair and 4 B each in the refit order and the per-pair sub-mesh table
    pairs = lambda cs: sum(int(((cs.accel[s:e].reshape(-1, 8)[:, 7] >> 16) == 0).sum()) for m in range(3)
                           for s, e in Wd.mesh_blocks(cs, m)["roots"])
    want, before = RC.rebuilt("sah"), RC.posed()
    assert s2["device_bytes"] - s1["device_bytes"] == (64 + 4 + 4) * (pairs(want) - pairs(before))
    assert s2["bvh_nodes"] == pairs(want) and s1["bvh_nodes"] == pairs(before)
    assert s2["max_bvh_depth"] == want.max_bvh_depth == r.compiled.max_bvh_depth
    assert s2["triangles"] == s1["triangles"] and info["mesh_nodes"] == RC.node_count(want, CHAIR)
    r.blas_cost(CHAIR)
    s3 = r.stats()
    assert s3["kernel_launches"][slot] - s2["kernel_launches"][slot] == 1 and s3["device_bytes"] == s2["device_bytes"]
    r.close()
