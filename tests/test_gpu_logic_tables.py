"""The logic kernels' shading tables (instances, materials, light records, light CDF) staged in
LDS (stage_shading, ptx_device.h) up to kShadeLdsMax = 16 KiB, read from global memory above it.

Two things the rest of the suite does not run:
* a scene BETWEEN the two caps -- its shading tables are over kShadeLdsMax while its root /
  instance tables still fit kLdsTableMax -- so the trace kernels take their LDS tables and the
  logic kernels the global ones;
* C3 frames so small that nearly every segment workgroup is empty or partly filled: the copy,
  the barrier it shares with the segment's counters, and the step kernels' empty-list skip.
Radiance and reservoirs are compared with the oracle BIT FOR BIT.
"""
import numpy as np
import pytest

from helpers import uniform_for
from test_gpu_large_tables import windows_scene

pytestmark = pytest.mark.gpu

K_LDS_TABLE_MAX = 24576  # ptx_device.h kLdsTableMax
K_SHADE_LDS_MAX = 16384  # ptx_device.h kShadeLdsMax
U_LIGHT_COUNT = 32
MOVE = (0.3, 0.1, 5.5)   # the camera of frame 3 in the moved case


def a16(n):
    return (n + 15) & ~15


def table_counts(cs):
    n_inst = cs.instance_count
    n_subs = sum(int(cs.scene[cs.offsets["mesh_descriptor"] + 6 * int(cs.scene[33 * i + 32]) + 5])
                 for i in range(n_inst))
    return n_inst, n_subs, int(uniform_for(cs, 8, 8)[U_LIGHT_COUNT])


def trace_table_bytes(cs):
    """tables_lds_bytes: 32 B per sub-mesh root, 176 B per instance."""
    n_inst, n_subs, _ = table_counts(cs)
    return a16(32 * n_subs) + 176 * n_inst


def shading_table_bytes(cs):
    """shading_lds_bytes: instances, 32 B of material per sub-mesh, 18 words per light, one CDF
    word per light; every section 16-byte aligned."""
    n_inst, n_subs, n_light = table_counts(cs)
    return a16(176 * n_inst) + a16(32 * n_subs) + a16(72 * n_light) + a16(4 * n_light)


def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != np.uint32:
        got, want = got.view(np.uint32), want.view(np.uint32)
    bad = np.any(got != want, axis=-1)
    assert bad.sum() == 0, f"{what}: {bad.sum()} pixels differ, first at {np.argwhere(bad)[:4].tolist()}"


@pytest.fixture(scope="module")
def between_caps():
    cs = windows_scene(100)  # 101 instances, 111 sub-meshes, 3 lights
    assert shading_table_bytes(cs) > K_SHADE_LDS_MAX   # the logic kernels read the global tables
    assert trace_table_bytes(cs) <= K_LDS_TABLE_MAX    # the trace kernels still stage theirs
    return cs


def test_c3_tables_fit(scene3):
    """The headline scene stages: its shading tables (3.4 KB) are far under the cap."""
    assert shading_table_bytes(scene3) <= K_SHADE_LDS_MAX // 4


def test_between_caps_restir(between_caps, oracle_mod):
    from pathtracerdemo_amd.renderer import Renderer
    cs, O, W, H = between_caps, oracle_mod, 40, 32
    r = Renderer(W, H, device=0, pipeline="restir")
    r.Initialize(cs)
    fr = O.Frame(uniform_for(cs, W, H, 1), cs.scene, cs.geometry, cs.accel)
    for f in (1, 2):
        r.Update()
        r.Render()
        fr.set_frame_index(f)
        fr.run(O.PASS_RESTIR, threads=8)
    assert_same(r.read_reservoir(), fr.reservoir, "PT_1 reservoirs")
    assert_same(r.read_image(), fr.accum, "accumulated radiance")
    r.close()


def reuse_frames(cs, O, W, H, move):
    """Three reuse frames on the GPU and in the oracle, optionally with a camera move between
    frames 2 and 3 (the motion temporal pass); compares frame 3's outputs."""
    from pathtracerdemo_amd.renderer import Renderer
    r = Renderer(W, H, device=0, pipeline="reuse")
    r.Initialize(cs)
    fr = O.Frame(uniform_for(cs, W, H, 1), cs.scene, cs.geometry, cs.accel)
    for f in (1, 2, 3):
        if move and f == 3:
            r.GetCamera().set_location(*MOVE)
        r.Update()
        r.Render()
        if move and f == 3:
            fr.set_camera(r.uniform)
        fr.set_frame_index(f)
        fr.run_reuse_frame(threads=8)
    assert_same(r.read_reservoir(), fr.reservoir, "temporal output")
    assert_same(r.read_history(), fr.res_hist, "spatial output")
    assert_same(r.read_image(), fr.accum, "accumulated radiance")
    r.close()


@pytest.mark.parametrize("move", [False, True], ids=["still", "moved"])
def test_between_caps_reuse(between_caps, oracle_mod, move):
    reuse_frames(between_caps, oracle_mod, 40, 32, move)


@pytest.mark.parametrize("W,H", [(8, 1), (37, 23)])
def test_c3_reuse_sparse_segments(scene3, oracle_mod, W, H):
    """LDS tables with (nearly) every segment workgroup empty or partly filled."""
    reuse_frames(scene3, oracle_mod, W, H, False)
