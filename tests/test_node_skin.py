"""ptx_set_skin, ptx_skin_vertices and ptx_read_vertices through the Node drop-in (pathtracerdemo_amd/js/:
ptx_node.c setSkin / skinVertices / readVertices, NativeRenderer.SetSkin / SkinVertices / ReadVertices):
tests/node/skin.js renders a frame, binds the chair's skin, poses it, reads the posed records and the refitted
accel array and renders the next frame; records, accel array and frame are the ctypes host's bit for bit, and
the library's refusals and the addon's argument errors throw and change nothing."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import scene_edits as E
import skin_edits as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
W, H = 48, 32


def test_the_addon_exports_the_skin_calls():
    """No GPU: the functions exist (non-enumerable, like updateVertices)."""
    src = ("try { const { addon, NativeRenderer } = require('./pathtracerdemo_amd/js/NativeRenderer.js');"
           "  const names = ['setSkin', 'skinVertices', 'readVertices'];"
           "  process.stdout.write(JSON.stringify([names.map((n) => typeof addon[n]),"
           "    names.map((n) => Object.keys(addon).includes(n)),"
           "    ['SetSkin', 'SkinVertices', 'ReadVertices'].map((n) => typeof NativeRenderer.prototype[n])])); }"
           "catch (e) { process.stdout.write(/Cannot find module|ptx_node/.test(String(e)) ? '\"noaddon\"' : JSON.stringify(String(e))); }")
    p = subprocess.run([NODE, "-e", src], capture_output=True, text=True, cwd=ROOT, timeout=60)
    assert p.returncode == 0, p.stderr
    got = json.loads(p.stdout)
    if got == "noaddon":  # (build() makes the addon wherever the N-API header is installed: there it must load)
        assert not os.path.exists("/usr/include/node/node_api.h"), got
        return
    assert got == [["function"] * 3, [False] * 3, ["function"] * 3], got


@pytest.mark.gpu
def test_skin_vertices_then_render_equals_the_python_handle(tmp_path):
    from pathtracerdemo_amd.renderer import Renderer
    from pathtracerdemo_amd.scene.export import export_compiled
    base = E.base()
    scene_dir = export_compiled(base, str(tmp_path / "base"), "base")
    mesh, joints, morph = S.CHAIR_MESH, 3, 2
    sk, pal = S.skin(mesh, joints, morph), S.palette(mesh, joints, S.POSE_A)
    files = {"joints.u32": sk.joints, "weights.f32": sk.weights, "bind.f32": sk.bind, "targets.f32": sk.target_pos,
             "normals.f32": sk.target_nrm, "palette.f32": pal, "tw.f32": S.TW}
    for name, a in files.items():
        np.ascontiguousarray(a).tofile(str(tmp_path / name))
    out = str(tmp_path / "frame")
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "node", "skin.js"), json.dumps(
        {"sceneDir": scene_dir, "dir": str(tmp_path), "mesh": mesh, "width": W, "height": H, "pipeline": "reuse",
         "out": out})], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stderr
    res = json.loads(p.stdout)
    assert res["unchanged"] and res["stillUploaded"] and res["worldAccel"] and res["worldGeometry"] and res["untouched"], res
    assert not {"setSkin", "skinVertices", "readVertices"} & set(res["keys"])
    ref = res["refused"]
    assert len(ref) == 14 and all(ref), ref
    assert "no skin" in ref[0]
    assert "(-1)" in ref[1] and "(-3)" in ref[2] and "(-1)" in ref[3] and "(-1)" in ref[10], ref
    for k in (4, 5, 6, 7, 8, 9, 13):  # thrown before the library is called
        assert ref[k].startswith("TypeError"), (k, ref[k])
    assert ref[11].startswith("RangeError") and ref[12].startswith("RangeError"), ref
    r = Renderer(W, H, device=0, pipeline="reuse")
    r.Initialize(base)
    r.Update()
    r.Render()
    S.set_skin(r, mesh, joints, morph)
    S.pose(r, mesh, joints, S.POSE_A, morph)
    want = S.compiled(mesh, joints, S.POSE_A, morph)
    np.testing.assert_array_equal(r.compiled.accel, want.accel)
    np.testing.assert_array_equal(np.fromfile(out + ".accel.u32", dtype=np.uint32), r.read_accel())
    np.testing.assert_array_equal(np.fromfile(out + ".records.u32", dtype=np.uint32).reshape(-1, 8), r.read_vertices(mesh))
    np.testing.assert_array_equal(r.read_vertices(mesh), S.block(want, mesh))
    r.Update()
    r.Render()
    np.testing.assert_array_equal(r.uniform, np.array(res["uniform"], dtype=np.uint64).astype(np.uint32))
    got = np.fromfile(out + ".f32", dtype=np.float32).reshape(H, W, 4)
    np.testing.assert_array_equal(got.view(np.uint32), r.read_image().view(np.uint32))
    r.close()
