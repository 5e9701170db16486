"""ptx_upsample_follow through the Node drop-in (pathtracerdemo_amd/js/: ptx_node.c upsampleFollow,
NativeRenderer.SetUpsampleFollow): tests/node/upsample_follow.js makes five UpsampleTemporal calls, moves the chair
with UpdateWorld on both renderers and makes one more.  With the switch on the history's n exceeds 1 somewhere and
the history equals the ctypes host's bit for bit; with it off the edit drops the history and n exceeds 1 nowhere."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import scene_edits as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
W, H, S, CALLS = 96, 72, 2, 5


def test_the_addon_exports_upsample_follow():
    """No GPU: the function exists (non-enumerable, like the denoiser's) and the renderer has the method."""
    src = ("try { const { addon, NativeRenderer } = require('./pathtracerdemo_amd/js/NativeRenderer.js');"
           "  process.stdout.write(JSON.stringify([typeof addon.upsampleFollow, Object.keys(addon).includes('upsampleFollow'),"
           "    typeof NativeRenderer.prototype.SetUpsampleFollow])); }"
           "catch (e) { process.stdout.write(/Cannot find module|ptx_node/.test(String(e)) ? '\"noaddon\"' : JSON.stringify(String(e))); }")
    p = subprocess.run([NODE, "-e", src], capture_output=True, text=True, cwd=ROOT, timeout=60)
    assert p.returncode == 0, p.stderr
    got = json.loads(p.stdout)
    if got == "noaddon":  # (build() makes the addon wherever the N-API header is installed: there it must load)
        assert not os.path.exists("/usr/include/node/node_api.h"), got
        return
    assert got == ["function", False, "function"], got


def python_side(follow):
    from pathtracerdemo_amd import _native as N
    from pathtracerdemo_amd.renderer import Renderer
    hi = Renderer(W, H, device=0, pipeline="reuse", frame_color=True)
    lo = Renderer(W // S, H // S, device=0, pipeline="reuse", frame_color=True)
    for r in (hi, lo):
        r.Initialize(E.base())
    if follow:
        hi.set_upsample_follow(True)
    for k in range(CALLS + 1):
        if k == CALLS:
            assert [r.UpdateScene(E.edited("move")) for r in (hi, lo)] == [1, 1]
        px, py = k % S, k // S % S
        hi.Update()
        hi.run_pass(N.PTX_PASS_GBUFFER)
        lo.set_phase_of(hi, S, px, py)
        lo.Render()
        lo.Denoise(temporal=True, iterations=2)
        hi.UpsampleTemporal(lo, px, py)
    out = hi.read_upsample_history(), hi.uniform.copy()
    hi.close()
    lo.close()
    return out


@pytest.mark.gpu
def test_update_world_keeps_the_history_with_the_switch_on_only(tmp_path):
    from pathtracerdemo_amd.scene.export import export_scene_assets
    assets = export_scene_assets(E.SCENE, str(tmp_path / "assets"))
    n = {}
    for follow in (True, False):
        out = str(tmp_path / f"follow{int(follow)}")
        p = subprocess.run([NODE, os.path.join(ROOT, "tests", "node", "upsample_follow.js"), json.dumps(
            {"assetsDir": assets, "move": [25, -90, 10], "width": W // S, "height": H // S, "scale": S, "pipeline": "reuse",
             "calls": CALLS, "follow": follow, "out": out})], capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert p.returncode == 0, p.stderr
        res = json.loads(p.stdout)
        assert res["masks"] == [1, 1] and "upsampleFollow" not in res["keys"]
        hist = np.fromfile(out + ".hist.f32", dtype=np.float32).reshape(H, W, 4)
        n[follow] = hist[..., 3]
        if follow:  # the same calls through the ctypes host: the same bits
            want, uniform = python_side(True)
            np.testing.assert_array_equal(uniform, np.array(res["uniform"], dtype=np.uint64).astype(np.uint32))
            np.testing.assert_array_equal(hist.view(np.uint32), want.view(np.uint32))
    assert (n[True] > 1).any(), "with the switch on the history must survive the move"
    assert n[False].max() <= 1, "with the switch off an instance edit drops the history"
