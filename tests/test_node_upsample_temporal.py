"""ptx_phase_uniform and ptx_upsample_temporal through the Node drop-in (pathtracerdemo_amd/js/:
ptx_node.c phaseUniform / upsampleTemporal, NativeRenderer.SetPhaseOf / UpsampleTemporal /
ReadUpsampleHistory): tests/node/upsample_temporal_pair.js cycles three phases on a small
NativeRenderer and integrates them on a full-size one; the result equals the ctypes host's bits for
the same uniforms."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
w, h, S = 16, 12, 2
PHASES = [(0, 0), (1, 1), (1, 0)]


def test_the_addon_exports_the_temporal_upsampler():
    """No GPU: the functions exist (non-enumerable, like the denoiser's) and phaseUniform equals the ctypes helper."""
    from pathtracerdemo_amd import _native as N
    from helpers import uniform_for
    from pathtracerdemo_amd.scene.world import compile_scene
    u = uniform_for(compile_scene("dummy_scene_1"), 96, 72, yaw=7.0, pitch=-3.0)
    src = ("try { const { addon, NativeRenderer } = require('./pathtracerdemo_amd/js/NativeRenderer.js');"
           f"  const u = Uint32Array.from({json.dumps([int(v) for v in u])});"
           "  let refused = false; try { addon.phaseUniform(u, 5, 0, 0); } catch (e) { refused = /\\(-1\\)/.test(String(e)); }"
           "  process.stdout.write(JSON.stringify([typeof addon.upsampleTemporal, typeof addon.phaseUniform,"
           "    Object.keys(addon).includes('upsampleTemporal') || Object.keys(addon).includes('phaseUniform'),"
           "    typeof NativeRenderer.prototype.UpsampleTemporal, typeof NativeRenderer.prototype.SetPhaseOf,"
           "    typeof NativeRenderer.prototype.ReadUpsampleHistory, Array.from(addon.phaseUniform(u, 3, 2, 0)), refused])); }"
           "catch (e) { process.stdout.write(/Cannot find module|ptx_node/.test(String(e)) ? '\"noaddon\"' : JSON.stringify(String(e))); }")
    p = subprocess.run([NODE, "-e", src], capture_output=True, text=True, cwd=ROOT, timeout=60)
    assert p.returncode == 0, p.stderr
    got = json.loads(p.stdout)
    if got == "noaddon":  # (build() makes the addon wherever the N-API header is installed: there it must load)
        assert not os.path.exists("/usr/include/node/node_api.h"), got
        return
    assert got[:6] == ["function", "function", False, "function", "function", "function"] and got[7] is True, got
    np.testing.assert_array_equal(np.array(got[6], dtype=np.uint64).astype(np.uint32), N.phase_uniform(u, 3, 2, 0))


@pytest.mark.gpu
def test_upsample_temporal_through_the_addon(scene3, tmp_path):
    from pathtracerdemo_amd import _native as N
    from pathtracerdemo_amd.renderer import Renderer
    from pathtracerdemo_amd.scene.export import export_compiled
    d = export_compiled(scene3, str(tmp_path / "scene"), "scene3")
    out = str(tmp_path / "ut")
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "node", "upsample_temporal_pair.js"), json.dumps(
        {"sceneDir": d, "width": w, "height": h, "scale": S, "pipeline": "restir", "phases": PHASES, "alphaFill": 0.3,
         "out": out})], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stderr
    res = json.loads(p.stdout)
    assert "upsampleTemporal" not in res["keys"]
    u_hi = np.array(res["hi"], dtype=np.uint64).astype(np.uint32)
    hi = Renderer(S * w, S * h, device=0)
    hi.Initialize(scene3)
    hi.set_uniform(u_hi)
    hi.run_pass(N.PTX_PASS_GBUFFER)
    lo = Renderer(w, h, device=0)
    lo.Initialize(scene3)
    for (px, py), words in zip(PHASES, res["lo"]):
        lo.set_phase_of(hi, S, px, py)
        np.testing.assert_array_equal(lo.uniform, np.array(words, dtype=np.uint64).astype(np.uint32))
        lo.Render()
        lo.Denoise()
        hi.UpsampleTemporal(lo, px, py, alpha_fill=0.3)
    want, want_hist = hi.read_denoised(), hi.read_upsample_history()
    got = np.fromfile(out + ".hi.f32", dtype=np.float32).reshape(S * h, S * w, 4)
    got_hist = np.fromfile(out + ".hist.f32", dtype=np.float32).reshape(S * h, S * w, 4)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(got_hist.view(np.uint32), want_hist.view(np.uint32))
    assert (got[..., 3] == 1).all() and set(np.unique(got_hist[..., 3])) == {0.0, 1.0}
    hi.close()
    lo.close()
