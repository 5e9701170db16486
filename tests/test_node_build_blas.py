"""ptx_build_blas through the Node drop-in (pathtracerdemo_amd/js/: ptx_node.c buildBlas, NativeRenderer.BuildBlas):
tests/node/build_blas.js builds cases e and f of tests/lbvh_cases.py on a renderer without a world; the roots,
the reordered indices and the depth are the numpy rule's (scene/lbvh.py) bit for bit, in the shapes js/bvh.js
produces, and a position that is not finite, overlapping groups, a max_leaf past 64 and arrays of the wrong
shape throw."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import lbvh_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")


def test_the_addon_exports_build_blas():
    """No GPU: the function exists (non-enumerable, like updateVertices)."""
    src = ("try { const { addon, NativeRenderer } = require('./pathtracerdemo_amd/js/NativeRenderer.js');"
           "  process.stdout.write(JSON.stringify([typeof addon.buildBlas, Object.keys(addon).includes('buildBlas'),"
           "    typeof NativeRenderer.prototype.BuildBlas])); }"
           "catch (e) { process.stdout.write(/Cannot find module|ptx_node/.test(String(e)) ? '\"noaddon\"' : JSON.stringify(String(e))); }")
    p = subprocess.run([NODE, "-e", src], capture_output=True, text=True, cwd=ROOT, timeout=60)
    assert p.returncode == 0, p.stderr
    got = json.loads(p.stdout)
    if got == "noaddon":  # (build() makes the addon wherever the N-API header is installed: there it must load)
        assert not os.path.exists("/usr/include/node/node_api.h"), got
        return
    assert got == ["function", False, "function"], got


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["e_groups_and_gaps", "f_random"])
def test_build_blas_equals_the_numpy_rule(tmp_path, name):
    pos, idx, groups, max_leaf = L.cases()[name]
    np.ascontiguousarray(pos, np.float32).tofile(str(tmp_path / "positions.f32"))
    np.ascontiguousarray(idx, np.uint32).tofile(str(tmp_path / "indices.u32"))
    out = str(tmp_path / "built")
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "node", "build_blas.js"), json.dumps(
        {"positions": str(tmp_path / "positions.f32"), "indices": str(tmp_path / "indices.u32"),
         "groups": [list(g) for g in groups], "maxLeaf": max_leaf, "out": out})],
        capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stderr
    res = json.loads(p.stdout)
    roots, new_idx, depth = L.reference(name)
    assert res["nodes"] == [len(r) // 8 for r in roots] and res["maxDepth"] == depth and res["sameIndex"]
    assert "buildBlas" not in res["keys"]
    nan, overlap, leaf, floats, triple = res["refused"]
    assert nan and "(-1)" in nan and overlap and "(-1)" in overlap and leaf and "(-1)" in leaf, res["refused"]
    assert floats and floats.startswith("TypeError") and triple and triple.startswith("TypeError"), res["refused"]
    got = np.fromfile(out + ".nodes.u32", dtype=np.uint32)
    assert np.array_equal(L.fold_zero(got), L.fold_zero(np.concatenate(roots)))
    assert np.array_equal(np.fromfile(out + ".indices.u32", dtype=np.uint32), new_idx)
