"""ptx_build_blas' SAH builder through the Node drop-in (ptx_node.c buildBlas, NativeRenderer.BuildBlas with
{builder: 'sah'}): tests/node/build_blas_sah.js builds case f of tests/lbvh_cases.py on a renderer without a
world; the roots, the reordered indices and the depth are the numpy rule's (scene/sah.py) bit for bit, {builder:
'lbvh'} and no options give the LBVH, and an unknown builder throws."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import lbvh_cases as L
import sah_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")


@pytest.mark.gpu
def test_build_blas_sah_equals_the_numpy_rule(tmp_path):
    name = "f_random"
    pos, idx, groups, max_leaf = S.cases()[name]
    np.ascontiguousarray(pos, np.float32).tofile(str(tmp_path / "positions.f32"))
    np.ascontiguousarray(idx, np.uint32).tofile(str(tmp_path / "indices.u32"))
    out = str(tmp_path / "built")
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "node", "build_blas_sah.js"), json.dumps(
        {"positions": str(tmp_path / "positions.f32"), "indices": str(tmp_path / "indices.u32"),
         "groups": [list(g) for g in groups], "maxLeaf": max_leaf, "out": out})],
        capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stderr
    res = json.loads(p.stdout)
    roots, new_idx, depth = S.reference(name)
    assert res["nodes"] == [len(r) // 8 for r in roots] and res["maxDepth"] == depth
    lbvh = [len(r) // 8 for r in L.reference(name)[0]]
    assert res["lbvhNodes"] == lbvh and res["defaultNodes"] == lbvh and lbvh != res["nodes"]
    assert all(m and m.startswith("TypeError") for m in res["refused"]), res["refused"]
    got = np.fromfile(out + ".nodes.u32", dtype=np.uint32)
    assert np.array_equal(L.fold_zero(got), L.fold_zero(np.concatenate(roots)))
    assert np.array_equal(np.fromfile(out + ".indices.u32", dtype=np.uint32), new_idx)
