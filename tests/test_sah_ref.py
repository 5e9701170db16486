"""The GPU SAH builder's rule without a GPU (scene/sah.py build_blas_sah, the definition of ptx_build_blas'
PTX_BLAS_SAH in include/ptx.h): on every case of tests/sah_cases.py its nodes and depth are the host builder's
(scene/bvh.py build_blas) raw, its leaves hold the same triangles in input order, the refit reproduces its
boxes; the ulp case takes the rule's two awkward branches."""
import numpy as np
import pytest

import lbvh_cases as L
import sah_cases as S


@pytest.mark.parametrize("name", S.NAMES)
def test_nodes_and_depth_are_the_host_builders(name):
    """The property the builder rests on: a stable partition changes no node word."""
    roots, _, depth = S.reference(name)
    host_roots, _, host_depth = S.host_reference(name)
    assert depth == host_depth
    assert len(roots) == len(host_roots)
    for k, (a, b) in enumerate(zip(roots, host_roots)):
        assert a.dtype == np.uint32 and np.array_equal(a, b), f"{name}: root {k} differs from build_blas'"


def _triangle_ids(name, new_idx):
    """The input position of the triangle at each output position ((T,) int; by vertex triple, so equal triples
    are interchangeable: ids of the first)."""
    idx = S.cases()[name][1].reshape(-1, 3)
    first_of = {}
    for t, tri in enumerate(map(tuple, idx.tolist())):
        first_of.setdefault(tri, t)
    return np.array([first_of[tuple(tri)] for tri in new_idx.reshape(-1, 3).tolist()], np.int64)


@pytest.mark.parametrize("name", S.NAMES)
def test_leaves_hold_the_host_builders_triangles_in_input_order(name):
    pos, idx, groups, _ = S.cases()[name]
    roots, new_idx, _ = S.reference(name)
    _, host_idx, _ = S.host_reference(name)
    assert new_idx.dtype == np.uint32 and new_idx.shape == idx.shape
    a, b = idx.reshape(-1, 3), new_idx.reshape(-1, 3)
    assert np.array_equal(a[np.lexsort(a.T[::-1])], b[np.lexsort(b.T[::-1])]), "a permutation of the triangles"
    grouped = np.zeros(len(a), bool)
    for first, count in groups:
        grouped[first:first + count] = True
    assert np.array_equal(b[~grouped], a[~grouped]), "an ungrouped triangle moved"
    mine, hosts = _triangle_ids(name, new_idx), _triangle_ids(name, host_idx)
    n_leaves = 0
    for root in roots:
        for first, count in S.leaves(root):
            n_leaves += 1
            assert sorted(mine[first:first + count]) == sorted(hosts[first:first + count]), f"{name}: leaf at {first}"
            if name != "c_identical":  # (its triangles are indistinguishable)
                assert (np.diff(mine[first:first + count]) > 0).all(), f"{name}: leaf at {first} is not in input order"
    assert n_leaves >= len(groups)


@pytest.mark.parametrize("name", S.NAMES)
def test_refit_reproduces_the_boxes(name):
    from pathtracerdemo_amd.scene.bvh import refit_blas
    pos = S.cases()[name][0]
    roots, new_idx, _ = S.reference(name)
    for k, (a, r) in enumerate(zip(refit_blas(pos, new_idx, roots), roots)):
        assert int((a != r).sum()) == 0, f"{name}: root {k}: {int((a != r).sum())} words differ after a refit"


def test_the_ulp_case_takes_both_awkward_branches():
    """Without them the case proves nothing: the compare and the bins disagree about a triangle, and a chosen
    split leaves one side empty."""
    from pathtracerdemo_amd.scene import bvh
    from pathtracerdemo_amd.scene.sah import _StableBuilder, build_blas_sah
    seen = {"splits": 0, "disagree": 0, "empty_side": 0, "largest_leaf": 0}

    class Instrumented(_StableBuilder):
        def partition(self, lo, hi, axis, pos):
            c = self.tb[lo:hi, axis, 0].astype(np.float64)
            cmin, cmax = float(c.min()), float(c.max())
            bin_w = (cmax - cmin) / bvh.BIN_COUNT
            bins = np.clip(np.floor((c - cmin) / bin_w), 0, bvh.BIN_COUNT - 1) if bin_w > 0 else np.zeros(len(c))
            cand = cmin + bin_w + np.arange(bvh.BIN_COUNT) * bin_w
            # (several candidates may round to the same f32 plane: a disagreement is one with every such i)
            at = np.nonzero(cand.astype(np.float32).astype(np.float64) == pos)[0]
            assert len(at) >= 1
            mid = super().partition(lo, hi, axis, pos)
            seen["splits"] += 1
            seen["disagree"] += all(int(np.count_nonzero(bins <= i)) != mid - lo for i in at)
            seen["empty_side"] += mid in (lo, hi)
            return mid

    pos, idx, groups, max_leaf = S.cases()["i_ulp"]
    roots, new_idx, depth = build_blas_sah(pos, idx, list(groups), max_leaf, builder_class=Instrumented)
    assert all(np.array_equal(a, b) for a, b in zip(roots, S.reference("i_ulp")[0])) and depth == S.reference("i_ulp")[2]
    seen["largest_leaf"] = max(c for _, c in S.leaves(roots[0]))
    print(seen, "depth", depth)
    assert seen["splits"] >= 50
    assert seen["disagree"] >= 1, "no split where the compare and the bins disagree"
    assert seen["empty_side"] >= 1, "no split that leaves a side empty"
    assert seen["largest_leaf"] > max_leaf, "a leaf larger than max_leaf is the mark of a refused split"


def test_the_renderer_names_the_builders():
    """The option's spelling, without a device: the descriptor's word and the Python names agree with the header."""
    import os
    import re
    from pathtracerdemo_amd import _native as native
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ptx.h")).read()
    assert int(re.search(r"#define PTX_BLAS_LBVH\s+(\d+)u", header).group(1)) == native.PTX_BLAS_LBVH == 0
    assert int(re.search(r"#define PTX_BLAS_SAH\s+(\d+)u", header).group(1)) == native.PTX_BLAS_SAH == 1
