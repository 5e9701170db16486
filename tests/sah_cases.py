"""The inputs of the GPU SAH builder's tests (test_sah_ref.py on the CPU, test_gpu_build_sah.py and
test_node_build_sah.py on the GPU): the nine cases of lbvh_cases.py and one chosen for the awkward branches
of the rule (include/ptx.h ptx_build_blas, PTX_BLAS_SAH)."""
import functools

import numpy as np

import lbvh_cases as L

ULP = 2.0 ** -23  # of an f32 in [1, 2)


def _ulp_triangles(n=400, seed=7):
    """n triangles one ulp across with centres 1 + k ulps, k uniform in 0..40 per axis: every bin of a node is
    a few ulps wide, so the candidate plane (rounded to f32) and the bin number (floor of an f64 quotient)
    disagree about triangles on a boundary, and a split can put every triangle on one side."""
    rng = np.random.default_rng(seed)
    centre = 1.0 + rng.integers(0, 41, size=(n, 1, 3)) * ULP
    offset = np.array([(-1, -1, 0), (1, 0, 0), (0, 1, 0)], np.float64) * ULP
    pos = (centre + offset[None]).reshape(-1, 3).astype(np.float32)
    assert np.array_equal(pos.astype(np.float64), (centre + offset[None]).reshape(-1, 3)), "exact in f32"
    return pos, np.arange(3 * n, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (positions (V, 3) f32, indices (3T,) u32, groups, max_leaf)"""
    out = dict(L.cases())
    pu, xu = _ulp_triangles()
    out["i_ulp"] = (pu, xu, ((0, 400),), 4)
    return out


NAMES = L.NAMES + ("i_ulp",)


@functools.lru_cache(maxsize=None)
def reference(name):
    """build_blas_sah's result for a case, computed once and left alone."""
    from pathtracerdemo_amd.scene.sah import build_blas_sah
    pos, idx, groups, max_leaf = cases()[name]
    roots, new_idx, depth = build_blas_sah(pos, idx, list(groups), max_leaf)
    for r in roots:
        r.setflags(write=False)
    new_idx.setflags(write=False)
    return roots, new_idx, depth


@functools.lru_cache(maxsize=None)
def host_reference(name):
    """scene.bvh.build_blas' result for a case (the Hoare partition), computed once and left alone."""
    from pathtracerdemo_amd.scene.bvh import build_blas
    pos, idx, groups, max_leaf = cases()[name]
    roots, new_idx, depth = build_blas(pos, idx, list(groups), max_leaf)
    for r in roots:
        r.setflags(write=False)
    new_idx.setflags(write=False)
    return roots, new_idx, depth


def leaves(root):
    """(first, count) of a root's leaves, in node order."""
    n = np.asarray(root, np.uint32).reshape(-1, 8)
    leaf = (n[:, 7] & L.LEAF_FLAG) != 0
    return [(int(f), int(w & 0xFFFF)) for f, w in zip(n[leaf, 6], n[leaf, 7])]


def assert_equal_trees(name, got, want):
    """`got` = (roots, indices, depth) equals `want` bit for bit, box zeros folded."""
    roots, new_idx, depth = got
    want_roots, want_idx, want_depth = want
    assert [len(r) for r in roots] == [len(r) for r in want_roots], f"{name}: nodes per root"
    for k, (a, b) in enumerate(zip(roots, want_roots)):
        a, b = L.fold_zero(a), L.fold_zero(b)
        bad = np.nonzero((a != b).reshape(-1, 8).any(axis=1))[0]
        assert len(bad) == 0, f"{name}: root {k}: {len(bad)} of {len(a) // 8} nodes differ, first {bad[:8].tolist()}"
    assert np.array_equal(new_idx, want_idx), f"{name}: {int((np.asarray(new_idx) != want_idx).sum())} index words differ"
    assert depth == want_depth, (name, depth, want_depth)
