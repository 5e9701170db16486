"""The inputs of the LBVH builder's tests (test_lbvh_ref.py on the CPU, test_gpu_build_blas.py and
test_node_build_blas.py on the GPU), each chosen for a branch of the tree's definition (include/ptx.h
ptx_build_blas), and the structural checks both sides share."""
import functools

import numpy as np

LEAF_FLAG = 0xFFFF0000


def _random_tris(n, seed, lo=1e-3, hi=1e3):
    """n triangles over coordinates of magnitude lo .. hi (log-uniform, both signs), each of a size near
    its centre's magnitude."""
    rng = np.random.default_rng(seed)
    centre = np.exp(rng.uniform(np.log(lo), np.log(hi), size=(n, 1, 3))) * rng.choice([-1.0, 1.0], size=(n, 1, 3))
    pos = (centre * (1.0 + 0.2 * rng.uniform(-1.0, 1.0, size=(n, 3, 3)))).reshape(-1, 3).astype(np.float32)
    idx = rng.permutation(3 * n).astype(np.uint32)  # (no shared vertices; the index order is shuffled)
    return pos, idx


def _grid(m, z):
    g = np.linspace(-1.0, 1.0, m + 1)
    x, y = (c.reshape(-1) for c in np.meshgrid(g, g, indexing="xy"))
    pos = np.stack([x, y, np.full_like(x, z)], axis=1).astype(np.float32)
    i, j = (c.reshape(-1) for c in np.meshgrid(np.arange(m), np.arange(m), indexing="xy"))
    a = j * (m + 1) + i
    idx = np.stack([a, a + 1, a + m + 2, a, a + m + 2, a + m + 1], axis=1).reshape(-1).astype(np.uint32)
    return pos, idx


@functools.lru_cache(maxsize=None)
def chair():
    """Chair.glb's merged geometry and groups, before any builder reorders it."""
    from pathtracerdemo_amd.scene.world import merged_geometry
    pos, _, _, idx, groups, _ = merged_geometry("Chair")
    return pos, idx, tuple(groups)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (positions (V, 3) f32, indices (3T,) u32, groups, max_leaf)"""
    out = {}
    pf, xf = _random_tris(1000, seed=5)
    out["a_one_triangle"] = (pf[xf[:3]], np.arange(3, dtype=np.uint32), ((0, 1),), 10)
    out["b_ten_and_eleven"] = (pf, xf[:63], ((0, 10), (10, 11)), 10)  # the leaf boundary
    one = np.array([[0.25, 0.5, 1.0], [1.25, 0.5, 1.0], [0.25, 1.5, 2.0]], np.float32)
    out["c_identical"] = (one, np.tile(np.arange(3, dtype=np.uint32), 25), ((0, 25),), 10)  # identical codes
    pg, xg = _grid(12, 0.5)
    out["d_planar_grid"] = (pg, xg, ((0, 288),), 10)  # cmax == cmin on z
    # three groups of 1, 37 and 300 triangles and 5 triangles in no group (2 ahead, 1 between, 2 behind)
    out["e_groups_and_gaps"] = (pf, xf[:3 * 343], ((2, 1), (3, 37), (41, 300)), 10)
    out["f_random"] = (pf, xf, ((0, 1000),), 10)
    out["g_leaf_1"] = (pf, xf, ((0, 1000),), 1)
    out["g_leaf_64"] = (pf, xf, ((0, 1000),), 64)
    pc, xc, gc = chair()
    out["h_chair"] = (pc, xc, gc, 10)
    return out


NAMES = ("a_one_triangle", "b_ten_and_eleven", "c_identical", "d_planar_grid", "e_groups_and_gaps", "f_random",
         "g_leaf_1", "g_leaf_64", "h_chair")


@functools.lru_cache(maxsize=None)
def reference(name):
    """build_blas_lbvh's result for a case, computed once and left alone."""
    from pathtracerdemo_amd.scene.lbvh import build_blas_lbvh
    pos, idx, groups, max_leaf = cases()[name]
    roots, new_idx, depth = build_blas_lbvh(pos, idx, list(groups), max_leaf)
    for r in roots:
        r.setflags(write=False)
    new_idx.setflags(write=False)
    return roots, new_idx, depth


def fold_zero(words):
    """Node words with a -0.0 in a box word (0..5 of each 8) folded to +0.0: min / max over a set that
    holds both zeros is order-dependent."""
    w = np.array(words, dtype=np.uint32).reshape(-1, 8)
    box = w[:, 0:6]
    box[box == 0x80000000] = 0
    return w.reshape(-1)


def check_structure(name, roots, new_idx, depth):
    """The serialisation's invariants for a result on case `name`."""
    pos, idx, groups, max_leaf = cases()[name]
    assert len(roots) == len(groups)
    assert new_idx.dtype == np.uint32 and new_idx.shape == idx.shape
    grouped = np.zeros(len(idx) // 3, bool)
    true_depth = 0
    for root, (first, count) in zip(roots, groups):
        assert root.dtype == np.uint32 and root.ndim == 1 and len(root) % 8 == 0
        n = root.reshape(-1, 8)
        grouped[first:first + count] = True
        covered = np.zeros(count, np.int64)
        stack = [(0, 0)]
        seen = 0
        while stack:
            node, d = stack.pop()
            seen += 1
            true_depth = max(true_depth, d)
            if n[node, 7] & LEAF_FLAG:
                assert n[node, 7] >> 16 == 0xFFFF
                lf, lc = int(n[node, 6]), int(n[node, 7] & 0xFFFF)
                assert 1 <= lc <= max_leaf and first <= lf and lf + lc <= first + count, (name, node)
                covered[lf - first:lf - first + lc] += 1
            else:
                assert n[node, 7] <= 2 and n[node, 6] % 8 == 0
                right = int(n[node, 6]) // 8
                assert node + 1 < right < len(n), (name, node)
                stack.append((right, d + 1))
                stack.append((node + 1, d + 1))
        assert seen == len(n), f"{name}: {len(n) - seen} nodes are not reachable"
        assert (covered == 1).all(), f"{name}: a triangle is in {covered.min()} or {covered.max()} leaves"
        # a permutation of the group's triangles
        a = idx.reshape(-1, 3)[first:first + count]
        b = new_idx.reshape(-1, 3)[first:first + count]
        assert np.array_equal(a[np.lexsort(a.T[::-1])], b[np.lexsort(b.T[::-1])]), name
    assert np.array_equal(new_idx.reshape(-1, 3)[~grouped], idx.reshape(-1, 3)[~grouped]), "an ungrouped triangle moved"
    assert depth == true_depth, (name, depth, true_depth)


def one_instance_scene(name, builder):
    """Case `name`'s mesh under one identity instance and a point light, its BLAS by `builder`
    (build_blas' signature): (CompiledScene, the builder's reordered indices)."""
    from pathtracerdemo_amd.scene import world as Wd
    from pathtracerdemo_amd.scene.gltf import GltfMaterial
    pos, idx, groups, max_leaf = cases()[name]
    roots, new_idx, depth = builder(pos, idx, list(groups), max_leaf)
    blas, root_offsets = Wd.merge_arrays(roots)
    vert = np.zeros((len(pos), Wd.STRIDE_VERTEX), np.float32)
    vert[:, 0:3] = pos
    vert[:, 5] = 1.0
    mats = [Wd.serialize_material(GltfMaterial()) for _ in groups]
    sm = Wd.SerializedMesh(blas=blas, sub_blas_roots=root_offsets, vertices=vert.reshape(-1).view(np.uint32),
                           indices=np.asarray(new_idx, np.uint32), materials=Wd.merge_arrays(mats)[0], max_depth=depth)

    class OneMesh(Wd.World):
        def pack(self):
            return list(self.instances.values()), [sm], {"mesh": 0}

    w = OneMesh()
    w.add_instance("only", "mesh")
    w.lights.append(Wd.Light.point((0.0, 0.0, 5.0), (1.0, 1.0, 1.0), 10.0))
    return Wd.serialize_world(w), new_idx
