"""Binned-SAH BLAS builder with a stable partition: the rule of ptx_build_blas' PTX_BLAS_SAH
(include/ptx.h) in numpy.

It is scene/bvh.py's builder, operation by operation, with one change: the partition keeps the lefts in
their order and then the rights in theirs, where bvh.py swaps pairs as three-mesh-bvh's Hoare partition
does.  A split is chosen from bin counts and bin boxes, which are functions of the *set* of triangles in
a node, so the topology -- every node word, the depth -- is build_blas' bit for bit; only the order of
the triangles inside a leaf differs (here: input order).  That makes the tree a pure function of the
input, and the GPU builder (csrc/ptx_build_sah.hip) is pinned against this file bit for bit.
"""
from __future__ import annotations

import numpy as np

from . import bvh


class _StableBuilder(bvh._Builder):
    def partition(self, lo: int, hi: int, axis: int, pos: float) -> int:
        """centre < pos goes left; lefts keep their relative order, then rights theirs."""
        c = self.tb[lo:hi, axis, 0].astype(np.float64)
        order = np.argsort(~(c < pos), kind="stable")
        self.tb[lo:hi] = self.tb[lo:hi][order]
        self.idx3[lo:hi] = self.idx3[lo:hi][order]
        return lo + int(np.count_nonzero(c < pos))


def build_blas_sah(positions: np.ndarray, indices: np.ndarray, groups, max_leaf_tris: int = 10, max_depth: int = 40,
                   builder_class=_StableBuilder):
    """build_blas' signature and results -- (roots: list of u32 node arrays, reordered indices u32, max
    depth) -- with the stable partition.  Triangles in no group keep their place in the index buffer."""
    positions = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    idx3 = np.array(indices, dtype=np.uint32).reshape(-1, 3)
    b = builder_class(bvh._triangle_bounds(positions, idx3.reshape(-1)), idx3, int(max_leaf_tris), max_depth)
    roots = []
    for first, count in groups:
        first, count = int(first), int(count)
        if count == 0:
            raise ValueError("empty sub-mesh")
        nodes: list = []
        nb, cb = b.bounds(first, first + count)
        b.build(first, first + count, nb, cb, 0, nodes)
        buf = np.zeros((len(nodes), 8), dtype=np.uint32)
        for i, n in enumerate(nodes):
            buf[i, 0:6] = np.asarray(n[1], dtype=np.float32).view(np.uint32)
            if n[0] == "leaf":
                if n[3] > 0xFFFF:
                    raise ValueError("leaf too large for the 16-bit count field")
                buf[i, 6:8] = n[2], bvh.LEAF_FLAG | n[3]
            else:
                buf[i, 6:8] = n[2] * 8, n[3]
        roots.append(buf.reshape(-1))
    return roots, idx3.reshape(-1).astype(np.uint32), b.max_depth_seen
