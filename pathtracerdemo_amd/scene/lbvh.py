"""LBVH BLAS builder: the rule of ptx_build_blas (include/ptx.h) in numpy.

Morton codes of the triangle centres, a stable sort, and the binary radix tree of the sorted keys,
collapsed into leaves of at most ``max_leaf_tris`` triangles and written in build_blas' serialisation
(bvh.py: 32-byte nodes, depth-first, left = node + 1, leaves as ranges of the reordered index buffer).
Unlike the SAH builder's partition the result is a pure function of the input, so the GPU builder
(csrc/ptx_build.hip) is pinned against this file bit for bit.

    per triangle   the builder's record (bvh._triangle_bounds): centre c and half h in f32;
                   lo = f32(f64(c) - f64(h)), hi = f32(f64(c) + f64(h))
    per group      cmin, cmax = per-axis min / max of its centres; per axis q = 0 where cmax == cmin, else
                   q = min(1023, floor(((f64(c) - f64(cmin)) * 1024.0) / (f64(cmax) - f64(cmin))))
                   code = the bits of q.x, q.y, q.z interleaved, x highest (30 bits)
                   order = (code, position in the input index buffer), ascending
    tree           keys K_p = code_p * 2^32 + p (p: sorted position within the group); node(a, b) is a leaf
                   when b - a + 1 <= max_leaf_tris; else it splits behind the last key in [a, b) whose highest
                   bit differing between K_a and K_b is clear
"""
from __future__ import annotations

import numpy as np

from .bvh import LEAF_FLAG, _triangle_bounds, refit_blas

CODE_BITS = 30


def _spread3(q: np.ndarray) -> np.ndarray:
    """Bit k of the 10-bit q to bit 3k."""
    out = np.zeros(q.shape, dtype=np.uint64)
    q = q.astype(np.uint64)
    for k in range(10):
        out |= ((q >> np.uint64(k)) & np.uint64(1)) << np.uint64(3 * k)
    return out


def morton_codes(centres: np.ndarray) -> np.ndarray:
    """(n,) u64 30-bit codes of one group's (n, 3) f32 centres."""
    c = centres.astype(np.float64)
    cmin = centres.min(axis=0).astype(np.float64)
    cmax = centres.max(axis=0).astype(np.float64)
    code = np.zeros(len(c), dtype=np.uint64)
    for axis in range(3):
        if cmax[axis] == cmin[axis]:
            continue
        q = np.floor(((c[:, axis] - cmin[axis]) * 1024.0) / (cmax[axis] - cmin[axis]))
        q = np.minimum(q, 1023.0).astype(np.uint64)
        code |= _spread3(q) << np.uint64(2 - axis)
    return code


def _emit_group(code: np.ndarray, first: int, max_leaf: int):
    """One group's nodes from its sorted codes: (n_nodes, 8) u32 with words 6 and 7 set, and its depth."""
    n = len(code)
    keys = (code << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    w67 = []
    depth_max = 0
    # depth-first, left before right: (a, b, depth, the interior node waiting for its right child's index)
    stack = [(0, n - 1, 0, -1)]
    while stack:
        a, b, depth, parent = stack.pop()
        me = len(w67)
        if parent >= 0:
            w67[parent][0] = 8 * me
        depth_max = max(depth_max, depth)
        count = b - a + 1
        if count <= max_leaf:
            w67.append([first + a, LEAF_FLAG | count])
            continue
        bit = int(keys[a] ^ keys[b]).bit_length() - 1
        # the keys of [a, b] agree above `bit`: the first one with it set
        bound = ((int(keys[a]) >> bit) | 1) << bit
        s = a + int(np.searchsorted(keys[a:b + 1], np.uint64(bound), side="left")) - 1
        axis = 2 - (bit - 32) % 3 if bit >= 32 else 0
        w67.append([0, axis])
        stack.append((s + 1, b, depth + 1, me))
        stack.append((a, s, depth + 1, -1))
    buf = np.zeros((len(w67), 8), dtype=np.uint32)
    buf[:, 6:8] = np.asarray(w67, dtype=np.uint64).astype(np.uint32)
    return buf, depth_max


def build_blas_lbvh(positions: np.ndarray, indices: np.ndarray, groups, max_leaf_tris: int = 10):
    """build_blas' signature and results -- (roots: list of u32 node arrays, reordered indices u32,
    max depth) -- by the LBVH rule.  Triangles in no group keep their place in the index buffer."""
    if not 1 <= int(max_leaf_tris) <= 64:
        raise ValueError("max_leaf_tris must be 1..64")
    positions = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    idx3 = np.array(indices, dtype=np.uint32).reshape(-1, 3)
    centres = _triangle_bounds(positions, idx3.reshape(-1))[:, :, 0]
    out3 = idx3.copy()
    shells = []
    max_depth = 0
    for first, count in groups:
        first, count = int(first), int(count)
        if count == 0:
            raise ValueError("empty sub-mesh")
        code = morton_codes(centres[first:first + count])
        order = np.argsort(code, kind="stable")
        out3[first:first + count] = idx3[first:first + count][order]
        buf, depth = _emit_group(code[order], first, int(max_leaf_tris))
        shells.append(buf.reshape(-1))
        max_depth = max(max_depth, depth)
    new_indices = out3.reshape(-1)
    # words 0..5 by refit_blas' rule: a leaf over its triangles, an interior node over its children
    roots = refit_blas(positions, new_indices, shells)
    return roots, new_indices, max_depth


def sah_cost(roots, traversal: float = 1.0, triangle: float = 1.25) -> float:
    """The surface-area cost of a mesh's trees under bvh.py's model, summed over its roots: each node's
    area relative to its root's, times the traversal cost (interior) or the triangle cost per triangle."""
    total = 0.0
    for root in roots:
        buf = np.asarray(root, dtype=np.uint32).reshape(-1, 8)
        box = buf[:, 0:6].view(np.float32).astype(np.float64)
        d = box[:, 3:6] - box[:, 0:3]
        area = 2.0 * (d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0])
        leaf = (buf[:, 7] & LEAF_FLAG) != 0
        rel = area / area[0] if area[0] > 0 else np.zeros_like(area)
        total += float((rel[~leaf] * traversal).sum() + (rel[leaf] * triangle * (buf[leaf, 7] & 0xFFFF)).sum())
    return total
