"""Linear-blend skinning with morph targets: the rule of ptx_skin_vertices (include/ptx.h) in numpy f32,
operation by operation -- the reference the GPU kernel (csrc/ptx_skin.hip) is compared with bit for bit.

Everything is f32; every product and every sum is rounded on its own (numpy's element-wise f32
operations never fuse), in exactly the order written in skin_vertices.  A vertex has four (joint,
weight) pairs; a palette entry is an affine matrix of 12 f32, three rows of four, row-major."""
from __future__ import annotations

import dataclasses

import numpy as np

MAX_JOINTS, MAX_TARGETS = 256, 8
BOUND = 2.0 ** 96  # ptx_skin_vertices refuses when overflow_bound(...) is not below it


@dataclasses.dataclass(frozen=True)
class Skin:
    """What ptx_set_skin binds to a range of a mesh's vertices (n of them)."""
    joints: np.ndarray                     # (n, 4) u32, each < the palette's joint count
    weights: np.ndarray                    # (n, 4) f32
    bind: np.ndarray                       # (n, 6) f32 {p.xyz, n.xyz}
    target_pos: np.ndarray | None = None   # (T, n, 3) f32 position deltas
    target_nrm: np.ndarray | None = None   # (T, n, 3) f32 normal deltas


def _f32(a, shape):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(shape)


def skin_vertices(bind, joints, weights, palette, target_pos=None, target_nrm=None, target_weights=None):
    """(positions, normals), each (n, 3) f32, of n vertices: `bind` (n, 6) f32 {p, n}, `joints` (n, 4)
    integers, `weights` (n, 4) f32, `palette` (J, 12) f32, `target_pos` / `target_nrm` (T, n, 3) f32
    deltas with `target_weights` (T,) f32."""
    bind = _f32(bind, (-1, 6))
    n = len(bind)
    j = np.ascontiguousarray(joints, dtype=np.int64).reshape(n, 4)
    w = _f32(weights, (n, 4))
    M = _f32(palette, (-1, 12))
    if j.size and (j.min() < 0 or j.max() >= len(M)):
        raise ValueError(f"a joint index outside the palette's {len(M)}")
    q, m = bind[:, 0:3].copy(), bind[:, 3:6].copy()
    if target_pos is not None:
        dP = _f32(target_pos, (-1, n, 3))
        tw = _f32(target_weights, (len(dP),))
        dN = None if target_nrm is None else _f32(target_nrm, (len(dP), n, 3))
        for k in range(len(dP)):
            q = q + tw[k] * dP[k]
            if dN is not None:
                m = m + tw[k] * dN[k]
    elif target_nrm is not None or target_weights is not None:
        raise ValueError("normal deltas or target weights without position deltas")
    w0, w1, w2, w3 = (w[:, k:k + 1] for k in range(4))
    B = ((w0 * M[j[:, 0]] + w1 * M[j[:, 1]]) + w2 * M[j[:, 2]]) + w3 * M[j[:, 3]]  # (n, 12)
    P, N = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
    for r in range(3):
        P[:, r] = ((B[:, 4 * r] * q[:, 0] + B[:, 4 * r + 1] * q[:, 1]) + B[:, 4 * r + 2] * q[:, 2]) + B[:, 4 * r + 3]
        N[:, r] = (B[:, 4 * r] * m[:, 0] + B[:, 4 * r + 1] * m[:, 1]) + B[:, 4 * r + 2] * m[:, 2]
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        l = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
        Nn = np.where((l > 0)[:, None], N / np.where(l > 0, l, np.float32(1))[:, None], N)
    assert P.dtype == np.float32 and Nn.dtype == np.float32 and B.dtype == np.float32
    return P, Nn


def overflow_bound(bind, weights, palette, target_pos=None, target_nrm=None, target_weights=None) -> float:
    """4 Wmax m (3 (Pmax + T Dmax) + 1) in f64: Wmax the largest per-vertex sum of |w|, Pmax the largest
    |bind word|, Dmax the largest |delta|, m the largest |palette element|, T the sum of |target weight|.
    Below 2^96 (BOUND) every skinned position is finite: |B[e]| <= Wmax m, |q_c| <= Pmax + T Dmax, and
    P'_r sums four terms of at most Wmax m max(|q|, 1)."""
    def top(a):
        a = np.abs(np.asarray(a, dtype=np.float64))
        return float(a.max()) if a.size else 0.0
    w_max = top(np.abs(np.asarray(weights, dtype=np.float64)).reshape(-1, 4).sum(axis=1))
    d_max = max(top(target_pos) if target_pos is not None else 0.0, top(target_nrm) if target_nrm is not None else 0.0)
    t_sum = float(np.abs(np.asarray(target_weights, dtype=np.float64)).sum()) if target_weights is not None else 0.0
    return 4.0 * w_max * top(palette) * (3.0 * (top(bind) + t_sum * d_max) + 1.0)
