"""Ray sets for the traversal tests (CPU: the oracle against a float64 brute force; GPU: the kernels
against the oracle), made from a compiled scene's world-space triangles with a seeded generator.

Families (rays in ptx_trace's layout {o.xyz, d.xyz, -, -}):
  random       origin uniform in the scene box grown by 10 %, unit normal direction
  axis         the same origins, directions +-x, +-y, +-z (1/0 = inf slabs, 0 * inf on a slab plane)
  planar       one direction component exactly 0
  tiny         one direction component +-1e-30 or +-1e-42 (a denormal f32)
  vertex_edge  aimed at a triangle's vertex or edge midpoint (ties between neighbours)
  on_surface   origin inside a triangle (the self-hit range t <= 1e-4)
  far          origin 1000 scene diagonals away, aimed at the scene (the instance cull's padding)
  nonfinite    64 rays with NaN or +-inf in one component of the origin or the direction
The first four have an independent float64 truth (brute_force); the others only make sense kernel
against oracle (f32 rounding decides them)."""
from __future__ import annotations

import numpy as np

BRUTE_FAMILIES = ("random", "axis", "planar", "tiny")
ORACLE_FAMILIES = ("vertex_edge", "on_surface", "far")
FAMILIES = BRUTE_FAMILIES + ORACLE_FAMILIES
Q_CLOSEST, Q_VIS, Q_OCC = 0, 1, 2


def scene_triangles_world(cs):
    """Every triangle of a CompiledScene in world space, float64: dict of inst, sub, prim (N,) and
    P (N, 3, 3) [triangle, vertex, xyz].  A triangle's (sub, prim) is the leaf of the mesh's sub-mesh
    trees that holds it, as TraceRay reports it."""
    S, G, o = cs.scene, cs.geometry, cs.offsets
    per_mesh = {}
    inst_l, sub_l, prim_l, P_l = [], [], [], []
    for inst in range(cs.instance_count):
        base = 33 * inst
        M = S[base:base + 16].view(np.float32).reshape(4, 4).T.astype(np.float64)
        mesh = int(S[base + 32])
        if mesh not in per_mesh:
            off_v, off_i, _, off_root, off_b, nsub = (int(v) for v in S[o["mesh_descriptor"] + 6 * mesh:
                                                                       o["mesh_descriptor"] + 6 * mesh + 6])
            subs, prims = [], []
            for sub in range(nsub):
                nb = o["blas"] + off_b + int(G[o["sub_blas_root"] + off_root + sub])
                stack = [0]
                while stack:
                    n = stack.pop()
                    w = cs.accel[nb + 8 * n: nb + 8 * n + 8]
                    if w[7] & 0xFFFF0000:
                        first, cnt = int(w[6]), int(w[7] & 0xFFFF)
                        prims.append(np.arange(first, first + cnt))
                        subs.append(np.full(cnt, sub))
                    else:
                        stack += [n + 1, int(w[6]) // 8]
            prims, subs = np.concatenate(prims), np.concatenate(subs)
            ids = G[o["index"] + off_i + 3 * prims[:, None] + np.arange(3)[None, :]].astype(np.int64)  # (N, 3)
            pos = G[off_v + 8 * ids[..., None] + np.arange(3)].view(np.float32).astype(np.float64)     # (N, 3, 3)
            per_mesh[mesh] = (subs, prims, pos)
        subs, prims, pos = per_mesh[mesh]
        Pw = pos @ M[:3, :3].T + M[:3, 3]
        inst_l.append(np.full(len(prims), inst))
        sub_l.append(subs)
        prim_l.append(prims)
        P_l.append(Pw)
    return {"inst": np.concatenate(inst_l), "sub": np.concatenate(sub_l), "prim": np.concatenate(prim_l),
            "P": np.concatenate(P_l)}


def scene_box(tris):
    P = tris["P"].reshape(-1, 3)
    return P.min(axis=0), P.max(axis=0)


def _unit(d):
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _pack(o, d):
    rays = np.zeros((len(o), 8), np.float32)
    rays[:, 0:3] = o
    rays[:, 3:6] = d
    return rays


def family(name, tris, n=256, seed=1):
    """(n, 8) f32 rays of one family (module docstring); the same (name, scene, n, seed) gives the same rays."""
    rng = np.random.default_rng([seed, FAMILIES.index(name) if name in FAMILIES else len(FAMILIES)])
    lo, hi = scene_box(tris)
    ext = hi - lo
    glo, ghi = lo - 0.05 * ext, hi + 0.05 * ext  # the box grown by 10 %
    o = rng.uniform(glo, ghi, size=(n, 3))
    d = _unit(rng.normal(size=(n, 3)))
    k = np.arange(n)
    if name == "random":
        pass
    elif name == "axis":
        d = np.zeros((n, 3))
        d[k, k % 3] = np.where((k // 3) % 2 == 0, 1.0, -1.0)
    elif name == "planar":
        d[k, k % 3] = 0.0
        d = _unit(d)
        d[k, k % 3] = 0.0
    elif name == "tiny":
        d[k, k % 3] = 0.0
        d = _unit(d)
        d[k, k % 3] = np.array([1e-30, -1e-30, 1e-42, -1e-42])[(k // 3) % 4]
    elif name == "vertex_edge":
        t = rng.integers(len(tris["P"]), size=n)
        P = tris["P"][t].astype(np.float32).astype(np.float64)
        v = k % 3
        vert = P[k, v]
        mid = (0.5 * (P[k, v].astype(np.float32) + P[k, (v + 1) % 3].astype(np.float32))).astype(np.float64)
        target = np.where(((k // 3) % 2 == 0)[:, None], vert, mid)
        d = _unit(target - o.astype(np.float32).astype(np.float64))
    elif name == "on_surface":
        t = rng.integers(len(tris["P"]), size=n)
        P = tris["P"][t]
        b = rng.dirichlet([1.0, 1.0, 1.0], size=n)
        o = (b[:, :, None] * P).sum(axis=1)
    elif name == "far":
        centre, diag = 0.5 * (lo + hi), np.linalg.norm(ext)
        target = rng.uniform(lo, hi, size=(n, 3))
        o = centre + 1000.0 * diag * _unit(rng.normal(size=(n, 3)))
        d = _unit(target - o)
    elif name == "nonfinite":
        rays = _pack(o, d)
        bad = np.array([np.nan, np.inf, -np.inf], np.float32)
        rays[k, k % 6] = bad[(k // 6) % 3]
        return rays
    else:
        raise KeyError(name)
    return _pack(o, d)


def brute_force(tris, rays, chunk=16):
    """Closest hit of each ray over every world-space triangle, float64 Moller-Trumbore with TraceRay's
    range (1e-4 < t <= 1e10), no determinant threshold: (valid, inst, sub, prim, t) arrays.
    Every (ray, triangle) pair is first put through the plane form of the same test -- t from the plane,
    (u, v) from the triangle's dual basis: six (rays x 3) @ (3 x triangles) products -- with 1e-6 of
    slack on every bound; the pairs that pass (a handful per ray) get Moller-Trumbore itself."""
    P = tris["P"]
    p0 = P[:, 0]
    e1, e2 = P[:, 1] - p0, P[:, 2] - p0
    N = np.cross(e1, e2)
    with np.errstate(divide="ignore", invalid="ignore"):
        nn = (N * N).sum(-1, keepdims=True)
        au, av = np.cross(e2, N) / nn, np.cross(N, e1) / nn  # (X - p0) = u e1 + v e2 in the plane
    cN, cu, cv = (p0 * N).sum(-1), (p0 * au).sum(-1), (p0 * av).sum(-1)
    n = len(rays)
    best_t = np.full(n, np.inf)
    best_i = np.full(n, -1, np.int64)
    O = rays[:, 0:3].astype(np.float64)
    D = rays[:, 3:6].astype(np.float64)
    slack = 1e-6
    for c0 in range(0, n, chunk):
        o, d = O[c0:c0 + chunk], D[c0:c0 + chunk]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            t = (cN[None] - o @ N.T) / (d @ N.T)
            u = o @ au.T + t * (d @ au.T) - cu[None]
            v = o @ av.T + t * (d @ av.T) - cv[None]
            cand = ((u >= -slack) & (v >= -slack) & (u + v <= 1.0 + slack) & (t > 1e-4 * (1.0 - slack))
                    & (t <= 1e10 * (1.0 + slack)))
        ri, ti = np.nonzero(cand)
        # Moller-Trumbore on the candidate pairs
        dd, oo = d[ri], o[ri]
        pvec = np.cross(dd, e2[ti])
        det = (e1[ti] * pvec).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            tvec = oo - p0[ti]
            u = (tvec * pvec).sum(-1) * inv
            qvec = np.cross(tvec, e1[ti])
            v = (dd * qvec).sum(-1) * inv
            t = (e2[ti] * qvec).sum(-1) * inv
            ok = (det != 0.0) & (u >= 0.0) & (u <= 1.0) & (v >= 0.0) & (u + v <= 1.0) & (t > 1e-4) & (t <= 1e10)
        for r, tri, tt in zip(ri[ok], ti[ok], t[ok]):
            if tt < best_t[c0 + r]:
                best_t[c0 + r], best_i[c0 + r] = tt, tri
    valid = best_i >= 0
    j = np.where(valid, best_i, 0)
    return valid, tris["inst"][j], tris["sub"][j], tris["prim"][j], best_t


def hit_fields(hits):
    """(valid, inst, sub, prim, t) of ptx_trace hit records."""
    w = np.ascontiguousarray(hits, np.float32).view(np.uint32)
    return (w[:, 1] >> 31) == 1, (w[:, 1] >> 16) & 0x7FFF, w[:, 1] & 0xFFFF, w[:, 2], hits[:, 0]


def disagreements(hits, truth):
    """Rays whose oracle hit record departs from the brute force: validity, instance or primitive, or
    |t - t64| > 1e-3 max(t64, 1e-3).  Returns the boolean mask and the worst relative t error among
    the rays that agree on the triangle."""
    valid, inst, sub, prim, t = hit_fields(hits)
    bv, bi, bs, bp, bt = truth
    both = valid & bv
    same = both & (inst == bi) & (sub == bs) & (prim == bp)
    with np.errstate(invalid="ignore"):
        terr = np.abs(t.astype(np.float64) - bt)
        bad_t = both & (terr > 1e-3 * np.maximum(bt, 1e-3))
    bad = (valid != bv) | (both & ~same) | bad_t
    rel = float((terr[same] / np.maximum(bt[same], 1e-3)).max()) if same.any() else 0.0
    return bad, rel


def to_queries(rays, remain=0.0, kind=Q_CLOSEST):
    """ptx_trace rays {o, d.x | d.y, d.z, -, -} as queue queries {o, remain | d, kind}."""
    rays = np.asarray(rays, np.float32).reshape(-1, 8)
    q = np.zeros_like(rays)
    q[:, 0:3] = rays[:, 0:3]
    q[:, 3] = remain
    q[:, 4:7] = rays[:, 3:6]
    q.view(np.uint32)[:, 7] = kind
    return q


def visibility_set(rays, hits, kinds=(Q_VIS, Q_OCC)):
    """Visibility / occlusion queries on `rays` with `remain` around their closest hit's t (the oracle's
    `hits`; 1 where a ray misses): t, the f32 on either side of it, 0.5 t, 2 t, 0, -1, 1e10, 3e38 --
    the nine values dealt over the rays, the kinds alternating every nine rays."""
    rays = np.asarray(rays, np.float32).reshape(-1, 8)
    valid, _, _, _, t = hit_fields(hits)
    t = np.where(valid, t, np.float32(1.0)).astype(np.float32)
    k = np.arange(len(rays))
    table = np.stack([t, np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(-np.inf)),
                      np.float32(0.5) * t, np.float32(2.0) * t, np.zeros_like(t), -np.ones_like(t),
                      np.full_like(t, 1e10), np.full_like(t, 3e38)], axis=1)
    remain = table[k, k % table.shape[1]]
    kind = np.asarray(kinds, np.uint32)[(k // table.shape[1]) % len(kinds)]
    return to_queries(rays, remain, kind)


def window_stack_rays(tris, window_insts, n=256, seed=1):
    """Rays along the stack of window instances (tests/helpers.py many_instances_scene): from just in
    front of a point of one pane towards a point of a pane at least three further along the stack, so
    that Visibility chains cross several panes (two faces each) and end by `remain`, by an opaque hit
    (the room's walls) or by the fifth segment."""
    rng = np.random.default_rng([seed, 99])
    boxes = [tris["P"][tris["inst"] == i].reshape(-1, 3) for i in window_insts]
    lo, hi = np.stack([b.min(axis=0) for b in boxes]), np.stack([b.max(axis=0) for b in boxes])
    cen = 0.5 * (lo + hi)
    axis = np.ptp(cen, axis=0).argmax()  # the direction the panes are stacked in
    rank = np.argsort(cen[:, axis])
    m = len(rank)
    a = rng.integers(m, size=n)
    step = rng.integers(3, m, size=n)
    b = np.where(a + step < m, a + step, a - step)
    b = np.where(b < 0, (a + 3) % m, b)
    a, b = rank[a], rank[b]
    pa = cen[a] + 0.3 * (hi[a] - lo[a]) * rng.uniform(-1, 1, size=(n, 3))
    pb = cen[b] + 0.3 * (hi[b] - lo[b]) * rng.uniform(-1, 1, size=(n, 3))
    d = _unit(pb - pa)
    o = pa - d * rng.uniform(0.05, 0.25, size=(n, 1))
    return _pack(o, d)
