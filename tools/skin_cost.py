#!/usr/bin/env python3
"""What posing a skinned mesh costs: ptx_skin_vertices against skinning on the host + ptx_update_vertices.

    python tools/skin_cost.py                 # 1920x1080, C3, reuse pipeline, 30 poses of each mesh, 32 joints

On one handle made with PTX_FLAG_TIME_LAUNCHES, idle (ptx_synchronize before every timed call), camera still,
per mesh -- the chair (mesh 2: 8242 vertices) and the room (mesh 0, the largest: 11644) --, every vertex
bound to --joints joints along the mesh's y extent (two linear weights per vertex), each figure as median,
minimum and maximum over --calls calls after --warmup:
  (a) the host wall clock of one ptx_skin_vertices (blocking: the span ends with the instance table
      uploaded), the device time of its kernels (PTX_STAT_REFIT: the skin kernel and the refit chain) and their
      number, and of Renderer.SkinVertices (the call, ptx_read_vertices, ptx_read_accel, the host's copies);
  (b) the baseline, what a host does without the call: scene/skin.py skin_vertices in numpy, then
      Renderer.UpdateVertices of its output (positions and normals) -- the two spans apart and together.
The poses alternate between two palettes (rotations about z growing with the joint index, up to +25 and
-15 degrees), so every call moves every vertex.  One JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_skin(rec, n_joints, np):
    """Joints, weights (n, 4) and the bind words (n, 6) of a mesh's records: a vertex's two nearest joints along y."""
    bind = rec[:, 0:6].copy().view(np.float32)
    y = bind[:, 1].astype(np.float64)
    s = (y - y.min()) / (y.max() - y.min()) * (n_joints - 1)
    j0 = np.clip(np.floor(s), 0, n_joints - 2).astype(np.uint32)
    w1 = (s - j0).astype(np.float32)
    joints = np.zeros((len(rec), 4), np.uint32)
    weights = np.zeros((len(rec), 4), np.float32)
    joints[:, 0], joints[:, 1] = j0, j0 + 1
    weights[:, 0], weights[:, 1] = np.float32(1.0) - w1, w1
    return joints, weights, bind


def make_palette(bind, n_joints, degrees, np):
    p = bind[:, 0:3].astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    out = np.zeros((n_joints, 12))
    for j in range(n_joints):
        a = np.deg2rad(degrees) * (j + 1) / n_joints
        R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        pivot = np.array([0.5 * (lo[0] + hi[0]), lo[1] + (hi[1] - lo[1]) * j / (n_joints - 1), 0.0])
        out[j] = np.concatenate([R, (pivot - R @ pivot)[:, None]], axis=1).reshape(12)
    return out.astype(np.float32)


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--pipeline", default="reuse")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--joints", type=int, default=32)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    from pathtracerdemo_amd import _native as N
    from pathtracerdemo_amd.renderer import Renderer
    from pathtracerdemo_amd.scene import world as world_mod
    from pathtracerdemo_amd.scene.skin import skin_vertices

    base = world_mod.compile_scene("c3_interior_32")
    r = Renderer(args.width, args.height, device=0, pipeline=args.pipeline, time_launches=True)
    r.Initialize(base)

    def frame():
        r.Update()
        r.Render()

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def refit_stats():
        s = r.stats()
        return s["kernel_ms_total"][N.PTX_STAT_REFIT], s["kernel_launches"][N.PTX_STAT_REFIT]

    for _ in range(10):  # warm-up: every kernel loaded, both frame contexts allocated
        frame()
    r.synchronize()
    out = {"tool": "skin_cost", "width": args.width, "height": args.height, "pipeline": args.pipeline,
           "calls": args.calls, "warmup": args.warmup, "joints": args.joints}
    total = args.warmup + args.calls
    for label, mesh in (("chair", 2), ("room", 0)):
        blk = world_mod.mesh_blocks(base, mesh)
        rec = base.geometry[blk["vertex"]:blk["vertex_end"]].reshape(-1, 8)
        joints, weights, bind = make_skin(rec, args.joints, np)
        palettes = [make_palette(bind, args.joints, d, np) for d in (25.0, -15.0)]
        out[f"{label}_vertices"] = int(len(rec))
        r.SetSkin(mesh, joints, weights, bind)
        # (a) the call alone, then through the Renderer
        t_abi, t_kern, launches = [], [], 0
        for k in range(total):
            pal = palettes[k % 2]
            frame()
            frame()
            r.synchronize()  # an idle handle: the call's own work
            ms0, n0 = refit_stats()
            t = timed(lambda: r._call("ptx_skin_vertices", r._h, mesh, pal.ctypes.data, None))
            ms1, n1 = refit_stats()
            if k >= args.warmup:
                t_abi.append(t)
                t_kern.append(ms1 - ms0)
                launches = n1 - n0
        t_host = []
        for k in range(total):
            frame()
            frame()
            r.synchronize()
            t = timed(lambda: r.SkinVertices(mesh, palettes[k % 2]))
            if k >= args.warmup:
                t_host.append(t)
        out[f"{label}_skin_vertices_abi_ms"] = spread(t_abi)
        out[f"{label}_skin_kernels_ms"] = spread(t_kern)
        out[f"{label}_skin_launches"] = int(launches)
        out[f"{label}_renderer_skin_vertices_ms"] = spread(t_host)
        # (b) the baseline: numpy skinning on the host, then Renderer.UpdateVertices
        t_numpy, t_update, t_both = [], [], []
        for k in range(total):
            frame()
            frame()
            r.synchronize()
            t0 = time.perf_counter()
            pos, nrm = skin_vertices(bind, joints, weights, palettes[k % 2])
            t1 = time.perf_counter()
            r.UpdateVertices(mesh, pos, nrm)
            t2 = time.perf_counter()
            if k >= args.warmup:
                t_numpy.append((t1 - t0) * 1e3)
                t_update.append((t2 - t1) * 1e3)
                t_both.append((t2 - t0) * 1e3)
        out[f"{label}_numpy_skin_ms"] = spread(t_numpy)
        out[f"{label}_renderer_update_vertices_ms"] = spread(t_update)
        out[f"{label}_baseline_ms"] = spread(t_both)
        r.Initialize(base)
        frame()
        r.synchronize()
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
