#!/usr/bin/env python3
"""What deforming a mesh costs: ptx_update_vertices against ptx_upload_scene + ptx_set_frame of the same scene.

    python tools/refit_cost.py                 # 1920x1080, C3, reuse pipeline, 30 updates of each mesh

On one handle made with PTX_FLAG_TIME_LAUNCHES, idle (ptx_synchronize before every timed call), camera still:
  (a) per mesh -- the chair (mesh 2: 15556 triangles) and the room (mesh 0, the largest: 22278) -- the host
      wall clock of one ptx_update_vertices of every vertex of the mesh (the call is blocking: the span
      ends with the instance table uploaded), the device time of its kernels (PTX_STAT_REFIT) and their
      number, each as median, minimum and maximum over --updates calls after --warmup;
  (b) the baseline: ptx_upload_scene + ptx_set_frame of the same deformed scene (the arrays made before the
      clock starts: the host's own refit or rebuild is not in it), which derives the whole layout on the
      host again and uploads it;
  (c) the host time of the first frame after either, from ptx_set_frame to its completion.
The shapes alternate between a bend and the mesh as loaded, so every call moves every vertex.  One JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bend(pos, np):
    p = pos.astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    p[:, 0] += 0.1 * (hi[0] - lo[0]) * np.sin(2.0 * np.pi / (hi[1] - lo[1]) * (p[:, 1] - lo[1]))
    return p.astype(np.float32)


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--pipeline", default="reuse")
    ap.add_argument("--updates", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--repo", default=ROOT, help="the tree whose package and library are measured")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo))
    import numpy as np
    from pathtracerdemo_amd import _native as N
    from pathtracerdemo_amd.renderer import Renderer
    from pathtracerdemo_amd.scene import world as world_mod

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

    def first_frame():
        frame()
        r.synchronize()

    def refit_stats():
        s = r.stats()
        return s["kernel_ms_total"][N.PTX_STAT_REFIT], s["kernel_launches"][N.PTX_STAT_REFIT]

    for _ in range(10):  # warm-up: every kernel loaded, both frame contexts allocated
        frame()
    r.synchronize()
    out = {"tool": "refit_cost", "width": args.width, "height": args.height, "pipeline": args.pipeline,
           "updates": args.updates, "warmup": args.warmup, "geometry_words": int(len(base.geometry)),
           "accel_words": int(len(base.accel))}
    for label, mesh in (("chair", 2), ("room", 0)):
        blk = world_mod.mesh_blocks(base, mesh)
        rec = base.geometry[blk["vertex"]:blk["vertex_end"]].reshape(-1, 8)
        shapes = [bend(rec[:, 0:3].copy().view(np.float32), np), rec[:, 0:3].copy().view(np.float32)]
        scenes = [world_mod.refit_mesh(base, mesh, shapes[0]), base]
        out[f"{label}_vertices"] = int(len(rec))
        out[f"{label}_triangles"] = int((blk["index_end"] - blk["index"]) // 3)
        t_call, t_kern, t_frame, launches = [], [], [], 0
        for k in range(args.warmup + args.updates):
            frame()
            frame()
            r.synchronize()  # an idle handle: the call's own work
            ms0, n0 = refit_stats()
            t = timed(lambda: r.UpdateVertices(mesh, shapes[k % 2]))
            ms1, n1 = refit_stats()
            r.ResetFrameCount()
            tf = timed(first_frame)
            if k >= args.warmup:
                t_call.append(t)
                t_kern.append(ms1 - ms0)
                t_frame.append(tf)
                launches = n1 - n0
        # (UpdateVertices reads the accel array back for r.compiled: a host that keeps no copy skips that)
        t_abi = []
        for k in range(args.warmup + args.updates):
            records = np.ascontiguousarray(scenes[k % 2].geometry[blk["vertex"]:blk["vertex_end"]])
            r.synchronize()
            t = timed(lambda: r._call("ptx_update_vertices", r._h, mesh, 0, len(rec), records.ctypes.data))
            if k >= args.warmup:
                t_abi.append(t)
        out[f"{label}_update_vertices_host_ms"] = spread(t_call)
        out[f"{label}_update_vertices_abi_ms"] = spread(t_abi)
        out[f"{label}_refit_kernels_ms"] = spread(t_kern)
        out[f"{label}_refit_launches"] = int(launches)
        out[f"{label}_update_first_frame_ms"] = spread(t_frame)
        t_up, t_frame = [], []
        for k in range(args.warmup + args.updates):
            cs = scenes[k % 2]
            frame()
            frame()
            r.synchronize()

            def upload():
                r.compiled = cs
                r._call("ptx_upload_scene", r._h, cs.scene.ctypes.data, len(cs.scene), cs.geometry.ctypes.data,
                        len(cs.geometry), cs.accel.ctypes.data, len(cs.accel))
                r._call("ptx_set_frame", r._h, r.uniform.ctypes.data)  # (the layout is derived here)
            t = timed(upload)
            r.ResetFrameCount()
            tf = timed(first_frame)
            if k >= args.warmup:
                t_up.append(t)
                t_frame.append(tf)
        out[f"{label}_upload_scene_set_frame_ms"] = spread(t_up)
        out[f"{label}_upload_first_frame_ms"] = spread(t_frame)
        r.Initialize(base)
        frame()
        r.synchronize()
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
