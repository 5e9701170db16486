#!/usr/bin/env python3
"""What rebuilding a loaded mesh's BLAS in place costs, and what the rebuilt tree is worth to a frame.

    python tools/rebuild_cost.py                 # 1920x1080, C3, reuse pipeline

The chair of c3_interior_32 (mesh 2) is skinned with 32 joints and posed by tests/skin_edits.py's palette at
scale 8 (tests/rebuild_cases.py: a 200 degree twist), the room (mesh 0) with 3 joints at POSE_A.
(a) Calls, on one idle handle made with PTX_FLAG_TIME_LAUNCHES: the host wall clock of one ptx_rebuild_mesh
    (blocking: the span ends with the layout derived again) with either builder, the device time of its kernels
    (PTX_STAT_BUILD) and their number, and the same for ptx_blas_cost, each as median, minimum and maximum over
    --calls calls after --warmup, for chair and room.
(b) The route the library had before: ptx_read_vertices + ptx_build_blas (SAH) + ptx_upload_scene + ptx_set_frame
    + ptx_set_skin again, on the same handle (the host's splice of the arrays is NOT in the span: the arrays
    uploaded are the ones a rebuild left).
(c) Frames: the scene with the chair at the scale-8 pose on the refitted tree and on the rebuilt tree, ONE HANDLE
    PER PROCESS (a handle's place among several moves its frame by up to 0.7 ms): this script starts
    itself once per measurement, refitted and rebuilt alternately, --turns times each; a child renders --runs
    runs of --frames frames after a warm-up run and reports each run's mean frame time.  Medians and ranges
    over all runs of a tree, their ratio, and the two trees' ptx_blas_cost.
One JSON line.  No threshold: the tool measures."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--pipeline", default="reuse")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--skip-frames", action="store_true", help="(a) and (b) only")
    ap.add_argument("--child", choices=("refit", "rebuilt"), help="(internal) one tree's frames in this process")
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import numpy as np
    import rebuild_cases as RC
    import scene_edits as E
    import skin_edits as S
    from pathtracerdemo_amd import _native as N
    from pathtracerdemo_amd.renderer import Renderer

    def pose_chair(r):
        S.set_skin(r, RC.CHAIR, RC.JOINTS)
        r.SkinVertices(RC.CHAIR, RC.palette8())

    if args.child:
        r = Renderer(args.width, args.height, device=0, pipeline=args.pipeline)
        r.Initialize(E.base())
        r.Update()
        pose_chair(r)
        if args.child == "rebuilt":
            r.RebuildMesh(RC.CHAIR, "sah")
        cost = r.blas_cost(RC.CHAIR)
        runs = []
        for k in range(1 + args.runs):
            r.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.frames):
                r.Update()
                r.Render()
            r.synchronize()
            if k >= 1:
                runs.append((time.perf_counter() - t0) * 1e3 / args.frames)
        r.close()
        print(json.dumps({"tree": args.child, "frame_ms": runs, "blas_cost": cost}))
        return

    out = {"tool": "rebuild_cost", "width": args.width, "height": args.height, "pipeline": args.pipeline,
           "calls": args.calls, "warmup": args.warmup, "turns": args.turns, "runs": args.runs, "frames": args.frames}
    r = Renderer(args.width, args.height, device=0, pipeline=args.pipeline, time_launches=True)
    r.Initialize(E.base())
    r.Update()
    pose_chair(r)
    S.set_skin(r, RC.ROOM, 3)
    S.pose(r, RC.ROOM, 3, S.POSE_A)

    def build_stats():
        s = r.stats()
        return s["kernel_ms_total"][N.PTX_STAT_BUILD], s["kernel_launches"][N.PTX_STAT_BUILD]

    def warm():  # two frames and a wait: an idle handle, not a cold one
        for _ in range(2):
            r.Update()
            r.Render()
        r.synchronize()

    def measure(call):
        wall, kern, launches = [], [], 0
        for k in range(args.warmup + args.calls):
            warm()
            ms0, n0 = build_stats()
            t, _ = timed(call)
            ms1, n1 = build_stats()
            if k >= args.warmup:
                wall.append(t)
                kern.append(ms1 - ms0)
                launches = n1 - n0
        return {"host_wall_ms": spread(wall), "kernel_ms": spread(kern), "launches": int(launches)}

    # ---------------------------------------------------------------- (a) the calls
    info = N.PtxRebuildInfo()
    import ctypes
    cost = ctypes.c_double(0.0)
    for name, mesh in (("chair", RC.CHAIR), ("room", RC.ROOM)):
        for builder, code in (("sah", N.PTX_BLAS_SAH), ("lbvh", N.PTX_BLAS_LBVH)):
            out[f"rebuild_{name}_{builder}"] = measure(
                lambda: r._call("ptx_rebuild_mesh", r._h, mesh, code, 0, ctypes.byref(info)))
            out[f"rebuild_{name}_{builder}"]["mesh_nodes"] = int(info.mesh_nodes)
        out[f"blas_cost_{name}"] = measure(lambda: r._call("ptx_blas_cost", r._h, mesh, ctypes.byref(cost)))
        out[f"blas_cost_{name}"]["cost"] = float(cost.value)
    r.RebuildMesh(RC.CHAIR, "sah")  # (compiled: the arrays route (b) uploads)

    # ---------------------------------------------------------------- (b) the route without the call
    from pathtracerdemo_amd.scene.world import mesh_blocks, mesh_groups
    cs = r.compiled
    sk = RC.chair_skin()
    b = mesh_blocks(cs, RC.CHAIR)
    groups = mesh_groups(cs, RC.CHAIR)
    idx = np.ascontiguousarray(cs.geometry[b["index"]:b["index_end"]])

    def old_route():
        rec = r.read_vertices(RC.CHAIR)
        r.build_blas(rec[:, 0:3].copy().view(np.float32), idx, groups, builder="sah")
        r._call("ptx_upload_scene", r._h, cs.scene.ctypes.data, len(cs.scene), cs.geometry.ctypes.data, len(cs.geometry),
                cs.accel.ctypes.data, len(cs.accel))
        r._call("ptx_set_frame", r._h, r.uniform.ctypes.data)
        r.SetSkin(RC.CHAIR, sk.joints, sk.weights, sk.bind)
    out["read_build_upload_setskin_chair_sah"] = measure(old_route)
    r.close()

    # ---------------------------------------------------------------- (c) frames, one handle per process
    if not args.skip_frames:
        per = {"refit": [], "rebuilt": []}
        costs = {}
        for k in range(args.turns):
            for tree in (("refit", "rebuilt") if k % 2 == 0 else ("rebuilt", "refit")):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, "--width", str(args.width),
                                    "--height", str(args.height), "--pipeline", args.pipeline, "--runs", str(args.runs),
                                    "--frames", str(args.frames)], capture_output=True, text=True, timeout=300)
                if p.returncode != 0:
                    raise SystemExit(f"the {tree} child failed ({p.returncode}):\n{p.stderr}")
                res = json.loads(p.stdout.strip().splitlines()[-1])
                per[tree] += res["frame_ms"]
                costs[tree] = res["blas_cost"]
        out["frame_ms_refit"] = spread(per["refit"])
        out["frame_ms_rebuilt"] = spread(per["rebuilt"])
        out["frame_time_ratio"] = round(statistics.median(per["rebuilt"]) / statistics.median(per["refit"]), 4)
        out["blas_cost_refit"], out["blas_cost_rebuilt"] = costs["refit"], costs["rebuilt"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
