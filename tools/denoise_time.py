#!/usr/bin/env python3
"""Time ptx_denoise (pathtracerdemo_amd/csrc/ptx_denoise.hip) on a rendered frame.

    python tools/denoise_time.py                        # 1920x1080, C3, reuse pipeline, 5 iterations
    rocprofv3 --kernel-trace -d OUT -o run --output-format csv -- python tools/denoise_time.py --no-events
    python tools/denoise_time.py --trace OUT/.../run_kernel_trace.csv      # per kernel, from that trace
    python tools/denoise_time.py --temporal [--yaw-step DEG]   # the temporal mode (both forms above take it too)
    python tools/denoise_time.py --bands 8 --width 3840 --height 2160 [--temporal]   # the frame split into row bands
    python tools/denoise_time.py --upsample 2           # ptx_upsample, 960x540 -> 1920x1080 (--no-events / --trace take it too)
    python tools/denoise_time.py --bands 8 --upsample 2 --width 3840 --height 2160   # ptx_upsample_bands, 8 pairs
    python tools/denoise_time.py --displayed-frame [--upsample 2]   # ms per displayed frame under a yawing camera
    python tools/denoise_time.py --upsample 2 --phases  # ptx_upsample_temporal, the phases cycling (--displayed-frame,
                                                        # --no-events and --trace take --phases too)
    python tools/denoise_time.py --bands 8 --upsample 2 --phases --width 3840 --height 2160 [--history-rows 32]
                                                        # ptx_upsample_temporal_bands, 8 pairs
    python tools/denoise_time.py --displayed-frame --bands 8 --upsample 2 --phases --width 3840 --height 2160 \
        --history-rows 16,32,64                         # clipped pixels per band along the yawing camera path
    python tools/denoise_time.py --upsample 2 --phases --follow            # the same call on a following handle, no edit
    python tools/denoise_time.py --upsample 2 --phases --edit move|pose [--follow]   # the chair moved / posed before
                                                        # every call (ptx_upsample_follow: DESIGN.md §4.6)
    python tools/denoise_time.py --upsample 2 --phases --edit pose --error --width 960 --height 540 --calls 64
                                                        # the error on the animated chair, following and not

The whole call is timed with device events around it on the handle's stream (a torch stream set
with ptx_set_stream): the median of --calls calls after --warmup.  The same calls on a
PTX_FLAG_TIME_LAUNCHES handle give the sum of the kernels' own times (stats slot
PTX_STAT_DENOISE), for 1..6 iterations.  Per-kernel times come from a rocprofv3 kernel trace of
this script, taken in a run of its own (--trace prints them with each kernel's compulsory bytes and
its share of the streaming bound).  One JSON line either way.
--temporal times the temporal mode on a frame_color handle: before every call the camera yaws by
--yaw-step degrees (0: a still camera, the same-pixel lookup) and a frame is rendered with the frame
index restarted, as the engine does on a move; only the ptx_denoise call is inside the events.
--bands N times ptx_denoise_bands on the frame as N equal row bands on this GPU (peer copies,
PTX_FLAG_TIME_LAUNCHES handles): the sum of the bands' kernel times per call against the whole-image
call's on the same build, with the rows each stage computes and the bytes a band receives.  For the
kernel times every band runs on ONE stream: on their own streams the bands' kernels share the GPU, and
an event pair then spans its neighbours' kernels too (that sum is reported as well, labelled).  The
time from the call to its completion on the bands' own streams, against the whole-image call's, is
taken with the host clock.
--upsample S times ptx_upsample the same way (events around the call on the full-size handle's stream):
a handle of 1/S the size renders --frames frames and denoises once, the full-size handle runs one
G-buffer pass; --width / --height are the full size.
--bands N --upsample S times ptx_upsample_bands on N equal pairs on this GPU (peer copies) the way
--bands times ptx_denoise_bands, against the whole-image ptx_upsample of the same frame on the same
build: the sum of the bands' kernel times and device events around the call with every full-size
handle on one stream, and the host's time from the call to its completion on the handles' own streams.
--bands N --upsample S --phases times ptx_upsample_temporal_bands on the same N pairs, beside
ptx_upsample_bands on them (small bands under the full-size camera) and beside the whole-image
ptx_upsample_temporal, all in one process: kernel sums and device events around each call with every
full-size handle on one stream.  The phases cycle and the camera yaws by --yaw-step before every call,
so the history is reprojected.  With --displayed-frame it counts instead, for every --history-rows
value, the pixels each band clips (PTX_COUNTER_UPSAMPLE_CLIP) over --calls displayed frames of that path.
--displayed-frame times what a host does per displayed frame while the camera moves (it yaws by
--yaw-step and the frame index restarts before every frame), with the host clock from the first call
to the completion of the last: a full-size frame + ptx_denoise, or with --upsample S a frame +
ptx_denoise at 1/S the size, then the G-buffer pass + ptx_upsample at full size.  The first form uses
nothing newer than ptx_denoise, so the same script times an older library.
"""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, the datasheet figure the bound is quoted against
# compulsory bytes per pixel: what each kernel must read and write once
# (temporal: this frame's guide record and colour, one previous guide / history / moments record,
# the new history and moments; its variance pass reads the guide record, history and moments)
# (upsample: per full-size pixel its guide record and the output; the small image's 48 B per pixel
# are added by upsample_bound_ms)
# (upsample_temporal: this call's and the previous call's guide records, the history read and written, the output)
BYTES = {"upsample_temporal": 32 + 32 + 16 + 16 + 16, "upsample": 32 + 16, "guide": 16 + 32, "variance": 48 + 16, "atrous": 48 + 16, "temporal": 32 + 16 + 32 + 16 + 8 + 16 + 8,
         "variance_moments": 32 + 16 + 8 + 16}


def bound_ms(kind, px):
    return BYTES[kind] * px / HBM_PEAK * 1e3


def render(args, **kw):
    from pathtracerdemo_amd.renderer import Renderer
    from pathtracerdemo_amd.scene.world import compile_scene
    r = Renderer(args.width, args.height, device=0, pipeline=args.pipeline, frame_color=args.temporal, **kw)
    r.Initialize(compile_scene(args.scene))
    for _ in range(args.frames):
        r.Update()
        r.Render()
    r.synchronize()
    return r


def next_frame(args, r, i):
    """Temporal mode: the frame the next call follows (outside the timed region)."""
    if not args.temporal:
        return
    if args.yaw_step:
        r.GetCamera().set_yaw(args.yaw_step * (i + 1))
        r.ResetFrameCount()
    r.Update()
    r.Render()
    r.synchronize()


def call_bound_ms(args, px):
    head = bound_ms("temporal", px) + bound_ms("variance_moments", px) if args.temporal else bound_ms("variance", px)
    return bound_ms("guide", px) + head + args.iterations * bound_ms("atrous", px)


def measure(args):
    px = args.width * args.height
    out = {"what": "ptx_denoise", "temporal": args.temporal, "yaw_step": args.yaw_step, "width": args.width, "height": args.height, "scene": args.scene,
           "pipeline": args.pipeline, "iterations": args.iterations, "calls": args.calls, "warmup": args.warmup,
           "bound_ms_at_8TBs": round(call_bound_ms(args, px), 4)}
    if not args.no_events:
        import torch
        r = render(args)
        stream = torch.cuda.Stream()
        r.set_stream(stream.cuda_stream)
        ms = []
        for i in range(args.warmup + args.calls):
            next_frame(args, r, i)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            r.Denoise(iterations=args.iterations, temporal=args.temporal)
            b.record(stream)
            b.synchronize()
            if i >= args.warmup:
                ms.append(a.elapsed_time(b))
        r.set_stream(None)
        r.close()
        out["whole_call_ms"] = {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}
        out["whole_call_fraction_of_bound"] = round(out["bound_ms_at_8TBs"] / statistics.median(ms), 3)
    # the kernels' own times, summed per call (events around every launch), for 1..6 iterations
    from pathtracerdemo_amd import _native as N
    r = render(args, time_launches=True)
    sums = {}
    for n in ([args.iterations] if args.no_events else range(1, 7)):
        per_call = []
        for i in range(args.warmup + args.calls):
            next_frame(args, r, i)
            before = r.stats()["kernel_ms_total"][N.PTX_STAT_DENOISE]
            r.Denoise(iterations=n, temporal=args.temporal)
            r.synchronize()
            if i >= args.warmup:
                per_call.append(r.stats()["kernel_ms_total"][N.PTX_STAT_DENOISE] - before)
        sums[n] = round(statistics.median(per_call), 4)
    r.close()
    out["kernel_sum_ms_by_iterations"] = sums
    return out


def upsample_bound_ms(args, kind):
    px = args.width * args.height
    return bound_ms(kind, px) + (48 * (px // args.upsample ** 2) / HBM_PEAK * 1e3 if kind.startswith("upsample") else 0.0)


def phase_of(args, i):
    """The phase of call i: every phase of the s x s block in turn, the diagonal first."""
    s = args.upsample
    ph = sorted(((px, py) for py in range(s) for px in range(s)), key=lambda p: (p[0] != p[1], p))
    return ph[i % len(ph)]


def upsample_call(args, lo, hi, i):
    """Call i on the pair: ptx_upsample, or with --phases a small frame through the call's phase, denoised and
    waited for, then ptx_upsample_temporal (returned as a closure: the part that is timed)."""
    if not args.phases:
        return lambda: hi.Upsample(lo)
    px, py = phase_of(args, i)
    lo.set_phase_of(hi, args.upsample, px, py)
    lo.Render()
    lo.Denoise(iterations=args.iterations)
    lo.synchronize()
    return lambda: hi.UpsampleTemporal(lo, px, py)


def upsample_pair(args, **kw):
    """(small, full-size): the small handle rendered and denoised, the full-size one with its G-buffer."""
    from pathtracerdemo_amd import _native as N
    from pathtracerdemo_amd.renderer import Renderer
    from pathtracerdemo_amd.scene.world import compile_scene
    s = args.upsample
    assert args.width % s == 0 and args.height % s == 0
    cs = compile_scene(args.scene)
    lo = Renderer(args.width // s, args.height // s, device=0, pipeline=args.pipeline)
    hi = Renderer(args.width, args.height, device=0, pipeline=args.pipeline, **kw)
    for r in (lo, hi):
        r.Initialize(cs)
    if args.follow:
        hi.set_upsample_follow(True)
    for _ in range(args.frames):
        lo.Update()
        lo.Render()
    lo.Denoise(iterations=args.iterations)
    hi.Update()
    hi.run_pass(N.PTX_PASS_GBUFFER)
    lo.synchronize()
    hi.synchronize()
    return lo, hi


def measure_upsample(args):
    from pathtracerdemo_amd import _native as N
    kind = "upsample_temporal" if args.phases else "upsample"
    bound = upsample_bound_ms(args, "guide") + upsample_bound_ms(args, kind)
    out = {"what": "ptx_" + kind, "scale": args.upsample, "width": args.width, "height": args.height, "scene": args.scene,
           "pipeline": args.pipeline, "calls": args.calls, "warmup": args.warmup, "bound_ms_at_8TBs": round(bound, 4)}
    if not args.no_events:
        import torch
        lo, hi = upsample_pair(args)
        stream = torch.cuda.Stream()
        hi.set_stream(stream.cuda_stream)
        ms = []
        for i in range(args.warmup + args.calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            call = upsample_call(args, lo, hi, i)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            if i >= args.warmup:
                ms.append(a.elapsed_time(b))
        hi.set_stream(None)
        for r in (hi, lo):
            r.close()
        out["whole_call_ms"] = {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}
        out["whole_call_fraction_of_bound"] = round(bound / statistics.median(ms), 3)
    lo, hi = upsample_pair(args, time_launches=True)
    per_call = []
    for i in range(args.warmup + args.calls):
        call = upsample_call(args, lo, hi, i)
        before = hi.stats()["kernel_ms_total"][N.PTX_STAT_DENOISE]
        call()
        hi.synchronize()
        if i >= args.warmup:
            per_call.append(hi.stats()["kernel_ms_total"][N.PTX_STAT_DENOISE] - before)
    for r in (hi, lo):
        r.close()
    out["kernel_sum_ms"] = round(statistics.median(per_call), 4)
    out["kernel_sum_ms_min_max"] = [round(min(per_call), 4), round(max(per_call), 4)]
    out["follow"] = bool(args.follow)
    return out


def measure_upsample_edits(args):
    """--upsample S --phases --edit move|pose [--follow]: ptx_upsample_temporal on a scene that is edited before
    every call, on both handles: "move" the chair between two places (ptx_update_scene), "pose" the chair between
    two palettes of a --joints skin (ptx_skin_vertices).  Per call: device events around the call on the full-size
    handle's stream (they span the table's synchronous upload), the sum of the two kernels' own times on a
    TIME_LAUNCHES handle, and the host's time for the full-size handle's edit itself (the handle idle), which on a
    following handle includes the copy of the mesh's triangle records.  share_n_above_1: pixels of the last call
    whose history holds more than one own sample."""
    import copy
    import time

    import numpy as np
    import torch
    from pathtracerdemo_amd import _native as N
    from pathtracerdemo_amd.renderer import Renderer
    from pathtracerdemo_amd.scene import world as world_mod
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from skin_cost import make_palette, make_skin
    s = args.upsample
    base = world_mod.compile_scene(args.scene)
    CHAIR_MESH, CHAIR = 2, 2
    sc = copy.deepcopy(world_mod.load_scene_json(args.scene))
    [a for a in sc["assets"] if a["type"] == "object"][CHAIR]["transform"]["position"] = [25, -90, 10]
    places = [base, world_mod.serialize_world(world_mod.World().load_from_scene(sc))]
    blk = world_mod.mesh_blocks(base, CHAIR_MESH)
    joints, weights, bind = make_skin(base.geometry[blk["vertex"]:blk["vertex_end"]].reshape(-1, 8), args.joints, np)
    palettes = [make_palette(bind, args.joints, d, np) for d in (25.0, -15.0)]

    def pair(**kw):
        lo = Renderer(args.width // s, args.height // s, device=0, pipeline=args.pipeline)
        hi = Renderer(args.width, args.height, device=0, pipeline=args.pipeline, **kw)
        for r in (lo, hi):
            r.Initialize(base)
            r.Update()
            if args.edit == "pose":
                r.SetSkin(CHAIR_MESH, joints, weights, bind)
        if args.follow:
            hi.set_upsample_follow(True)
        return lo, hi

    def edit(r, i):
        if args.edit == "move":
            cs = places[(i + 1) % 2]
            return lambda: r._call("ptx_update_scene", r._h, cs.scene.ctypes.data, len(cs.scene), None)
        pal = palettes[i % 2]
        return lambda: r._call("ptx_skin_vertices", r._h, CHAIR_MESH, pal.ctypes.data, None)

    def step(lo, hi, i):
        """Edit both handles, hi's G-buffer pass, lo's frame through the phase, denoised; hi's edit's host ms."""
        hi.synchronize()
        t0 = time.perf_counter()
        edit(hi, i)()
        t = (time.perf_counter() - t0) * 1e3
        edit(lo, i)()
        px, py = phase_of(args, i)
        hi.Update()
        hi.run_pass(N.PTX_PASS_GBUFFER)
        lo.set_phase_of(hi, s, px, py)
        lo.Render()
        lo.Denoise(iterations=args.iterations)
        lo.synchronize()
        hi.synchronize()
        return px, py, t

    def mmm(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    out = {"what": "ptx_upsample_temporal after an edit", "edit": args.edit, "follow": bool(args.follow), "scale": s,
           "width": args.width, "height": args.height, "scene": args.scene, "pipeline": args.pipeline, "joints": args.joints,
           "calls": args.calls, "warmup": args.warmup}
    lo, hi = pair()
    stream = torch.cuda.Stream()
    hi.set_stream(stream.cuda_stream)
    ms, edits = [], []
    for i in range(args.warmup + args.calls):
        px, py, t = step(lo, hi, i)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        hi.UpsampleTemporal(lo, px, py)
        b.record(stream)
        b.synchronize()
        if i >= args.warmup:
            ms.append(a.elapsed_time(b))
            edits.append(t)
    n = hi.read_upsample_history()[..., 3]
    out["share_n_above_1"] = round(float((n > 1).mean()), 4)
    hi.set_stream(None)
    for r in (hi, lo):
        r.close()
    out["whole_call_ms"] = mmm(ms)
    out["edit_host_ms"] = mmm(edits)
    lo, hi = pair(time_launches=True)
    per_call = []
    for i in range(args.warmup + args.calls):
        px, py, _ = step(lo, hi, i)
        before = hi.stats()
        hi.UpsampleTemporal(lo, px, py)
        hi.synchronize()
        after = hi.stats()
        if i >= args.warmup:
            per_call.append(after["kernel_ms_total"][N.PTX_STAT_DENOISE] - before["kernel_ms_total"][N.PTX_STAT_DENOISE])
        out["launches_per_call"] = after["kernel_launches"][N.PTX_STAT_DENOISE] - before["kernel_launches"][N.PTX_STAT_DENOISE]
    for r in (hi, lo):
        r.close()
    out["kernel_sum_ms"] = mmm(per_call)
    return out


def measure_upsample_error(args):
    """--upsample S --phases --edit pose --error: what following buys on the animated chair.  The chair is posed
    before every call (two palettes alternating, still camera, 1 spp per small frame); one small handle (temporal
    denoise, following vertices) feeds two full-size handles, one following and one not, for --calls phase-cycled
    frames after --warmup.  The reference of a pose is the full-size scene accumulated over --converge frames with
    the pose held; the error is the mean squared difference of PTX_BUF_DENOISED over the chair's pixels (the
    pose's own G-buffer), averaged over the frames."""
    import numpy as np
    from pathtracerdemo_amd import _native as N
    from pathtracerdemo_amd.renderer import Renderer
    from pathtracerdemo_amd.scene import world as world_mod
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from skin_cost import make_palette, make_skin
    s, CHAIR_MESH, CHAIR = args.upsample, 2, 2
    base = world_mod.compile_scene(args.scene)
    blk = world_mod.mesh_blocks(base, CHAIR_MESH)
    joints, weights, bind = make_skin(base.geometry[blk["vertex"]:blk["vertex_end"]].reshape(-1, 8), args.joints, np)
    palettes = [make_palette(bind, args.joints, d, np) for d in (25.0, -15.0)]

    def make(w, h):
        r = Renderer(w, h, device=0, pipeline=args.pipeline, frame_color=True)
        r.Initialize(base)
        r.Update()
        r.SetSkin(CHAIR_MESH, joints, weights, bind)
        return r

    ref, mask = [], []
    r = make(args.width, args.height)
    for pal in palettes:
        r.SkinVertices(CHAIR_MESH, pal)
        r.ResetFrameCount()
        for _ in range(args.converge):
            r.Update()
            r.Render()
        ref.append(r.read_image()[..., :3].astype(np.float64))
        g = r.read_gbuffer()[..., 0]
        mask.append((g >> 31 == 1) & ((g >> 16) & 0x7FFF == CHAIR))
    r.close()
    lo = make(args.width // s, args.height // s)
    lo.follow_vertices = True
    his = {"follow": make(args.width, args.height), "not_following": make(args.width, args.height)}
    his["follow"].set_upsample_follow(True)
    err = {k: [] for k in his}
    for i in range(args.warmup + args.calls):
        px, py = phase_of(args, i)
        for r in [lo] + list(his.values()):
            r.SkinVertices(CHAIR_MESH, palettes[i % 2])
        for hi in his.values():
            hi.Update()
            hi.run_pass(N.PTX_PASS_GBUFFER)
        lo.set_phase_of(his["follow"], s, px, py)
        lo.Render()
        lo.Denoise(iterations=args.iterations, temporal=True)
        for name, hi in his.items():
            hi.UpsampleTemporal(lo, px, py)
            if i >= args.warmup:
                d = hi.read_denoised()[..., :3].astype(np.float64) - ref[i % 2]
                err[name].append(float((d[mask[i % 2]] ** 2).mean()))
    last = (args.warmup + args.calls - 1) % 2
    out = {"what": "ptx_upsample_temporal on the animated chair, error against the converged pose", "scale": s,
           "width": args.width, "height": args.height, "scene": args.scene, "pipeline": args.pipeline, "joints": args.joints,
           "iterations": args.iterations, "frames": args.calls, "warmup": args.warmup, "converge": args.converge,
           "chair_pixels": [int(m.sum()) for m in mask],
           "mse_on_chair": {k: float(np.mean(v)) for k, v in err.items()},
           "mean_n_on_chair": {k: round(float(hi.read_upsample_history()[..., 3][mask[last]].mean()), 2) for k, hi in his.items()}}
    out["follow_over_not_following"] = round(out["mse_on_chair"]["follow"] / out["mse_on_chair"]["not_following"], 4)
    for r in [lo] + list(his.values()):
        r.close()
    return out


def measure_displayed_frame(args):
    """Host milliseconds per displayed frame under a yawing camera, every frame waited for."""
    import time
    from pathtracerdemo_amd import _native as N
    from pathtracerdemo_amd.renderer import Renderer
    from pathtracerdemo_amd.scene.world import compile_scene
    s = args.upsample
    cs = compile_scene(args.scene)
    full = Renderer(args.width, args.height, device=0, pipeline=args.pipeline)
    small = Renderer(args.width // s, args.height // s, device=0, pipeline=args.pipeline) if s else None
    rs = [r for r in (small, full) if r is not None]
    for r in rs:
        r.Initialize(cs)
    ms = []
    for i in range(args.warmup + args.calls):
        t0 = time.perf_counter()
        for r in rs:
            r.GetCamera().set_yaw(args.yaw_step * (i + 1))
            r.ResetFrameCount()
            r.Update()
        if s and args.phases:
            px, py = phase_of(args, i)
            small.set_phase_of(full, s, px, py)  # (instead of the camera its Update() just set)
            small.Render()
            small.Denoise(iterations=args.iterations)
            full.run_pass(N.PTX_PASS_GBUFFER)
            full.UpsampleTemporal(small, px, py)
        elif s:
            small.Render()
            small.Denoise(iterations=args.iterations)
            full.run_pass(N.PTX_PASS_GBUFFER)
            full.Upsample(small)
        else:
            full.Render()
            full.Denoise(iterations=args.iterations)
        for r in rs:
            r.synchronize()
        if i >= args.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    for r in rs:
        r.close()
    return {"what": "displayed frame, moving camera", "form": f"1/{s} size + G-buffer pass + ptx_upsample{'_temporal, phases cycling' if args.phases else ''}" if s else "full size + ptx_denoise",
            "yaw_step": args.yaw_step, "width": args.width, "height": args.height, "scene": args.scene, "pipeline": args.pipeline,
            "iterations": args.iterations, "frames": args.calls, "warmup": args.warmup,
            "host_ms_per_frame": {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}}


def upsample_from_trace(args):
    """Median duration of the two kernels of a ptx_upsample call (dn_guide, dn_upsample) over the traced calls."""
    rows = [r for r in csv.DictReader(open(args.trace)) if "dn_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls = [(a, b) for a, b in zip(rows, rows[1:]) if "dn_guide" in a["Kernel_Name"] and "dn_upsample" in b["Kernel_Name"]][-args.calls:]
    out = {"what": f"ptx_upsample{'_temporal' if args.phases else ''} per kernel (rocprofv3 kernel trace)", "scale": args.upsample, "width": args.width,
           "height": args.height, "calls": len(calls), "kernels": []}
    for k, kind in enumerate(("guide", "upsample_temporal" if args.phases else "upsample")):
        us = statistics.median((int(c[k]["End_Timestamp"]) - int(c[k]["Start_Timestamp"])) / 1e3 for c in calls)
        bound = upsample_bound_ms(args, kind) * 1e3
        out["kernels"].append({"kernel": calls[0][k]["Kernel_Name"].split("(")[0].replace("void ", ""), "median_us": round(us, 2),
                               "lds": int(calls[0][k]["LDS_Block_Size"]), "scratch": int(calls[0][k]["Scratch_Size"]),
                               "bound_us_at_8TBs": round(bound, 2), "fraction_of_bound": round(bound / us, 3)})
    out["sum_us"] = round(sum(k["median_us"] for k in out["kernels"]), 2)
    return out


def stage_rows(rows, top, band_h, n):
    """Rows per launch of a band with `top` halo rows above and rows - top - band_h below: guide,
    variance, iteration 0..n-1 (ptx_api.cpp denoise_stage_rows)."""
    R = 2 << n

    def span(e):
        return min(rows, top + band_h + e) - (top - min(top, e))

    return [rows, span(R - 2)] + [span(R - (4 << k)) for k in range(n)]


def measure_bands(args):
    from pathtracerdemo_amd import _native as N
    from pathtracerdemo_amd.renderer import Renderer
    from pathtracerdemo_amd.scene.world import compile_scene
    W, H, n = args.width, args.height, args.iterations
    cs = compile_scene(args.scene)
    cuts = [H * i // args.bands for i in range(args.bands + 1)]

    def make(a=0, b=0):
        r = Renderer(W, H, device=0, pipeline=args.pipeline, row_begin=a, row_end=b, frame_color=args.temporal,
                     time_launches=True)
        r.Initialize(cs)
        return r

    one, bands = make(), [make(a, b) for a, b in zip(cuts, cuts[1:])]

    def frame(i=None):
        for r in [one] + bands:
            if i is not None and args.yaw_step:
                r.GetCamera().set_yaw(args.yaw_step * (i + 1))
                r.ResetFrameCount()
            r.Update()
        one.Render()
        Renderer.render_bands(bands)
        for r in [one] + bands:
            r.synchronize()

    def spent(rs):
        return sum(r.stats()["kernel_ms_total"][N.PTX_STAT_DENOISE] for r in rs)

    import time

    import torch

    def timed_calls(first):
        whole, split, wall_whole, wall_split = [], [], [], []
        for i in range(first, first + args.warmup + args.calls):
            if args.temporal:
                frame(i)
            w0, s0 = spent([one]), spent(bands)
            t0 = time.perf_counter()
            one.Denoise(iterations=n, temporal=args.temporal)
            one.synchronize()
            t1 = time.perf_counter()
            Renderer.denoise_bands(bands, iterations=n, temporal=args.temporal)
            for b in bands:
                b.synchronize()
            t2 = time.perf_counter()
            if i >= first + args.warmup:
                whole.append(spent([one]) - w0)
                split.append(spent(bands) - s0)
                wall_whole.append((t1 - t0) * 1e3)
                wall_split.append((t2 - t1) * 1e3)
        return whole, split, wall_whole, wall_split

    def mmm(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    for _ in range(args.frames):
        frame()
    # the bands' own streams: what a host sees, and event pairs that span concurrent kernels
    _, overlapped, wall_whole, wall_split = timed_calls(0)
    # one stream for every band: each launch's events time that kernel alone
    shared = torch.cuda.Stream()
    for b in bands:
        b.set_stream(shared.cuda_stream)
    whole, split, _, _ = timed_calls(args.warmup + args.calls)
    same = all((b.read_denoised().view("uint32") == one.read_denoised()[a:z].view("uint32")).all()
               for b, a, z in zip(bands, cuts, cuts[1:]))
    R = 2 << n
    per_px = 16 + 16 + (8 if args.temporal else 0)
    halo = [(min(R, a), min(R, H - z)) for a, z in zip(cuts, cuts[1:])]
    rows = [stage_rows(t + (z - a) + b, t, z - a, n) for (t, b), a, z in zip(halo, cuts, cuts[1:])]
    out = {"what": "ptx_denoise_bands", "temporal": args.temporal, "yaw_step": args.yaw_step, "width": W, "height": H,
           "scene": args.scene, "pipeline": args.pipeline, "iterations": n, "bands": args.bands, "calls": args.calls,
           "warmup": args.warmup, "equals_whole_image": bool(same),
           "whole_image_kernel_ms": mmm(whole), "bands_kernel_ms_sum": mmm(split),
           "ratio": round(statistics.median(split) / statistics.median(whole), 3),
           "bands_kernel_ms_sum_on_own_streams_overlapped": mmm(overlapped),
           "host_ms_call_to_completion": {"whole_image": mmm(wall_whole), "bands_own_streams": mmm(wall_split)},
           "rows_per_stage": rows,
           "rows_ratio_expected": round(sum(sum(r) for r in rows) / ((2 + n) * H), 3),
           "halo_bytes_received_per_band": [[t * W * per_px, b * W * per_px] for t, b in halo],
           "denoise_clips": [b.denoise_clips() for b in bands]}
    for b in bands:
        b.set_stream(None)
    for r in [one] + bands:
        r.close()
    return out


def measure_upsample_bands(args):
    """ptx_upsample_bands on --bands equal pairs on this GPU (peer copies) against the whole-image
    ptx_upsample of the same frame on the same build."""
    import time

    import torch
    from pathtracerdemo_amd import _native as N
    from pathtracerdemo_amd.renderer import Renderer
    from pathtracerdemo_amd.scene.world import compile_scene
    s, W, H, n = args.upsample, args.width, args.height, args.iterations
    assert W % s == 0 and H % s == 0
    w, h = W // s, H // s
    cs = compile_scene(args.scene)
    cuts = [h * i // args.bands for i in range(args.bands + 1)]

    def make(ww, hh, a=0, b=0):
        r = Renderer(ww, hh, device=0, pipeline=args.pipeline, row_begin=a, row_end=b, time_launches=True)
        r.Initialize(cs)
        return r

    one, bands = make(w, h), [make(w, h, a, b) for a, b in zip(cuts, cuts[1:])]
    for _ in range(args.frames):
        for r in [one] + bands:
            r.Update()
        one.Render()
        Renderer.render_bands(bands)
    one.Denoise(iterations=n)
    Renderer.denoise_bands(bands, iterations=n)
    hi_one, his = make(W, H), [make(W, H, s * a, s * b) for a, b in zip(cuts, cuts[1:])]
    for r in [hi_one] + his:
        r.Update()
        r.run_pass(N.PTX_PASS_GBUFFER)
    for r in [one, hi_one] + bands + his:
        r.synchronize()

    def spent(rs):
        return sum(r.stats()["kernel_ms_total"][N.PTX_STAT_DENOISE] for r in rs)

    def mmm(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    def timed_calls(stream=None):
        """Per call: kernel sums and the host's call-to-completion time of the whole image and of the bands;
        with a stream (every full-size handle runs on it) also device events around each call."""
        ks_whole, ks_split, wall_whole, wall_split, ev_whole, ev_split = [], [], [], [], [], []
        for i in range(args.warmup + args.calls):
            k0, k1 = spent([hi_one]), spent(his)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if stream else None
            t0 = time.perf_counter()
            if ev:
                ev[0].record(stream)
            hi_one.Upsample(one)
            if ev:
                ev[1].record(stream)
            hi_one.synchronize()
            t1 = time.perf_counter()
            if ev:
                ev[2].record(stream)
            Renderer.upsample_bands(his, bands)
            if ev:
                ev[3].record(stream)
            for r in his:
                r.synchronize()
            t2 = time.perf_counter()
            if i >= args.warmup:
                ks_whole.append(spent([hi_one]) - k0)
                ks_split.append(spent(his) - k1)
                wall_whole.append((t1 - t0) * 1e3)
                wall_split.append((t2 - t1) * 1e3)
                if ev:
                    ev[3].synchronize()
                    ev_whole.append(ev[0].elapsed_time(ev[1]))
                    ev_split.append(ev[2].elapsed_time(ev[3]))
        return ks_whole, ks_split, wall_whole, wall_split, ev_whole, ev_split

    # the handles' own streams: what a host sees (the bands' kernels share the GPU)
    _, overlapped, wall_whole, wall_split, _, _ = timed_calls()
    # one stream for every full-size handle: each launch's events time that kernel alone, and device
    # events around a call span exactly its copies and kernels
    shared = torch.cuda.Stream()
    for r in [hi_one] + his:
        r.set_stream(shared.cuda_stream)
    ks_whole, ks_split, _, _, ev_whole, ev_split = timed_calls(shared)
    same = all((b.read_denoised().view("uint32") == hi_one.read_denoised()[s * a:s * z].view("uint32")).all()
               for b, a, z in zip(his, cuts, cuts[1:]))
    out = {"what": "ptx_upsample_bands", "scale": s, "width": W, "height": H, "scene": args.scene, "pipeline": args.pipeline,
           "iterations": n, "bands": args.bands, "calls": args.calls, "warmup": args.warmup, "equals_whole_image": bool(same),
           "whole_image_kernel_ms": mmm(ks_whole), "bands_kernel_ms_sum": mmm(ks_split),
           "kernel_ratio": round(statistics.median(ks_split) / statistics.median(ks_whole), 3),
           "bands_kernel_ms_sum_on_own_streams_overlapped": mmm(overlapped),
           "events_around_call_ms_one_stream": {"whole_image": mmm(ev_whole), "bands": mmm(ev_split)},
           "call_ratio": round(statistics.median(ev_split) / statistics.median(ev_whole), 3),
           "host_ms_call_to_completion": {"whole_image": mmm(wall_whole), "bands_own_streams": mmm(wall_split)},
           "halo_bytes_received_per_band": [[(2 if a else 0) * w * 16, (2 if z != h else 0) * w * 16] for a, z in zip(cuts, cuts[1:])]}
    for r in [hi_one] + his:
        r.set_stream(None)
    for r in [one, hi_one] + bands + his:
        r.close()
    return out


def measure_upsample_temporal_bands(args):
    """ptx_upsample_temporal_bands on --bands equal pairs on this GPU (peer copies), beside ptx_upsample_bands on
    the same pairs and the whole-image ptx_upsample_temporal; or (--displayed-frame) its clipped pixels per
    band and history_rows along the yawing camera path."""
    import torch
    from pathtracerdemo_amd import _native as N
    from pathtracerdemo_amd.renderer import Renderer
    from pathtracerdemo_amd.scene.world import compile_scene
    s, W, H, n = args.upsample, args.width, args.height, args.iterations
    assert W % s == 0 and H % s == 0
    w, h = W // s, H // s
    cs = compile_scene(args.scene)
    cuts = [h * i // args.bands for i in range(args.bands + 1)]
    Ts = [int(t) for t in str(args.history_rows).split(",")]

    def make(ww, hh, a=0, b=0):
        r = Renderer(ww, hh, device=0, pipeline=args.pipeline, row_begin=a, row_end=b, time_launches=True)
        r.Initialize(cs)
        return r

    def mmm(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    def spent(rs):
        return sum(r.stats()["kernel_ms_total"][N.PTX_STAT_DENOISE] for r in rs)

    bands = [make(w, h, a, b) for a, b in zip(cuts, cuts[1:])]
    his = [make(W, H, s * a, s * b) for a, b in zip(cuts, cuts[1:])]

    def pose(rs, i):
        for r in rs:
            r.GetCamera().set_yaw(args.yaw_step * (i + 1))
            r.ResetFrameCount()
            r.Update()

    def small_frame(los, full, phase):
        """The small handles' frame of this camera (through the phase, if any), denoised and waited for."""
        if phase is not None:
            for lo, hi in zip(los, full):
                lo.set_phase_of(hi, s, *phase)
        if len(los) > 1:
            Renderer.render_bands(los)
            Renderer.denoise_bands(los, iterations=n)
        else:
            los[0].Render()
            los[0].Denoise(iterations=n)
        for r in los:
            r.synchronize()

    if args.displayed_frame:
        clips = {}
        for T in Ts:
            for r in his:
                r.reset_accumulation()  # (drops the state: every history_rows starts from a first call)
                r.reset_stats()
            for i in range(args.warmup + args.calls):
                pose(bands + his, i)
                small_frame(bands, his, phase_of(args, i))
                for r in his:
                    r.run_pass(N.PTX_PASS_GBUFFER)
                px, py = phase_of(args, i)
                Renderer.upsample_temporal_bands(his, bands, px, py, history_rows=T)
            clips[str(T)] = [r.upsample_clips() for r in his]
        for r in bands + his:
            r.close()
        return {"what": "ptx_upsample_temporal_bands clipped pixels, moving camera", "scale": s, "width": W, "height": H,
                "scene": args.scene, "pipeline": args.pipeline, "bands": args.bands, "yaw_step": args.yaw_step,
                "frames": args.warmup + args.calls, "clips_per_band_by_history_rows": clips}

    T = Ts[0]
    one, hi_one = make(w, h), make(W, H)
    shared = torch.cuda.Stream()
    for r in [hi_one] + his:
        r.set_stream(shared.cuda_stream)
    res = {k: ([], []) for k in ("upsample_bands", "upsample_temporal", "upsample_temporal_bands")}

    def timed(kind, rs, call, keep):
        k0 = spent(rs)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(shared)
        call()
        b.record(shared)
        b.synchronize()
        for r in rs:
            r.synchronize()
        if keep:
            res[kind][0].append(spent(rs) - k0)
            res[kind][1].append(a.elapsed_time(b))

    # ptx_upsample_bands first (it drops the temporal state): the small bands under the full-size camera
    for i in range(args.warmup + args.calls):
        pose([one] + bands + his, i)
        small_frame([one], [hi_one], None)  # (the whole-image small handle renders the same frames as the bands)
        small_frame(bands, his, None)
        for r in his:
            r.run_pass(N.PTX_PASS_GBUFFER)
            r.synchronize()
        timed("upsample_bands", his, lambda: Renderer.upsample_bands(his, bands), i >= args.warmup)
    # then the temporal calls, the whole image and the bands on the same frames
    for i in range(args.warmup + args.calls):
        pose([one, hi_one] + bands + his, i)
        px, py = phase_of(args, i)
        small_frame([one], [hi_one], (px, py))
        small_frame(bands, his, (px, py))
        for r in [hi_one] + his:
            r.run_pass(N.PTX_PASS_GBUFFER)
            r.synchronize()
        timed("upsample_temporal", [hi_one], lambda: hi_one.UpsampleTemporal(one, px, py), i >= args.warmup)
        timed("upsample_temporal_bands", his, lambda: Renderer.upsample_temporal_bands(his, bands, px, py, history_rows=T),
              i >= args.warmup)
    clips = [r.upsample_clips() for r in his]
    same = all((b.read_denoised().view("uint32") == hi_one.read_denoised()[s * a:s * z].view("uint32")).all() and
               (b.read_upsample_history().view("uint32") == hi_one.read_upsample_history()[s * a:s * z].view("uint32")).all()
               for b, a, z in zip(his, cuts, cuts[1:]))
    small_same = all((b.read_denoised().view("uint32") == one.read_denoised()[a:z].view("uint32")).all()
                     for b, a, z in zip(bands, cuts, cuts[1:]))
    med = {k: statistics.median(v[0]) for k, v in res.items()}
    out = {"what": "ptx_upsample_temporal_bands", "scale": s, "width": W, "height": H, "scene": args.scene, "pipeline": args.pipeline,
           "iterations": n, "bands": args.bands, "history_rows": T, "yaw_step": args.yaw_step, "calls": args.calls,
           "warmup": args.warmup, "clips_per_band": clips, "equals_whole_image": bool(same),
           "small_bands_equal_whole_image": bool(small_same),
           "kernel_ms_sum": {k: mmm(v[0]) for k, v in res.items()},
           "events_around_call_ms_one_stream": {k: mmm(v[1]) for k, v in res.items()},
           "kernel_ratio_to_upsample_bands": round(med["upsample_temporal_bands"] / med["upsample_bands"], 3),
           "kernel_ratio_to_whole_image": round(med["upsample_temporal_bands"] / med["upsample_temporal"], 3),
           "halo_bytes_received_per_band": [[(2 * w * 16 + T * W * 48) if a else 0, (2 * w * 16 + T * W * 48) if z != h else 0]
                                            for a, z in zip(cuts, cuts[1:])]}
    for r in [hi_one] + his:
        r.set_stream(None)
    for r in [one, hi_one] + bands + his:
        r.close()
    return out


def from_trace(args):
    """Median duration of each kernel of a call (guide, [temporal,] variance, iteration 0..n-1) over the traced
    calls of the last handle (the TIME_LAUNCHES one), warm-up calls dropped."""
    px = args.width * args.height
    rows = [r for r in csv.DictReader(open(args.trace)) if "dn_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    head = ["guide", "temporal", "variance_moments"] if args.temporal else ["guide", "variance"]
    per = len(head) + args.iterations
    calls, cur = [], []
    for r in rows:  # a call starts at dn_guide
        if "dn_guide" in r["Kernel_Name"] and cur:
            calls.append(cur)
            cur = []
        cur.append(r)
    calls.append(cur)
    calls = [c for c in calls if len(c) == per][-args.calls:]
    out = {"what": "ptx_denoise per kernel (rocprofv3 kernel trace)", "width": args.width, "height": args.height,
           "iterations": args.iterations, "calls": len(calls), "kernels": []}
    for k in range(per):
        us = statistics.median((int(c[k]["End_Timestamp"]) - int(c[k]["Start_Timestamp"])) / 1e3 for c in calls)
        kind = head[k] if k < len(head) else "atrous"
        name = calls[0][k]["Kernel_Name"].split("(")[0].replace("void ", "")
        out["kernels"].append({"kernel": name + ("" if k < len(head) else f" step {1 << (k - len(head))}"), "median_us": round(us, 2),
                               "lds": int(calls[0][k]["LDS_Block_Size"]),
                               "scratch": int(calls[0][k]["Scratch_Size"]),
                               "bound_us_at_8TBs": round(bound_ms(kind, px) * 1e3, 2),
                               "fraction_of_bound": round(bound_ms(kind, px) * 1e3 / us, 3)})
    out["sum_us"] = round(sum(k["median_us"] for k in out["kernels"]), 2)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scene", default="c3_interior_32")
    ap.add_argument("--pipeline", default="reuse")
    ap.add_argument("--frames", type=int, default=2, help="frames rendered before the timed calls")
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--temporal", action="store_true", help="the temporal mode on a frame_color handle")
    ap.add_argument("--yaw-step", type=float, default=0.5, help="--temporal: degrees the camera yaws before every call (0: still)")
    ap.add_argument("--bands", type=int, default=0, help="time ptx_denoise_bands on the frame as this many equal row bands")
    ap.add_argument("--upsample", type=int, default=0, help="time ptx_upsample from 1/S of --width x --height (S: 2, 3 or 4)")
    ap.add_argument("--phases", action="store_true", help="--upsample: ptx_upsample_temporal on small frames whose phase cycles")
    ap.add_argument("--history-rows", default="32", help="--bands --upsample --phases: history_rows (--displayed-frame: a comma list)")
    ap.add_argument("--displayed-frame", action="store_true", help="host ms per displayed frame under a yawing camera")
    ap.add_argument("--no-events", action="store_true", help="only the TIME_LAUNCHES handle (the run a profiler traces)")
    ap.add_argument("--trace", help="a rocprofv3 run_kernel_trace.csv of this script: print per-kernel medians")
    ap.add_argument("--follow", action="store_true", help="--upsample --phases: the full-size handle follows (ptx_upsample_follow)")
    ap.add_argument("--edit", choices=("move", "pose"), help="--upsample --phases: edit the scene before every call "
                    "(move: the chair's instance, pose: the chair through a skin), on both handles")
    ap.add_argument("--joints", type=int, default=32, help="--edit pose: joints of the chair's skin")
    ap.add_argument("--error", action="store_true", help="--edit pose: the error on the animated chair, following and not, "
                    "over --calls phase-cycled frames")
    ap.add_argument("--converge", type=int, default=256, help="--error: frames a pose's reference accumulates")
    ap.add_argument("--repo", help="the tree whose package is measured (an older one: without --follow), "
                    "its library or PTX_LIB_PATH's")
    args = ap.parse_args()
    if args.repo:
        sys.path.insert(0, os.path.abspath(args.repo))
    if args.edit:
        assert args.upsample and args.phases and not args.bands, "--edit goes with --upsample S --phases"
        assert not args.error or args.edit == "pose", "--error goes with --edit pose"
        out = measure_upsample_error(args) if args.error else measure_upsample_edits(args)
    elif args.bands and args.upsample and args.phases:
        out = measure_upsample_temporal_bands(args)
    elif args.displayed_frame:
        out = measure_displayed_frame(args)
    elif args.upsample:
        out = upsample_from_trace(args) if args.trace else measure_upsample_bands(args) if args.bands else measure_upsample(args)
    else:
        out = from_trace(args) if args.trace else measure_bands(args) if args.bands else measure(args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
