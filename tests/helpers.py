"""Shared helpers for the parity tests."""
import copy
import json
import os

import numpy as np

from pathtracerdemo_amd.scene.camera import Camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stress_scene():
    """C3 with 11 chairs under anisotropic scales and rotations about all three axes, some of
    them overlapping the camera's line of sight and each other."""
    from pathtracerdemo_amd.scene.world import compile_scene
    d = json.load(open(os.path.join(ROOT, "scenes", "c3_furnished.json")))
    k = 0
    for a in d["assets"]:
        if a.get("meshName") == "Chair" and a["id"] != "chair_instance_0":
            k += 1
            t = a["transform"]
            t["scale"] = [0.02 * (1 + 0.3 * (k % 3)), 0.02 * (1 + 0.2 * (k % 4)), 0.01 + 0.004 * k]
            t["rotation"] = [11.0 * k, 37.0 * k, -23.0 * k]
            t["position"] = [t["position"][0] * 0.6, -90 + 15 * (k % 3), t["position"][2] * 0.5 + 40]
    return compile_scene(d)


def many_instances_scene():
    """DUMMY_SCENE_1 with ten PureWindow instances (11 instances > the 8 staged in LDS)."""
    from pathtracerdemo_amd.scene.world import compile_scene
    d = json.load(open(os.path.join(ROOT, "scenes", "dummy_scene_1.json")))
    win = next(a for a in d["assets"] if a.get("meshName") == "PureWindow")
    extra = []
    for k in range(1, 10):
        w = copy.deepcopy(win)
        w["id"] = f"window_instance_{k}"
        w["transform"]["position"] = [-3.0 + 0.6 * k, 0.1 * k, -2.0 - 0.3 * k]
        extra.append(w)
    d["assets"] = d["assets"][:2] + extra + d["assets"][2:]
    cs = compile_scene(d)
    assert cs.instance_count == 11
    return cs


def windows_scene(n):
    from pathtracerdemo_amd.scene.world import compile_scene
    d = json.load(open(os.path.join(ROOT, "scenes", "dummy_scene_1.json")))
    win = next(a for a in d["assets"] if a.get("meshName") == "PureWindow")
    extra = []
    for k in range(1, n):
        w = copy.deepcopy(win)
        w["id"] = f"window_instance_{k}"
        w["transform"]["position"] = [-3.0 + 0.035 * k, 0.006 * k, -2.0 - 0.02 * k]
        extra.append(w)
    d["assets"] = d["assets"][:2] + extra + d["assets"][2:]
    return compile_scene(d)


def table_bytes(cs):
    n_subs = sum(int(cs.scene[cs.offsets["mesh_descriptor"] + 6 * int(cs.scene[33 * i + 32]) + 5])
                 for i in range(cs.instance_count))
    return ((32 * n_subs + 15) & ~15) + 144 * cs.instance_count


def huge_tables_scene():
    cs = windows_scene(170)
    assert table_bytes(cs) > 24576  # past kLdsTableMax: the global-table kernels
    return cs


def uniform_for(cs, W, H, frame=1, location=(0.0, 0.0, 6.0), yaw=0.0, pitch=0.0):
    cam = Camera(W, H)
    cam.set_location(*location)
    if yaw:
        cam.set_yaw(yaw)
    if pitch:
        cam.set_pitch(pitch)
    return cs.uniform(W, H, cam.view_projection_inverse(), cam.location, frame)


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    finite = np.isfinite(a) & np.isfinite(b)
    num = np.sqrt(((a - b)[finite] ** 2).sum())
    den = np.sqrt((b[finite] ** 2).sum())
    return float(num / den) if den > 0 else float(num)
