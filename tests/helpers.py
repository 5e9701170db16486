"""Shared helpers for the parity tests."""
import copy
import json
import os
import struct

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


def write_grid_glb(path, n_prims, seed):
    """A GLB of one node, one mesh and `n_prims` primitives sharing one opaque material.  Primitive k
    is an m x m grid of quads, m = 1 + k % 3 (every third sub-mesh root is a single leaf), of side
    0.36 around ((k % 10) 0.4 - 1.8, (k // 10) 0.4 - 1.4, -2 - 0.05 (k % 7)), with a little seeded z
    noise and +z normals; each primitive has its own POSITION / NORMAL / u32 index accessors."""
    rng = np.random.default_rng(seed)
    blob, views, accessors, prims = b"", [], [], []

    def accessor(a, kind, target):
        nonlocal blob
        views.append({"buffer": 0, "byteOffset": len(blob), "byteLength": a.nbytes, "target": target})
        acc = {"bufferView": len(views) - 1, "componentType": 5126 if a.dtype == np.float32 else 5125,
               "count": len(a), "type": kind}
        if kind == "VEC3":
            acc["min"], acc["max"] = a.min(axis=0).tolist(), a.max(axis=0).tolist()
        accessors.append(acc)
        blob += a.tobytes()
        return len(accessors) - 1

    for k in range(n_prims):
        m = 1 + k % 3
        g = np.linspace(-0.18, 0.18, m + 1)
        x, y = (c.reshape(-1) for c in np.meshgrid(g, g, indexing="xy"))
        pos = np.stack([x + (k % 10) * 0.4 - 1.8, y + (k // 10) * 0.4 - 1.4,
                        -2.0 - 0.05 * (k % 7) + rng.uniform(-0.01, 0.01, size=len(x))], axis=1).astype(np.float32)
        nrm = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (len(pos), 1))
        i, j = (c.reshape(-1) for c in np.meshgrid(np.arange(m), np.arange(m), indexing="xy"))
        a = j * (m + 1) + i
        idx = np.stack([a, a + 1, a + m + 2, a, a + m + 2, a + m + 1], axis=1).reshape(-1).astype(np.uint32)
        prims.append({"attributes": {"POSITION": accessor(pos, "VEC3", 34962), "NORMAL": accessor(nrm, "VEC3", 34962)},
                      "indices": accessor(idx, "SCALAR", 34963), "material": 0})
    doc = {"asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": [0]}], "nodes": [{"mesh": 0}],
           "meshes": [{"primitives": prims}], "buffers": [{"byteLength": len(blob)}], "bufferViews": views,
           "accessors": accessors,
           "materials": [{"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.7, 0.6, 1.0], "metallicFactor": 0.0,
                                                   "roughnessFactor": 0.9}}]}
    js = json.dumps(doc).encode()
    js += b" " * (-len(js) % 4)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<III", 0x46546C67, 2, 12 + 8 + len(js) + 8 + len(blob)))
        fh.write(struct.pack("<II", len(js), 0x4E4F534A) + js)
        fh.write(struct.pack("<II", len(blob), 0x004E4942) + blob)


def root_chunks_scene(asset_dir):
    """Three instances of two generated meshes of 70 and 33 sub-meshes (write_grid_glb, written into
    `asset_dir`) and a point light: sub-mesh counts [70, 33, 70], so a walk takes an instance's roots
    in three chunks of 32, in two, and in a last chunk of one root.  The tables fit the LDS."""
    from pathtracerdemo_amd.scene.world import compile_scene
    write_grid_glb(os.path.join(str(asset_dir), "Grid70.glb"), 70, seed=70)
    write_grid_glb(os.path.join(str(asset_dir), "Grid33.glb"), 33, seed=33)

    def obj(name, mesh, pos, rot, scale):
        return {"id": name, "type": "object", "meshName": mesh,
                "transform": {"position": pos, "rotation": rot, "scale": scale}}
    d = {"id": "root_chunks", "name": "root chunks", "assets": [
        obj("grid_a", "Grid70", [0, 0, 0], [0, 0, 0], [1, 1, 1]),
        obj("grid_b", "Grid33", [0.1, 0.05, -0.6], [0, 10, 5], [1.2, 0.9, 1]),
        obj("grid_c", "Grid70", [-0.1, 0.1, -1.3], [7, -12, 0], [1, 1, 1]),
        {"id": "bulb", "type": "point-light",
         "lightParams": {"position": [0, 0, 1], "color": [1, 1, 1], "intensity": 10.0}}]}
    cs = compile_scene(d, str(asset_dir))
    assert cs.instance_count == 3 and table_bytes(cs) <= 24576
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
