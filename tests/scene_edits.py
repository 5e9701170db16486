"""The scene edits the ptx_update_scene tests share (test infrastructure): c3_interior_32 with its chair
(instance 2) moved, turned or scaled, its rect lights dimmed, a material recoloured.  Every edit keeps the
layout -- length, offsets, geometry, accel -- and is serialised once per process."""
from __future__ import annotations

import copy
import dataclasses

import numpy as np

from pathtracerdemo_amd.scene.world import (STRIDE_INSTANCE, STRIDE_MATERIAL, World, load_scene_json,
                                            serialize_world)

SCENE = "c3_interior_32"
CHAIR = 2  # the chair's instance index (and its asset's place among the objects)
EDITS = ("move", "turn", "scale", "light", "mat", "light_mat")
# E_mat: the albedo of the first material of mesh 0 (the room), words 0..2 of its record
MAT_ALBEDO = (0.8, 0.2, 0.2)
WINDOW_AT = (0.5, -0.5, 1.0)  # where the switched instance stands: in front of the default camera

_cache: dict = {}


def _json(move=None, turn=None, scale=None, light=None):
    sc = copy.deepcopy(load_scene_json(SCENE))
    objects = [a for a in sc["assets"] if a["type"] == "object"]
    tr = objects[CHAIR]["transform"]
    assert objects[CHAIR]["meshName"] == "Chair" and tr["position"] == [0, -90, 0] and tr["scale"] == [0.02] * 3
    if move is not None:
        tr["position"] = list(move)
    if turn is not None:
        tr["rotation"] = list(turn)
    if scale is not None:
        tr["scale"] = [scale] * 3
    if light is not None:
        for a in sc["assets"]:
            if a["type"] == "rect-light":
                a["lightParams"]["intensity"] *= light
    return sc


_CHAIR = {"base": {}, "move": dict(move=(25, -90, 10)), "turn": dict(move=(25, -90, 10), turn=(0, 30, 0)),
          "scale": dict(scale=0.025)}


def compose(chair: str = "base", light: int = 0, mat=False):
    """The scene with the chair as after edit `chair` ("base": where it stands; "window": instance 2
    switched to the PureWindow mesh, a smaller one, mesh 1 of 3), E_light applied `light` times (every
    rect light's intensity x 0.5 each time) and, with `mat`, E_mat (True: the albedo; "trans": the
    transmission word turned on as well, which the root records carry too)."""
    key = (chair, light, mat)
    if key not in _cache:
        cs = serialize_world(World().load_from_scene(_json(light=0.5 ** light if light else None,
                                                           **_CHAIR.get(chair, {}))))
        scene = cs.scene.copy()
        if chair == "window":
            from pathtracerdemo_amd.scene.world import Instance, euler_degrees_to_quat
            d = cs.offsets["mesh_descriptor"]
            assert scene[33 * CHAIR + 32] == 2 and scene[d + 6 + 5] < scene[d + 12 + 5]  # fewer sub-meshes than the chair
            w = Instance("PureWindow", WINDOW_AT, euler_degrees_to_quat((0, 60, 0)), (0.5, 0.5, 0.5))
            scene[33 * CHAIR:33 * CHAIR + 33] = w.serialize({"PureWindow": 1})
        if mat:
            m = cs.offsets["material"]
            assert scene[m + 10] == 0  # (no transmission: the albedo is what the kernels read)
            scene[m:m + 3] = np.array(MAT_ALBEDO, np.float32).view(np.uint32)
            if mat == "trans":
                scene[m + 10] = np.float32(1.0).view(np.uint32)
        cs = dataclasses.replace(cs, scene=scene)
        cs.scene.setflags(write=False)
        _cache[key] = cs
    return _cache[key]


def base():
    return compose()


def edited(name: str):
    """One edit of the unedited scene: "move" E_move, "turn" E_turn (E_move plus a 30 degree turn about Y),
    "scale" E_scale, "light" E_light, "mat" E_mat, "light_mat" both of the last."""
    if name in _CHAIR:
        return compose(chair=name)
    return compose(light=int("light" in name), mat="mat" in name)


def instance_block(cs) -> np.ndarray:
    return cs.scene[:STRIDE_INSTANCE * cs.instance_count]


def changed_words(cs) -> np.ndarray:
    return np.nonzero(cs.scene != base().scene)[0]


def block_of(cs, word: int) -> str:
    o = cs.offsets
    if word < STRIDE_INSTANCE * cs.instance_count:
        return "instances"
    if word < o["material"]:
        return "descriptors"
    if word < o["light"]:
        return "materials"
    return "lights"


assert STRIDE_MATERIAL == 15
