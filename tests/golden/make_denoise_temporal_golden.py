#!/usr/bin/env python3
"""Generate tests/golden/denoise_temporal_c1_48x36.npz: three consecutive oracle frames of C1
(dummy_scene_1, the reference ReSTIR pipeline, 48x36) under a camera that yaws 2 degrees before the
second and third frame, accumulated as frames 1..3 -- per frame the uniform, the G-buffer, the
accumulation and the frame's own colour (the same frame rendered once more into a zeroed
accumulation, which then holds c / (F + 1): c = accum * (F + 1), good to an ulp) -- and the history
{C.rgb, n} and the denoised image of tests/denoise_temporal_ref.py after each, default parameters.
The fixture pins the restatement: a later change to it, to the oracle or to the scene compiler that
alters the output is a regression.
Run:  python tests/golden/make_denoise_temporal_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import denoise_ref as D  # noqa: E402
import denoise_temporal_ref as T  # noqa: E402
from helpers import uniform_for  # noqa: E402
from oracle import oracle as O  # noqa: E402
from pathtracerdemo_amd.scene.world import compile_scene  # noqa: E402

W, H = 48, 36
FIXTURE = "denoise_temporal_c1_48x36.npz"
YAWS = (0.0, 2.0, 4.0)


def main():
    O.build()
    cs = compile_scene("dummy_scene_1")
    t = T.TemporalDenoiser()
    rec = {k: [] for k in ("uniform", "gbuffer", "frame_color", "accum", "history", "denoised")}
    accum = np.zeros((H, W, 4), np.float32)
    for k, yaw in enumerate(YAWS):
        u = uniform_for(cs, W, H, 1, yaw=yaw)
        alone = O.Frame(u, cs.scene, cs.geometry, cs.accel)  # the same frame into a zeroed accumulation: mix(0, c, 1 / (k + 2))
        alone.set_frame_index(k + 1)
        alone.run(O.PASS_RESTIR, threads=1)
        fr = O.Frame(u, cs.scene, cs.geometry, cs.accel)
        fr.set_frame_index(k + 1)
        fr.accum[...] = accum
        fr.run(O.PASS_RESTIR, threads=1)
        accum = fr.accum.copy()
        color = alone.accum.copy()
        color[..., :3] = alone.accum[..., :3] * np.float32(k + 2)  # (good to an ulp: a fixture, not a parity check)
        G = D.guides_from_gbuffer(fr.uniform, cs.scene, cs.geometry, cs.accel, fr.gbuffer)
        out = t.denoise(color, accum, G, fr.uniform)
        for name, v in (("uniform", fr.uniform), ("gbuffer", fr.gbuffer), ("frame_color", color), ("accum", accum),
                        ("history", t.history), ("denoised", out)):
            rec[name].append(np.array(v))
    np.savez_compressed(os.path.join(HERE, FIXTURE), **{k: np.stack(v) for k, v in rec.items()})
    print("wrote", FIXTURE)


if __name__ == "__main__":
    main()
