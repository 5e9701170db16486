#!/usr/bin/env python3
"""Generate tests/golden/denoise_c1_48x36.npz: one oracle frame of C1 (dummy_scene_1, the reference
ReSTIR pipeline, 48x36, default test camera) and its denoised image by tests/denoise_ref.py with
the default parameters.  The fixture pins the restatement: a later change to it, to the oracle or
to the scene compiler that alters the output is a regression.
Run:  python tests/golden/make_denoise_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import denoise_ref as D  # noqa: E402
from helpers import uniform_for  # noqa: E402
from oracle import oracle as O  # noqa: E402
from pathtracerdemo_amd.scene.world import compile_scene  # noqa: E402

W, H = 48, 36
FIXTURE = "denoise_c1_48x36.npz"


def main():
    O.build()
    cs = compile_scene("dummy_scene_1")
    fr = O.Frame(uniform_for(cs, W, H, 1), cs.scene, cs.geometry, cs.accel)
    fr.run(O.PASS_RESTIR, threads=1)
    out = D.denoise_frame(fr.accum, fr.uniform, cs, fr.gbuffer)
    np.savez_compressed(os.path.join(HERE, FIXTURE), uniform=fr.uniform, gbuffer=fr.gbuffer, accum=fr.accum,
                        denoised=out)
    print("wrote", FIXTURE)


if __name__ == "__main__":
    main()
