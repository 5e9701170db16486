"""ptx_denoise_bands over communicators, in ONE process on ONE GPU, through the loopback communicator
(tests/loopback/loopback_rccl.cpp).  Run by tests/test_gpu_denoise_bands.py as a child process with
PTX_RCCL_LIB set; prints one JSON object with what it measured.

Three band handles of a 64x200 frame, each with a communicator made from its own host thread.  The
denoiser's halo moves first as three rank-form calls (n = 1, every rank makes the call from its own
thread, as the ranks of a multi-GPU job do), then through the n = 3 communicator branch from one
thread: a spatial call and two temporal calls each (the camera yaws between the temporal ones), every
result compared with one whole-image handle making the same calls.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from loopback_bands import connect, differs, run_threads  # noqa: E402
from pathtracerdemo_amd import _native as native  # noqa: E402
from pathtracerdemo_amd.renderer import Renderer  # noqa: E402
from pathtracerdemo_amd.scene.world import compile_scene  # noqa: E402

W, H, R = 64, 200, 12
CUTS = [0, 66, 133, 200]


def make(cs, a=0, b=0):
    r = Renderer(W, H, device=0, pipeline="reuse", reuse_radius=R, row_begin=a, row_end=b, frame_color=True)
    r.Initialize(cs)
    return r


def next_frame(one, bands, yaw):
    for r in [one] + bands:
        r.GetCamera().set_yaw(yaw)
        r.ResetFrameCount()
        r.Update()
    one.Render()
    errs = run_threads([b.Render for b in bands])
    assert not any(errs), errs


def main():
    cs = compile_scene("c3_interior_32")
    one = make(cs)
    bands = [make(cs, a, b) for a, b in zip(CUTS, CUTS[1:])]
    connect(bands)
    calls = []

    def call(form, temporal):
        sent = [b.comm_info()["halo_bytes_sent"] for b in bands]
        one.Denoise(temporal=temporal)
        if form == "rank":
            errs = run_threads([lambda b=b: Renderer.denoise_bands([b], temporal=temporal) for b in bands])
            assert not any(errs), errs
        else:
            Renderer.denoise_bands(bands, temporal=temporal)
        res = {"form": form, "temporal": temporal, "history": 0,
               "denoised": differs(np.concatenate([b.read_denoised() for b in bands]), one.read_denoised()),
               "halo_bytes_grew": [b.comm_info()["halo_bytes_sent"] - s for b, s in zip(bands, sent)]}
        if temporal:
            res["history"] = differs(np.concatenate([b.read_denoise_history() for b in bands]), one.read_denoise_history())
        calls.append(res)

    yaw = 0.0
    for form in ("rank", "bands"):
        next_frame(one, bands, yaw)
        call(form, False)
        call(form, True)
        yaw += 1.5
        next_frame(one, bands, yaw)
        call(form, True)
        yaw += 1.5
    hist = one.read_denoise_history()
    refused = False
    try:  # 6 iterations need 128 rows of every band: refused on every rank before anything is sent
        Renderer.denoise_bands([bands[1]], iterations=6)
    except native.PtxError as e:
        refused = "128 rows" in str(e)
    out = {"calls": calls, "clips": [b.denoise_clips() for b in bands],
           "mean_n": float(hist[..., 3][hist[..., 3] > 0].mean()), "refused_small_band": refused}
    for r in [one] + bands:
        r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
