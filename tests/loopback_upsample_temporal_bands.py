"""ptx_upsample_temporal_bands over communicators, in ONE process on ONE GPU, through the loopback
communicator (tests/loopback/loopback_rccl.cpp).  Run by tests/test_gpu_upsample_temporal_bands.py as a
child process with PTX_RCCL_LIB set; prints one JSON object with what it measured.

Three band handles of a 64x200 frame, each with a communicator made from its own host thread, render
through a phase of the 128x400 frame and denoise themselves (ptx_denoise_bands, the n = 3 communicator
branch); three full-size band handles hold a G-buffer.  Per form -- three rank-form calls (n = 1, every
rank makes the call from its own thread, as the ranks of a multi-GPU job do), then the n = 3 communicator
branch from one thread -- fresh full-size handles make two calls with a yaw between them: the first
sends the rows of bands without a state, the second reprojects through the rows it received.  Both are
compared with a whole-image pair, and every small band's halo_bytes_sent with
2 x 64 x 16 + T x 128 x 48 bytes per neighbour and call.
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

W, H, R, S, T = 64, 200, 12, 2, 40
CUTS = [0, 66, 133, 200]
PHASES = [(1, 0), (0, 1)]


def make(cs, a=0, b=0):
    r = Renderer(W, H, device=0, pipeline="reuse", reuse_radius=R, row_begin=a, row_end=b)
    r.Initialize(cs)
    return r


def full_size(cs, a=0, b=0):
    hi = Renderer(S * W, S * H, device=0, pipeline="restir", row_begin=S * a, row_end=S * b)
    hi.Initialize(cs)
    return hi


def pose(his, yaw):
    for r in his:
        r.GetCamera().set_yaw(yaw)
        r.Update()
        r.run_pass(native.PTX_PASS_GBUFFER)


def main():
    cs = compile_scene("c3_interior_32")
    one = make(cs)
    bands = [make(cs, a, b) for a, b in zip(CUTS, CUTS[1:])]
    connect(bands)
    calls, yaw = [], 0.0
    for form in ("rank", "bands"):
        hi_one = full_size(cs)  # (fresh: the form's first call is a first call)
        his = [full_size(cs, a, b) for a, b in zip(CUTS, CUTS[1:])]
        for k, (px, py) in enumerate(PHASES):
            yaw += 1.5
            pose([hi_one] + his, yaw)
            for lo, hi in zip([one] + bands, [hi_one] + his):
                lo.set_phase_of(hi, S, px, py)
            one.Render()
            errs = run_threads([b.Render for b in bands])
            assert not any(errs), errs
            one.Denoise()
            Renderer.denoise_bands(bands)
            hi_one.UpsampleTemporal(one, px, py)
            sent = [b.comm_info()["halo_bytes_sent"] for b in bands]
            if form == "rank":
                errs = run_threads([lambda a=a, b=b: Renderer.upsample_temporal_bands([a], [b], px, py, history_rows=T)
                                    for a, b in zip(his, bands)])
                assert not any(errs), errs
            else:
                Renderer.upsample_temporal_bands(his, bands, px, py, history_rows=T)
            hist = hi_one.read_upsample_history()
            grid = ((np.arange(S * H) % S) == py)[:, None] & ((np.arange(S * W) % S) == px)[None, :]
            calls.append({"form": form,
                          "upsampled": differs(np.concatenate([a.read_denoised() for a in his]), hi_one.read_denoised()),
                          "history": differs(np.concatenate([a.read_upsample_history() for a in his]), hist),
                          "small": differs(np.concatenate([b.read_denoised() for b in bands]), one.read_denoised()),
                          "clips": [a.upsample_clips() for a in his],
                          # (a pixel off this phase's grid has own samples only through the moved camera's history)
                          "reprojected": bool(k > 0 and (hist[..., 3][~grid] >= 1).any()),
                          "halo_bytes_grew": [b.comm_info()["halo_bytes_sent"] - s for b, s in zip(bands, sent)]})
        if form == "bands":  # a small band without a communicator beside two with one: refused before anything is sent
            lone = make(cs, CUTS[1], CUTS[2])
            refused = False
            try:
                Renderer.upsample_temporal_bands(his, [bands[0], lone, bands[2]], 0, 1, history_rows=T)
            except native.PtxError as e:
                refused = "either every small band owns a communicator or none" in str(e)
            lone.close()
        for a in [hi_one] + his:
            a.close()
    out = {"calls": calls, "refused_mixed": refused, "history_rows": T}
    for r in [one] + bands:
        r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
