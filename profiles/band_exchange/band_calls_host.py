"""Host time of ptx_denoise_bands and ptx_upsample_bands on 4 bands of 1920x1080 (peer copies), many
calls: the call alone (enqueue) and the call to completion.  One JSON line."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from pathtracerdemo_amd import _native as N  # noqa: E402
from pathtracerdemo_amd.renderer import Renderer  # noqa: E402
from pathtracerdemo_amd.scene.world import compile_scene  # noqa: E402

W, H, NB, CALLS = 1920, 1080, 4, int(os.environ.get("CALLS", "200"))


def med(v):
    return round(statistics.median(v), 4)


def bands_of(cs, w, h):
    cuts = [h * i // NB for i in range(NB + 1)]
    rs = [Renderer(w, h, device=0, pipeline="reuse", row_begin=a, row_end=b) for a, b in zip(cuts, cuts[1:])]
    for r in rs:
        r.Initialize(cs)
    return rs, cuts


def timed(call, rs):
    enq, done = [], []
    for i in range(CALLS + 20):
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        for r in rs:
            r.synchronize()
        t2 = time.perf_counter()
        if i >= 20:
            enq.append((t1 - t0) * 1e3)
            done.append((t2 - t0) * 1e3)
    return {"call_ms": med(enq), "to_completion_ms": med(done)}


def main():
    cs = compile_scene("c3_interior_32")
    out = {"lib": os.path.basename(os.environ.get("PTX_LIB_PATH", "default")), "calls": CALLS}
    rs, _ = bands_of(cs, W, H)
    for _ in range(2):
        for r in rs:
            r.Update()
        Renderer.render_bands(rs)
    out["denoise_bands"] = timed(lambda: Renderer.denoise_bands(rs, iterations=5), rs)
    for r in rs:
        r.close()
    los, cuts = bands_of(cs, W // 2, H // 2)
    for _ in range(2):
        for r in los:
            r.Update()
        Renderer.render_bands(los)
    Renderer.denoise_bands(los, iterations=5)
    his = [Renderer(W, H, device=0, pipeline="reuse", row_begin=2 * a, row_end=2 * b) for a, b in zip(cuts, cuts[1:])]
    for r in his:
        r.Initialize(cs)
        r.Update()
        r.run_pass(N.PTX_PASS_GBUFFER)
    out["upsample_bands"] = timed(lambda: Renderer.upsample_bands(his, los), his)
    for r in his + los:
        r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
