"""ptx_denoise_bands on the CPU: the halo constant it rests on, pinned with the numpy restatement
(tests/denoise_ref.py), and the C ABI's new surface.  A band that filters the window of its rows and
R rows on either side, as if the window were the whole image, reproduces the whole image's result on
its rows exactly when R = 2^(iterations + 1) -- and not with one row fewer.  The HIP path is compared
with one whole-image handle bit for bit in tests/test_gpu_denoise_bands.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import denoise_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 20, 96
B0, B1 = 40, 52


def random_guides():
    """Several keys in column stripes, misses sprinkled in, surfaces near one plane so that the
    plane and normal weights stay above zero far away: every tap the reach allows can count."""
    rng = np.random.default_rng(23)
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    P = np.stack([xs * np.float32(0.05), ys * np.float32(0.05),
                  rng.uniform(-0.002, 0.002, (H, W)).astype(np.float32)], -1).astype(np.float32)
    n = np.stack([rng.uniform(-0.05, 0.05, (H, W)), rng.uniform(-0.05, 0.05, (H, W)), np.ones((H, W))], -1).astype(np.float32)
    N = (n / np.sqrt(D.dot3(n, n))[..., None]).astype(np.float32)
    key = (1 + (xs // 5) % 4).astype(np.uint32)  # (column stripes: a chain of taps runs down a column unbroken)
    key[rng.uniform(size=(H, W)) < 0.04] = D.MISS
    G = D.guides_from_surfaces(key, P, N, (0.5, 2.4, 4.0))
    img = np.ones((H, W, 4), np.float32)
    img[..., :3] = rng.gamma(0.6, 0.5, (H, W, 3)).astype(np.float32)
    return G, img


def window(G, img, lo, hi):
    return D.Guides(G.key[lo:hi], G.P[lo:hi], G.N[lo:hi], G.r[lo:hi]), img[lo:hi]


@pytest.fixture(scope="module")
def frame():
    G, img = random_guides()
    assert len(np.unique(G.key[G.hit])) >= 4 and (~G.hit).any()
    return G, img, {n: D.denoise(img, G, iterations=n) for n in (1, 2, 3)}


@pytest.mark.parametrize("n", [1, 2, 3])
def test_a_window_with_the_reach_reproduces_the_band_and_one_row_fewer_does_not(frame, n):
    G, img, whole = frame
    R = 2 ** (n + 1)
    assert B0 - R >= 0 and B1 + R <= H
    want = whole[n][B0:B1].view(np.uint32)
    for halo, equal in ((R, True), (R - 1, False)):
        Gw, iw = window(G, img, B0 - halo, B1 + halo)
        got = D.denoise(iw, Gw, iterations=n)[halo:halo + (B1 - B0)].view(np.uint32)
        assert (got == want).all() == equal, f"{n} iterations, {halo} halo rows"


def test_the_reach_recursion_gives_the_constant():
    """r = reach of the colour, s = of the variance (include/ptx.h, ptx_denoise_bands): r_n = 2^(n+1)."""
    r, s = 0, 3
    for k in range(6):
        r, s = max(r + 2 ** (k + 1), s + 1), max(r, s) + 2 ** (k + 1)
        assert r == 2 ** (k + 2)


def test_the_library_exports_ptx_denoise_bands():
    from pathtracerdemo_amd import _native as N
    lib = N.load()
    assert hasattr(lib, "ptx_denoise_bands") and "ptx_denoise_bands" in N.EXPORTED
    assert lib.ptx_denoise_bands(None, 0, None) == -1  # PTX_E_INVALID
    h = (ctypes.c_void_p * 1)(None)
    assert lib.ptx_denoise_bands(h, 1, None) == -1
    txt = open(os.path.join(ROOT, "include", "ptx.h")).read()
    assert re.search(r"^int ptx_denoise_bands\(ptx_handle \*const \*handles, int n, const ptx_denoise_params \*p", txt, re.M)
    defs = {k: int(v) for k, v in re.findall(r"^#define\s+(PTX_\w+)\s+(\d+)\b", txt, re.M)}
    assert defs["PTX_COUNTER_DENOISE_CLIP"] == N.PTX_COUNTER_DENOISE_CLIP == 7
    assert defs["PTX_ABI_VERSION"] == N.PTX_ABI_VERSION == lib.ptx_abi_version() == 5
    assert ctypes.sizeof(N.PtxDenoiseParams) == 32
