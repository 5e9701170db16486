"""ptx_present on a value table (tests/synthetic_frames.py present_values): every k / 255, the f32
around every (k + 0.5) / 255 and each x whose x * 255 is exactly k + 0.5 (round half to even: 256 of
the 256 ties are met in f32, tests/test_synthetic_frames_ref.py), +-0, denormals, 1 +- ulp, values
outside [0, 1], +-inf and NaN of both signs, quiet and signalling.  The table is dealt over r, g and b
independently, written as the accumulation of a handle that has rendered one frame, and presented in
RGBA and BGRA onto canvases whose texel arithmetic is exact, degenerate or long.  Byte-exact against
oracle.present."""
import numpy as np
import pytest

import synthetic_frames as S

pytestmark = pytest.mark.gpu

CANVASES = [(600, 450), (300, 225), (1, 1), (70000, 1), (1, 70000)]


def make(cs, W, H):
    from pathtracerdemo_amd.renderer import Renderer
    r = Renderer(W, H, device=0, pipeline="restir")
    r.Initialize(cs)
    r.Update()
    r.Render()
    return r


@pytest.fixture(scope="module")
def table_handle(scene1):
    """A 600x450 handle (the render pass's whole texel window) whose accumulation is the table."""
    from pathtracerdemo_amd import _native as N
    r = make(scene1, 600, 450)
    img = S.present_image(600, 450)
    r.write_buffer(N.PTX_BUF_ACCUM, img)
    np.testing.assert_array_equal(S.bits(r.read_image()), S.bits(img))
    yield r, img
    r.close()


def polled(r):
    got = None
    r.synchronize()
    while got is None:
        got = r.present_poll()
    return got


@pytest.mark.parametrize("bgra", [False, True], ids=["rgba", "bgra"])
@pytest.mark.parametrize("cw,ch", CANVASES)
def test_the_table_is_presented_byte_for_byte(table_handle, oracle_mod, cw, ch, bgra):
    r, img = table_handle
    want = oracle_mod.present(img, cw, ch, bgra)
    got = r.Present(cw, ch, bgra=bgra)
    np.testing.assert_array_equal(got, want, f"{cw}x{ch} bgra={bgra}")
    assert (got[..., 3] == 255).all()
    if (cw, ch) == (300, 225):  # (2 px + 1) * 600 / 2 cw = 2 px + 1: exact for every pixel
        px = np.arange(cw)
        assert (((2 * px + 1) * 600) % (2 * cw) == 0).all()
    if (cw, ch) == (600, 450):  # every texel once, rows flipped: the bytes are the table's, channel by channel
        q = oracle_mod.present(img, cw, ch, False)[::-1, :, :3]
        v = img[..., :3]
        ties = S.present_ties()
        for k in (0, 1, 2, 127, 128, 253, 254):
            at = np.isin(S.bits(v), S.bits(ties[k]))
            assert at.any() and (q[at] == (k if k % 2 == 0 else k + 1)).all(), k
        assert (q[np.isnan(v)] == 0).all() and (q[v == np.inf] == 255).all() and (q[v < 0] == 0).all()
        order = [2, 1, 0] if bgra else [0, 1, 2]
        np.testing.assert_array_equal(got[::-1][..., order], q)


def test_present_async_shows_the_table(table_handle, oracle_mod):
    r, img = table_handle
    r.present_async(300, 225, bgra=True)
    np.testing.assert_array_equal(polled(r), oracle_mod.present(img, 300, 225, True))


def test_a_small_handle_on_the_full_window_reads_zero_outside(scene1, oracle_mod):
    """A 64x48 handle on a 600x450 canvas: texels outside the image read 0.  Then the same table through
    the denoised image: an all-miss G-buffer makes ptx_denoise return its input, alpha 1."""
    from pathtracerdemo_amd import _native as N
    r = make(scene1, 64, 48)
    img = S.present_image(64, 48, seed=1)
    r.write_buffer(N.PTX_BUF_ACCUM, img)
    for bgra in (False, True):
        got = r.Present(600, 450, bgra=bgra)
        np.testing.assert_array_equal(got, oracle_mod.present(img, 600, 450, bgra))
        assert (got[:450 - 48, :, :3] == 0).all() and (got[:, 64:, :3] == 0).all() and (got[450 - 48:, :64, :3] != 0).any()
    r.write_buffer(N.PTX_BUF_GBUFFER, np.zeros((48, 64, 4), np.uint32))
    r.Denoise(iterations=1)
    den = r.read_denoised()
    S.assert_bits(den, img, "the denoised image of an all-miss G-buffer")
    r.set_present_source("denoised")
    for cw, ch, bgra in [(64, 48, False), (600, 450, True), (300, 225, False)]:
        np.testing.assert_array_equal(r.Present(cw, ch, bgra=bgra), oracle_mod.present(den, cw, ch, bgra))
    r.present_async(600, 450)
    np.testing.assert_array_equal(polled(r), oracle_mod.present(den, 600, 450))
    r.close()
