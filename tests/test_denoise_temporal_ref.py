"""The temporal mode's numpy restatement (tests/denoise_temporal_ref.py) on the CPU: the properties
the definition in include/ptx.h promises (running mean, history at the reprojected pixel, nothing
from other keys, resets), what it buys under a moving camera on oracle frames, the committed golden
sequence, and the C ABI's new surface.  The HIP kernels are compared with the same restatement bit
for bit in tests/test_gpu_denoise_temporal.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import denoise_ref as D
import denoise_temporal_ref as T
from helpers import rel_l2, uniform_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ synthetic guide sets
W0, H0 = 32, 16  # powers of two: pixel centres are exact in NDC


def plane_world(w=W0 + 1, h=H0):
    """A plane z = 0 facing the camera whose points are the pixel centres in NDC (column c at
    x = (2c + 1) / W0 - 1, one column more than the image); key 1 on the left, 2 on the right, a band
    of sky along the top."""
    cs, ys = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    P = np.stack([(cs * 2 + 1) / f32(W0) - 1, (ys * 2 + 1) / f32(H0) - 1, np.zeros_like(cs)], -1).astype(np.float32)
    N = np.broadcast_to(np.array([0, 0, 1], np.float32), P.shape).copy()
    key = np.where(cs < 14, 1, 2).astype(np.uint32)
    key[:2] = D.MISS
    return key, P, N


def window(c0):
    """The guides of a camera that sees world column c0 + x at pixel x."""
    key, P, N = plane_world()
    return D.guides_from_surfaces(key[:, c0:c0 + W0], P[:, c0:c0 + W0], N[:, c0:c0 + W0], (0.0, 0.0, 4.0))


def camera_words(shift):
    """Uniform words of a camera whose VP^-1 is the translation by `shift` pixels along x in NDC:
    its VP takes world column c to pixel c - shift, exactly (every value a power of two)."""
    u = np.zeros(33, np.uint32)
    u[0], u[1] = W0, H0
    m = np.eye(4, dtype=np.float32)
    m[3, 0] = f32(2 * shift) / f32(W0)  # column-major: element 12
    u[4:20] = m.reshape(-1).view(np.uint32)
    u[20:23] = np.array([0, 0, 4], np.float32).view(np.uint32)
    return u


def noise(seed, shape=(H0, W0)):
    img = np.ones(shape + (4,), np.float32)
    img[..., :3] = np.random.default_rng(seed).gamma(0.6, 0.5, shape + (3,)).astype(np.float32)
    return img


def test_mat4_inverse_is_the_oracles(oracle_mod, scene1):
    u = uniform_for(scene1, 96, 72, yaw=7.0, pitch=-3.0)
    m = np.ascontiguousarray(u[4:20]).view(np.float32)
    want = np.zeros(16, np.float32)
    oracle_mod.lib().pto_mat4_inverse(m.ctypes.data, want.ctypes.data)
    np.testing.assert_array_equal(bits(T.mat4_inverse(m)), bits(want))


def test_still_camera_is_the_running_mean():
    """alpha_min below 1/K: C is the sequential mixf running mean of the frame colours bit for bit
    (the accumulation's own arithmetic), n = K."""
    G, u = window(0), camera_words(0)
    t = T.TemporalDenoiser()
    mean = None
    for k in range(1, 9):
        F = noise(k)
        t.denoise(F, F, G, u, alpha_min=1e-6)
        a = f32(1) / f32(k)
        mean = F[..., :3].copy() if mean is None else mean * (f32(1) - a) + F[..., :3] * a
        assert t.same_pixel == (k > 1)
        h = t.history
        np.testing.assert_array_equal(bits(h[G.hit][:, :3]), bits(mean[G.hit]))
        assert (h[G.hit][:, 3] == k).all() and (h[~G.hit][:, 3] == 0).all()
        np.testing.assert_array_equal(bits(h[~G.hit][:, :3]), bits(F[~G.hit][:, :3]))


def shifted_pair(n_prev=1, poke=None):
    """`n_prev` still calls at the camera that sees column x + 1 at pixel x, then one at the camera
    that sees column x there: the history of pixel x is at pixel x - 1."""
    t = T.TemporalDenoiser()
    Gp, up = window(1), camera_words(1)
    for k in range(n_prev):
        Fp = noise(100 + k)
        t.denoise(Fp, Fp, Gp, up)
    if poke:
        poke(t.state)
    prev = (t.state.C.copy(), t.state.n.copy(), t.state.G.key.copy())
    G, u, F = window(0), camera_words(0), noise(200)
    out = t.denoise(F, F, G, u)
    return t, prev, G, F, out


def test_history_is_found_at_the_shifted_pixel():
    def poke(s):
        s.G.key[5, 20] = 1      # another key where (21, 5) looks
        s.G.key[6, 20] = D.MISS  # a miss where (21, 6) looks
        s.n[7, 20] = 0          # an empty history where (21, 7) looks
    t, (Cp, n_p, _), G, F, out = shifted_pair(1, poke)
    assert not t.same_pixel
    # the reprojection is exact: the lookup of pixel x is pixel x - 1 with weight 1
    vp = T.mat4_inverse(camera_words(1)[4:20].view(np.float32))
    cx = ((vp[0] * G.P[..., 0] + vp[4] * G.P[..., 1]) + vp[8] * G.P[..., 2]) + vp[12]
    cw = ((vp[3] * G.P[..., 0] + vp[7] * G.P[..., 1]) + vp[11] * G.P[..., 2]) + vp[15]
    fx = ((cx / cw + f32(1)) * f32(0.5)) * f32(W0) - f32(0.5)
    ax = fx - np.floor(fx)
    assert (cw == 1).all() and (ax == 0).all() and (np.floor(fx) == np.arange(W0, dtype=np.float32) - 1).all()
    h = t.history
    n = h[..., 3]
    a = f32(0.5)
    want = np.zeros((H0, W0, 3), np.float32)
    want[:, 1:] = Cp[:, :-1] * (f32(1) - a) + F[:, 1:, :3] * a
    # outside the image (x = 0), another key, a miss, an empty history: no history, n = 1, C = F
    none = np.zeros((H0, W0), bool)
    none[2:, 0] = True
    none[5:8, 21] = True
    found = G.hit & ~none
    assert G.hit[2:].all() and not G.hit[:2].any() and G.key[5, 21] == 2
    assert (n[found] == 2).all(), np.argwhere(found & (n != 2))[:4]
    np.testing.assert_array_equal(bits(h[..., :3][found]), bits(want[found]))
    assert (n[none] == 1).all(), np.argwhere(none & (n != 1))[:4]
    np.testing.assert_array_equal(bits(h[..., :3][none]), bits(F[..., :3][none]))
    assert (t.taps[found] >= 1).all() and (t.taps[~G.hit] == -1).all()
    # the key boundary moved with the world: column 14 is key 2 and looks at key 2 (column 13 of the previous frame)
    assert G.key[4, 14] == 2 and n[4, 14] == 2
    # every n < 4: the variance is the spatial estimate everywhere, so the output is the spatial
    # filter of the integrated image
    assert n.max() < T.N_MOMENTS
    np.testing.assert_array_equal(bits(out), bits(D.denoise(h, G)))


def test_long_history_takes_its_variance_from_the_moments():
    t, _, G, F, out = shifted_pair(5)
    n = t.history[..., 3]
    assert (n[G.hit] >= T.N_MOMENTS).any() and (n[G.hit] < T.N_MOMENTS).any()
    assert (bits(out) != bits(D.denoise(t.history, G))).any()
    m1, m2 = t.moments
    assert (m2[n >= 4] - m1[n >= 4] * m1[n >= 4] > 0).any()


def test_other_keys_do_not_leak_through_the_history():
    base = shifted_pair(3)
    rng = np.random.default_rng(3)

    def poke(s):
        other = s.G.key == 2
        s.C[other] = rng.uniform(0, 1e6, (int(other.sum()), 3)).astype(np.float32)
        s.m1[other] = 1e6
        s.m2[other] = 1e12
        s.n[other & (np.arange(W0) % 2 == 0)[None, :]] = 0
    moved = shifted_pair(3, poke)
    left = base[2].key == 1
    assert left.any() and (base[2].key == 2).any()
    np.testing.assert_array_equal(bits(moved[0].history[left]), bits(base[0].history[left]))
    np.testing.assert_array_equal(bits(moved[4][left]), bits(base[4][left]))
    assert (bits(moved[4]) != bits(base[4])).any()


def test_resets_and_spatial_calls():
    G, u = window(0), camera_words(0)
    fresh = T.TemporalDenoiser()
    first = fresh.denoise(noise(2), noise(2), G, u)
    t = T.TemporalDenoiser()
    t.denoise(noise(1), noise(1), G, u)
    # a spatial call in between: today's filter, the state untouched
    before = (t.history.copy(), t.moments[0].copy(), t.state.camera.copy())
    spatial = t.denoise(noise(9), noise(9), G, camera_words(1), temporal=False)
    np.testing.assert_array_equal(bits(spatial), bits(D.denoise(noise(9), G)))
    np.testing.assert_array_equal(bits(t.history), bits(before[0]))
    np.testing.assert_array_equal(bits(t.moments[0]), bits(before[1]))
    np.testing.assert_array_equal(t.state.camera, before[2])
    second = t.denoise(noise(2), noise(2), G, u)
    assert (t.history[G.hit][:, 3] == 2).all()
    assert (bits(second) != bits(first)).any()
    # a reset: the next call is a fresh handle's first
    t.reset()
    np.testing.assert_array_equal(bits(t.denoise(noise(2), noise(2), G, u)), bits(first))
    np.testing.assert_array_equal(bits(t.history), bits(fresh.history))


# ------------------------------------------------------------------ what it buys under a moving camera
W, H = 96, 72
YAW_STEP, MOVES = 1.5, 8
#            scene, reuse pipeline, frames of the long accumulation, asserted bound: halfway between the
# measured ratio (C1 0.363, C3 0.622) and 1, so that one frame's noise cannot flip it while a lookup that finds
# nothing (ratio 1) or the wrong pixels (above 1) fails
CASES = [("scene1", False, 512, 0.68), ("scene3", True, 256, 0.81)]


@pytest.fixture(scope="module", params=CASES, ids=["c1_restir", "c3_reuse"])
def moving_camera(request, oracle_mod):
    """Oracle frames at 96x72: the camera yaws by YAW_STEP degrees before each of MOVES frames, the
    frame index restarts every frame (the engine's ResetFrameCount), each frame's colour taken from a
    zeroed accumulation; then the long accumulation at the last camera."""
    scene, reuse, n_long, bound = request.param
    cs = request.getfixturevalue(scene)
    O = oracle_mod
    fr = O.Frame(uniform_for(cs, W, H), cs.scene, cs.geometry, cs.accel)

    def frame(f):
        fr.set_frame_index(f)
        fr.run_reuse_frame(threads=8) if reuse else fr.run(O.PASS_RESTIR, threads=8)

    t = T.TemporalDenoiser()
    out = G = color = None
    for k in range(MOVES):
        fr.set_camera(uniform_for(cs, W, H, yaw=YAW_STEP * (k + 1)))
        fr.accum[...] = 0
        frame(1)
        G = D.guides_from_gbuffer(fr.uniform, cs.scene, cs.geometry, cs.accel, fr.gbuffer)
        # accum = mix(0, c, 1 / 2) where the pixel has a hit, the environment colour elsewhere
        color = np.where(G.hit[..., None], fr.accum * f32(2), fr.accum).astype(np.float32)
        out = t.denoise(color, color, G, fr.uniform)
    spatial = D.denoise(color, G)
    n = t.history[..., 3].copy()
    for f in range(2, n_long + 1):
        frame(f)
    return out, spatial, color, fr.accum.copy(), n, G, bound


def test_temporal_error_is_below_the_spatial_filters(moving_camera):
    """Relative L2 against the long accumulation at the last camera: the temporal result's over the
    spatial-only filter's of the last frame's colour (measured: C1 raw 0.924, spatial 0.403, temporal
    0.146, ratio 0.363; C3 1.061, 0.502, 0.312, ratio 0.622)."""
    out, spatial, color, ref, n, G, bound = moving_camera
    assert G.hit.any() and not G.hit.all()
    assert (n[G.hit] >= MOVES - 1).mean() > 0.5 and (n[G.hit] == 1).any(), "most pixels keep their history, some are disoccluded"
    raw = rel_l2(color[..., :3], ref[..., :3])
    spa = rel_l2(spatial[..., :3], ref[..., :3])
    tem = rel_l2(out[..., :3], ref[..., :3])
    print(f"raw {raw:.4f} spatial {spa:.4f} temporal {tem:.4f} ratio {tem / spa:.3f}")
    assert tem <= bound * spa, (raw, spa, tem, tem / spa)


# ------------------------------------------------------------------ golden
def test_golden_sequence_is_reproduced(scene1):
    """tests/golden/denoise_temporal_c1_48x36.npz (make_denoise_temporal_golden.py): uniform, G-buffer,
    frame colour and accumulation of three consecutive oracle frames under a yawing camera, and the
    history and denoised image after each, reproduced exactly."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "denoise_temporal_c1_48x36.npz"))
    t = T.TemporalDenoiser()
    for k in range(3):
        G = D.guides_from_gbuffer(z["uniform"][k], scene1.scene, scene1.geometry, scene1.accel, z["gbuffer"][k])
        out = t.denoise(z["frame_color"][k], z["accum"][k], G, z["uniform"][k])
        np.testing.assert_array_equal(bits(out), bits(z["denoised"][k]), f"frame {k}")
        np.testing.assert_array_equal(bits(t.history), bits(z["history"][k]), f"frame {k}")
    n = z["history"][2][..., 3]
    assert (n == 3).any() and (n == 1).any() and (n == 0).any()
    assert (z["uniform"][0][4:23] != z["uniform"][1][4:23]).any()


# ------------------------------------------------------------------ the ABI's new surface
def test_header_declares_the_temporal_mode_and_the_binding_mirrors_it():
    import inspect

    from pathtracerdemo_amd import _native as N
    from pathtracerdemo_amd.renderer import Renderer
    txt = open(os.path.join(ROOT, "include", "ptx.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define\s+(PTX_\w+)\s+(\d+)u?\b", txt, re.M)}
    assert defs["PTX_BUF_FRAME_COLOR"] == N.PTX_BUF_FRAME_COLOR == 7
    assert defs["PTX_BUF_DENOISE_HISTORY"] == N.PTX_BUF_DENOISE_HISTORY == 8
    assert defs["PTX_FLAG_FRAME_COLOR"] == N.PTX_FLAG_FRAME_COLOR == 512
    assert defs["PTX_ABI_VERSION"] == N.PTX_ABI_VERSION == 5
    assert ctypes.sizeof(N.PtxDenoiseParams) == 32
    assert [f[0] for f in N.PtxDenoiseParams._fields_] == ["iterations", "sigma_lum", "sigma_plane", "reserved"]
    assert "3 + iterations" in txt
    sig = inspect.signature(Renderer.Denoise).parameters
    assert list(sig)[1:] == ["iterations", "sigma_lum", "sigma_plane", "temporal", "alpha_min"]
    assert sig["temporal"].default is False and sig["alpha_min"].default == 0.0
    assert inspect.signature(Renderer.__init__).parameters["frame_color"].default is False
    assert callable(Renderer.read_frame_color) and callable(Renderer.read_denoise_history)


def test_null_handle_is_refused():
    from pathtracerdemo_amd import _native as N
    lib = N.load()
    p = N.PtxDenoiseParams()
    p.reserved[0] = 1
    assert lib.ptx_denoise(None, ctypes.byref(p)) == -1
    buf = (ctypes.c_float * 4)()
    assert lib.ptx_read_buffer(None, N.PTX_BUF_FRAME_COLOR, buf, 16) == -1
    assert lib.ptx_read_buffer(None, N.PTX_BUF_DENOISE_HISTORY, buf, 16) == -1
