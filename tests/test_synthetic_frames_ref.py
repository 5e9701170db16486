"""tests/synthetic_frames.py and the restatements alone (CPU): that the constructed frames say
something.  A GPU comparison that passes on inputs whose outputs are all NaN, or all unchanged, proves
nothing; so the shares asserted here -- finite, subnormal, changed pixels, upsampling stages, present
ties -- are properties of tests/denoise_ref.py, tests/upsample_ref.py and the helper on scene texels,
at the sizes tests/test_gpu_denoise_synthetic.py and tests/test_gpu_upsample_synthetic.py use."""
import numpy as np
import pytest

import denoise_ref as D
import synthetic_frames as S
import upsample_ref as U
from helpers import uniform_for

W, H = 33, 31
MULTI_KEY = [n for n in S.LAYOUTS if n not in ("one", "all_miss", "miss_checker")]  # a key with at most half the hits


@pytest.fixture(scope="module")
def pool(scene3):
    return S.Pool(scene3)


@pytest.fixture(scope="module")
def guides_of(scene3, pool):
    cache = {}

    def get(name, mode, w=W, h=H):
        if (name, mode, w, h) not in cache:
            m = S.layout(name, w, h)
            cache[name, mode, w, h] = (m, S.guides(scene3, uniform_for(scene3, w, h), pool.texels(m, mode)))
        return cache[name, mode, w, h]
    return get


def test_the_pool_has_more_keys_than_any_layout_needs(pool):
    assert len(pool.keys) > 11 and len(np.unique(pool.keys)) == len(pool.keys)
    assert (pool.keys >> 31 == 0).all()


@pytest.mark.parametrize("mode", ["planar", "scattered"])
@pytest.mark.parametrize("name", S.LAYOUTS)
def test_layouts_give_back_their_keys(pool, guides_of, name, mode):
    m, G = guides_of(name, mode)
    np.testing.assert_array_equal(G.key, pool.want_keys(m))
    assert np.isfinite(G.P).all() and np.isfinite(G.N).all() and np.isfinite(G.r).all()
    if name == "all_miss":
        assert not G.hit.any()
    else:
        assert G.hit.any() and not G.hit.all()
        assert (G.r[G.hit] > 0).all()


def test_layout_geometry():
    m = S.layout("tile_edges", W, H, misses=False)
    assert m[0, 15] == 0 and m[0, 16] == 1 and m[15, 0] == 0 and m[16, 0] == 2 and m[16, 16] == 3
    m = S.layout("tile_edges_15_17", W, H, misses=False)
    assert m[0, 14] == 0 and m[0, 15] == 1 and m[16, 0] == 0 and m[17, 0] == 2
    m = S.layout("islands", W, H)
    for x, y in [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (15, 15), (16, 16), (15, 16), (7, 5), (14, 10)]:
        assert m[y, x] >= 2, (x, y)
    assert (m >= 2).sum() == len(S._islands_at(W, H))
    for s in (1, 2, 4, 8, 16):
        m = S.layout(f"stripes_{s}", 48, 40, misses=False)
        assert m[0, 0] == 0 and m[0, s] == 1 and m[s, 0] == 2 and m[s, s] == 3 and (m[0, 2 * s] == 0 if 2 * s < 48 else True)
    m = S.layout("checker", W, H, misses=False)
    assert m[0, 1] == 1 and m[1, 0] == 1 and m[1, 1] == 0
    for name in S.LAYOUTS:  # seeded
        np.testing.assert_array_equal(S.layout(name, W, H), S.layout(name, W, H))


def test_planar_neighbours_weigh_and_scattered_ones_mostly_do_not(guides_of):
    _, G = guides_of("one", "planar")
    n = S.positive_taps(G)[G.hit]
    print("planar: median positive taps of 25:", np.median(n))
    assert np.median(n) >= 12
    _, G = guides_of("one", "scattered")
    n = S.positive_taps(G)[G.hit]
    print("scattered: median positive taps of 25:", np.median(n), "centre alone:", float((n == 1).mean()))
    assert np.median(n) <= 6 and (n == 1).any()


@pytest.mark.parametrize("name", MULTI_KEY)
def test_nonfinite_stays_inside_one_key(guides_of, name):
    """1, 2 and 6 iterations: at least 40 % of the hit pixels come out finite, at least 16 do not."""
    w, h = (48, 40) if name in ("stripes_8", "stripes_16") else (W, H)
    for mode in ("planar", "scattered"):
        m, G = guides_of(name, mode, w, h)
        img = S.colours("nonfinite", m)
        k = S.nonfinite_key(m)
        bad = ~np.isfinite(img[..., :3]).all(-1)
        assert bad.any() and (m[bad] == k).all() and (m == k).sum() * 2 <= (m >= 0).sum()
        for n in (1, 2, 6):
            share, nonfinite = S.finite_share(D.denoise(img, G, n), G.hit)
            print(f"nonfinite {name} {mode} {w}x{h} n={n}: finite {share:.3f}, not finite {nonfinite}")
            assert share >= 0.40 and nonfinite >= 16, (name, mode, n, share, nonfinite)


@pytest.mark.parametrize("name", ["one", "checker", "tile_edges", "islands"])
def test_denormal_outputs_stay_subnormal(guides_of, name):
    for mode in ("planar", "scattered"):
        m, G = guides_of(name, mode)
        out = D.denoise(S.colours("denormal", m), G, 1)
        share = S.subnormal_share(out)
        print(f"denormal {name} {mode}: subnormal {share:.3f}")
        assert share >= 0.10, (name, mode, share)


@pytest.mark.parametrize("name", [n for n in S.LAYOUTS if n != "all_miss"])
def test_range_changes_and_huge_stays_finite(guides_of, name):
    w, h = (48, 40) if name in ("stripes_8", "stripes_16") else (W, H)
    m, G = guides_of(name, "planar", w, h)
    img = S.colours("range", m)
    for n in (1, 6):
        share = S.changed_share(D.denoise(img, G, n), img, G.hit)
        print(f"range {name} planar {w}x{h} n={n}: changed {share:.3f}")
        # (islands and the miss checkerboard keep their pixels apart: the centre tap alone, c w / w, which
        # still rounds; measured, not asserted, for those two)
        if name not in ("islands", "miss_checker"):
            assert share >= 0.5, (name, n, share)
    img = S.colours("huge", m)
    for n in (1, 6):
        out = D.denoise(img, G, n)
        share = S.changed_share(out, img, G.hit)
        print(f"huge {name} planar {w}x{h} n={n}: changed {share:.3f}, finite {np.isfinite(out).all()}")
        assert share >= 0.10 and np.isfinite(out).all(), (name, n, share)


def test_flat_zero_and_misses(guides_of):
    for name in ("all_miss", "miss_checker", "one"):
        m, G = guides_of(name, "planar")
        img = S.colours("zero", m)
        out = D.denoise(img, G, 3)
        if name == "one":
            continue
        np.testing.assert_array_equal(S.bits(out), S.bits(img))
    m, G = guides_of("all_miss", "planar")
    img = S.colours("range", m)
    np.testing.assert_array_equal(S.bits(D.denoise(img, G, 5)), S.bits(img))
    m, G = guides_of("miss_checker", "planar")  # every hit pixel's same-key taps: the diagonals and distance 2
    img = S.colours("range", m)
    out = D.denoise(img, G, 2)
    np.testing.assert_array_equal(S.bits(out[~G.hit]), S.bits(img[~G.hit]))


def cutoff_pairs(c, v, G, step, sigma_lum=D.DEFAULT_SIGMA_LUM, ulps=4):
    """Pairs (pixel, taken tap) of the iteration at `step` on (c, v) whose (|dl| / dp) / 4 lies within
    `ulps` of 1: (below 1, at or above it)."""
    Hh, Ww = G.key.shape
    with np.errstate(all="ignore"):
        T = D._Taps(Hh, Ww, 2 * step)
        vb = np.zeros((Hh, Ww), np.float32)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                ok = G.hit & (T.at(G.key, dx, dy, fill=D.MISS) == G.key)
                vb = np.where(ok, vb + (D.W3[dy + 1] * D.W3[dx + 1]) * T.at(v, dx, dy), vb)
        dp = np.float32(sigma_lum) * np.sqrt(vb) + np.float32(1e-6)
        lum = D.luminance(c)
        below = above = 0
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ok = G.hit & (T.at(G.key, step * dx, step * dy, fill=D.MISS) == G.key)
                q = (np.abs(lum - T.at(lum, step * dx, step * dy)) / dp) / np.float32(4)
                near = ok & (np.abs(q.view(np.int32).astype(np.int64) - int(np.float32(1).view(np.int32))) <= ulps)
                below += int((near & (q < 1)).sum())
                above += int((near & (q >= 1)).sum())
    return below, above


def test_luminance_lattice_reaches_both_sides_of_the_cutoff(guides_of):
    """lattice_4, planar: at step 4 (iteration 3) there are taken taps whose luminance weight's
    argument is within 4 ulp of the cutoff, on both sides."""
    m, G = guides_of("lattice_4", "planar")
    img = S.colours("luminance_lattice", m)
    c = np.ascontiguousarray(img[..., :3])
    with np.errstate(all="ignore"):
        v = D.variance(c, G)
        for i in range(3):
            if i == 2:
                below, above = cutoff_pairs(c, v, G, 1 << i)
                print(f"luminance_lattice step {1 << i}: pairs within 4 ulp of the cutoff: below {below}, at or above {above}")
                assert below >= 8 and above >= 8, (i, below, above)
            c, v = D.atrous(c, v, G, 1 << i, D.DEFAULT_SIGMA_LUM)
    assert np.isfinite(c).all()


def test_luminance_edge_is_two_flat_halves(guides_of):
    m, G = guides_of("one", "planar")
    img = S.colours("luminance_edge", m)
    assert (img[:, :W // 2, :3] == 0).all() and (img[:, W // 2:, :3] > 0).all()
    assert (np.abs(img[:, W // 2:, :3] / np.float32(4e-6) - 1) < 1e-6).all()
    out = D.denoise(img, G, 2)
    assert np.isfinite(out).all() and S.changed_share(out, img, G.hit) >= 0.10


# ------------------------------------------------------------------ upsampling stages
UPSAMPLE_SIZES = S.UPSAMPLE_SIZES


def upsample_guides(cs, pool, case, s, w, h, mode):
    lo, hi = S.upsample_maps(case, s, w, h)
    u = uniform_for(cs, w, h)
    uh = u.copy()
    uh[0], uh[1] = s * w, s * h
    return lo, hi, S.guides(cs, u, pool.texels(lo, mode)), S.guides(cs, uh, pool.texels(hi, mode, seed=1))


@pytest.mark.parametrize("s,w,h", UPSAMPLE_SIZES)
def test_upsample_cases_force_every_stage_in_bulk(scene3, pool, s, w, h):
    for case, stage_wanted in (("stage1", 1), ("stage2", 2), ("stage3", 3)):
        lo, hi, G_lo, G_hi = upsample_guides(scene3, pool, case, s, w, h, "planar")
        np.testing.assert_array_equal(G_hi.key, pool.want_keys(hi))
        den = D.denoise(S.colours("range", lo), G_lo, 1)
        _, stage = U.upsample(den, G_lo, G_hi, s)
        share = float((stage[G_hi.hit] == stage_wanted).mean())
        print(f"upsample s={s} {w}x{h} {case}: stage {stage_wanted} on {share:.3f} of the hit pixels")
        assert share >= 0.10, (case, s, share)
    # scattered guides: the bilinear weights vanish, so stage 2 is reached through sw == 0 as well
    lo, hi, G_lo, G_hi = upsample_guides(scene3, pool, "stage1", s, w, h, "scattered")
    _, stage = U.upsample(D.denoise(S.colours("range", lo), G_lo, 1), G_lo, G_hi, s)
    share = float((stage[G_hi.hit] == 2).mean())
    print(f"upsample s={s} {w}x{h} stage1 scattered: stage 2 on {share:.3f}")
    assert share >= 0.10
    for case in ("miss_over_misses", "miss_over_hits"):
        lo, hi, G_lo, G_hi = upsample_guides(scene3, pool, case, s, w, h, "planar")
        assert not G_hi.hit.any()
        _, stage = U.upsample(D.denoise(S.colours("range", lo), G_lo, 1), G_lo, G_hi, s)
        assert (stage == (1 if case == "miss_over_misses" else 3)).mean() >= 0.5, (case, np.bincount(stage.ravel()))


@pytest.mark.parametrize("s,w,h", UPSAMPLE_SIZES)
def test_upsampled_nonfinite_stays_inside_one_key(scene3, pool, s, w, h):
    for case in ("stage1", "stage2", "stage3"):
        lo, hi, G_lo, G_hi = upsample_guides(scene3, pool, case, s, w, h, "planar")
        den = D.denoise(S.colours("nonfinite", lo), G_lo, 1)
        out, _ = U.upsample(den, G_lo, G_hi, s)
        share, nonfinite = S.finite_share(out, G_hi.hit)
        print(f"upsample nonfinite s={s} {w}x{h} {case}: finite {share:.3f}, not finite {nonfinite}")
        assert share >= 0.40 and nonfinite >= 16, (case, s, share, nonfinite)


@pytest.mark.parametrize("w,h", [(12, 9), (17, 11)])
def test_upsampled_denormals_stay_subnormal(scene3, pool, w, h):
    for case in ("stage1", "stage2", "stage3", "miss_over_misses"):
        lo, hi, G_lo, G_hi = upsample_guides(scene3, pool, case, 2, w, h, "planar")
        out, _ = U.upsample(D.denoise(S.colours("denormal", lo), G_lo, 1), G_lo, G_hi, 2)
        share = S.subnormal_share(out)
        print(f"upsample denormal {w}x{h} {case}: subnormal {share:.3f}")
        assert share >= 0.10


def test_upsample_bands_case_sees_stages_1_and_2_at_the_cut(scene3, pool):
    s, w, h, cut = 3, 17, 12, 6
    for mode in ("planar", "scattered"):
        lo, hi = S.layout(f"borders_8_{cut}", w, h), S.layout(f"borders_{s * 8}_{s * cut}", s * w, s * h)
        u = uniform_for(scene3, w, h)
        uh = u.copy()
        uh[0], uh[1] = s * w, s * h
        G_lo, G_hi = S.guides(scene3, u, pool.texels(lo, mode)), S.guides(scene3, uh, pool.texels(hi, mode, seed=1))
        _, stage = U.upsample(D.denoise(S.colours("range", lo), G_lo, 1), G_lo, G_hi, s)
        print(f"upsample bands {mode}: stages in the 4 rows around the cut", np.bincount(stage[s * cut - 2:s * cut + 2].ravel(), minlength=4)[1:])
        assert all((stage[s * cut - 2:s * cut + 2] == k).any() for k in (1, 2))


# ------------------------------------------------------------------ the band cases
@pytest.mark.parametrize("case", list(S.BAND_CASES))
def test_band_cases(scene3, pool, case):
    name, lkw, family, ckw = S.BAND_CASES[case]
    m = S.layout(name, S.BAND_W, S.BAND_H, **lkw)
    if case == "borders_on_the_cuts":
        full = S.layout(name, S.BAND_W, S.BAND_H, misses=False)
        for cut in S.BAND_CUTS:
            assert (full[cut - 1] != full[cut]).all() and (full[cut - 2] == full[cut - 1]).all() and (full[cut] == full[cut + 1]).all()
    for y in lkw.get("island_rows", []):
        assert (m[y] >= 2).sum() >= 6
    img = S.colours(family, m, **ckw)
    if family == "nonfinite":
        bad = ~np.isfinite(img[..., :3]).all(-1)
        assert bad.any() and not bad[[r for r in range(S.BAND_H) if r not in ckw["only_rows"]]].any()
    for mode in ("planar", "scattered"):
        G = S.guides(scene3, uniform_for(scene3, S.BAND_W, S.BAND_H), pool.texels(m, mode))
        for n in (1, 2, 3):
            out = D.denoise(img, G, n)
            share, nonfinite = S.finite_share(out, G.hit)
            print(f"bands {case} {mode} n={n}: finite {share:.3f} ({nonfinite} not), changed {S.changed_share(out, img, G.hit):.3f}")
            if family == "nonfinite":
                assert share >= 0.40 and nonfinite >= 16
            else:
                assert nonfinite == 0 and S.changed_share(out, img, G.hit) >= 0.10


# ------------------------------------------------------------------ the present table
def test_present_table_meets_the_ties(oracle_mod):
    ties = S.present_ties()
    print("ties met exactly in f32:", len(ties), "of 256")
    assert len(ties) >= 200
    for k, xs in ties.items():
        assert (xs * np.float32(255.0) == np.float32(k + 0.5)).all()
    down = [k for k in ties if k % 2 == 0 and k < 255]  # k + 0.5 -> k
    up = [k for k in ties if k % 2 == 1 and k < 255]    # k + 0.5 -> k + 1
    assert len(down) >= 50 and len(up) >= 50
    # and the restatement rounds them to even
    for k in down[:3] + up[:3]:
        img = np.ones((1, 1, 4), np.float32)
        img[0, 0, :3] = ties[k][0]
        got = oracle_mod.present(img, 1, 1)
        # (canvas 1x1 reads texel (300, 225): outside a 1x1 image; read it through a 600x450 one)
        big = np.ones((450, 600, 4), np.float32)
        big[225, 300, :3] = ties[k][0]
        got = oracle_mod.present(big, 1, 1)
        assert got[0, 0, 0] == (k if k % 2 == 0 else k + 1), (k, got[0, 0])
    v = S.present_values()
    assert np.isnan(v).sum() == 4 and np.isinf(v).sum() == 2 and (v < 0).sum() >= 3
    assert np.signbit(v[v == 0]).any() and not np.signbit(v[v == 0]).all()
    tiny = np.finfo(np.float32).tiny
    assert ((np.abs(v) > 0) & (np.abs(v) < tiny)).sum() >= 3
    img = S.present_image(64, 48)
    assert (img[..., 3] == 1).all()
    for c in range(3):  # the whole table in every channel, dealt independently
        assert set(S.bits(v).tolist()) <= set(S.bits(img[..., c]).ravel().tolist())
    assert (S.bits(img[..., 0]) != S.bits(img[..., 1])).any() and (S.bits(img[..., 1]) != S.bits(img[..., 2])).any()
