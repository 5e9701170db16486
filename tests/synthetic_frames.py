"""Constructed G-buffers and images for the image kernels (denoise, upsample, present): key borders put
on the filters' tile and tap geometry, colours away from 1.0, and unorm8's ties and ends.  Rendered
frames give none of these.  Importable without a GPU, seeded throughout.

A texel is {0x80000000 | inst << 16 | sub, prim, bits(u), bits(v)}, a miss all zero: what
denoise_ref.guides_from_gbuffer decodes and dn_guide reads.  Every texel names a triangle that
trace_rays.scene_triangles_world lists, with finite barycentrics u, v >= 0, u + v <= 1: a texel
outside the scene's tables would make the guide pass read outside them, and nothing here writes one.

Geometry modes of a key (instance | sub-mesh):
  planar     every pixel of the key is a point of the sub-mesh's largest triangle, its barycentrics an
             affine function of the pixel's position in the image (of (x + 0.5) / W, (y + 0.5) / H, so
             that images of several sizes show the same points): neighbours weigh > 0, the filter mixes
  scattered  every pixel takes a random triangle of the sub-mesh and random barycentrics: normals
             oppose, points leave the plane, most taps weigh 0

Layouts are maps of key indices into Pool.keys, -1 a miss (LAYOUTS; layout()): one, checker, stripes_s
(four keys, ((x // s) & 1) + 2 ((y // s) & 1)), tile_edges (borders at x = 16, y = 16; _15_17 a pixel to
either side; borders_X_Y anywhere), islands (one-pixel keys on two half-image backgrounds), lattice_4
(a key that meets itself only at steps 4 and 8), all_miss, miss_checker.  Colour families (FAMILIES;
colours()): range, huge, denormal, nonfinite, flat, zero, luminance_edge, luminance_lattice.
assert_bits compares words as uint32; a word is equal when both sides are NaN and for no other reason
(the GPU's default NaN and numpy's differ in sign and payload: tests/test_gpu_trace_queries.py's rule).
"""
from __future__ import annotations

import numpy as np

import denoise_ref as D
from trace_rays import scene_triangles_world

f32 = np.float32
LAYOUTS = ("one", "checker", "stripes_1", "stripes_2", "stripes_4", "stripes_8", "stripes_16", "tile_edges",
           "tile_edges_15_17", "islands", "lattice_4", "all_miss", "miss_checker")
FAMILIES = ("range", "huge", "denormal", "nonfinite", "flat", "zero", "luminance_edge", "luminance_lattice")
FLAT = (0.31, 0.62, 0.17)
N_ISLAND_KEYS = 6  # islands cycle over keys 2 .. 7; keys 0 and 1 are the background's halves


# ------------------------------------------------------------------ texel pools
class Pool:
    """The keys of a compiled scene with their triangles: sub-meshes whose faces oppose first, then the
    flat ones, each group by its largest triangle."""

    def __init__(self, cs, min_keys=2 + N_ISLAND_KEYS):
        t = scene_triangles_world(cs)
        key = (t["inst"].astype(np.int64) << 16) | t["sub"].astype(np.int64)
        P = t["P"]
        cr = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
        area = 0.5 * np.linalg.norm(cr, axis=1)
        ok = np.isfinite(area) & (area > 0)
        groups = []
        for k in np.unique(key[ok]):
            idx = np.nonzero(ok & (key == k))[0]
            best = idx[np.argmax(area[idx])]
            # a sub-mesh whose area-weighted mean normal is short has faces that oppose: those come
            # first, so that the few keys most layouts use are not flat in scattered mode
            flat = np.linalg.norm(cr[idx].sum(axis=0)) > area[idx].sum()
            groups.append((bool(flat), -float(area[best]), int(k), idx, int(best)))
        groups.sort(key=lambda g: g[:3])
        assert len(groups) >= min_keys, f"the scene has {len(groups)} keys"
        self.keys = np.array([g[2] for g in groups], np.uint32)
        self.prims = [t["prim"][g[3]].astype(np.uint32) for g in groups]  # every triangle of the key
        self.best = np.array([t["prim"][g[4]] for g in groups], np.uint32)  # its largest

    def texels(self, layout, mode="planar", seed=0, size=None, origin=(0, 0)):
        """(H, W, 4) u32 texels of a key-index map.  `size` (W, H) and `origin` (x, y): the map is a
        window of an image of that size (a band), positioned as the whole image's pixels are."""
        layout = np.asarray(layout)
        H, W = layout.shape
        FW, FH = size or (W, H)
        out = np.zeros((H, W, 4), np.uint32)
        hit = layout >= 0
        k = np.where(hit, layout, 0)
        out[..., 0] = np.where(hit, np.uint32(0x80000000) | self.keys[k], 0)
        if mode == "planar":
            xs = (np.arange(W) + origin[0] + 0.5) / FW
            ys = (np.arange(H) + origin[1] + 0.5) / FH
            u = np.broadcast_to((0.05 + 0.4 * xs)[None, :], (H, W)).astype(np.float32)
            v = np.broadcast_to((0.05 + 0.4 * ys)[:, None], (H, W)).astype(np.float32)
            prim = self.best[k]
        else:
            assert mode == "scattered"
            rng = np.random.default_rng([seed, FW, FH])
            pick, a, b = rng.random((3, FH, FW))  # drawn for the whole image: a band sees its rows of it
            sl = (slice(origin[1], origin[1] + H), slice(origin[0], origin[0] + W))
            pick, a, b = pick[sl], a[sl], b[sl]
            fold = a + b > 1
            u = (np.where(fold, 1 - a, a) * 0.98).astype(np.float32)
            v = (np.where(fold, 1 - b, b) * 0.98).astype(np.float32)
            prim = np.zeros((H, W), np.uint32)
            for i in np.unique(k[hit]):
                m = hit & (k == i)
                prim[m] = self.prims[i][(pick[m] * len(self.prims[i])).astype(np.int64)]
        assert np.isfinite(u).all() and (u >= 0).all() and (v >= 0).all() and (u + v <= 1).all()
        out[..., 1] = np.where(hit, prim, 0)
        out[..., 2] = np.where(hit, u.view(np.uint32), 0)
        out[..., 3] = np.where(hit, v.view(np.uint32), 0)
        return out

    def want_keys(self, layout):
        """The guide keys a key-index map stands for."""
        layout = np.asarray(layout)
        return np.where(layout >= 0, self.keys[np.where(layout >= 0, layout, 0)], D.MISS).astype(np.uint32)


# ------------------------------------------------------------------ key layouts
def _islands_at(W, H):
    """(x, y) of the one-pixel keys: every 5 rows and 7 columns, the image's corners, a tile's corner."""
    at = [(x, y) for y in range(0, H, 5) for x in range(0, W, 7)]
    at += [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (15, 15), (16, 16), (15, 16)]
    seen, out = set(), []
    for p in at:
        if p not in seen and p[0] < W and p[1] < H:
            seen.add(p)
            out.append(p)
    return out


def layout(name, W, H, seed=0, misses=True, island_rows=None):
    """(H, W) key-index map of a named layout, -1 = miss.  Every layout but all_miss / miss_checker
    gets max(1, W H / 64) seeded miss pixels (never on an island).  island_rows: further rows of
    `islands` with an island every 7 columns (the first and last row of a band)."""
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    keep = np.zeros((H, W), bool)
    if name == "one":
        m = np.zeros((H, W), np.int64)
    elif name == "checker":
        m = (xs + ys) & 1
    elif name.startswith("stripes_"):
        s = int(name.split("_")[1])
        m = ((xs // s) & 1) + 2 * ((ys // s) & 1)
    elif name in ("tile_edges", "tile_edges_15_17") or name.startswith("borders_"):
        # (borders_X_Y: tile_edges with its borders at x = X and y = Y, for a band cut or another scale)
        bx, by = (16, 16) if name == "tile_edges" else (15, 17) if name == "tile_edges_15_17" else map(int, name.split("_")[1:])
        m = (xs >= bx) + 2 * (ys >= by)
    elif name == "islands":
        m = (xs >= W // 2).astype(np.int64)  # two halves, so that no key holds more than half the pixels
        at = _islands_at(W, H) + [(x, y) for y in (island_rows or []) for x in range(3, W, 7)]
        for n, (x, y) in enumerate(at):
            m[y, x] = 2 + n % N_ISLAND_KEYS
            keep[y, x] = True
    elif name == "lattice_4":
        # key 0 on every fourth pixel of every fourth row, two other keys in between: a key-0 pixel is
        # alone in its 3x3 and 7x7 windows and at steps 1 and 2, and meets its like at steps 4 and 8
        m = np.where((xs % 4 == 0) & (ys % 4 == 0), 0, 1 + ((xs + ys) & 1))
        keep = m == 0
    elif name == "all_miss":
        return np.full((H, W), -1, np.int64)
    elif name == "miss_checker":
        return np.where((xs + ys) & 1, -1, 0).astype(np.int64)
    else:
        raise ValueError(name)
    m = m.astype(np.int64)
    if misses:
        rng = np.random.default_rng([seed, W, H, 77])
        free = np.nonzero(~keep.ravel())[0]
        m.ravel()[rng.choice(free, max(1, W * H // 64), replace=False)] = -1
    return m


def outer_ring(lo, s):
    """A full-size map over small map `lo` at scale s for the upsampler's stage 2: each pixel takes the
    least key that its 4x4 candidates (x0 - 1 .. x0 + 2)^2 hold and its 2x2 bilinear candidates
    (x0 .. x0 + 1)^2 lack; where there is none, the key of small pixel (x / s, y / s)."""
    import upsample_ref as U
    h, w = lo.shape
    H, W = s * h, s * w
    x0, y0 = U.positions(W, s)[0], U.positions(H, s)[0]
    out = np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            def keys(a, b):
                ys, xs = range(max(y0[y] + a, 0), min(y0[y] + b, h)), range(max(x0[x] + a, 0), min(x0[x] + b, w))
                return {int(lo[j, i]) for j in ys for i in xs} - {-1}
            ring = sorted(keys(-1, 3) - keys(0, 2))
            out[y, x] = ring[0] if ring else lo[y // s, x // s]
    return out


def upsample_maps(case, s, w, h):
    """(small key map, full-size key map) of a case of the upsampling tests."""
    Wf, Hf = s * w, s * h
    if case == "stage1":  # the same layout at both sizes
        return layout("stripes_2", w, h), layout(f"stripes_{2 * s}", Wf, Hf)
    if case == "stage2":  # full-size keys that only the outer ring of the 4x4 candidates holds
        lo = layout("stripes_2", w, h, misses=False)
        hi = outer_ring(lo, s)
        hi[0, :3] = -1
        return lo, hi
    if case == "stage3":  # full-size keys absent from the small image
        return layout("checker", w, h), np.where(layout("stripes_4", Wf, Hf) >= 0, layout("stripes_4", Wf, Hf) + 4, -1)
    if case == "miss_over_misses":
        return layout("miss_checker", w, h), np.full((Hf, Wf), -1, np.int64)
    if case == "miss_over_hits":
        return layout("checker", w, h, misses=False), np.full((Hf, Wf), -1, np.int64)
    raise ValueError(case)


UPSAMPLE_CASES = ("stage1", "stage2", "stage3", "miss_over_misses", "miss_over_hits")
UPSAMPLE_SIZES = [(2, 12, 9), (3, 12, 9), (4, 12, 9), (2, 17, 11), (3, 17, 11), (4, 17, 11)]  # (s, w, h)

# ptx_denoise_bands: 48x72 cut at rows 24 and 48 (24 rows per band allow 1, 2 and 3 iterations: halos of
# 4, 8 and 16 rows).  case: (layout, its arguments, colour family, its arguments)
BAND_W, BAND_H, BAND_CUTS = 48, 72, [24, 48]
BAND_CASES = {
    "borders_on_the_cuts": ("stripes_24", {}, "range", {}),  # (stripes of 24 rows: a key border on both cuts)
    "border_above_cut_1": ("borders_16_23", {}, "range", {}),
    "border_below_cut_1": ("borders_16_25", {}, "range", {}),
    "border_above_cut_2": ("borders_16_47", {}, "range", {}),
    "border_below_cut_2": ("borders_16_49", {}, "range", {}),
    "islands_in_the_bands_edge_rows": ("islands", dict(island_rows=[0, 23, 24, 47, 48, 71]), "range", {}),
    "nonfinite_next_to_the_cuts": ("stripes_24", {}, "nonfinite", dict(only_rows=[22, 23, 24, 25, 46, 47, 48, 49])),
    "huge": ("stripes_24", {}, "huge", {}),
}


# ------------------------------------------------------------------ colour families
def nonfinite_key(m):
    """The key index the non-finite colours go to: the most frequent one among those that hold at
    most half the hit pixels (keys do not leak, so the rest of the image stays finite); None if there
    is none (a single key)."""
    ks, n = np.unique(m[m >= 0], return_counts=True)
    ok = n * 2 <= n.sum()
    return int(ks[ok][np.argmax(n[ok])]) if ok.any() else None


def colours(family, m, seed=0, only_rows=None):
    """(H, W, 4) f32 image of a family over key-index map `m`, alpha 1.  only_rows (nonfinite): the
    non-finite pixels are drawn among these rows alone."""
    m = np.asarray(m)
    H, W = m.shape
    rng = np.random.default_rng([seed, W, H, FAMILIES.index(family)])
    img = np.ones((H, W, 4), np.float32)
    if family == "range":
        rgb = 10.0 ** rng.uniform(-6, 6, (H, W, 3))
    elif family == "huge":
        rgb = 10.0 ** rng.uniform(-3, np.log10(3e38), (H, W, 3))
    elif family == "denormal":
        rgb = 10.0 ** rng.uniform(-45, -36, (H, W, 3))
        rgb[rng.random((H, W)) < 0.2] = 0
    elif family == "nonfinite":
        rgb = rng.gamma(0.6, 0.5, (H, W, 3))
        k = nonfinite_key(m)
        if k is None:
            raise ValueError("nonfinite needs a key that holds at most half the hit pixels")
        rows = np.zeros((H, W), bool)
        rows[list(range(H)) if only_rows is None else list(only_rows)] = True
        cand = np.nonzero(((m == k) & rows).ravel())[0]
        bad = rng.choice(cand, -(-len(cand) // (16 if only_rows is None else 4)), replace=False)
        vals = np.array([np.nan, np.inf, -np.inf, -1.0])
        flat = rgb.reshape(-1, 3)
        flat[bad, rng.integers(0, 3, len(bad))] = vals[np.arange(len(bad)) % 4]
    elif family == "flat":
        rgb = np.broadcast_to(np.array(FLAT), (H, W, 3))
    elif family == "zero":
        rgb = np.zeros((H, W, 3))
    elif family == "luminance_edge":
        # Two flat halves, grey: 0 on the left, on the right d = 4e-6 (1 + k 2^-22), k = -3 .. 3 by row.
        # The luminance weight's t = 1 - (|dl| / dp) / 4 has dp = sigma_lum sqrt(blurred variance) + 1e-6,
        # and 4e-6 is the cutoff t = 0 at dp's floor.  Inside one key a pixel that has a tap across the
        # edge also has it in its variance window, so dp is above the floor there and t > 0 by a little:
        # these halves test differences of a few 1e-6 against dp; luminance_lattice reaches the cutoff.
        d = (f32(4e-6) * (f32(1) + (np.arange(H) % 7 - 3).astype(np.float32) * f32(2.0 ** -22))).astype(np.float32)
        rgb = np.zeros((H, W, 3), np.float32)
        rgb[:, W // 2:] = d[:, None, None]
    elif family == "luminance_lattice":
        # For lattice_4: 4x4 blocks alternately 0 and grey d = 4e-6 (1 + k 2^-22), k = -3 .. 3 by block.
        # A key-0 pixel with colour 0 keeps variance 0 and colour 0 through steps 1 and 2 (its centre tap
        # alone), so at step 4 its dp is 1e-6f exactly and its four nearest taps are grey: (|dl| / dp) / 4
        # lies within a few ulp of 1, on either side.
        bx, by = np.meshgrid(np.arange(W) // 4, np.arange(H) // 4)
        d = f32(4e-6) * (f32(1) + ((bx + 3 * by) % 7 - 3).astype(np.float32) * f32(2.0 ** -22))
        rgb = np.where(((bx + by) & 1)[..., None] == 1, d[..., None], f32(0)) * np.ones(3, np.float32)
    else:
        raise ValueError(family)
    with np.errstate(over="ignore", under="ignore"):
        img[..., :3] = np.asarray(rgb).astype(np.float32)
    return img


# ------------------------------------------------------------------ guides and comparison
def guides(cs, uniform, texels, sigma_plane=D.DEFAULT_SIGMA_PLANE):
    return D.guides_from_gbuffer(uniform, cs.scene, cs.geometry, cs.accel, texels, sigma_plane)


def with_sigma(G, uniform, sigma_plane):
    """The same guides under another sigma_plane or camera position (r is the only field they enter)."""
    cam = np.asarray(uniform, np.uint32)[20:23].view(np.float32)
    out = D.guides_from_surfaces(G.key, G.P, G.N, cam, sigma_plane)
    out.r[G.key == D.MISS] = 0
    return out


def positive_taps(G, reach=2):
    """Per pixel: the number of taps of the (2 reach + 1)^2 window with its key and a guide weight > 0."""
    H, W = G.key.shape
    T = D._Taps(H, W, reach)
    n = np.zeros((H, W), np.int64)
    with np.errstate(all="ignore"):
        for dy in range(-reach, reach + 1):
            for dx in range(-reach, reach + 1):
                ok, gm = D._gamma(G, T, dx, dy)
                n += ok & (gm > 0)
    return n


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_bits(got, want, what=""):
    """Equal word for word as uint32; a word also counts as equal when both sides are NaN."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, f"{what}: shapes {got.shape} and {want.shape}"
    bad = (bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))
    if bad.any():
        px = np.argwhere(bad.any(-1))
        y, x = px[0]
        raise AssertionError(f"{what}: {len(px)} pixels differ, first at {px[:4].tolist()}: got {got[y, x].tolist()} "
                             f"({[hex(w) for w in bits(got)[y, x]]}), want {want[y, x].tolist()} ({[hex(w) for w in bits(want)[y, x]]})")


def finite_share(out, hit):
    """(share of the hit pixels finite in all three channels, number that are not)."""
    fin = np.isfinite(out[..., :3]).all(-1)[hit]
    return float(fin.mean()), int((~fin).sum())


def subnormal_share(out):
    """Share of the pixels with a subnormal (non-zero, below the least normal f32) channel."""
    a = np.abs(out[..., :3])
    return float(((a > 0) & (a < np.finfo(np.float32).tiny)).any(-1).mean())


def changed_share(out, img, hit):
    return float((bits(out[..., :3]) != bits(img[..., :3])).any(-1)[hit].mean())


# ------------------------------------------------------------------ the present table
def _step(x, n):
    """The f32 n steps above (below, n < 0) positive f32 x."""
    return (np.asarray(x, np.float32).view(np.int32) + np.int32(n)).view(np.float32)


def present_ties():
    """{k: the f32 x with f32(x * 255) == k + 0.5 exactly}, searched among the f32 values around (k + 0.5) / 255."""
    out = {}
    for k in range(256):
        x0 = f32((k + 0.5) / 255.0)
        cand = _step(np.full(33, x0, np.float32), np.arange(-16, 17))
        hit = cand[cand * f32(255.0) == f32(k + 0.5)]
        if len(hit):
            out[k] = hit
    return out


def present_values():
    """The value table of the present tests: for every k in 0 .. 255, k / 255, the f32 nearest
    (k + 0.5) / 255 with two f32 neighbours on each side, and every x whose x * 255 is exactly k + 0.5;
    the ends, values outside [0, 1] and the non-finite ones."""
    ties = present_ties()
    vals = []
    for k in range(256):
        x0 = f32((k + 0.5) / 255.0)
        vals += [f32(k / 255.0)] + list(_step(np.full(5, x0, np.float32), np.arange(-2, 3))) + list(ties.get(k, []))
    one = f32(1)
    vals += [f32(0.0), f32(-0.0), f32(1e-45), f32(1e-40), _step(one, -1), one, _step(one, 1), f32(2), f32(3e38),
             f32(-1e-45), f32(-1), f32(np.inf), f32(-np.inf)]
    v = np.array(vals, np.float32)
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001], np.uint32).view(np.float32)
    return np.concatenate([v, nans])


def present_image(W, H, seed=0):
    """(H, W, 4) f32: the table dealt over r, g and b independently (each a seeded permutation of it,
    repeated over the image), alpha 1."""
    v = present_values()
    rng = np.random.default_rng([seed, W, H])
    img = np.ones((H, W, 4), np.float32)
    n = W * H
    for c in range(3):
        reps = -(-n // len(v))
        col = np.concatenate([v[rng.permutation(len(v))] for _ in range(reps)])[:n]
        img.reshape(-1, 4)[:, c] = col
    return img
