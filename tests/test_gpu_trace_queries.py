"""ptx_trace_queries: chosen rays through the kernel the frames trace with (wave_trace -> trace_queue:
the streamed walk with the instance cull and the cooperative leaves, its any-hit instance, the
global-table fallback, the counting instance), against the CPU oracle bit for bit on all 8 result
words.  ptx_trace runs a kernel of its own (trace_queue_sm); test 6 pins both to one truth.

The ray families are tests/trace_rays.py's: the production walk otherwise only sees the rays that
frames of the test scenes generate, which hold next to no axis-parallel rays on slab planes, rays
through shared edges and vertices, far origins, Visibility queries whose `remain` is a hit's t, or
chains through five panes of glass.  NaN words compare equal when both sides are NaN (the `nonfinite`
family); everything else compares by bits.

`nonfinite` runs on ptx_trace_queries only: trace_stream's and trace_core_tab's loops are bounded by
the tree and the instance list whatever the ray holds (a node is popped once, a root taken once, a
Visibility walk has five segments); ptx_trace's older walk is not given it."""
import numpy as np
import pytest

import trace_rays as TR
from helpers import huge_tables_scene, many_instances_scene, root_chunks_scene, stress_scene, uniform_for

pytestmark = pytest.mark.gpu

W = H = 32
SCENES = ("c1", "c3", "stress", "many", "huge", "chunks")
KEYS = ("rays", "instance_xforms", "aabb_tests", "tri_tests", "hits")


@pytest.fixture(scope="module")
def native():
    from pathtracerdemo_amd import _native
    return _native


class SceneData:
    """A compiled scene, its oracle frame, its world-space triangles, each family's rays and -- per eps
    mode -- the oracle's hits for them; made on first use and then left alone."""

    def __init__(self, cs, oracle_mod):
        self.cs = cs
        self.fr = oracle_mod.Frame(uniform_for(cs, W, H), cs.scene, cs.geometry, cs.accel)
        self.tris = TR.scene_triangles_world(cs)
        self._rays, self._hits = {}, {}

    def rays(self, fam):
        if fam not in self._rays:
            self._rays[fam] = TR.family(fam, self.tris, 64 if fam == "nonfinite" else 256, seed=1)
        return self._rays[fam]

    def hits(self, fam, eps):
        if (fam, eps) not in self._hits:
            self._hits[fam, eps] = self.fr.trace(self.rays(fam), eps)
        return self._hits[fam, eps]

    def window_insts(self):
        """The instances of the mesh most instances share (the PureWindow panes of `many` / `huge`)."""
        mesh = np.array([int(self.cs.scene[33 * i + 32]) for i in range(self.cs.instance_count)])
        return np.nonzero(mesh == np.bincount(mesh).argmax())[0]


@pytest.fixture(scope="module")
def world(scene1, scene3, oracle_mod, tmp_path_factory):
    makers = {"c1": lambda: scene1, "c3": lambda: scene3, "stress": stress_scene, "many": many_instances_scene,
              "huge": huge_tables_scene, "chunks": lambda: root_chunks_scene(tmp_path_factory.mktemp("chunks"))}
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = SceneData(makers[name](), oracle_mod)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def handle(world):
    """32 x 32 renderers per (scene, pipeline, counting), scene uploaded and the oracle frame's uniform set."""
    from pathtracerdemo_amd.renderer import Renderer
    made = {}

    def get(name, pipeline="reuse", count_work=False):
        key = (name, pipeline, count_work)
        if key not in made:
            r = Renderer(W, H, device=0, pipeline=pipeline, count_work=count_work)
            r.Initialize(world(name).cs)
            r.set_uniform(world(name).fr.uniform)
            made[key] = r
        return made[key]
    yield get
    for r in made.values():
        r.close()


def assert_words(got, ref, what):
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    assert got.shape == ref.shape, what
    bad = (got.view(np.uint32) != ref.view(np.uint32)) & ~(np.isnan(got) & np.isnan(ref))
    rows = np.nonzero(bad.reshape(len(bad), -1).any(axis=1))[0]
    assert len(rows) == 0, f"{what}: {len(rows)} of {len(got)} results differ from the oracle, first {rows[:8].tolist()}"


def oracle_results(sc, q, eps):
    """The (n, 8) result array ptx_trace_queries owes for queries `q`: the oracle's hit record for a
    closest query, {Frame.visibility, 0 x 7} for a Visibility or occlusion query."""
    kind = q.view(np.uint32)[:, 7]
    out = np.zeros_like(q)
    c = kind == TR.Q_CLOSEST
    if c.any():
        rays = np.zeros((int(c.sum()), 8), np.float32)
        rays[:, 0:3], rays[:, 3:6] = q[c, 0:3], q[c, 4:7]
        out[c] = sc.fr.trace(rays, eps)
    if (~c).any():
        out[~c, 0] = sc.fr.visibility(q[~c], eps)
    return out


def mixed_queries(sc, eps, fams=("random", "vertex_edge", "on_surface", "axis")):
    """Closest, Visibility and occlusion queries of several families, interleaved query by query."""
    rays = np.concatenate([sc.rays(f) for f in fams])
    hits = np.concatenate([sc.hits(f, eps) for f in fams])
    vis = TR.visibility_set(rays, hits)
    q = np.concatenate([TR.to_queries(rays), vis])
    order = np.arange(len(q)).reshape(2, -1).T.reshape(-1)  # closest, visibility, closest, ...
    return q[order]


# ------------------------------------------------------------------ 1: closest hits, every family
@pytest.mark.parametrize("eps", [0, 1])
@pytest.mark.parametrize("pipeline", ["reuse", "gi"])
@pytest.mark.parametrize("name", SCENES)
def test_closest_families_bit_exact(world, handle, name, pipeline, eps):
    sc, r = world(name), handle(name, pipeline)
    some_hit = False
    for fam in TR.FAMILIES + ("nonfinite",):
        got = r.trace_queries(TR.to_queries(sc.rays(fam)), eps)
        assert_words(got, sc.hits(fam, eps), f"{name} {pipeline} eps {eps} {fam}")
        some_hit |= bool(TR.hit_fields(got)[0].any())
    assert some_hit


def test_root_chunk_scene_reaches_every_chunk(world):
    """The `chunks` scene (helpers.root_chunks_scene: instances of 70, 33 and 70 sub-meshes) is there for
    the walk's root chunks of 32: over the seven finite families the oracle's hits must land in second
    and third chunks and in every instance, or the scene's cases above would pin nothing."""
    sc = world("chunks")
    valid, inst, sub = (np.concatenate(c) for c in zip(*(TR.hit_fields(sc.hits(f, 1))[:3] for f in TR.FAMILIES)))
    assert len(valid) == 1792
    assert (valid & (sub >= 32)).sum() >= 100 and (valid & (sub >= 64)).sum() >= 20
    assert all((valid & (inst == i)).any() for i in range(3))


# ------------------------------------------------------------------ 2: queue-size edges
def test_queue_size_edges(world, handle):
    """One mixed set cut to n queries, calls back to back on one handle, a larger call before each
    smaller one: every result is the first n of the full result (no stale count, no leftover)."""
    sc, r = world("stress"), handle("stress")
    q = mixed_queries(sc, 1)[:1541]
    assert len(q) == 1541
    full = r.trace_queries(q, 1)
    assert_words(full, oracle_results(sc, q, 1), "1541 mixed queries")
    for n in (1, 769, 63, 768, 64, 767, 65, 257, 255, 256, 1541):
        assert_words(r.trace_queries(q[:n], 1), full[:n], f"the first {n} queries")


# ------------------------------------------------------------------ 3: divergence (lane refill)
@pytest.fixture(scope="module")
def deep_and_miss(world):
    """The stress scene's deepest walks (by the oracle's per-ray AABB tests, among the random, far and
    vertex_edge families) and immediate misses (origin outside the scene box, pointing away)."""
    sc = world("stress")
    cand = np.concatenate([sc.rays(f) for f in ("random", "far", "vertex_edge")])
    work = np.array([sc.fr.trace(cand[i:i + 1], 1, return_counters=True)[1]["aabb_tests"] for i in range(len(cand))])
    deep = cand[np.argsort(-work)[:384]]
    lo, hi = TR.scene_box(sc.tris)
    rng = np.random.default_rng(3)
    away = rng.normal(size=(384, 3))
    away /= np.linalg.norm(away, axis=1, keepdims=True)
    miss = np.zeros((384, 8), np.float32)
    miss[:, 0:3] = 0.5 * (lo + hi) + away * np.linalg.norm(hi - lo)
    miss[:, 3:6] = away
    assert not TR.hit_fields(sc.fr.trace(miss, 1))[0].any()
    return deep, miss


@pytest.mark.parametrize("deep_of_64", [1, 32, 33])
def test_divergent_batches(world, handle, deep_and_miss, deep_of_64):
    """Immediate misses interleaved with the deepest walks: 1 in 64, 1 in 2, and 33 of every 64 (which
    crosses PTX_STREAM_REFILL = 32 waiting lanes)."""
    sc, (deep, miss) = world("stress"), deep_and_miss
    n = 1536
    k = np.arange(n) % 64
    is_deep = (k % 2 == 0) if deep_of_64 == 32 else (k < deep_of_64)
    rays = np.where(is_deep[:, None], deep[np.arange(n) % len(deep)], miss[np.arange(n) % len(miss)])
    ref = sc.fr.trace(rays, 1)
    for pipeline in ("reuse", "gi"):
        assert_words(handle("stress", pipeline).trace_queries(TR.to_queries(rays), 1), ref,
                     f"{deep_of_64} deep walks of 64, {pipeline}")


# ------------------------------------------------------------------ 4: Visibility and occlusion
def window_queries(sc):
    """Visibility queries along the window stack, `remain` from 0.3 to 1e10."""
    rays = TR.window_stack_rays(sc.tris, sc.window_insts(), 256, seed=1)
    remain = np.array([1e10, 0.3, 1.0, 2.0, 4.0, 8.0, 3e38], np.float32)[np.arange(len(rays)) % 7]
    return TR.to_queries(rays, remain, TR.Q_VIS)


def chain_ends(sc, q, eps):
    """How each Visibility query's chain ends, walked with the oracle's closest hits: 0 by `remain` (or
    a miss), 1 by an opaque hit, 2 by the fifth segment.  A hit is transmissive when Visibility over
    exactly its t is positive."""
    o, d, remain = q[:, 0:3].copy(), q[:, 4:7], q[:, 3].copy()
    end = np.zeros(len(q), np.int64)
    alive = np.ones(len(q), bool)
    for _ in range(5):
        rays = np.zeros((len(q), 8), np.float32)
        rays[:, 0:3], rays[:, 3:6] = o, d
        hits = sc.fr.trace(rays, eps)
        valid, t = TR.hit_fields(hits)[0], hits[:, 0]
        hit = alive & valid & ~(t > remain)
        clear = sc.fr.visibility(TR.to_queries(rays, t, TR.Q_VIS), eps) > 0
        end[hit & ~clear] = 1
        go = hit & clear
        remain[go] -= t[go]
        o[go] = hits[go, 5:8]
        alive = go
    end[alive] = 2
    return end


@pytest.mark.parametrize("eps", [0, 1])
@pytest.mark.parametrize("name", ["many", "stress", "huge", "chunks"])
def test_visibility_and_occlusion(world, handle, name, eps):
    sc = world(name)
    q = mixed_queries(sc, eps)
    windows = name in ("many", "huge")
    if windows:
        wq = window_queries(sc)
        q = np.concatenate([q, wq])
    ref = oracle_results(sc, q, eps)
    kind = q.view(np.uint32)[:, 7]
    assert (ref[kind != TR.Q_CLOSEST, 0] == 0).sum() >= 64 and (ref[kind != TR.Q_CLOSEST, 0] == 1).sum() >= 64
    if windows:  # (the panes: Visibility walks on through them, an occlusion query stops)
        walked = sc.fr.visibility(wq, eps, return_counters=True)[1]["rays"]
        assert walked >= 2 * len(wq), "the window chains walk several segments each"
    if name == "many":
        end = chain_ends(sc, wq, eps)
        wref = ref[-len(wq):, 0]
        assert (end == 2).sum() >= 4 and not wref[end == 2].any(), "chains that end at the fifth segment give 0"
        assert (end == 1).any() and (end == 0).any()
        assert not wref[end == 1].any()
    occ = q[kind == TR.Q_OCC]
    for pipeline in ("reuse", "gi"):
        r = handle(name, pipeline)
        assert_words(r.trace_queries(q, eps), ref, f"{name} {pipeline} eps {eps}: mixed kinds in one launch")
        assert_words(r.trace_queries(occ, eps, occ_only=True), ref[kind == TR.Q_OCC],
                     f"{name} {pipeline} eps {eps}: occ_only launch")


# ------------------------------------------------------------------ 5: the counting instance
def counting_closest(sc, r):
    for fam in TR.FAMILIES:
        ref, c_or = sc.fr.trace(sc.rays(fam), 1, return_counters=True)
        r.reset_stats()
        got = r.trace_queries(TR.to_queries(sc.rays(fam)), 1)
        assert_words(got, ref, f"counting handle, {fam}")
        c = r.read_counters()
        assert {k: c[k] for k in KEYS} == c_or, fam
        if fam in ("far", "axis", "planar", "on_surface"):
            assert c["cull_misses"] == 0, f"{fam}: {c['cull_misses']} queries would have lost an instance to the cull"


def test_counting_handle_closest(world, handle):
    """count_work=True: the same words, the oracle's traversal work, and an instance cull that would
    not have lost a root on the families that strain it."""
    counting_closest(world("stress"), handle("stress", count_work=True))


def test_counting_handle_closest_root_chunks(world, handle):
    counting_closest(world("chunks"), handle("chunks", count_work=True))


@pytest.mark.parametrize("name", ["many", "stress", "chunks"])
def test_counting_handle_visibility(world, handle, name):
    """Visibility work.  The kernels walk a Visibility segment under a bound just past `remain`
    (vis_bound, ptx_device.h; at most 1e10) where TraceRay's is 1e10: the smaller bound only prunes
    hits the query ignores, so box and triangle
    counts are the oracle's where remain >= 1e10 and stays so along the chain (1e10 - t == 1e10 in
    f32 for the scenes' t): those queries' five counters are compared.  Over the whole Visibility set
    the results, the rays (one per segment walked) and the instance transforms still are the oracle's."""
    sc, r = world(name), handle(name, count_work=True)
    q = mixed_queries(sc, 1)
    q = q[q.view(np.uint32)[:, 7] != TR.Q_CLOSEST]
    if name == "many":
        q = np.concatenate([q, window_queries(sc)])
    far = q[q[:, 3] >= np.float32(1e10)]
    assert len(far) >= 64
    for qs, keys in ((far, KEYS), (q, KEYS[:2])):
        ref, c_or = sc.fr.visibility(qs, 1, return_counters=True)
        r.reset_stats()
        got = r.trace_queries(qs, 1)
        assert_words(got[:, 0], ref, f"counting handle, {name}")
        assert not got[:, 1:].any()
        c = r.read_counters()
        assert {k: c[k] for k in keys} == {k: c_or[k] for k in keys}
        assert c_or["rays"] > len(qs) or name != "many", "no chain walked a second segment"


# ------------------------------------------------------------------ 6: ptx_trace agrees
@pytest.mark.parametrize("name", ["c1", "stress"])
def test_ptx_trace_agrees(world, handle, name):
    sc, r = world(name), handle(name)
    for eps in (0, 1):
        rays = np.concatenate([sc.rays(f) for f in TR.FAMILIES])
        a = r.trace(rays, eps)
        b = r.trace_queries(TR.to_queries(rays), eps)
        assert_words(a, b, f"{name} eps {eps}: ptx_trace against ptx_trace_queries")
        assert_words(a, np.concatenate([sc.hits(f, eps) for f in TR.FAMILIES]), f"{name} eps {eps}: ptx_trace")


# ------------------------------------------------------------------ 7: ptx_trace_device from torch
def test_trace_device_on_torch_stream(world, oracle_mod):
    import torch
    from pathtracerdemo_amd.renderer import Renderer
    sc = world("c1")
    rays = np.concatenate([sc.rays(f) for f in TR.FAMILIES])
    r = Renderer(W, H, device=0, pipeline="restir")
    r.Initialize(sc.cs)
    r.set_uniform(sc.fr.uniform)
    ref = r.trace(rays, 1)
    assert_words(ref, np.concatenate([sc.hits(f, 1) for f in TR.FAMILIES]), "ptx_trace")
    d_rays = torch.from_numpy(rays).cuda()
    d_hits = torch.zeros_like(d_rays)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        r.set_stream(torch.cuda.current_stream().cuda_stream)
        r._call("ptx_trace_device", r._h, d_rays.data_ptr(), d_hits.data_ptr(), len(rays), 1)
    torch.cuda.synchronize()
    assert_words(d_hits.cpu().numpy(), ref, "ptx_trace_device on torch's stream")
    r.set_stream(None)
    fr = oracle_mod.Frame(uniform_for(sc.cs, W, H, 1), sc.cs.scene, sc.cs.geometry, sc.cs.accel)
    fr.run(oracle_mod.PASS_RESTIR, threads=8)
    r.ResetFrameCount()
    r.Update()
    r.Render()
    assert np.array_equal(r.uniform, fr.uniform)
    assert np.array_equal(r.read_image().view(np.uint32), fr.accum.view(np.uint32))
    r.close()


# ------------------------------------------------------------------ 8: refusals
def test_refusals(world, handle, oracle_mod, native):
    """Every refusal is PTX_E_INVALID with a message, before any GPU work; the handle renders a
    bit-exact frame afterwards."""
    from pathtracerdemo_amd.renderer import Renderer
    N, sc = native, world("c3")
    lib = N.load()
    q = TR.to_queries(sc.rays("random"))
    out = np.zeros_like(q)
    bad_kind = q.copy()
    bad_kind.view(np.uint32)[100, 7] = 3
    occ = TR.to_queries(sc.rays("random"), 1.0, TR.Q_OCC)
    occ.view(np.uint32)[17, 7] = TR.Q_VIS

    def refused(r, queries, results, n, eps, occ_only, what):
        rc = lib.ptx_trace_queries(r._h, queries.ctypes.data if queries is not None else None,
                                   results.ctypes.data if results is not None else None, n, eps, occ_only)
        assert rc == N.PTX_E_INVALID, f"{what}: {rc}"
        assert lib.ptx_last_error(r._h), what

    r = Renderer(W, H, device=0, pipeline="reuse")
    refused(r, q, out, len(q), 1, 0, "no scene")
    r.Initialize(sc.cs)
    refused(r, q, out, len(q), 1, 0, "no frame")
    r.set_uniform(sc.fr.uniform)
    refused(r, None, out, len(q), 1, 0, "null queries")
    refused(r, q, None, len(q), 1, 0, "null results")
    refused(r, q, out, len(q), 2, 0, "eps_mode 2")
    refused(r, q, out, len(q), -1, 0, "eps_mode -1")
    refused(r, bad_kind, out, len(q), 1, 0, "kind 3")
    refused(r, q, out, len(q), 1, 1, "occ_only with closest queries")
    refused(r, occ, out, len(q), 1, 1, "occ_only with one Visibility query")
    assert not out.any()
    assert lib.ptx_trace_queries(r._h, None, None, 0, 1, 0) == N.PTX_OK
    for kw in ({"variant": "simple", "pipeline": "restir"}, {"row_census": True, "pipeline": "reuse"}):
        s = Renderer(W, H, device=0, **kw)
        s.Initialize(sc.cs)
        s.set_uniform(sc.fr.uniform)
        refused(s, q, out, len(q), 1, 0, str(kw))
        s.close()
    assert_words(r.trace_queries(q, 1), sc.hits("random", 1), "the handle after the refusals")
    fr = oracle_mod.Frame(uniform_for(sc.cs, W, H, 1), sc.cs.scene, sc.cs.geometry, sc.cs.accel)
    fr.run_reuse_frame(threads=8)
    r.ResetFrameCount()
    r.Update()
    r.Render()
    assert np.array_equal(r.read_history(), fr.res_hist)
    assert np.array_equal(r.read_image().view(np.uint32), fr.accum.view(np.uint32))
    r.close()
