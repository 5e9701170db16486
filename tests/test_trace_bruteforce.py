"""The oracle's TraceRay (BVH traversal, f32) against an independent float64 brute force over every
world-space triangle (tests/trace_rays.py), on the ray families that have such a truth -- random,
axis-parallel, planar and tiny-component directions -- on C1, C3, the instance cull's stress scene and
the root-chunk scene (instances of 70 and 33 sub-meshes), under both epsilon sets.  The GPU tests compare the kernels with the oracle bit for bit; this pins
the oracle itself, beyond the 24 camera pixels of test_scene_layout.py.

A ray disagrees when validity, instance, sub-mesh or primitive differ or |t - t64| > 1e-3 max(t64, 1e-3).
At most 2 of 256 may (f32 rounding at a silhouette; the secondary passes' |det| < 1e-4 threshold on a
grazing triangle): measured with seed 1, every (scene, family, eps) has 0 except C1 / axis / eps 1
with 1; worst relative t error among agreeing rays 6.3e-5 (stress / tiny)."""
import numpy as np
import pytest

import trace_rays as TR
from helpers import root_chunks_scene, stress_scene, uniform_for

N_RAYS = 256
MAX_DISAGREE = 2
# How many of a family's rays must hit.  `chunks` (helpers.root_chunks_scene) is three layers of sheets
# facing +z that fill 0.36^2 / 0.4^2 = 0.81 of their layer: of the axis family only the third along
# +-z (85 rays) can meet them at all, and a direction with a zero or tiny component sees them
# edge-on in that plane, so an eighth of the rays is what such a scene can owe.
MIN_HIT = {"chunks": N_RAYS // 8}


@pytest.fixture(scope="module")
def scenes(scene1, scene3, tmp_path_factory):
    return {"c1": scene1, "c3": scene3, "stress": stress_scene(),
            "chunks": root_chunks_scene(tmp_path_factory.mktemp("chunks"))}


@pytest.fixture(scope="module")
def truth(scenes):
    """Per scene: the world-space triangles (made once, shared by the families) and, per family, the
    rays with their brute-force closest hits (made on first use, not changed afterwards)."""
    cache = {}

    def get(which, fam):
        if which not in cache:
            cache[which] = {"tris": TR.scene_triangles_world(scenes[which])}
        c = cache[which]
        if fam not in c:
            rays = TR.family(fam, c["tris"], N_RAYS, seed=1)
            c[fam] = (rays, TR.brute_force(c["tris"], rays))
        return c[fam]
    return get


@pytest.mark.parametrize("eps_mode", [0, 1])
@pytest.mark.parametrize("fam", TR.BRUTE_FAMILIES)
@pytest.mark.parametrize("which", ["c1", "c3", "stress", "chunks"])
def test_oracle_trace_matches_float64_bruteforce(scenes, truth, oracle_mod, which, fam, eps_mode):
    cs = scenes[which]
    rays, bf = truth(which, fam)
    fr = oracle_mod.Frame(uniform_for(cs, 32, 32), cs.scene, cs.geometry, cs.accel)
    hits = fr.trace(rays, eps_mode)
    bad, rel = TR.disagreements(hits, bf)
    print(f"{which} {fam} eps {eps_mode}: {int(bad.sum())} of {len(rays)} disagree, {int(bf[0].sum())} hit, "
          f"worst relative t error {rel:.2e}")
    assert bf[0].sum() >= MIN_HIT.get(which, N_RAYS // 4), "the family must hit the scene"
    assert bad.sum() <= MAX_DISAGREE, f"rays {np.nonzero(bad)[0].tolist()} differ from the float64 brute force"


def test_bruteforce_sees_a_wrong_hit(scenes, truth, oracle_mod):
    """The comparison is not vacuous: hit records moved to another primitive, or with t off by 1 %,
    all disagree."""
    cs = scenes["c1"]
    rays, bf = truth("c1", "random")
    hits = oracle_mod.Frame(uniform_for(cs, 32, 32), cs.scene, cs.geometry, cs.accel).trace(rays, 0)
    valid = TR.hit_fields(hits)[0]
    moved = hits.copy()
    moved.view(np.uint32)[:, 2] += 1
    assert TR.disagreements(moved, bf)[0][valid].all()
    far = hits.copy()
    far[:, 0] *= np.float32(1.01)
    assert TR.disagreements(far, bf)[0][valid].all()
