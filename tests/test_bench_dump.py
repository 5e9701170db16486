"""bench.py --dump-outputs (bench.dump_outputs): the byte cap, the seeded pixel sample, the
per-rank file names and the exact uint32 -> float64 conversion.  Pure numpy, no GPU."""
import os

import numpy as np
import pytest

import bench

LIMIT = 64 * 1000 * 1000  # "at most 64 MB in all"


def _sizes(d):
    return {f: os.path.getsize(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("W,H,world", [(1920, 1080, 1), (3840, 2160, 1), (3840, 2160, 8)])
def test_dump_stays_under_64_mb_with_the_right_dtypes(tmp_path, W, H, world):
    rows = H // world
    img = np.zeros((rows, W, 4), np.float32)
    res = np.zeros((rows, W, 32), np.uint32)  # (never touched: the pages stay unmapped)
    for rank in range(world):
        done = bench.dump_outputs(str(tmp_path), {"image": img, "reservoirs": res}, rank, world)
        sfx = f"_rank{rank}" if world > 1 else ""
        assert sorted(done) == [f"image{sfx}.npy", f"reservoirs{sfx}.npy"]
    sizes = _sizes(tmp_path)
    assert len(sizes) == 2 * world and sum(sizes.values()) <= LIMIT
    for f in sizes:
        a = np.load(tmp_path / f, mmap_mode="r")
        assert a.dtype == (np.float32 if f.startswith("image") else np.float64)
        assert a.shape[-1] == (4 if f.startswith("image") else 32)
    if (W, H, world) == (1920, 1080, 1):  # the headline frame's image is written whole
        assert np.load(tmp_path / "image.npy", mmap_mode="r").shape == (1080, 1920, 4)


def test_sample_is_deterministic_sorted_and_made_of_source_pixels(tmp_path):
    H, W = 2160, 3840
    img = np.zeros((H, W, 4), np.float32)
    img[..., 0] = np.arange(H * W, dtype=np.float32).reshape(H, W)  # < 2^24: exact in float32
    img[..., 3] = 1.0
    a = bench.dump_outputs(str(tmp_path / "a"), {"image": img})
    b = bench.dump_outputs(str(tmp_path / "b"), {"image": 2 * img})
    assert a == b == {"image.npy": [bench.DUMP_CAP["image"] // 16, 4]}
    x, y = np.load(tmp_path / "a" / "image.npy"), np.load(tmp_path / "b" / "image.npy")
    idx = x[:, 0].astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < H * W  # distinct pixels, in order
    assert np.array_equal(x, img.reshape(-1, 4)[idx])
    assert np.array_equal(y, 2 * x)  # the same pixels whatever the values: a function of the shape


def test_words_convert_exactly_and_small_outputs_are_whole(tmp_path, monkeypatch):
    rng = np.random.default_rng(1)
    res = rng.integers(0, 2 ** 32, size=(5, 7, 16), dtype=np.uint64).astype(np.uint32)
    res[0, 0, :3] = (0, 0xFFFFFFFF, 0x80000000)
    img = rng.random((5, 7, 4), dtype=np.float32)
    img[1, 1, 0] = np.nan
    bench.dump_outputs(str(tmp_path), {"image": img, "reservoirs": res})
    got = np.load(tmp_path / "reservoirs.npy")
    assert got.dtype == np.float64 and got.shape == res.shape
    assert np.array_equal(got.astype(np.uint32), res) and np.array_equal(got, res.astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "image.npy").view(np.uint32), img.view(np.uint32))
    # over the cap: a sample of whole pixels
    monkeypatch.setitem(bench.DUMP_CAP, "reservoirs", 10 * 16 * 8)
    done = bench.dump_outputs(str(tmp_path / "s"), {"reservoirs": res})
    assert done == {"reservoirs.npy": [10, 16]}
    s = np.load(tmp_path / "s" / "reservoirs.npy").astype(np.uint32)
    flat = res.reshape(-1, 16)
    assert all(any(np.array_equal(row, p) for p in flat) for row in s)
