"""CPU: bench.py --dump-outputs (dump_outputs): the last step's page results as float32 .npy files, their layout, and the seeded
page sample that keeps a large dump under its size cap."""
import numpy as np

import bench
from tuatara_amd.engine import PageResult


def _page(rng, n, texts):
    return PageResult(texts[:n], rng.uniform(0, 768, (n, 4)).astype(np.float32), rng.integers(0, 98, (n, 26)).astype(np.int32))


def _load(d):
    return {k: np.load(d / f"{k}.npy") for k in ("page_seed", "words_per_page", "bbox", "ids", "text")}


def test_dump_layout_round_trips(tmp_path):
    rng = np.random.default_rng(3)
    pages = [_page(rng, 3, ["ab", "", "x" * 26]), _page(rng, 0, []), _page(rng, 2, ["\xe9t\xe9", "Q"])]
    bench.dump_outputs(str(tmp_path), pages, [7, 8, 9])
    a = _load(tmp_path)
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["page_seed"].tolist() == [7, 8, 9] and a["words_per_page"].tolist() == [3, 0, 2]
    assert a["bbox"].shape == (5, 4) and a["ids"].shape == (5, 26) and a["text"].shape == (5, 26)
    assert np.array_equal(a["bbox"], np.concatenate([p.bbox for p in pages]))
    assert np.array_equal(a["ids"], np.concatenate([p.ids for p in pages]).astype(np.float32))
    got = [bytes(int(c) for c in row if c).decode("latin1") for row in a["text"]]
    assert got == ["ab", "", "x" * 26, "\xe9t\xe9", "Q"]


def test_dump_over_the_cap_is_a_fixed_sample_of_whole_pages(tmp_path, monkeypatch):
    rng = np.random.default_rng(4)
    pages = [_page(rng, 40, ["w"] * 40) for _ in range(20)]
    per_page = 2 * 4 + 40 * (4 + 26 + bench.DUMP_TEXT_WIDTH) * 4
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 5 * 128 + 5 * per_page)     # (five .npy headers)
    bench.dump_outputs(str(tmp_path / "a"), pages, list(range(100, 120)))
    bench.dump_outputs(str(tmp_path / "b"), pages, list(range(100, 120)))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert all(np.array_equal(a[k], b[k]) for k in a)
    seeds = a["page_seed"].astype(int).tolist()
    assert len(seeds) == 5 and seeds == sorted(seeds)
    kept = [s - 100 for s in seeds]
    assert np.array_equal(a["bbox"], np.concatenate([pages[i].bbox for i in kept]))
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= bench.DUMP_MAX_BYTES
