"""bench.py's host-side helpers (no GPU): which PMC file `roofline.traffic` is taken from, and when it is withheld."""
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("cimg_bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_traffic_comes_from_the_newest_round_whose_sources_match(tmp_path, monkeypatch):
    b = _bench()
    h = b.kernel_source_hash()
    assert len(h) == 16 and h == b.kernel_source_hash()
    prof = tmp_path / "profiles"
    for rnd, sh, fetch in (("r03", h, 100), ("r07", "0" * 16, 200), ("r05", h, 300)):
        (prof / rnd).mkdir(parents=True)
        (prof / rnd / "pmc_per_launch.json").write_text(json.dumps(
            {"_source_hash": sh, "cimg_encode_streams": {"FETCH_SIZE": fetch, "WRITE_SIZE": 50}}))
    monkeypatch.setattr(b, "ROOT", str(tmp_path))
    monkeypatch.setattr(b, "kernel_source_hash", lambda: h)
    # the newest directory (r07) is from other sources: nothing is reported, and the reason is
    t, why = b.pmc_traffic("cimg_encode_streams")
    assert t is None and "other kernel sources" in why and "r07" in why
    (prof / "r07" / "pmc_per_launch.json").unlink()
    t, why = b.pmc_traffic("cimg_encode_streams")
    assert t == (300 * b.FETCH_FACTOR + 50) * 1024 and "r05" in why        # FETCH_SIZE doubled (the gfx950 rule), KiB -> bytes
    # an explicit file is taken as given
    t, _ = b.pmc_traffic("cimg_encode_streams", str(prof / "r03" / "pmc_per_launch.json"))
    assert t == (100 * b.FETCH_FACTOR + 50) * 1024


def test_committed_counters_name_their_sources():
    """profiles/rNN/pmc_per_launch.json carries the hash of the kernel sources it was collected on (bench.py reports the traffic
    only on a match -- a mismatch is a null in the line, never a stale number)."""
    prof = os.path.join(ROOT, "profiles")
    rounds = sorted(r for r in os.listdir(prof) if r[:1] == "r" and r[1:].isdigit())
    newest = os.path.join(prof, rounds[-1], "pmc_per_launch.json")
    with open(newest) as f:
        table = json.load(f)
    assert isinstance(table.get("_source_hash"), str) and len(table["_source_hash"]) >= 16
    assert "FETCH_SIZE" in table["cimg_encode_streams"] and "WRITE_SIZE" in table["cimg_decode_lean"]


def test_dump_outputs_writes_what_the_step_returned(tmp_path):
    """--dump-outputs: float32 / float64 arrays only, CRC-32 over every chunk, the sampled bytes and pixels at positions that
    depend on the geometry alone (two builds compare position by position), -1 past the end of a compressed chunk."""
    import zlib

    import numpy as np
    b = _bench()
    rng = np.random.default_rng(5)
    n, chunk, stride = 3, 8192, 8192 + 64
    comp = rng.integers(0, 256, n * stride, dtype=np.uint8)
    comp_off = np.arange(n) * stride
    sizes = np.array([100, 5000, stride], np.int64)
    pixels = rng.standard_normal(n * chunk // 2).astype(np.float16).view(np.uint8)     # finite values: NaN is in no set
    pix_off, pix_n = np.arange(n) * chunk, np.full(n, chunk)
    shapes = b.dump_outputs(str(tmp_path / "a"), comp, comp_off, sizes, pixels, pix_off, pix_n, np.float16)
    got = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in shapes}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["compressed_sizes"].tolist() == sizes.tolist()
    assert got["compressed_crc32"].tolist() == [zlib.crc32(comp[o:o + s]) for o, s in zip(comp_off, sizes)]
    assert got["pixels_crc32"].tolist() == [zlib.crc32(pixels[o:o + chunk]) for o in pix_off]
    pos = got["compressed_byte_positions"].astype(np.int64)
    for i in range(n):
        inside = pos < sizes[i]
        assert np.array_equal(got["compressed_bytes_sample"][i, inside], comp[comp_off[i] + pos[inside]])
        assert np.all(got["compressed_bytes_sample"][i, ~inside] == -1)
    assert np.all(np.isin(got["pixels_sample"], pixels.view(np.float16).astype(np.float32)))
    # other bytes, same geometry: the same positions
    b.dump_outputs(str(tmp_path / "b"), comp[::-1].copy(), comp_off, sizes, pixels[::-1].copy(), pix_off, pix_n, np.float16)
    assert np.array_equal(np.load(tmp_path / "b" / "compressed_byte_positions.npy"), got["compressed_byte_positions"])


def test_dump_outputs_fits_64_mb_at_the_headline_geometry():
    """BASELINE configs[1]: 32 chunks of 4 MiB float16; the dump stays within 64 MB whatever the chunks compress to."""
    b = _bench()
    n = 128 << 20 >> 22
    stride = b.CHUNK + 64
    rows = b.DUMP_LEAD + b.DUMP_CHUNK_SAMPLES
    total = 2 * 8 * n + 8 * n + 8 * rows + 4 * n * rows + 4 * b.DUMP_PIXEL_SAMPLES
    assert rows <= stride and total <= b.DUMP_LIMIT <= 64 << 20
