"""Writes tests/golden/zstd_streams_digests.json: the sha256 of every frame tests/_zstd_streams.py generates and of its expected
output, of every negative frame, and of every zstd plane of tests/_streams.py (chunks and pixels) -- but only after the box's
libzstd has decoded every positive frame to the expected bytes and has refused every negative one (or decoded it to the size its
good twin has).  The CPU and the GPU tests assert that what they generate has these digests, so a box without libzstd still
runs frames that libzstd validated.  Run from the repository root: python tests/golden/make_zstd_streams_digests.py"""
import ctypes as C
import ctypes.util
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _streams as S            # noqa: E402
import _zstd_streams as Z       # noqa: E402


def main():
    name = ctypes.util.find_library("zstd")
    if not name:
        raise SystemExit("no libzstd on this box: the digests are only written behind its verdict")
    z = C.CDLL(name)
    z.ZSTD_decompress.restype = C.c_size_t
    z.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
    z.ZSTD_isError.argtypes = [C.c_size_t]
    z.ZSTD_versionString.restype = C.c_char_p
    frames = Z.frame_cases()
    for nm, fr, want in frames:
        out = np.zeros(want.size + 1, np.uint8)
        r = z.ZSTD_decompress(out.ctypes.data, want.size, fr, len(fr))
        if z.ZSTD_isError(r) or r != want.size or not np.array_equal(out[:r], want):
            raise SystemExit("libzstd does not decode %s to the expected bytes" % nm)
    bad = Z.bad_frames()
    for nm, fr, n, _ in bad:
        out = np.zeros(n + 1, np.uint8)
        r = z.ZSTD_decompress(out.ctypes.data, n, fr, len(fr))
        if not z.ZSTD_isError(r) and r != n:
            raise SystemExit("libzstd decodes %s to %d bytes" % (nm, r))
    planes = {}
    for nm, codec, ts, kw in S.zstd_plane_cases():
        chunks, plane, _ = S.build_plane(nm, codec, ts, kw)
        planes[nm] = [hashlib.sha256(b"".join(chunks)).hexdigest(), hashlib.sha256(plane.tobytes()).hexdigest()]
    doc = {"libzstd": z.ZSTD_versionString().decode(), "frames": Z.digests(frames),
           "bad_frames": {nm: hashlib.sha256(fr).hexdigest() for nm, fr, _, _ in bad}, "planes": planes}
    with open(os.path.join(HERE, "zstd_streams_digests.json"), "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d frames, %d negative frames, %d planes validated by libzstd %s" % (len(frames), len(bad), len(planes), doc["libzstd"]))


if __name__ == "__main__":
    main()
