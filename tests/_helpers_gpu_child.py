"""Child process of tests/test_gpu_helpers_place.py: engines with helpers switched on (CIMG_ENC_HELPERS=1) or forced off
(CIMG_ENC_NO_HELPERS=1) as the argument says (the engine reads both when it is created), every shape of the test through them, oracle bytes and pixels checked.  Prints "ok <shape>" per shape and "done <n>"."""
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [_HERE, os.path.join(os.path.dirname(_HERE), "compressed-image_amd")]

import numpy as np

BLOCK = 32768


def shapes():
    from cimg import synth
    rng = np.random.Generator(np.random.PCG64(7))
    u8 = lambda a: np.ascontiguousarray(a).view(np.uint8).ravel()
    chunk = 8 * BLOCK
    t16 = u8(synth.tiled_channel(np.float16, 1024, 256))[:2 * chunk]
    t32 = u8(synth.tiled_channel(np.float32, 1024, 128))[:2 * chunk]
    out = []
    # (name, typesize, pixels, chunk sizes, comp stride or None, workgroups per CU or None)
    out.append(("two_chunks_of_8_blocks_ts2", 2, t16, [chunk] * 2, None, None))     # 32 items, a thousand waves: nearly all pure helpers
    out.append(("two_chunks_of_8_blocks_ts4", 4, t32, [chunk] * 2, None, None))
    out.append(("one_block", 2, t16[:BLOCK], [BLOCK], None, None))
    mixed = np.concatenate([t16[:chunk], rng.integers(0, 256, chunk, dtype=np.uint8), t16[chunk:2 * chunk]])
    out.append(("random_chunk_memcpyed", 2, mixed, [chunk] * 3, None, None))
    out.append(("odd_comp_off", 2, t16, [chunk] * 2, chunk + 32 + 65, None))
    big = u8(synth.tiled_channel(np.float16, 4096, 2560))                           # 20 MiB: 20 chunks of 1 MiB, 640 blocks
    out.append(("twenty_chunks_one_workgroup_per_cu", 2, big, [1 << 20] * 20, None, 1))
    return out


def check(eng, hip, O, ts, raw, sizes, stride):
    n = len(sizes)
    dest = max(sizes) + 32
    stride = dest + 64 if stride is None else stride
    raw_off = np.concatenate([[0], np.cumsum(sizes[:-1])]).astype(np.int64)
    comp_off = np.arange(n, dtype=np.int64) * stride
    d_raw, d_out, d_comp = eng.alloc(raw.size), eng.alloc(raw.size), eng.alloc(n * stride + 64)
    try:
        d_raw.upload(raw)
        d_comp.upload(np.full(n * stride + 64, 0x5A, np.uint8))
        p, po = hip.cparams(ts), O.cparams(ts)
        want = [O.compress(po, raw[o:o + s], destsize=dest) for o, s in zip(raw_off, sizes)]
        for rep in range(2):                                  # the second batch meets the marks the first one left behind
            cbytes = eng.compress_device(p, d_raw.ptr, raw_off, sizes, d_comp.ptr, comp_off, [dest] * n)
            comp = d_comp.download()
            for i, (r, c) in enumerate(want):
                assert cbytes[i] == r, (rep, i, cbytes[i], r)
                assert comp[comp_off[i]:comp_off[i] + r].tobytes() == c, (rep, i)
                assert (comp[comp_off[i] + dest:comp_off[i] + stride] == 0x5A).all(), (rep, i)
        eng.decompress_device(d_comp.ptr, comp_off, sizes, [BLOCK] * n, d_out.ptr, raw_off)
        assert d_out.download().tobytes() == raw.tobytes()
    finally:
        for b in (d_raw, d_out, d_comp):
            b.free()


def main():
    no_helpers = sys.argv[1] == "off"
    os.environ.pop("CIMG_ENC_NO_HELPERS", None)
    os.environ.pop("CIMG_ENC_HELPERS", None)
    if no_helpers:
        os.environ["CIMG_ENC_NO_HELPERS"] = "1"
    else:
        os.environ["CIMG_ENC_HELPERS"] = "1"
    from cimg import hip
    import _oracle as O
    done = 0
    engines = {}
    try:
        for name, ts, raw, sizes, stride, wgs in shapes():
            if wgs not in engines:
                if wgs:
                    os.environ["CIMG_ENC_WGS_PER_CU"] = str(wgs)
                try:
                    engines[wgs] = hip.Engine(0)
                finally:
                    os.environ.pop("CIMG_ENC_WGS_PER_CU", None)
            check(engines[wgs], hip, O, ts, raw, sizes, stride)
            print("ok", name, flush=True)
            done += 1
    finally:
        for e in engines.values():
            e.close()
    print("done", done, flush=True)


if __name__ == "__main__":
    main()
