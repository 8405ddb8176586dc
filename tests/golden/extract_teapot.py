#!/usr/bin/env python3
"""Regenerates tests/golden/teapot/ from a checkout of the reference:

    python tests/golden/extract_teapot.py <reference>/models/teapot

scene.xml is copied as it is.  textures/envmap.hdr (1024 x 512 RGBE, larger than a committed
file may be) is stored at half resolution: each 2 x 2 block of decoded pixels is averaged and
re-encoded as RGBE (RGBE_FromFloat, oracle/film.py rgbe_encode), written as run-length
scanlines that hold literal runs only, which both the product's and the oracle's readers
accept.  tests/test_c1_teapot.py pins no pixel to the environment map's content.  The fixture
is committed and travels; the reference does not.
"""
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import film as ref  # noqa: E402


def write_rgbe(path, rgbe):
    h, w, _ = rgbe.shape
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w))
        for y in range(h):
            f.write(bytes([2, 2, w >> 8, w & 255]))
            for c in range(4):
                row = rgbe[y, :, c].tobytes()
                for x in range(0, w, 128):
                    chunk = row[x:x + 128]
                    f.write(bytes([len(chunk)]) + chunk)


def main(src):
    dst = os.path.join(HERE, "teapot")
    os.makedirs(os.path.join(dst, "textures"), exist_ok=True)
    shutil.copyfile(os.path.join(src, "scene.xml"), os.path.join(dst, "scene.xml"))
    rgb, _ = ref.read_rgbe(os.path.join(src, "textures", "envmap.hdr"))
    h, w, _ = rgb.shape
    half = rgb.astype(np.float64).reshape(h // 2, 2, w // 2, 2, 3).mean(axis=(1, 3)).astype(np.float32)
    out = os.path.join(dst, "textures", "envmap.hdr")
    write_rgbe(out, ref.rgbe_encode(half))
    back, _ = ref.read_rgbe(out)
    assert back.shape == half.shape and np.all(np.abs(back - half) <= half.max(axis=-1, keepdims=True) / 128)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv[1])
