#!/usr/bin/env python3
"""Makes tests/golden/jpeg_roundtrip.npz: Pillow's JPEG round trip (Image.save(buf, 'JPEG', quality=q, subsampling=s), Image.open)
of small images, the fixture the device's sr3_jpeg_u8 and the NumPy restatement of tests/test_jpeg_cpu.py are compared with byte for
byte.  The committed file pins the bytes of ONE libjpeg (Pillow built on libjpeg-turbo, the default "islow"
integer DCT), so the gate does not depend on which libjpeg the testing machine's Pillow was built on.

The npz holds
    cases       (n, 5) int32: [size index, kind index, quality, subsampling (Pillow's number: 0 = 4:4:4, 2 = 4:2:0; -1 = greyscale), C]
    in_<s>_<k>  (H, W, 3) uint8 input of size SIZES[s], kind k (0 random bytes, 1 smooth, 2 random 0 / 255); a greyscale case reads
                its channel 1
    out_<i>     (H, W, C) uint8: Pillow's round trip of case i
case_list(seed) and round_trip() are what tests/test_jpeg_cpu.py imports for its live comparison on a second seed.
    python tools/make_jpeg_golden.py [--out tests/golden/jpeg_roundtrip.npz]"""
import argparse
import io
import os

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (8, 8), (16, 16), (17, 23), (7, 33), (24, 40), (40, 24), (64, 48)]
QUALITIES = [1, 10, 50, 75, 95, 100]
KINDS = ['random', 'smooth', 'extremes']
MODES = [(0, 3), (2, 3), (-1, 1)]                # (subsampling, C)
SEED = 20


def make_input(hw, kind, rng):
    H, W = hw
    if kind == 0:
        return rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    if kind == 1:
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        ph = rng.rand(3) * 6.28
        a = np.stack([127.5 + 100 * np.sin(yy / 5.0 + ph[c]) * np.cos(xx / 7.0 + c) + 20 * np.sin((xx + yy) / 3.0) for c in range(3)], -1)
        return np.clip(np.rint(a), 0, 255).astype(np.uint8)
    return (rng.randint(0, 2, size=(H, W, 3)) * 255).astype(np.uint8)


def round_trip(img, quality, subsampling):
    """(H, W, C) uint8 -> Pillow's decoded bytes of its JPEG at `quality`; C == 1: mode 'L' (subsampling is not passed)"""
    buf = io.BytesIO()
    if img.shape[2] == 1:
        Image.fromarray(img[:, :, 0], 'L').save(buf, 'JPEG', quality=int(quality))
    else:
        Image.fromarray(img, 'RGB').save(buf, 'JPEG', quality=int(quality), subsampling=int(subsampling))
    out = np.asarray(Image.open(io.BytesIO(buf.getvalue())))
    return out[:, :, None] if out.ndim == 2 else out


def case_list(seed):
    """-> (inputs {(s, k): (H, W, 3) uint8}, cases [(s, k, quality, subsampling, C)]) in the fixture's order"""
    rng = np.random.RandomState(seed)
    inputs = {(s, k): make_input(SIZES[s], k, rng) for s in range(len(SIZES)) for k in range(len(KINDS))}
    cases = [(s, k, q, sub, C) for s in range(len(SIZES)) for k in range(len(KINDS)) for q in QUALITIES for sub, C in MODES]
    return inputs, cases


def case_input(inputs, case):
    s, k, _, _, C = case
    return inputs[(s, k)] if C == 3 else np.ascontiguousarray(inputs[(s, k)][:, :, 1:2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'jpeg_roundtrip.npz'))
    a = ap.parse_args()
    from PIL import features
    assert features.check_feature('libjpeg_turbo'), 'the fixture pins libjpeg-turbo\'s bytes: make it with a Pillow built on it'
    inputs, cases = case_list(SEED)
    arrays = {'cases': np.array(cases, np.int32)}
    for (s, k), v in inputs.items():
        arrays['in_%d_%d' % (s, k)] = v
    for i, c in enumerate(cases):
        arrays['out_%d' % i] = round_trip(case_input(inputs, c), c[2], c[3])
    np.savez_compressed(a.out, **arrays)
    print('%s: %d cases, %d bytes (Pillow %s, libjpeg %s)' % (a.out, len(cases), os.path.getsize(a.out), Image.__version__,
                                                             features.version('jpg')))


if __name__ == '__main__':
    main()
