"""The weight gradient's launch geometry, without a device: sr3_conv_wgrad_scratch_bytes over a grid of layer shapes against the values
recorded in tests/golden/wgrad_scratch_bytes.npy (int64, in the order of `grid()`), which were taken from the library before the kernel
choice and the pixel split moved into wgrad_pick (csrc/wgrad.hip).  The query is the larger of the two `split` geometries' slabs, so on
shapes where only one rule applies -- 1x1 layers, 3x3 layers with 64 channels or fewer on a side -- this pins that rule alone; the msplit
values tests/scratch_rows.py and tests/edge_rows.py assert pin the rest."""
import itertools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wgrad_scratch_bytes.npy')
CHANNELS, MAPS = (4, 64, 68, 128, 320), (8, 10, 16, 24, 64)


def grid():
    """(B, Hs, Ws, ups, stride, ksize, C0, C1, Cout, split) in the order of the fixture"""
    for k, stride, ups, cin, cout, h, w, b, split in itertools.product((1, 3), (1, 2), (0, 1), CHANNELS, CHANNELS, MAPS, MAPS, (1, 2, 16), (0, 1)):
        yield (b, h, w, ups, stride, k, cin, 0, cout, split)


def query_all(lib):
    return np.array([int(lib.sr3_conv_wgrad_scratch_bytes(*g)) for g in grid()], dtype=np.int64)


def test_scratch_bytes_are_the_recorded_ones():
    from sr3_hip import lib as L
    want, got = np.load(GOLDEN), query_all(L.load())
    assert want.dtype == np.int64 and want.shape == got.shape
    assert int((want > 0).sum()) > want.size // 2          # the grid is mostly split layers
    bad = np.nonzero(want != got)[0]
    assert bad.size == 0, [(g, int(want[i]), int(got[i])) for i, g in enumerate(grid()) if i in set(bad[:8].tolist())]
