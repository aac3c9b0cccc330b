"""The zero-position argument of the UP instantiation of csrc/conv3x3_wino2.hip, in numpy: on a nearest x2
upsampled map, a 4 x 4 Winograd input patch at an even offset has rows (and columns) 1 and 2 equal, so row 2 and column 2 of B^T d B are
exactly zero in fp32 -- at every border with zero padding too -- and the other nine positions are a 3 x 3-source formula."""
import numpy as np

BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float32)
ZERO = [(i, j) for i in range(4) for j in range(4) if i == 2 or j == 2]
LIVE = [(i, j) for i in range(4) for j in range(4) if i != 2 and j != 2]


def _transform(d):
    """B^T d B in fp32, the order of the kernel: columns first (c = d[:, ca] +- d[:, cb]), then rows."""
    c = np.stack([d[:, 0] - d[:, 2], d[:, 1] + d[:, 2], d[:, 2] - d[:, 1], d[:, 1] - d[:, 3]], axis=1).astype(np.float32)
    return np.stack([c[0] - c[2], c[1] + c[2], c[2] - c[1], c[1] - c[3]], axis=0).astype(np.float32)


def _patches(Hs, Ws, seed, act=None):
    """Every 4 x 4 patch of the tile grid of the upsampled, zero-padded map with the 3 x 3 source neighbourhood it comes from."""
    rng = np.random.default_rng(seed)
    src = (rng.standard_normal((Hs, Ws)) * np.exp(2 * rng.standard_normal((Hs, Ws)))).astype(np.float32)
    if act is not None:
        src = act(src)
    up = np.repeat(np.repeat(src, 2, axis=0), 2, axis=1)
    pad = np.pad(up, 1)                                # pad[y + 1][x + 1] = up[y][x]
    spad = np.pad(src, 1)
    for m in range(Hs):
        for n in range(Ws):
            # output block (2m, 2n): input rows 2m - 1 .. 2m + 2, columns 2n - 1 .. 2n + 2; source rows m - 1 .. m + 1
            yield (m, n), pad[2 * m: 2 * m + 4, 2 * n: 2 * n + 4], spad[m: m + 3, n: n + 3]


def test_patch_rows_and_columns_1_and_2_are_equal():
    for _, d, s in _patches(5, 7, 0):
        assert np.array_equal(d[1], d[2]) and np.array_equal(d[:, 1], d[:, 2])
        assert np.array_equal(d, s[np.ix_([0, 1, 1, 2], [0, 1, 1, 2])])


def test_seven_positions_are_exactly_zero_everywhere():
    seen = set()
    for (m, n), d, _ in _patches(6, 9, 1):
        v = _transform(d)
        for (i, j) in ZERO:
            assert v[i, j] == 0.0, ((m, n), (i, j), v[i, j])
        seen.add((m == 0, m == 5, n == 0, n == 8))
    # interior patches, the four borders and the corners all occurred
    assert (False, False, False, False) in seen and len(seen) == 9
    # the generic B^T d B agrees (the argument does not depend on the order of the two passes)
    for _, d, _ in _patches(4, 4, 2):
        v = (BT @ d @ BT.T).astype(np.float32)
        assert all(v[i, j] == 0.0 for (i, j) in ZERO)


def test_nine_positions_equal_the_source_formula():
    """With source neighbourhood s (3 x 3: rows a, b, c), the live rows of B^T d are a - b, b + b, b - c, and the same for the columns:
    bit for bit in fp32 with the same order of the two passes, and B3 s B3^T in exact arithmetic."""
    B3 = np.array([[1, -1, 0], [0, 2, 0], [0, 1, -1]], dtype=np.float64)      # rows 0, 1, 3 of B^T applied to [a, b, b, c]
    for _, d, s in _patches(6, 9, 3):
        v = _transform(d)
        c = np.stack([s[:, 0] - s[:, 1], s[:, 1] + s[:, 1], s[:, 1] - s[:, 2]], axis=1).astype(np.float32)
        want = np.stack([c[0] - c[1], c[1] + c[1], c[1] - c[2]], axis=0).astype(np.float32)
        got = v[np.ix_([0, 1, 3], [0, 1, 3])]
        assert np.array_equal(got, want)
        # against exact arithmetic: two fp32 roundings per value, of magnitudes <= 2 |s| and <= 4 |s| (u = 2^-24)
        exact = B3 @ s.astype(np.float64) @ B3.T
        assert np.abs(got - exact).max() <= 2.0 ** -24 * (2 * 2 + 4) * np.abs(s).max()
    assert len(LIVE) == 9 and len(ZERO) == 7


def test_affine_and_silu_of_the_staging_keep_the_argument():
    """The staging applies the GroupNorm affine / SiLU to every staged value and the zero padding after it: equal source values stay
    equal, and padding still replaces only patch row / column 0 or 3."""
    def act(x):
        a = np.float32(1.7) * x + np.float32(-0.3)
        return (a / (np.float32(1) + np.exp(-a))).astype(np.float32)
    for _, d, _ in _patches(4, 6, 4, act):
        v = _transform(d)
        assert all(v[i, j] == 0.0 for (i, j) in ZERO)
