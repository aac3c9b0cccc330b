"""The JPEG link of the degradation chain, the parts that need no GPU: jpeg_oracle -- the NumPy integer restatement
of libjpeg's lossy half as Pillow drives it (colour conversion, chroma down-sampling, the "islow" forward DCT, quantisation, the
inverse DCT, fancy up-sampling, conversion back) -- against the committed Pillow round trips of tests/golden/jpeg_roundtrip.npz and,
where Pillow is built on libjpeg-turbo, against a live round trip; the config's "jpeg" block; draw_deg's sixth number; and the
argument refusals of sr3_jpeg_u8 / sr3_jpeg_scratch_bytes (checked before anything is launched).  tests/test_gpu_jpeg.py compares the
device against jpeg_oracle and the fixture byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from helpers import ROOT

# ---- the oracle ------------------------------------------------------------------------------------------------------------------------

# Annex K of the JPEG standard, natural (row-major) order
LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                   72, 92, 95, 98, 112, 100, 103, 99], np.int64).reshape(8, 8)
CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                    + [99] * 32, np.int64).reshape(8, 8)
F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def FIX(v):
    return int(v * 65536 + 0.5)


def descale(x, n):
    return (x + (1 << (n - 1))) >> n


def quant_table(base, quality):
    q = min(max(int(quality), 1), 100)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((base * s + 50) // 100, 1, 255)


def _odd_part(t4, t5, t6, t7):
    """the shared odd half of the Loeffler-Ligtenberg-Moschytz butterflies: four inputs -> the four rotated sums (before descaling)"""
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175
    t4, t5, t6, t7 = t4 * F_0_298, t5 * F_2_053, t6 * F_3_072, t7 * F_1_501
    z1, z2, z3, z4 = z1 * -F_0_899, z2 * -F_2_562, z3 * -F_1_961 + z5, z4 * -F_0_390 + z5
    return t4 + z1 + z3, t5 + z2 + z4, t6 + z2 + z3, t7 + z1 + z4


def _fdct_pass(d, first):
    """one 1-D forward pass along the last axis of (..., 8) int64"""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else descale(t10 - t11, 2)
    z1 = (t12 + t13) * F_0_541
    o[2] = descale(z1 + t13 * F_0_765, n)
    o[6] = descale(z1 - t12 * F_1_847, n)
    a4, a5, a6, a7 = _odd_part(t4, t5, t6, t7)
    o[7], o[5], o[3], o[1] = descale(a4, n), descale(a5, n), descale(a6, n), descale(a7, n)
    return np.stack(o, -1)


def _idct_pass(c, n):
    """one 1-D inverse pass along the last axis of (..., 8) int64, descaled by n bits"""
    z2, z3 = c[..., 2], c[..., 6]
    z1 = (z2 + z3) * F_0_541
    t2, t3 = z1 - z3 * F_1_847, z1 + z2 * F_0_765
    t0, t1 = (c[..., 0] + c[..., 4]) << 13, (c[..., 0] - c[..., 4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = _odd_part(c[..., 7], c[..., 5], c[..., 3], c[..., 1])
    o = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    assert max(int(np.abs(v).max()) for v in o) < 2 ** 31 - 2 ** 17      # the device computes in int
    return np.stack([descale(v, n) for v in o], -1)


def _codec_plane(p, table):
    """(h, w) int64 samples, h and w multiples of 8 -> the decoded plane: FDCT rows then columns, quantise, dequantise, IDCT columns
    then rows, + 128, clamp"""
    h, w = p.shape
    b = p.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3) - 128                 # (by, bx, row, col)
    f = _fdct_pass(b, True)
    f = _fdct_pass(f.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)           # f[row = vertical frequency][col]
    assert np.abs(f).max() < 2 ** 31
    qv = table << 3
    coef = np.sign(f) * ((np.abs(f) + (qv >> 1)) // qv) * table
    g = _idct_pass(coef.transpose(0, 1, 3, 2), 11).transpose(0, 1, 3, 2)
    g = _idct_pass(g, 18)
    return np.clip(g + 128, 0, 255).transpose(0, 2, 1, 3).reshape(h, w)


def _pad_edge(p, h, w):
    return np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode='edge')


def _up8(v):
    return (v + 7) // 8 * 8


def jpeg_oracle(img, quality, subsampling):
    """(H, W, C) uint8, C 1 or 3 -> the bytes Pillow's JPEG round trip at `quality` gives (subsampling 0 = 4:4:4, 2 = 4:2:0; ignored for
    C == 1).  Everything in int64; the device computes the same in int."""
    H, W, Cc = img.shape
    a = img.astype(np.int64)
    lt, ct = quant_table(LUMA_Q, quality), quant_table(CHROMA_Q, quality)
    if Cc == 1:
        return _codec_plane(_pad_edge(a[:, :, 0], _up8(H), _up8(W)), lt)[:H, :W, None].astype(np.uint8)
    R, G, B = a[:, :, 0], a[:, :, 1], a[:, :, 2]
    Y = (FIX(.299) * R + FIX(.587) * G + FIX(.114) * B + 32768) >> 16
    Cb = (-FIX(.16874) * R - FIX(.33126) * G + FIX(.5) * B + (128 << 16) + 32767) >> 16
    Cr = (FIX(.5) * R - FIX(.41869) * G - FIX(.08131) * B + (128 << 16) + 32767) >> 16
    Yd = _codec_plane(_pad_edge(Y, _up8(H), _up8(W)), lt)[:H, :W]
    if subsampling == 0:
        Cbu, Cru = (_codec_plane(_pad_edge(p, _up8(H), _up8(W)), ct)[:H, :W] for p in (Cb, Cr))
    else:
        Hc, Wc = (H + 1) // 2, (W + 1) // 2
        ups = []
        for p in (Cb, Cr):
            # horizontally: the full-resolution plane to a multiple of 16 columns; vertically: to an even row count only ...
            f = _pad_edge(p, H + (H & 1), (W + 15) // 16 * 16)
            bias = np.where(np.arange(f.shape[1] // 2) % 2 == 0, 1, 2)[None, :]
            d = (f[0::2, 0::2] + f[0::2, 1::2] + f[1::2, 0::2] + f[1::2, 1::2] + bias) >> 2
            # ... then the DOWN-SAMPLED plane's last row to a multiple of 8 rows
            d = _codec_plane(_pad_edge(d, _up8(Hc), d.shape[1]), ct)[:Hc, :Wc]
            # fancy up-sampling over the real samples: 3 * this + neighbour vertically, then (3 * this + previous / next + 8 / 7) >> 4
            up = np.zeros((2 * Hc, 2 * Wc), np.int64)
            idx = np.arange(Hc)
            for par, nb in ((0, np.maximum(idx - 1, 0)), (1, np.minimum(idx + 1, Hc - 1))):
                s = 3 * d + d[nb]
                up[par::2, 0::2] = (3 * s + s[:, np.maximum(np.arange(Wc) - 1, 0)] + 8) >> 4
                up[par::2, 1::2] = (3 * s + s[:, np.minimum(np.arange(Wc) + 1, Wc - 1)] + 7) >> 4
            ups.append(up[:H, :W])
        Cbu, Cru = ups
    x, z = Cbu - 128, Cru - 128
    out = np.stack([Yd + ((FIX(1.402) * z + 32768) >> 16), Yd + ((-FIX(.34414) * x - FIX(.71414) * z + 32768) >> 16),
                    Yd + ((FIX(1.772) * x + 32768) >> 16)], -1)
    return np.clip(out, 0, 255).astype(np.uint8)


# ---- the fixture and Pillow ------------------------------------------------------------------------------------------------------------

def load_fixture():
    """-> [(input (H, W, C), quality, subsampling, Pillow's bytes (H, W, C))] in the fixture's order"""
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_roundtrip.npz'))
    out = []
    for i, (s, k, q, sub, Cc) in enumerate(z['cases'].tolist()):
        rgb = z['in_%d_%d' % (s, k)]
        out.append((rgb if Cc == 3 else np.ascontiguousarray(rgb[:, :, 1:2]), q, sub, z['out_%d' % i]))
    return out


def test_fixture_holds_the_issue_case_list():
    from tools.make_jpeg_golden import KINDS, MODES, QUALITIES, SIZES
    fx = load_fixture()
    assert len(fx) == len(SIZES) * len(KINDS) * len(QUALITIES) * len(MODES) == 432
    assert {x[0].shape[:2] for x in fx} == {(1, 1), (8, 8), (16, 16), (17, 23), (7, 33), (24, 40), (40, 24), (64, 48)}
    assert {x[1] for x in fx} == {1, 10, 50, 75, 95, 100} and {(x[2], x[0].shape[2]) for x in fx} == {(0, 3), (2, 3), (-1, 1)}
    assert all(x[0].shape == x[3].shape and x[3].dtype == np.uint8 for x in fx)
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'jpeg_roundtrip.npz')) < (1 << 20)


def test_jpeg_oracle_equals_the_fixture():
    bad = [(i, img.shape, q, sub) for i, (img, q, sub, ref) in enumerate(load_fixture()) if not np.array_equal(jpeg_oracle(img, q, sub), ref)]
    assert not bad, bad[:10]


def test_jpeg_oracle_equals_live_pillow():
    """a second seed of the same case list; skipped only as a whole, and only where this Pillow is not built on libjpeg-turbo"""
    from PIL import features
    if not features.check_feature('libjpeg_turbo'):
        pytest.skip('this Pillow is not built on libjpeg-turbo: the committed fixture is the gate')
    from tools.make_jpeg_golden import SEED, case_input, case_list, round_trip
    inputs, cases = case_list(SEED + 1)
    bad = []
    for c in cases:
        img = case_input(inputs, c)
        if not np.array_equal(jpeg_oracle(img, c[2], c[3]), round_trip(img, c[2], c[3])):
            bad.append(c)
    assert not bad, bad[:10]


def test_jpeg_oracle_flat_images_and_quality_clamp():
    for v in (0, 255):
        for Cc in (1, 3):
            img = np.full((9, 10, Cc), v, np.uint8)
            assert np.array_equal(jpeg_oracle(img, 100, 2), img)
    assert quant_table(LUMA_Q, 100).max() == 1 and quant_table(LUMA_Q, 1).min() == 255 and quant_table(CHROMA_Q, 50)[0, 0] == 17
    assert np.array_equal(quant_table(LUMA_Q, 0), quant_table(LUMA_Q, 1)) and np.array_equal(quant_table(LUMA_Q, 300), quant_table(LUMA_Q, 100))


# ---- config ----------------------------------------------------------------------------------------------------------------------------

def test_degrade_config_jpeg_defaults_and_normalisation():
    from data.degrade import degrade_config
    c = degrade_config({}, 8)
    assert c['jpeg'] == {'prob': 0.0, 'quality': (30, 95), 'subsampling': '4:2:0', 'given': False}
    assert degrade_config({'jpeg': {}}, 8)['jpeg'] == {'prob': 1.0, 'quality': (30, 95), 'subsampling': '4:2:0', 'given': True}
    c = degrade_config({'jpeg': {'prob': 0.7, 'quality': [40, 90], 'subsampling': '4:4:4'}, 'noise': {'sigma': [1, 2]}}, 8)
    assert c['jpeg'] == {'prob': 0.7, 'quality': (40, 90), 'subsampling': '4:4:4', 'given': True} and c['noise']['prob'] == 1.0
    assert degrade_config({'jpeg': {'prob': 0, 'quality': (1, 100)}}, 8)['jpeg'] == {'prob': 0.0, 'quality': (1, 100), 'subsampling': '4:2:0',
                                                                                  'given': True}
    assert degrade_config({'jpeg': {'quality': [77, 77]}}, 8)['jpeg']['quality'] == (77, 77)


@pytest.mark.parametrize('block, word', [
    ({'qualty': [1, 2]}, 'jpeg.qualty'), ({'sigma': [1, 2]}, 'jpeg.sigma'),
    ({'quality': [0, 50]}, 'jpeg.quality'), ({'quality': [50, 101]}, 'jpeg.quality'), ({'quality': [60, 50]}, 'jpeg.quality'),
    ({'quality': [30.0, 95]}, 'jpeg.quality'), ({'quality': [30, 95.5]}, 'jpeg.quality'), ({'quality': [True, 95]}, 'jpeg.quality'),
    ({'quality': 75}, 'jpeg.quality'), ({'quality': [30, 60, 90]}, 'jpeg.quality'), ({'quality': ['30', '95']}, 'jpeg.quality'),
    ({'prob': 1.5}, 'jpeg.prob'), ({'prob': -0.1}, 'jpeg.prob'), ({'prob': 'x'}, 'jpeg.prob'), ({'prob': True}, 'jpeg.prob'),
    ({'subsampling': '4:2:2'}, 'jpeg.subsampling'), ({'subsampling': 2}, 'jpeg.subsampling'), ({'subsampling': None}, 'jpeg.subsampling'),
])
def test_degrade_config_jpeg_refusals(block, word):
    from data.degrade import degrade_config
    with pytest.raises(ValueError) as e:
        degrade_config({'jpeg': block}, 8)
    assert word in str(e.value), str(e.value)


@pytest.mark.parametrize('value', [3, 'on', [30, 95], None, True])
def test_degrade_config_jpeg_refuses_a_non_dict(value):
    from data.degrade import degrade_config
    with pytest.raises(ValueError, match='jpeg'):
        degrade_config({'jpeg': value}, 8)


# ---- draw_deg --------------------------------------------------------------------------------------------------------------------------

BASE = {'blur': {'prob': 0.5, 'kernel': 5, 'sigma': [0.5, 2], 'anisotropic': True}, 'noise': {'prob': 0.5, 'sigma': [1, 9]}}


def test_draw_deg_first_five_numbers_do_not_move():
    from data.degrade import degrade_config, draw_deg
    plain = degrade_config(BASE, 8)
    with_jpeg = degrade_config(dict(BASE, jpeg={'prob': 0.5, 'quality': [30, 95]}), 8)
    on = set()
    for seed in range(50):
        a = draw_deg(plain, torch.Generator().manual_seed(seed))
        g = torch.Generator().manual_seed(seed)
        b = draw_deg(with_jpeg, g)
        assert a.dtype == b.dtype == torch.float32 and tuple(a.shape) == (5,) and tuple(b.shape) == (6,)
        assert torch.equal(a, b[:5])
        q = float(b[5])
        assert q == 0.0 or (30 <= q <= 95 and q == int(q))
        on.add(q != 0.0)
        # seven draws, whatever is on: the generator stands where seven torch.rand draws leave it
        h = torch.Generator().manual_seed(seed)
        torch.rand(7, generator=h)
        assert torch.equal(torch.rand(3, generator=g), torch.rand(3, generator=h))
    assert on == {False, True}
    torch.manual_seed(4)
    a = draw_deg(plain)
    torch.manual_seed(4)
    assert torch.equal(a, draw_deg(with_jpeg)[:5])                       # the global generator too


def test_draw_deg_quality_distribution():
    from data.degrade import degrade_config, draw_deg
    off = degrade_config({'jpeg': {'prob': 0, 'quality': [30, 95]}}, 8)
    fixed = degrade_config({'jpeg': {'prob': 1, 'quality': [61, 61]}}, 8)
    four = degrade_config({'jpeg': {'prob': 0.6, 'quality': [30, 33]}}, 8)
    full = degrade_config({'jpeg': {'quality': [1, 100]}}, 8)
    g = torch.Generator().manual_seed(11)
    seen, n_on = set(), 0
    for _ in range(2000):
        assert float(draw_deg(off, g)[5]) == 0.0
        assert float(draw_deg(fixed, g)[5]) == 61.0
        assert 1 <= float(draw_deg(full, g)[5]) <= 100
        q = float(draw_deg(four, g)[5])
        if q != 0.0:
            assert q in (30.0, 31.0, 32.0, 33.0)
            seen.add(q)
            n_on += 1
    assert seen == {30.0, 31.0, 32.0, 33.0}
    assert abs(n_on / 2000 - 0.6) < 0.05                                 # (a binomial's 4.5 sigma at n = 2000)


def test_hr_crop_dataset_carries_the_sixth_number(tmp_path):
    import data as Data
    from test_degrade_cpu import dataset_opt, write_folder
    root = str(tmp_path / 'hr')
    write_folder(root)
    ds = Data.create_dataset(dataset_opt(root, degrade={'jpeg': {'quality': [50, 50]}}), 'train')
    assert ds.degrade['jpeg']['given'] is True
    torch.manual_seed(1)
    items = [ds[i] for i in range(3)]
    assert all(tuple(it['deg'].shape) == (6,) and float(it['deg'][5]) == 50.0 for it in items)
    assert tuple(torch.utils.data.default_collate(items)['deg'].shape) == (3, 6)
    va = Data.create_dataset(dataset_opt(root, degrade={'jpeg': {'prob': 0.5}}), 'val')
    assert torch.equal(va[1]['deg'], va[1]['deg']) and tuple(va[1]['deg'].shape) == (6,)


# ---- the C entries' refusals: before any launch, so no device is needed -----------------------------------------------------------------

def _p(v):
    return C.c_void_p(v)


# 2 x 16 x 20 x 3 = 1920 bytes per buffer; the scratch far from both
JPEG_OK = dict(inp=_p(1 << 20), n=2, H=16, W=20, C=3, q=_p(1 << 12), sub=2, out=_p(1 << 21), scratch=_p(1 << 24), sbytes=1 << 16)
JPEG_REFUSALS = [
    (dict(inp=None), 'in_hwc'), (dict(out=None), 'out_hwc'), (dict(q=None), 'quality'), (dict(scratch=None), 'scratch'),
    (dict(n=0), 'n_images'), (dict(n=-1), 'n_images'), (dict(H=0), 'H 0'), (dict(W=-3), 'W -3'),
    (dict(C=2), 'C 2'), (dict(C=4), 'C 4'), (dict(sub=1), 'subsampling 1'), (dict(sub=3), 'subsampling 3'), (dict(sub=-1), 'subsampling -1'),
    (dict(sbytes=0), 'scratch_bytes'), (dict(sbytes=100), 'scratch_bytes'),
    (dict(out=_p((1 << 20) + 100)), 'out_hwc'), (dict(out=_p((1 << 20) - 100)), 'out_hwc'),
    (dict(scratch=_p((1 << 20) + 64)), 'scratch'), (dict(scratch=_p((1 << 21) - 64)), 'scratch'),
    (dict(out=_p(1 << 20), scratch=_p((1 << 20) + 1024)), 'scratch'),
    (dict(n=16, H=8192, W=8192, C=3, sbytes=1 << 40, out=_p(1 << 40), scratch=_p(1 << 42)), '2^31'),
    (dict(n=2, H=1 << 15, W=1 << 15, C=1, sbytes=1 << 40, out=_p(1 << 40), scratch=_p(1 << 42)), '2^31'),
]


@pytest.mark.parametrize('kw, word', JPEG_REFUSALS)
def test_jpeg_u8_refusals_no_gpu(kw, word):
    from sr3_hip import lib as L
    lib = L.load()
    a = dict(JPEG_OK, **kw)
    rc = lib.sr3_jpeg_u8(a['inp'], a['n'], a['H'], a['W'], a['C'], a['q'], a['sub'], a['out'], a['scratch'], a['sbytes'], None)
    assert rc == -1, kw
    msg = lib.sr3_last_error().decode()
    assert msg.startswith('jpeg_u8') and word in msg, (kw, msg)


def test_jpeg_scratch_bytes_query():
    from sr3_hip import lib as L
    lib = L.load()
    q = lib.sr3_jpeg_scratch_bytes
    assert q(2, 16, 20, 3, 0) == 2 * 3 * 16 * 20 and q(2, 16, 20, 3, 2) == 2 * (16 * 20 + 2 * 8 * 10)
    assert q(1, 17, 23, 3, 2) == 17 * 23 + 2 * 9 * 12 and q(3, 17, 23, 1, 2) == q(3, 17, 23, 1, 7) == 3 * 17 * 23      # C == 1: ignored
    assert q(1, 1, 1, 3, 2) == 3
    for bad in ((0, 16, 20, 3, 2), (2, 0, 20, 3, 2), (2, 16, -1, 3, 2), (2, 16, 20, 2, 2), (2, 16, 20, 3, 1), (16, 8192, 8192, 3, 0),
                (2, 1 << 15, 1 << 15, 1, 0)):
        assert q(*bad) == 0, bad
    # the query is what the call demands: one byte less is refused
    a = dict(JPEG_OK, sbytes=q(2, 16, 20, 3, 2) - 1)
    assert lib.sr3_jpeg_u8(a['inp'], a['n'], a['H'], a['W'], a['C'], a['q'], a['sub'], a['out'], a['scratch'], a['sbytes'], None) == -1
    assert 'scratch_bytes 959' in lib.sr3_last_error().decode()


def test_jpeg_batch_checks_its_arguments_and_has_no_cpu_fallback():
    from data.degrade import jpeg_batch
    a = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    q = torch.tensor([50, 60], dtype=torch.int32)
    with pytest.raises(TypeError, match='jpeg_batch'):
        jpeg_batch(a, q)                                                 # host tensors: no CPU fallback
    with pytest.raises(ValueError, match='subsampling'):
        jpeg_batch(a, q, subsampling='4:2:2')
