"""The second-order degradation, the parts that need no GPU: the config's new keys, draw_deg2 and the draw stream,
sinc_weights, poisson_table, and the argument refusals of sr3_noise_ex_u8 and resize_batch (checked before anything is launched).
The NumPy restatements of the new device arithmetic live here (noise_ex_oracle, degrade2_oracle); tests/test_gpu_degrade2.py
compares the device against them bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
from PIL import Image

from test_degrade_cpu import blur_oracle, dataset_opt, noise_oracle, pil_resize, write_folder
from test_jpeg_cpu import jpeg_oracle

SUB = {'4:4:4': 0, '4:2:0': 2}


# ---- oracles ---------------------------------------------------------------------------------------------------------------------------

def poisson_draw(table, lam, r):
    """k = #{j : table[lam][j] <= r}, elementwise over integer arrays lam and r"""
    return (table[lam] <= np.asarray(r)[..., None]).sum(-1).astype(np.int64)


def _shift(v, d):
    """clamp(rint(v + d)) with the sum rounded once in fp32"""
    s = v.astype(np.float32) + d
    assert s.dtype == np.float32
    return np.clip(np.rint(s), 0, 255).astype(np.uint8)


def noise_ex_oracle(img, mode, strength, z, r, table):
    """(H, W, C) uint8 -> sr3_noise_ex_u8's bytes for one image: every product and sum one fp32 rounding, rint half to even."""
    s = np.float32(strength)
    if s == 0:
        return img.copy()
    Cc = img.shape[2]
    if mode in (0, 1):
        zz = z.astype(np.float32)
        return noise_oracle(img, s, np.repeat(zz[:, :, :1], Cc, 2) if mode == 1 else zz)
    v = img.astype(np.int64)
    if mode == 3 and Cc == 3:
        Y = (19595 * v[:, :, 0] + 38470 * v[:, :, 1] + 7471 * v[:, :, 2] + 32768) >> 16
        d = s * (poisson_draw(table, Y, r[:, :, 0]) - Y).astype(np.float32)
        assert d.dtype == np.float32
        return _shift(img, d[:, :, None])
    d = s * (poisson_draw(table, v, r) - v).astype(np.float32)
    assert d.dtype == np.float32
    return _shift(img, d)


def degrade2_oracle(hr, deg, deg2, cfg, M, rs1, rs2, z=None, r=None, z2=None, r2=None):
    """One image through the second-order chain: NumPy blur / noise / JPEG, Pillow resizes.  deg, deg2: the image's numbers
    (float64); M, rs1, rs2: the batch's (row 0 of deg2)."""
    from data.degrade import blur_weights, poisson_table, sinc_weights
    table = poisson_table()
    top = {'bicubic': Image.BICUBIC, 'bilinear': Image.BILINEAR}[cfg['resample']]
    sec, Lr = cfg['second'], cfg['l_resolution']

    def blur(x, on, sinc_on, omega, sx, sy, th, k):
        if not on:
            return x
        return blur_oracle(x, sinc_weights(min(omega, np.pi), k) if sinc_on else blur_weights(sx, sy, th, k))

    def noise(x, on, sigma, mode, scale, zz, rr):
        return noise_ex_oracle(x, int(mode), scale if mode >= 2 else sigma, zz, rr, table) if on else x

    x = blur(hr, deg[0] != 0, deg2[0] != 0, deg2[1], deg[1], deg[2], deg[3], cfg['blur']['kernel'])
    x = pil_resize(x, (M, M) if sec is not None else (Lr, Lr), rs1)
    x = noise(x, deg[4] != 0, deg[4], deg2[2], deg2[3], z, r)
    if len(deg) == 6 and deg[5] != 0:
        x = jpeg_oracle(x, int(deg[5]), SUB[cfg['jpeg']['subsampling']])
    if sec is not None:
        x = blur(x, deg2[7] != 0, deg2[11] != 0, deg2[12], deg2[8], deg2[9], deg2[10], sec['blur']['kernel'])
        x = pil_resize(x, (Lr, Lr), rs2)
        x = noise(x, deg2[13] != 0, deg2[13], deg2[14], deg2[15], z2, r2)
        for stage in (('jpeg', 'sinc') if deg2[19] != 0 else ('sinc', 'jpeg')):
            if stage == 'jpeg' and deg2[16] != 0:
                x = jpeg_oracle(x, int(deg2[16]), SUB[sec['jpeg']['subsampling']])
            if stage == 'sinc' and deg2[17] != 0:
                x = blur_oracle(x, sinc_weights(min(deg2[18], np.pi), sec['final_sinc']['kernel']))
    return x, pil_resize(x, hr.shape[:2], top)


# ---- config ----------------------------------------------------------------------------------------------------------------------------

OLD = {'blur': {'prob': 0.5, 'kernel': 7, 'sigma': [0.3, 2], 'anisotropic': True}, 'noise': {'prob': 0.5, 'sigma': [1, 25]},
       'jpeg': {'prob': 0.5, 'quality': [40, 90], 'subsampling': '4:4:4'}, 'resample': 'bilinear', 'seed': 4}
NEW = {'sinc': {'prob': 0.1, 'omega': [1.05, 3.14]}, 'shot': {'prob': 0.5, 'scale': [0.05, 3.0]}, 'gray_noise': 0.4,
       'second': {'mid': [12, 40], 'resample': ['box', 'bilinear', 'bicubic'],
                  'blur': {'prob': 0.8, 'kernel': 5, 'sigma': [0.2, 1.5]}, 'sinc': {'prob': 0.2, 'omega': [1.5, math.pi]},
                  'noise': {'prob': 0.5, 'sigma': [1, 10]}, 'shot': {'prob': 0.3, 'scale': [0.5, 2]}, 'gray_noise': 0.25,
                  'jpeg': {'quality': [30, 60]}, 'final_sinc': {'prob': 0.8, 'kernel': 7, 'omega': [1.05, 3.14]}}}


def test_config_without_new_keys_is_not_extended():
    from data.degrade import degrade_config
    for block in ({}, OLD):
        c = degrade_config(block, 8)
        assert c['extended'] is False and c['second'] is None
        assert c['sinc']['prob'] == 0.0 and c['shot']['prob'] == 0.0 and c['gray_noise'] == 0.0
    c = degrade_config(OLD, 8)
    assert c['blur'] == {'prob': 0.5, 'kernel': 7, 'sigma': (0.3, 2.0), 'anisotropic': True}
    assert c['noise'] == {'prob': 0.5, 'sigma': (1.0, 25.0)}
    assert c['jpeg'] == {'prob': 0.5, 'quality': (40, 90), 'subsampling': '4:4:4', 'given': True}
    assert c['resample'] == 'bilinear' and c['seed'] == 4 and c['l_resolution'] == 8


def test_config_full_new_set_normalises():
    from data.degrade import degrade_config
    c = degrade_config(dict(OLD, **NEW), 8)
    plain = degrade_config(OLD, 8)
    assert c['extended'] is True
    for key in ('blur', 'noise', 'jpeg', 'resample', 'seed', 'l_resolution'):
        assert c[key] == plain[key], key                                      # the old keys keep their values, whole
    assert c['sinc'] == {'prob': 0.1, 'omega': (1.05, 3.14)} and c['shot'] == {'prob': 0.5, 'scale': (0.05, 3.0)} and c['gray_noise'] == 0.4
    s = c['second']
    assert s['mid'] == (12, 40) and s['resample'] == ('box', 'bilinear', 'bicubic')
    assert s['blur'] == {'prob': 0.8, 'kernel': 5, 'sigma': (0.2, 1.5), 'anisotropic': False}
    assert s['sinc'] == {'prob': 0.2, 'omega': (1.5, math.pi)} and s['noise'] == {'prob': 0.5, 'sigma': (1.0, 10.0)}
    assert s['shot'] == {'prob': 0.3, 'scale': (0.5, 2.0)} and s['gray_noise'] == 0.25
    assert s['jpeg'] == {'prob': 1.0, 'quality': (30, 60), 'subsampling': '4:2:0', 'given': True}
    assert s['final_sinc'] == {'prob': 0.8, 'kernel': 7, 'omega': (1.05, 3.14)}
    # each new key alone extends; an empty "second" is a second round with everything off at M = L and the top-level filter
    for key in NEW:
        assert degrade_config({key: NEW[key]}, 8)['extended'] is True, key
    s = degrade_config({'second': {}, 'resample': 'bilinear'}, 8)['second']
    assert s['mid'] == (8, 8) and s['resample'] == ('bilinear',) and s['blur']['prob'] == 0.0 and s['final_sinc']['prob'] == 0.0
    assert s['jpeg']['given'] is False and s['noise']['prob'] == 0.0
    # M may exceed r_resolution; a kernel that fits the smallest mid is fine
    assert degrade_config({'second': {'mid': [4, 200], 'blur': {'kernel': 7}}}, 8)['second']['mid'] == (4, 200)


@pytest.mark.parametrize('cfg, word', [
    ({'sinc': {'omega': [1.0, 3.2]}}, 'sinc.omega'), ({'sinc': {'omega': [2.0, 1.5]}}, 'sinc.omega'), ({'sinc': {'omega': [0, 1.5]}}, 'sinc.omega'),
    ({'sinc': {'prob': 1.5}}, 'sinc.prob'), ({'sinc': {'kernel': 7}}, 'sinc.kernel'),
    ({'shot': {'scale': [0, 1]}}, 'shot.scale'), ({'shot': {'scale': [2, 1]}}, 'shot.scale'), ({'shot': {'prob': -1}}, 'shot.prob'),
    ({'gray_noise': 1.5}, 'gray_noise'), ({'gray_noise': 'x'}, 'gray_noise'),
    ({'second': {'mid': [12.0, 40]}}, 'second.mid'), ({'second': {'mid': [12, 40.5]}}, 'second.mid'), ({'second': {'mid': [0, 4]}}, 'second.mid'),
    ({'second': {'mid': [9, 8]}}, 'second.mid'), ({'second': {'mid': 12}}, 'second.mid'),
    ({'second': {'mid': [3, 40], 'blur': {'kernel': 7}}}, 'second.mid'), ({'second': {'mid': [10, 40], 'blur': {'kernel': 21}}}, 'second.mid'),
    ({'second': {'resample': []}}, 'second.resample'), ({'second': {'resample': ['box', 'lanczos']}}, 'second.resample'),
    ({'second': {'resample': ['nearest']}}, 'second.resample'), ({'second': {'resample': 'box'}}, 'second.resample'),
    ({'second': {'final_sinc': {'kernel': 6}}}, 'second.final_sinc.kernel'), ({'second': {'final_sinc': {'kernel': 17}}}, 'second.final_sinc.kernel'),
    ({'second': {'final_sinc': {'kernel': 23}}}, 'second.final_sinc.kernel'), ({'second': {'final_sinc': {'omega': [1, 4]}}}, 'second.final_sinc.omega'),
    ({'second': {'final_sinc': {'sigma': [1, 2]}}}, 'second.final_sinc.sigma'),
    ({'second': {'gray_noise': 1.5}}, 'second.gray_noise'), ({'second': {'midd': [8, 8]}}, 'second.midd'), ({'second': {'second': {}}}, 'second.second'),
    ({'second': {'blur': {'kernel': 4}}}, 'second.blur.kernel'), ({'second': {'blur': {'kernal': 3}}}, 'second.blur.kernal'),
    ({'second': {'noise': {'sigma': [5, 1]}}}, 'second.noise.sigma'), ({'second': {'jpeg': {'subsampling': '4:2:2'}}}, 'second.jpeg.subsampling'),
    ({'second': {'jpeg': {'quality': [0, 50]}}}, 'second.jpeg.quality'), ({'second': {'sinc': {'omega': [1, 3.2]}}}, 'second.sinc.omega'),
    ({'second': {'shot': {'scale': [0, 1]}}}, 'second.shot.scale'), ({'second': 3}, 'second'), ({'resample': 'nearest', 'second': {}}, 'resample'),
    ({'resample': 'box'}, 'resample'),
])
def test_config_refusals_name_the_dotted_key(cfg, word):
    from data.degrade import degrade_config
    with pytest.raises(ValueError) as e:
        degrade_config(cfg, 8)                                                # L = 8: a final-sinc kernel of 17 = 2 L + 1 reflects past it
    assert word in str(e.value), str(e.value)
    assert degrade_config({'second': {'final_sinc': {'kernel': 15}}}, 8)['second']['final_sinc']['kernel'] == 15


# ---- draws -----------------------------------------------------------------------------------------------------------------------------

HALF = {'blur': {'prob': 0.5, 'kernel': 5, 'sigma': [0.5, 2], 'anisotropic': True}, 'noise': {'prob': 0.5, 'sigma': [1, 9]},
        'jpeg': {'prob': 0.5, 'quality': [30, 95]},
        'sinc': {'prob': 0.5, 'omega': [1.05, math.pi]}, 'shot': {'prob': 0.5, 'scale': [0.05, 3.0]}, 'gray_noise': 0.5,
        'second': {'mid': [12, 40], 'resample': ['box', 'bilinear', 'bicubic'],
                   'blur': {'prob': 0.5, 'kernel': 5, 'sigma': [0.2, 1.5], 'anisotropic': True}, 'sinc': {'prob': 0.5, 'omega': [1.5, 3.0]},
                   'noise': {'prob': 0.5, 'sigma': [1, 10]}, 'shot': {'prob': 0.5, 'scale': [0.5, 2]}, 'gray_noise': 0.5,
                   'jpeg': {'prob': 0.5, 'quality': [30, 60]}, 'final_sinc': {'prob': 0.5, 'kernel': 7, 'omega': [1.05, 3.14]}}}


def _in_range(d, second):
    pi32 = float(np.float32(math.pi))
    ok = d[0] in (0, 1) and 1.05 <= d[1] <= pi32 and d[2] in (0, 1, 2, 3) and 0.05 <= d[3] <= 3.0 + 1e-6
    if not second:
        return ok and d[4] == 8 and d[5] == d[6] == 3 and all(v == 0 for v in d[7:])
    ok = ok and 12 <= d[4] <= 40 and d[4] == int(d[4]) and d[5] in (2, 3, 4) and d[6] in (2, 3, 4)
    ok = ok and d[7] in (0, 1) and 0.2 <= d[8] <= 1.5 + 1e-6 and 0.2 <= d[9] <= 1.5 + 1e-6 and 0 <= d[10] <= pi32
    ok = ok and d[11] in (0, 1) and 1.5 <= d[12] <= 3.0 + 1e-6 and (d[13] == 0 or 1 <= d[13] <= 10) and d[14] in (0, 1, 2, 3)
    ok = ok and 0.5 <= d[15] <= 2 and (d[16] == 0 or (30 <= d[16] <= 60 and d[16] == int(d[16])))
    return ok and d[17] in (0, 1) and 1.05 <= d[18] <= 3.14 + 1e-6 and d[19] in (0, 1)


def test_draw_stream():
    from data.degrade import degrade_config, draw_deg, draw_deg2
    ext = degrade_config(HALF, 8)
    old = degrade_config({k: v for k, v in HALF.items() if k in ('blur', 'noise', 'jpeg')}, 8)
    first_only = degrade_config({k: v for k, v in HALF.items() if k != 'second'}, 8)
    assert ext['extended'] and first_only['extended'] and not old['extended']
    modes1, modes2, orders, mids, filters = set(), set(), set(), set(), set()
    for seed in range(200):
        g = torch.Generator().manual_seed(seed)
        a = draw_deg(ext, g)
        assert torch.equal(a, draw_deg(old, torch.Generator().manual_seed(seed)))          # the new keys move nothing of the first draw
        b = draw_deg2(ext, g)
        assert b.dtype == torch.float32 and tuple(b.shape) == (20,) and _in_range(b.tolist(), True), b
        # seven + twenty-four draws, whatever is on: the generator stands where 31 torch.rand draws leave it
        h = torch.Generator().manual_seed(seed)
        torch.rand(7, generator=h)
        torch.rand(24, generator=h)
        assert torch.equal(torch.rand(3, generator=g), torch.rand(3, generator=h))
        g1 = torch.Generator().manual_seed(seed)
        c = draw_deg2(first_only, g1)
        assert _in_range(c.tolist(), False), c
        assert torch.equal(c[:4], draw_deg2(ext, torch.Generator().manual_seed(seed))[:4])  # round 1's numbers do not depend on "second"
        h1 = torch.Generator().manual_seed(seed)
        torch.rand(24, generator=h1)
        assert torch.equal(torch.rand(3, generator=g1), torch.rand(3, generator=h1))
        modes1.add(b[2].item()); modes2.add(b[14].item()); orders.add(b[19].item()); mids.add(b[4].item()); filters.add(b[5].item()); filters.add(b[6].item())
    assert modes1 == modes2 == {0.0, 1.0, 2.0, 3.0} and orders == {0.0, 1.0} and filters == {2.0, 3.0, 4.0}
    assert min(mids) == 12 and max(mids) == 40
    torch.manual_seed(4)
    a = draw_deg2(ext)
    torch.manual_seed(4)
    assert torch.equal(a, draw_deg2(ext))                                                    # the global generator too


def test_hr_crop_dataset_carries_deg2_only_when_extended(tmp_path):
    import data as Data
    from data.degrade import draw_deg, draw_deg2
    root = str(tmp_path / 'hr')
    write_folder(root)
    plain = Data.create_dataset(dataset_opt(root, degrade={k: v for k, v in HALF.items() if k in ('blur', 'noise', 'jpeg')}), 'train')
    ext = Data.create_dataset(dataset_opt(root, degrade=HALF), 'train')
    torch.manual_seed(3)
    a = [plain[i] for i in range(3)]
    assert all(set(it) == {'HR', 'Index', 'flip', 'deg'} for it in a)
    torch.manual_seed(3)
    b = [ext[i] for i in range(3)]
    for it in b:
        assert set(it) == {'HR', 'Index', 'flip', 'deg', 'deg2'}
        assert it['deg2'].dtype == torch.float32 and tuple(it['deg2'].shape) == (20,) and _in_range(it['deg2'].tolist(), True)
    assert torch.equal(a[0]['HR'], b[0]['HR']) and torch.equal(a[0]['deg'], b[0]['deg'])      # the first item's crop and draws do not move
    batch = torch.utils.data.default_collate(b)
    assert tuple(batch['deg2'].shape) == (3, 20) and tuple(batch['deg'].shape) == (3, 6)
    # val: seed + index governs both vectors, whatever the global generator does
    va = Data.create_dataset(dataset_opt(root, degrade=dict(HALF, seed=2)), 'val')
    x = va[1]
    torch.manual_seed(99)
    y = va[1]
    assert torch.equal(x['deg'], y['deg']) and torch.equal(x['deg2'], y['deg2']) and not torch.equal(x['deg2'], va[2]['deg2'])
    g = torch.Generator().manual_seed(2 + 1)
    assert torch.equal(x['deg'], draw_deg(va.degrade, g)) and torch.equal(x['deg2'], draw_deg2(va.degrade, g))


# ---- sinc_weights ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('k', [1, 3, 7, 13, 21])
@pytest.mark.parametrize('omega', [1.05, 2.0, 3.14, math.pi])
def test_sinc_weights_follow_the_formula(omega, k):
    from scipy.special import j1
    from data.degrade import sinc_weights
    w = sinc_weights(omega, k)
    assert w.dtype == np.int32 and w.shape == (k, k) and int(w.astype(np.int64).sum()) == 65536
    assert np.array_equal(w, w.T) and np.array_equal(w, w[::-1, ::-1])
    if k >= 7:
        assert (w < 0).any()                                                  # the ringing lobes
    # what sr3_blur_u8 documents: |w| < 2^23 (v_mad_i32_i24) and an int32 accumulator, rounding term included
    assert np.abs(w).max() < 2 ** 23 and int(np.abs(w.astype(np.int64)).sum()) * 255 + 32768 < 2 ** 31
    h = np.zeros((k, k))
    for iy in range(k):
        for ix in range(k):
            r = math.sqrt((ix - k // 2) ** 2 + (iy - k // 2) ** 2)
            h[iy, ix] = omega * omega / (4 * math.pi) if r == 0 else omega * float(j1(omega * r)) / (2 * math.pi * r)
    q = np.floor(h / h.sum() * 65536 + 0.5).astype(np.int64)
    q[k // 2, k // 2] += 65536 - q.sum()
    assert np.array_equal(w.astype(np.int64), q)


def test_sinc_weights_refusals():
    from data.degrade import sinc_weights
    for k in (0, 2, 8, 23):
        with pytest.raises(ValueError, match='k'):
            sinc_weights(2.0, k)
    for om in (0.0, -1.0, 3.1416, 4.0):
        with pytest.raises(ValueError, match='omega'):
            sinc_weights(om, 7)


# ---- poisson_table ---------------------------------------------------------------------------------------------------------------------

def test_poisson_table():
    from scipy.stats import poisson
    from data.degrade import poisson_table
    T = poisson_table()
    assert T.shape == (256, 384) and T.dtype == np.int32
    t = T.astype(np.int64)
    assert (np.diff(t, axis=1) >= 0).all() and (t >= 0).all() and (t[0] == 2 ** 31 - 1).all() and (t[:, -1] == 2 ** 31 - 1).all()
    assert int(np.argmax(t[255] == 2 ** 31 - 1)) == 359
    ref = np.minimum(np.floor(poisson.cdf(np.arange(384)[None, :], np.arange(256)[:, None]) * 2.0 ** 31), 2.0 ** 31 - 1).astype(np.int64)
    assert np.array_equal(t, ref)
    # a draw is k = #{j : T[v][j] <= r}, r uniform over the 2^31 - 1 integers of [0, 2^31 - 1): P(k <= j) = T[v][j] / (2^31 - 1) exactly
    cdf = t / float(2 ** 31 - 1)
    pmf = np.diff(np.concatenate([np.zeros((256, 1)), cdf], axis=1), axis=1)
    j, lam = np.arange(384, dtype=np.float64), np.arange(256, dtype=np.float64)
    mean = (pmf * j).sum(1)
    var = (pmf * j * j).sum(1) - mean ** 2
    print('poisson_table: max |mean - lambda| %.3g, max |var - lambda| %.3g' % (np.abs(mean - lam).max(), np.abs(var - lam).max()))
    assert np.abs(mean - lam).max() <= 1e-6 and np.abs(var - lam).max() <= 1e-4
    # the draw itself, at the ends of r
    assert poisson_draw(T, np.array([0, 0, 255, 255, 7]), np.array([0, 2 ** 31 - 2, 0, 2 ** 31 - 2, 2 ** 30])).tolist() == [0, 0, 164, 359, 7]
    assert poisson_table() is T and not T.flags.writeable


def test_noise_ex_oracle_modes():
    from data.degrade import poisson_table
    T = poisson_table()
    img = np.array([[[0, 0, 0], [255, 255, 255], [10, 200, 30], [100, 100, 100]]], np.uint8)
    z = np.array([[[1, -1, 2], [1, 1, 1], [0.5, 9, 9], [-3, 0, 0]]], np.float32)
    r = np.full((1, 4, 3), 2 ** 30, np.int32)
    assert np.array_equal(noise_ex_oracle(img, 0, 0.0, z, r, T), img) and np.array_equal(noise_ex_oracle(img, 3, 0.0, z, r, T), img)
    assert np.array_equal(noise_ex_oracle(img, 0, 2.0, z, r, T), noise_oracle(img, 2.0, z))
    g = noise_ex_oracle(img, 1, 2.0, z, r, T)
    assert g.tolist() == [[[2, 2, 2], [255, 255, 255], [11, 201, 31], [94, 94, 94]]]
    p = noise_ex_oracle(img, 2, 1.0, z, r, T)
    assert p[0, 0].tolist() == [0, 0, 0]                                      # lambda 0: k = 0
    k = poisson_draw(T, img.astype(np.int64), r)
    assert np.array_equal(p, np.clip(k, 0, 255).astype(np.uint8))             # scale 1: the byte becomes the draw
    pg = noise_ex_oracle(img, 3, 2.0, z, r, T)
    Y = 124                                                                   # (19595 * 10 + 38470 * 200 + 7471 * 30 + 32768) >> 16
    d = 2 * (int(poisson_draw(T, np.array(Y), np.array(2 ** 30))) - Y)
    assert pg[0, 2].tolist() == [10 + d, 200 + d, 30 + d] and pg[0, 0].tolist() == [0, 0, 0]
    one = img[:, :, :1]
    assert np.array_equal(noise_ex_oracle(one, 3, 1.5, z[:, :, :1], r[:, :, :1], T), noise_ex_oracle(one, 2, 1.5, z[:, :, :1], r[:, :, :1], T))
    assert np.array_equal(noise_ex_oracle(one, 1, 1.5, z[:, :, :1], r[:, :, :1], T), noise_ex_oracle(one, 0, 1.5, z[:, :, :1], r[:, :, :1], T))


# ---- the C entry's refusals: before any launch, so no device is needed -------------------------------------------------------------------

def _p(v):
    return C.c_void_p(v)


# 2 x 16 x 20 x 3 = 1920 bytes per buffer
NOISE_EX_OK = dict(inp=_p(1 << 20), n=2, H=16, W=20, C=3, mode=_p(1 << 12), s=_p(1 << 13), z=_p(1 << 24), r=_p(1 << 25), table=_p(1 << 26),
                   kmax=384, out=_p(1 << 22))
NOISE_EX_REFUSALS = [
    (dict(inp=None), 'in_hwc'), (dict(mode=None), 'mode'), (dict(s=None), 'strength'), (dict(out=None), 'out_hwc'),
    (dict(n=0), 'n_images'), (dict(n=-2), 'n_images'), (dict(n=65536), 'n_images'), (dict(H=0), 'H 0'), (dict(W=-3), 'W -3'),
    (dict(C=2), 'C 2'), (dict(C=4), 'C 4'), (dict(kmax=0), 'kmax 0'), (dict(kmax=1025), 'kmax 1025'), (dict(kmax=-1), 'kmax -1'),
    (dict(n=16, H=8192, W=8192, out=_p(1 << 40)), '2^31'),
    (dict(out=_p((1 << 20) + 100)), 'out_hwc'), (dict(out=_p((1 << 20) - 100)), 'out_hwc'),
]


@pytest.mark.parametrize('kw, word', NOISE_EX_REFUSALS)
def test_noise_ex_u8_refusals_no_gpu(kw, word):
    from sr3_hip import lib as L
    lib = L.load()
    a = dict(NOISE_EX_OK, **kw)
    rc = lib.sr3_noise_ex_u8(a['inp'], a['n'], a['H'], a['W'], a['C'], a['mode'], a['s'], a['z'], a['r'], a['table'], a['kmax'], a['out'], None)
    assert rc == -1, kw                                                       # refused: nothing was launched (no device here)
    msg = lib.sr3_last_error().decode()
    assert msg.startswith('noise_ex_u8') and word in msg, (kw, msg)


def test_noise_ex_u8_refusal_order():
    """pointers, then sizes, then C, then the overlap -- sr3_noise_u8's order: the first offence is the one named"""
    from sr3_hip import lib as L
    lib = L.load()
    for kw, word in ((dict(inp=None, n=0, C=2), 'in_hwc'), (dict(out=None, n=0), 'out_hwc'), (dict(n=0, C=2), 'n_images'),
                     (dict(H=0, C=2, kmax=0), 'H 0'), (dict(C=2, kmax=0, out=_p((1 << 20) + 4)), 'C 2'), (dict(kmax=0, out=_p((1 << 20) + 4)), 'kmax')):
        a = dict(NOISE_EX_OK, **kw)
        assert lib.sr3_noise_ex_u8(a['inp'], a['n'], a['H'], a['W'], a['C'], a['mode'], a['s'], a['z'], a['r'], a['table'], a['kmax'], a['out'],
                                   None) == -1
        assert word in lib.sr3_last_error().decode(), (kw, lib.sr3_last_error().decode())


def test_noise_ex_batch_and_resize_batch_check_before_the_device():
    import data.prepare_data as P
    from data.degrade import noise_ex_batch
    from sr3_hip import lib as L
    a = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(TypeError, match='noise_ex_batch'):
        noise_ex_batch(a, torch.zeros(2, dtype=torch.int32), torch.zeros(2))      # host tensors: no CPU fallback
    with pytest.raises(NotImplementedError):
        P.resize_batch(a, (4, 4), Image.NEAREST)
    assert P._RESAMPLE[Image.BOX] == 4
    if not torch.cuda.is_available():                                         # BOX passes the filter check and reaches the device check
        with pytest.raises(L.Sr3Error, match='no CPU fallback'):
            P.resize_batch(a, (4, 4), Image.BOX)
