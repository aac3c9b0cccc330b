"""Training from an HR-only folder, the parts that need no GPU: the blur weights, the config's one validation,
HRCropDataset / create_dataset, and the argument refusals of sr3_blur_u8 / sr3_noise_u8 (checked before anything is launched).
The NumPy restatements of the two kernels live here (blur_oracle, noise_oracle, degrade_oracle); tests/test_gpu_degrade.py compares
the device against them bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from PIL import Image

FOLDER_SIZES = [(40, 56), (32, 32), (64, 48)]         # (H, W) of the test folder's PNGs


# ---- oracles ---------------------------------------------------------------------------------------------------------------------------

def blur_oracle(img, w):
    """(H, W, C) uint8, (k, k) int32 16-bit fixed point -> correlation over np.pad(mode='reflect'), (acc + 32768) >> 16, clamp."""
    k = w.shape[0]
    r = k // 2
    H, Wd = img.shape[:2]
    p = np.pad(img.astype(np.int64), ((r, r), (r, r), (0, 0)), mode='reflect')
    acc = np.zeros(img.shape, dtype=np.int64)
    for dy in range(k):
        for dx in range(k):
            acc += int(w[dy, dx]) * p[dy:dy + H, dx:dx + Wd]
    assert np.abs(acc).max() < 2 ** 31 - 32768           # the device accumulates in int32
    return np.clip((acc + 32768) >> 16, 0, 255).astype(np.uint8)


def noise_oracle(img, sigma, z):
    """t = sigma * z and v = img + t, each one fp32 rounding; rint (half to even); clamp."""
    t = np.float32(sigma) * z.astype(np.float32)
    v = img.astype(np.float32) + t
    assert t.dtype == np.float32 and v.dtype == np.float32
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def pil_resize(img, hw, resample):
    a = img[:, :, 0] if img.shape[2] == 1 else img
    r = np.asarray(Image.fromarray(a).resize((hw[1], hw[0]), resample))
    return r[:, :, None] if r.ndim == 2 else r


def degrade_oracle(hr, deg, cfg, z=None):
    """One image through the chain: NumPy blur -> Pillow down -> NumPy noise -> Pillow up.  deg: the five numbers (float64)."""
    from data.degrade import blur_weights
    rs = {'bicubic': Image.BICUBIC, 'bilinear': Image.BILINEAR}[cfg['resample']]
    x = hr
    if deg[0] != 0:
        x = blur_oracle(x, blur_weights(deg[1], deg[2], deg[3], cfg['blur']['kernel']))
    lr = pil_resize(x, (cfg['l_resolution'],) * 2, rs)
    if deg[4] != 0:
        lr = noise_oracle(lr, np.float32(deg[4]), z)
    return lr, pil_resize(lr, hr.shape[:2], rs)


def write_folder(root, sizes=FOLDER_SIZES, seed=3):
    """PNGs 0.png, 1.png, ... of the given (H, W): smooth structure plus noise, so crops differ and resizes are not trivial."""
    os.makedirs(root, exist_ok=True)
    rng = np.random.RandomState(seed)
    imgs = []
    for i, (h, w) in enumerate(sizes):
        yy, xx = np.mgrid[0:h, 0:w]
        base = 127 + 90 * np.sin(yy / 5.0 + i)[:, :, None] * np.cos(xx / 7.0)[:, :, None] * np.ones((1, 1, 3))
        a = np.clip(base + rng.randn(h, w, 3) * 25, 0, 255).astype(np.uint8)
        Image.fromarray(a).save(os.path.join(root, '%d.png' % i))
        imgs.append(a)
    return imgs


def dataset_opt(root, **kw):
    opt = dict(name='t', mode='HR', dataroot=root, datatype='img', l_resolution=8, r_resolution=32, data_len=-1, batch_size=4,
               use_shuffle=False, num_workers=0, degrade={})
    opt.update(kw)
    return opt


# ---- blur_weights ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('k', [1, 3, 7, 21])
@pytest.mark.parametrize('sigma', [0.2, 1, 3, 10])
def test_blur_weights_sum_symmetry(sigma, k):
    from data.degrade import blur_weights
    for theta in (0, 0.7):
        for sy in (sigma, 2.5 * sigma):
            w = blur_weights(sigma, sy, theta, k)
            assert w.dtype == np.int32 and w.shape == (k, k)
            assert int(w.astype(np.int64).sum()) == 65536
            assert (w >= 0).all() and np.array_equal(w, w[::-1, ::-1])
    # a circle does not turn
    assert np.array_equal(blur_weights(sigma, sigma, 0.7, k), blur_weights(sigma, sigma, 0, k))
    assert np.array_equal(blur_weights(sigma, sigma, 0, k), blur_weights(sigma, sigma, 0, k).T)
    if k > 1 and sigma >= 1:        # ... and an ellipse does
        assert not np.array_equal(blur_weights(sigma, 2.5 * sigma, 0.7, k), blur_weights(sigma, 2.5 * sigma, 0, k))


def test_blur_weights_off_is_the_delta_and_refusals():
    from data.degrade import blur_weights
    for k in (1, 3, 21):
        w = blur_weights(2.0, 2.0, 0.0, k, on=False)
        ref = np.zeros((k, k), np.int32)
        ref[k // 2, k // 2] = 65536
        assert w.dtype == np.int32 and np.array_equal(w, ref)
    assert np.array_equal(blur_weights(5.0, 1.0, 0.3, 1), [[65536]])
    for k in (0, 2, 23):
        with pytest.raises(ValueError, match='k'):
            blur_weights(1.0, 1.0, 0.0, k)
    with pytest.raises(ValueError, match='sigma'):
        blur_weights(0.0, 1.0, 0.0, 3)


def test_blur_weights_follow_the_formula():
    """an independent restatement, tap by tap, for a rotated ellipse"""
    import math
    from data.degrade import blur_weights
    sx, sy, th, k = 2.0, 0.8, 0.7, 7
    w = np.zeros((k, k))
    for iy in range(k):
        for ix in range(k):
            dx, dy = ix - 3, iy - 3
            u, v = math.cos(th) * dx + math.sin(th) * dy, -math.sin(th) * dx + math.cos(th) * dy
            w[iy, ix] = math.exp(-0.5 * (u * u / sx ** 2 + v * v / sy ** 2))
    q = np.floor(w / w.sum() * 65536 + 0.5).astype(np.int64)
    q[3, 3] += 65536 - q.sum()
    got = blur_weights(sx, sy, th, k).astype(np.int64)
    assert np.abs(got - q).max() <= 1 and got.sum() == 65536          # (libm vs NumPy exp: a tap may sit on a rounding edge)


# ---- the NumPy oracles themselves ------------------------------------------------------------------------------------------------------

def test_blur_oracle_constant_and_delta():
    from data.degrade import blur_weights
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, size=(16, 20, 3)).astype(np.uint8)
    full = np.full((16, 20, 3), 255, np.uint8)
    for k in (1, 3, 7, 21):
        for w in (blur_weights(1.7, 1.7, 0, k), blur_weights(3.0, 0.6, 0.7, k)):
            assert np.array_equal(blur_oracle(full, w), full)
            assert np.array_equal(blur_oracle(np.zeros_like(full), w), np.zeros_like(full))
        assert np.array_equal(blur_oracle(img, blur_weights(1.0, 1.0, 0, k, on=False)), img)
    # reflect-101: the border pixel is not repeated
    row = np.repeat(np.array([10, 20, 30, 40], np.uint8).reshape(1, 4, 1), 3, 0)
    w = np.zeros((3, 3), np.int32)
    w[1, 0] = 65536                                                       # out[x] = in[reflect(x - 1)]
    assert blur_oracle(row, w)[0, :, 0].tolist() == [20, 10, 20, 30]


def test_noise_oracle_ties_and_clamp():
    img = np.array([0, 1, 2, 3, 254, 255, 100, 7], np.uint8)
    z = np.array([1, 1, -1, -1, 1e3, -1e3, 0.3, 1], np.float32)
    assert noise_oracle(img, 0.5, z).tolist() == [0, 2, 2, 2, 255, 0, 100, 8]      # x.5 rounds to even
    assert np.array_equal(noise_oracle(img, 0.0, z), img)


# ---- config ----------------------------------------------------------------------------------------------------------------------------

def test_degrade_config_defaults_and_full_set():
    from data.degrade import degrade_config
    c = degrade_config({}, 8)
    assert c['blur']['prob'] == 0.0 and c['noise']['prob'] == 0.0 and c['resample'] == 'bicubic' and c['seed'] == 0
    assert c['l_resolution'] == 8 and c['blur']['kernel'] % 2 == 1 and c['blur']['anisotropic'] is False
    full = {'blur': {'prob': 0.5, 'kernel': 7, 'sigma': [0.3, 2], 'anisotropic': True}, 'noise': {'prob': 1, 'sigma': [0, 25]},
            'resample': 'bilinear', 'seed': 4}
    c = degrade_config(full, 16)
    assert c['blur'] == {'prob': 0.5, 'kernel': 7, 'sigma': (0.3, 2.0), 'anisotropic': True}
    assert c['noise'] == {'prob': 1.0, 'sigma': (0.0, 25.0)} and c['resample'] == 'bilinear' and c['seed'] == 4
    assert degrade_config({'noise': {'sigma': [3, 3]}}, 8)['noise'] == {'prob': 1.0, 'sigma': (3.0, 3.0)}


@pytest.mark.parametrize('cfg, word', [
    ({'blurr': {}}, 'blurr'), ({'blur': {'kernal': 3}}, 'blur.kernal'), ({'noise': {'kernel': 3}}, 'noise.kernel'), ({'jpeg': 3}, 'jpeg'),
    ({'blur': {'kernel': 4}}, 'blur.kernel'), ({'blur': {'kernel': 23}}, 'blur.kernel'), ({'blur': {'kernel': 0}}, 'blur.kernel'),
    ({'blur': {'kernel': 3.0}}, 'blur.kernel'),
    ({'blur': {'sigma': [0, 1]}}, 'blur.sigma'), ({'blur': {'sigma': [2, 1]}}, 'blur.sigma'), ({'blur': {'sigma': [-1, 1]}}, 'blur.sigma'),
    ({'blur': {'sigma': 2}}, 'blur.sigma'), ({'blur': {'sigma': [1, 2, 3]}}, 'blur.sigma'),
    ({'noise': {'sigma': [-0.1, 1]}}, 'noise.sigma'), ({'noise': {'sigma': [5, 1]}}, 'noise.sigma'),
    ({'blur': {'prob': 1.5}}, 'blur.prob'), ({'blur': {'prob': -0.1}}, 'blur.prob'), ({'noise': {'prob': 2}}, 'noise.prob'),
    ({'noise': {'prob': 'x'}}, 'noise.prob'), ({'blur': {'anisotropic': 1}}, 'blur.anisotropic'),
    ({'resample': 'nearest'}, 'resample'), ({'seed': 1.5}, 'seed'), ({'blur': 3}, 'blur'),
])
def test_degrade_config_refusals(cfg, word):
    from data.degrade import degrade_config
    with pytest.raises(ValueError) as e:
        degrade_config(cfg, 8)
    assert word in str(e.value), str(e.value)


def test_draw_deg_ranges_and_isotropy():
    from data.degrade import degrade_config, draw_deg
    iso = degrade_config({'blur': {'prob': 0.5, 'kernel': 5, 'sigma': [0.5, 2]}, 'noise': {'prob': 0.5, 'sigma': [1, 9]}}, 8)
    ani = degrade_config({'blur': {'sigma': [0.5, 2], 'anisotropic': True}}, 8)
    torch.manual_seed(0)
    on = set()
    for _ in range(40):
        d = draw_deg(iso)
        assert d.dtype == torch.float32 and tuple(d.shape) == (5,)
        b, sx, sy, th, ns = d.tolist()
        assert b in (0.0, 1.0) and 0.5 <= sx <= 2 and sy == sx and th == 0 and (ns == 0 or 1 <= ns <= 9)
        on.add((b, ns != 0))
        b, sx, sy, th, ns = draw_deg(ani).tolist()
        assert b == 1.0 and 0.5 <= sy <= 2 and 0 <= th <= 3.1416 and ns == 0
    assert len(on) == 4
    g = torch.Generator().manual_seed(5)
    a = draw_deg(ani, g)
    assert torch.equal(a, draw_deg(ani, torch.Generator().manual_seed(5))) and not torch.equal(a, draw_deg(ani, g))


# ---- dataset ---------------------------------------------------------------------------------------------------------------------------

def test_hr_crop_dataset_items(tmp_path):
    import data as Data
    from data.HR_dataset import HRCropDataset
    root = str(tmp_path / 'hr')
    imgs = write_folder(root)
    cfg = {'blur': {'prob': 0.5, 'kernel': 7, 'sigma': [0.5, 2], 'anisotropic': True}, 'noise': {'prob': 0.5, 'sigma': [1, 9]}, 'seed': 2}
    tr = Data.create_dataset(dataset_opt(root, degrade=cfg), 'train')
    assert isinstance(tr, HRCropDataset) and len(tr) == 3 and tr.degrade['blur']['kernel'] == 7 and tr.need_LR is False
    assert Data.create_dataset(dataset_opt(root, mode='LRHR'), 'train').need_LR is True
    torch.manual_seed(8)
    a = [tr[i] for i in range(3)]
    for i, it in enumerate(a):
        assert set(it) == {'HR', 'Index', 'flip', 'deg'} and it['Index'] == i and isinstance(it['flip'], bool)
        assert it['HR'].dtype == torch.uint8 and tuple(it['HR'].shape) == (32, 32, 3) and it['HR'].is_contiguous()
        assert it['deg'].dtype == torch.float32 and tuple(it['deg'].shape) == (5,)
        H, W = FOLDER_SIZES[i]
        hits = [(t, l) for t in range(H - 31) for l in range(W - 31) if np.array_equal(imgs[i][t:t + 32, l:l + 32], it['HR'].numpy())]
        assert len(hits) == 1                                            # a crop of its own file
    torch.manual_seed(8)
    b = [tr[i] for i in range(3)]
    for x, y in zip(a, b):
        assert torch.equal(x['HR'], y['HR']) and x['flip'] == y['flip'] and torch.equal(x['deg'], y['deg'])
    torch.manual_seed(9)
    c = [tr[i] for i in range(3)]
    assert any(not torch.equal(x['deg'], y['deg']) for x, y in zip(a, c))
    # val: the centre crop, no flip, draws fixed by seed + index -- whatever the global generator does
    va = Data.create_dataset(dataset_opt(root, degrade=cfg), 'val')
    p1 = [va[i] for i in range(3)]
    torch.manual_seed(123)
    p2 = [va[i] for i in range(3)]
    for i, (x, y) in enumerate(zip(p1, p2)):
        H, W = FOLDER_SIZES[i]
        t, l = (H - 32) // 2, (W - 32) // 2
        assert np.array_equal(x['HR'].numpy(), imgs[i][t:t + 32, l:l + 32]) and x['flip'] is False
        assert torch.equal(x['HR'], y['HR']) and torch.equal(x['deg'], y['deg'])
    assert not torch.equal(p1[0]['deg'], p1[1]['deg'])
    other = Data.create_dataset(dataset_opt(root, degrade=dict(cfg, seed=3)), 'val')
    assert torch.equal(other[0]['deg'], p1[1]['deg'])                   # seed + index
    assert len(Data.create_dataset(dataset_opt(root, data_len=2), 'val')) == 2
    # the default collate keeps what DeviceBatches reads
    batch = torch.utils.data.default_collate(a)
    assert tuple(batch['HR'].shape) == (3, 32, 32, 3) and tuple(batch['deg'].shape) == (3, 5) and batch['flip'].dtype == torch.bool


def test_hr_crop_dataset_refusals(tmp_path):
    import data as Data
    root = str(tmp_path / 'hr')
    write_folder(root)
    ds = Data.create_dataset(dataset_opt(root, r_resolution=48, l_resolution=12), 'train')
    with pytest.raises(ValueError, match='0.png'):
        ds[0]                                                            # 40 x 56 < 48
    assert tuple(ds[2]['HR'].shape) == (48, 48, 3)
    with pytest.raises(NotImplementedError, match='lmdb'):
        Data.create_dataset(dataset_opt(root, datatype='lmdb'), 'train')
    with pytest.raises(ValueError, match='blur.kernel'):
        Data.create_dataset(dataset_opt(root, degrade={'blur': {'kernel': 8}}), 'train')
    with pytest.raises(ValueError, match='jpeg'):
        Data.create_dataset(dataset_opt(root, degrade={'jpeg': 1}), 'val')


def test_block_without_degrade_still_builds_lrhr_dataset(tmp_path):
    import data as Data
    from data.LRHR_dataset import LRHRDataset
    from test_oracle_io import _write_triplets
    root = str(tmp_path / 'ds')
    _write_triplets(root, 2, l=8, r=32)
    opt = dataset_opt(root)
    del opt['degrade']
    ds = Data.create_dataset(opt, 'train')
    assert type(ds) is LRHRDataset and set(ds[0]) == {'HR', 'SR', 'Index', 'flip'}


def test_lr_folder_dataset(tmp_path):
    import data as Data
    from data.HR_dataset import LRFolderDataset
    root = str(tmp_path / 'lr')
    imgs = write_folder(root, [(8, 12), (8, 8)])
    ds = Data.create_dataset(dataset_opt(root, mode='LR', l_resolution=4, r_resolution=16), 'val')
    assert isinstance(ds, LRFolderDataset) and len(ds) == 2 and ds.lr_scale == 4 and ds.resample == 'bicubic'
    assert set(ds[0]) == {'LR', 'Index'} and np.array_equal(ds[0]['LR'].numpy(), imgs[0]) and tuple(ds[1]['LR'].shape) == (8, 8, 3)
    with pytest.raises(NotImplementedError):
        Data.create_dataset(dataset_opt(root, mode='LR'), 'train')
    with pytest.raises(ValueError, match='r_resolution'):
        Data.create_dataset(dataset_opt(root, mode='LR', l_resolution=5, r_resolution=16), 'val')


# ---- the C entries' refusals: before any launch, so no device is needed -----------------------------------------------------------------

def _p(v):
    return C.c_void_p(v)


BLUR_OK = dict(inp=_p(1 << 20), n=2, H=16, W=20, C=3, w=_p(1 << 16), k=7, out=_p(1 << 21))
BLUR_REFUSALS = [
    (dict(inp=None), 'in_hwc'), (dict(w=None), 'weights'), (dict(out=None), 'out_hwc'), (dict(n=0), 'n_images'), (dict(H=0), 'H 0'),
    (dict(W=-1), 'W -1'), (dict(C=2), 'C 2'), (dict(C=4), 'C 4'), (dict(k=4), 'k 4'), (dict(k=0), 'k 0'), (dict(k=-3), 'k -3'),
    (dict(k=23), 'k 23'), (dict(k=21, H=10), 'k 21'), (dict(k=21, W=10), 'k 21'), (dict(k=3, H=1), 'k 3'),
    (dict(out=_p(1 << 20)), 'out_hwc'), (dict(out=_p((1 << 20) + 100)), 'out_hwc'),
]


@pytest.mark.parametrize('kw, word', BLUR_REFUSALS)
def test_blur_u8_refusals_no_gpu(kw, word):
    from sr3_hip import lib as L
    lib = L.load()
    a = dict(BLUR_OK, **kw)
    assert lib.sr3_blur_u8(a['inp'], a['n'], a['H'], a['W'], a['C'], a['w'], a['k'], a['out'], None) == -1, kw
    msg = lib.sr3_last_error().decode()
    assert msg.startswith('blur_u8') and word in msg, (kw, msg)


NOISE_OK = dict(inp=_p(1 << 20), n=2, per=768, sigma=_p(1 << 12), z=_p(1 << 24), out=_p(1 << 22))
NOISE_REFUSALS = [
    (dict(inp=None), ' in '), (dict(sigma=None), 'sigma'), (dict(z=None), ' z '), (dict(out=None), ' out '), (dict(n=0), 'n_images'),
    (dict(n=-2), 'n_images'), (dict(per=0), 'elems_per_image'), (dict(out=_p((1 << 20) + 4)), ' out '),
]


@pytest.mark.parametrize('kw, word', NOISE_REFUSALS)
def test_noise_u8_refusals_no_gpu(kw, word):
    from sr3_hip import lib as L
    lib = L.load()
    a = dict(NOISE_OK, **kw)
    assert lib.sr3_noise_u8(a['inp'], a['n'], a['per'], a['sigma'], a['z'], a['out'], None) == -1, kw
    msg = lib.sr3_last_error().decode()
    assert msg.startswith('noise_u8') and word in msg, (kw, msg)


def test_degrade_batch_refuses_a_raw_dict_and_has_no_cpu_fallback():
    from data.degrade import degrade_batch, degrade_config
    from sr3_hip import lib as L
    hr = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(TypeError):
        degrade_batch(hr, torch.zeros(1, 5), {})
    if not torch.cuda.is_available():
        with pytest.raises(L.Sr3Error, match='no CPU fallback'):
            degrade_batch(hr, torch.zeros(1, 5), degrade_config({}, 2))
