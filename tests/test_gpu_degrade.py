"""Training from an HR-only folder on the GPU: sr3_blur_u8 and sr3_noise_u8 against the NumPy restatements of
tests/test_degrade_cpu.py, degrade_batch against NumPy + Pillow, the loader end to end, one training step on the tiny model, and
"mode": "LR".  Every comparison is bit-exact: the blur is integer arithmetic, the noise is one rounding per operation, the resizes
are Pillow-exact."""
import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from helpers import load_golden, opt_for                                                     # noqa: E402
from oracle import io_metrics_oracle as O                                                    # noqa: E402
from test_degrade_cpu import (FOLDER_SIZES, blur_oracle, dataset_opt, degrade_oracle, noise_oracle, pil_resize,   # noqa: E402
                              write_folder)

RS = {'bicubic': Image.BICUBIC, 'bilinear': Image.BILINEAR}


@pytest.fixture(autouse=True)
def _load_in_process(monkeypatch):
    """The validation loader forks one worker; forking a process with a live HIP context takes tens of seconds on the GPU box.  Load
    in-process here: the batches are the same."""
    import torch.utils.data as _tud
    _DL = _tud.DataLoader
    monkeypatch.setattr(_tud, 'DataLoader', lambda *a, **k: _DL(*a, **dict(k, num_workers=0)))


def _images(n, H, W, C, seed):
    """random bytes; the top half of every image a 0 / 255 checkerboard (the extremes next to each other)"""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, size=(n, H, W, C)).astype(np.uint8)
    yy, xx = np.mgrid[0:H // 2, 0:W]
    a[:, :H // 2] = (((yy + xx) % 2) * 255).astype(np.uint8)[None, :, :, None]
    return a


def _three_kernels(k):
    """image 0: the delta, image 1: isotropic, image 2: a rotated ellipse"""
    from data.degrade import blur_weights
    return np.stack([blur_weights(1.0, 1.0, 0.0, k, on=False), blur_weights(1.3, 1.3, 0.0, k), blur_weights(4.0, 0.7, 0.7, k)])


@pytest.mark.parametrize('C', [3, 1])
@pytest.mark.parametrize('hw', [(16, 16), (20, 37), (128, 128)])
def test_blur_u8_matches_the_integer_oracle(hw, C):
    from data.degrade import blur_batch
    H, W = hw
    a = _images(3, H, W, C, seed=H + W + C)
    full = np.full((3, H, W, C), 255, np.uint8)
    for k in (1, 3, 7, 21):
        w = _three_kernels(k)
        wd = torch.from_numpy(w).cuda()
        got = blur_batch(torch.from_numpy(a).cuda(), wd).cpu().numpy()
        for i in range(3):
            assert np.array_equal(got[i], blur_oracle(a[i], w[i])), (hw, C, k, i)
        assert np.array_equal(got[0], a[0])
        if k > 1:
            assert not np.array_equal(got[1], a[1]) and not np.array_equal(got[2], a[2])
        assert np.array_equal(blur_batch(torch.from_numpy(full).cuda(), wd).cpu().numpy(), full), (hw, C, k)
        # the delta image is skipped inside the kernel; the same kernels in another order give the same images
        perm = [2, 0, 1]
        got_p = blur_batch(torch.from_numpy(a[perm]).cuda(), torch.from_numpy(w[perm]).cuda()).cpu().numpy()
        assert np.array_equal(got_p, got[perm])


def test_noise_u8_matches_numpy_fp32():
    from data.degrade import noise_batch
    rng = np.random.RandomState(1)
    a = rng.randint(0, 256, size=(3, 16, 16, 3)).astype(np.uint8)
    sigma = np.array([0.0, 0.5, 25.0], np.float32)
    z = rng.randn(3, 16, 16, 3).astype(np.float32)
    z[1] = np.where(rng.rand(16, 16, 3) < 0.5, 1.0, -1.0)           # exact ties x.5 at sigma 0.5
    z[2, 0] = 40.0                                                    # + 1000 levels: clamps at 255
    z[2, 1] = -40.0                                                   # clamps at 0
    a[1, 0, :8] = np.arange(8, dtype=np.uint8)[:, None]              # ties at both parities, down at 0
    a[1, 1, :8] = (255 - np.arange(8, dtype=np.uint8))[:, None]
    ref = np.stack([noise_oracle(a[i], sigma[i], z[i]) for i in range(3)])
    assert np.array_equal(ref[0], a[0]) and (ref[2, 0] == 255).all() and (ref[2, 1] == 0).all()
    assert ((ref[1] % 2 == 0) | (a[1] == 255)).all()                 # every tie went to the even neighbour (255.5 -> 256 clamps)
    ad, sd, zd = torch.from_numpy(a).cuda(), torch.from_numpy(sigma).cuda(), torch.from_numpy(z).cuda()
    out = noise_batch(ad, sd, zd)
    assert np.array_equal(out.cpu().numpy(), ref) and np.array_equal(ad.cpu().numpy(), a)
    same = noise_batch(ad, sd, zd, out=ad)                           # in place
    assert same.data_ptr() == ad.data_ptr() and np.array_equal(ad.cpu().numpy(), ref)


@pytest.mark.parametrize('resample', ['bicubic', 'bilinear'])
@pytest.mark.parametrize('R, Lr', [(32, 8), (128, 16)])
def test_degrade_batch_plain_is_the_prepare_data_pair(R, Lr, resample):
    """{}: LR = Image.resize down, SR = Image.resize of that back up -- what prepare_data.py writes for the crop"""
    from data.degrade import degrade_batch, degrade_config
    cfg = degrade_config({'resample': resample}, Lr)
    hr = _images(3, R, R, 3, seed=R)
    deg = torch.tensor([[0.0, 1.0, 1.0, 0.0, 0.0]] * 3)
    lr, sr = degrade_batch(torch.from_numpy(hr), deg, cfg)
    assert lr.is_cuda and lr.dtype == torch.uint8 and tuple(lr.shape) == (3, Lr, Lr, 3) and tuple(sr.shape) == (3, R, R, 3)
    for i in range(3):
        ref_lr = np.asarray(Image.fromarray(hr[i]).resize((Lr, Lr), RS[resample]))
        assert np.array_equal(lr[i].cpu().numpy(), ref_lr)
        assert np.array_equal(sr[i].cpu().numpy(), np.asarray(Image.fromarray(ref_lr).resize((R, R), RS[resample])))


def test_degrade_batch_everything_on_matches_the_composed_oracle():
    from data.degrade import degrade_batch, degrade_config
    R, Lr, n = 32, 8, 5
    cfg = degrade_config({'blur': {'kernel': 7, 'sigma': [0.3, 3], 'anisotropic': True}, 'noise': {'sigma': [1, 30]}}, Lr)
    hr = _images(n, R, R, 3, seed=11)
    # [blur_on, sigma_x, sigma_y, theta, noise_sigma]: all on; blur only; noise only; neither; another pair
    deg = torch.tensor([[1, 2.0, 0.6, 0.7, 12.5], [1, 1.1, 1.1, 0.0, 0.0], [0, 1.0, 1.0, 0.0, 30.0], [0, 1.0, 1.0, 0.0, 0.0],
                        [1, 0.3, 3.0, 2.9, 1.0]], dtype=torch.float32)
    z = torch.randn(n, Lr, Lr, 3, generator=torch.Generator().manual_seed(3))
    lr, sr = degrade_batch(torch.from_numpy(hr).cuda(), deg, cfg, z=z)
    d64 = deg.double().numpy()
    for i in range(n):
        ref_lr, ref_sr = degrade_oracle(hr[i], d64[i], cfg, z[i].numpy())
        assert np.array_equal(lr[i].cpu().numpy(), ref_lr), i
        assert np.array_equal(sr[i].cpu().numpy(), ref_sr), i
    plain = degrade_oracle(hr[0], d64[3], cfg)[1]
    assert not np.array_equal(sr[0].cpu().numpy(), plain) and np.array_equal(sr[3].cpu().numpy(), degrade_oracle(hr[3], d64[3], cfg)[1])
    with pytest.raises(ValueError, match='shape'):
        degrade_batch(torch.from_numpy(hr), deg, cfg, z=z[:, :4])


# ---- the loader, end to end ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def folder(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('hr_folder'))
    return root, write_folder(root)


def _f32(u8, flip):
    return O.transform_augment([u8], 'train', (-1, 1), flip=flip)[0]


def _find_crop(img, got_hr):
    """the (top, left, flip) whose crop of `img`, as the loader converts it, is got_hr (C, 32, 32): exactly one"""
    H, W = img.shape[:2]
    hits = [(t, l, f) for t in range(H - 31) for l in range(W - 31) for f in (False, True)
            if np.array_equal(_f32(img[t:t + 32, l:l + 32], f), got_hr)]
    assert len(hits) == 1, hits
    return hits[0]


def _batches(root, phase, seed, **kw):
    import data as Data
    opt = dataset_opt(root, **kw)
    ds = Data.create_dataset(opt, phase)
    torch.manual_seed(seed)
    return [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()} for b in Data.create_dataloader(ds, opt, phase)]


def test_loader_plain_bicubic_end_to_end(folder):
    root, imgs = folder
    bs = _batches(root, 'train', 5, batch_size=4, data_len=-1)
    assert len(bs) == 1 and set(bs[0]) == {'HR', 'SR', 'Index'}                # the dict a prepared dataset gives
    b = bs[0]
    assert tuple(b['HR'].shape) == (3, 3, 32, 32) and b['HR'].is_cuda and b['HR'].dtype == torch.float32 and b['Index'].tolist() == [0, 1, 2]
    from data.degrade import degrade_config
    cfg = degrade_config({}, 8)
    flips = []
    for j in range(3):
        t, l, f = _find_crop(imgs[j], b['HR'][j].cpu().numpy())
        lr, sr = degrade_oracle(imgs[j][t:t + 32, l:l + 32], np.zeros(5), cfg)
        assert np.array_equal(b['SR'][j].cpu().numpy(), _f32(sr, f)), j       # one flip flag for the pair
        flips.append(f)
    # mode LRHR adds the LR image, same flip
    bl = _batches(root, 'train', 5, mode='LRHR')[0]
    assert set(bl) == {'HR', 'SR', 'LR', 'Index'} and tuple(bl['LR'].shape) == (3, 3, 8, 8) and torch.equal(bl['HR'], b['HR'])
    for j in range(3):
        t, l, f = _find_crop(imgs[j], bl['HR'][j].cpu().numpy())
        lr, _ = degrade_oracle(imgs[j][t:t + 32, l:l + 32], np.zeros(5), cfg)
        assert f == flips[j] and np.array_equal(bl['LR'][j].cpu().numpy(), _f32(lr, f))


FULL = {'blur': {'kernel': 7, 'sigma': [0.5, 3], 'anisotropic': True}, 'noise': {'sigma': [2, 20]}, 'seed': 1}


def test_loader_seeds_govern_the_batches(folder):
    root, imgs = folder
    a, b, c = (_batches(root, 'train', s, degrade=FULL, mode='LRHR')[0] for s in (5, 5, 6))
    for k in ('HR', 'SR', 'LR'):
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a['SR'], c['SR'])
    # blur and noise are on: SR is not the plain chain of its crop
    plain = _batches(root, 'train', 5, mode='LRHR')[0]
    assert torch.equal(plain['HR'], a['HR']) and not torch.equal(plain['SR'], a['SR'])
    # val: the same images on every pass, whatever the global generators do; the centre crop, unflipped
    v1 = _batches(root, 'val', 1, degrade=FULL)
    v2 = _batches(root, 'val', 2, degrade=FULL)
    assert len(v1) == 3 and all(tuple(x['HR'].shape) == (1, 3, 32, 32) for x in v1)
    for j, (x, y) in enumerate(zip(v1, v2)):
        assert torch.equal(x['HR'], y['HR']) and torch.equal(x['SR'], y['SR'])
        H, W = FOLDER_SIZES[j]
        assert _find_crop(imgs[j], x['HR'][0].cpu().numpy()) == ((H - 32) // 2, (W - 32) // 2, False)
    assert not torch.equal(v1[0]['SR'], _batches(root, 'val', 1, degrade=dict(FULL, seed=2))[0]['SR'])


def _tiny(phase):
    import model as Model
    m = Model.create_model(opt_for('sr3_tiny', phase=phase, gpu=True))
    _, sd = load_golden('sr3_tiny')
    m.netG.load_state_dict(sd, strict=True)
    m.netG.show_progress = False
    return m


def test_loader_batch_trains_the_tiny_model(folder):
    import data as Data
    root, _ = folder
    opt = dataset_opt(root, degrade=FULL)
    torch.manual_seed(7)
    batch = next(iter(Data.create_dataloader(Data.create_dataset(opt, 'train'), opt, 'train')))
    m = _tiny('train')
    m.feed_data(batch)
    m.optimize_parameters()
    loss = m.get_current_log()['l_pix']
    assert np.isfinite(loss) and loss > 0


def test_mode_lr_super_resolves_a_plain_folder(tmp_path):
    import data as Data
    root = str(tmp_path / 'lr')
    imgs = write_folder(root, [(8, 12), (8, 8)])
    opt = dataset_opt(root, mode='LR', l_resolution=4, r_resolution=16)
    del opt['degrade']
    loader = Data.create_dataloader(Data.create_dataset(opt, 'val'), opt, 'val')
    m = _tiny('val')
    waves, n = [], 0
    for j, b in enumerate(loader):
        assert {'HR', 'SR', 'LR', 'Index'} <= set(b)
        h, w = imgs[j].shape[:2]
        ref = pil_resize(imgs[j], (4 * h, 4 * w), Image.BICUBIC)
        assert tuple(b['SR'].shape) == (1, 3, 4 * h, 4 * w) and np.array_equal(b['SR'][0].cpu().numpy(), _f32(ref, False))
        assert torch.equal(b['HR'], b['SR']) and np.array_equal(b['LR'][0].cpu().numpy(), _f32(imgs[j], False))
        waves.append(b['_dp_wave'])
        assert b['_dp_pos'] == 0
        m.feed_data(b)
        m.test(continous=False)
        vis = m.get_current_visuals(need_LR=False)
        assert tuple(vis['SR'].shape) == (3, 4 * h, 4 * w) and bool(torch.isfinite(vis['SR']).all())
        assert tuple(vis['HR'].shape) == (1, 3, 4 * h, 4 * w) and torch.equal(vis['HR'], vis['INF'])
        n += 1
    assert n == 2 and waves[0] is not waves[1]                    # a change of size starts a new wave
