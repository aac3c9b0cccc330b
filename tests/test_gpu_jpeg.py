"""The JPEG link of the degradation chain on the GPU: sr3_jpeg_u8 against the committed Pillow round trips
(tests/golden/jpeg_roundtrip.npz) and the NumPy restatement of tests/test_jpeg_cpu.py, its order / in-place / slice behaviour,
degrade_batch with a sixth number against NumPy + Pillow, and the loader end to end with one training step.  Every comparison is
np.array_equal: the whole link is integer arithmetic."""
import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from helpers import load_golden, opt_for                                                     # noqa: E402
from test_degrade_cpu import dataset_opt, degrade_oracle, pil_resize, write_folder           # noqa: E402
from test_jpeg_cpu import jpeg_oracle, load_fixture                                           # noqa: E402

SUB = {0: '4:4:4', 2: '4:2:0', -1: '4:2:0'}       # (greyscale ignores it)


@pytest.fixture(autouse=True)
def _load_in_process(monkeypatch):
    """as tests/test_gpu_degrade.py: no forked loader worker under a live HIP context"""
    import torch.utils.data as _tud
    _DL = _tud.DataLoader
    monkeypatch.setattr(_tud, 'DataLoader', lambda *a, **k: _DL(*a, **dict(k, num_workers=0)))


@pytest.fixture(scope='module')
def cases():
    """the fixture's cases with the oracle's bytes, grouped by (H, W, C, subsampling): {key: [(input, quality, Pillow, oracle)]}"""
    groups = {}
    for img, q, sub, ref in load_fixture():
        groups.setdefault(img.shape + (sub,), []).append((img, q, ref, jpeg_oracle(img, q, sub)))
    assert len(groups) == 24 and all(len(v) == 18 for v in groups.values())
    return groups


def _run(imgs, qualities, sub, **kw):
    from data.degrade import jpeg_batch
    a = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    out = jpeg_batch(a, torch.tensor(list(qualities), dtype=torch.int32).cuda(), SUB[sub], **kw)
    assert np.array_equal(a.cpu().numpy(), imgs)                          # out of place: the input stays
    return out.cpu().numpy()


@pytest.mark.parametrize('sub', [0, 2, -1])
def test_jpeg_batch_equals_the_fixture_and_the_oracle(cases, sub):
    """one call per size: the 18 (kind, quality) cases with their own qualities, and a 19th image at quality 0 in the middle"""
    for key, group in cases.items():
        if key[3] != sub:
            continue
        imgs = np.stack([g[0] for g in group[:9]] + [group[0][0]] + [g[0] for g in group[9:]])
        qs = [g[1] for g in group[:9]] + [0] + [g[1] for g in group[9:]]
        assert len(set(qs)) == 7
        got = _run(imgs, qs, sub)
        assert np.array_equal(got[9], group[0][0]), key                   # quality 0: unchanged
        for i, (img, q, ref, orc) in enumerate(group):
            g = got[i if i < 9 else i + 1]
            assert np.array_equal(g, ref), (key, q, i, 'fixture')
            assert np.array_equal(g, orc), (key, q, i, 'oracle')


@pytest.mark.parametrize('C', [3, 1])
def test_jpeg_batch_flat_images_and_quality_clamp(C):
    flat = np.stack([np.full((17, 23, C), 255, np.uint8), np.zeros((17, 23, C), np.uint8)])
    for sub in (0, 2):
        assert np.array_equal(_run(flat, [100, 100], sub), flat)
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, size=(17, 23, C)).astype(np.uint8)
    got = _run(np.stack([img] * 4), [-5, 1000, 100, 1], 2)
    assert np.array_equal(got[0], img) and np.array_equal(got[1], got[2]) and np.array_equal(got[2], jpeg_oracle(img, 100, 2))
    assert np.array_equal(got[3], jpeg_oracle(img, 1, 2))


@pytest.mark.parametrize('key', [(24, 40, 3, 2), (17, 23, 3, 0), (7, 33, 1, -1)])
def test_jpeg_batch_order_in_place_and_slices(cases, key):
    from data.degrade import jpeg_batch
    group, sub = cases[key], key[3]
    imgs = np.stack([g[0] for g in group])
    qs = [g[1] for g in group]
    qs[4] = 0
    whole = _run(imgs, qs, sub)
    perm = np.random.RandomState(1).permutation(len(group))
    assert np.array_equal(_run(imgs[perm], [qs[i] for i in perm], sub), whole[perm])
    # in place: out is the batch itself
    a = torch.from_numpy(imgs).cuda()
    qd = torch.tensor(qs, dtype=torch.int32).cuda()
    same = jpeg_batch(a, qd, SUB[sub], out=a)
    assert same.data_ptr() == a.data_ptr() and np.array_equal(a.cpu().numpy(), whole)
    # a slice of a larger batch (a pointer into the middle of it): the same bytes as the whole batch gave there, the rest untouched
    b = torch.from_numpy(imgs).cuda()
    part = jpeg_batch(b[3:11], qd[3:11].contiguous(), SUB[sub])
    assert np.array_equal(part.cpu().numpy(), whole[3:11])
    jpeg_batch(b[3:11], qd[3:11].contiguous(), SUB[sub], out=b[3:11])
    assert np.array_equal(b[3:11].cpu().numpy(), whole[3:11]) and np.array_equal(b[:3].cpu().numpy(), imgs[:3])
    assert np.array_equal(b[11:].cpu().numpy(), imgs[11:])


# ---- the chain -------------------------------------------------------------------------------------------------------------------------

def _chain_oracle(hr, d, cfg, z):
    """degrade_oracle's LR image through jpeg_oracle, then Pillow's resize back up"""
    lr, sr = degrade_oracle(hr, d[:5], cfg, z)
    if len(d) == 6 and d[5] != 0:
        lr = jpeg_oracle(lr, int(d[5]), {'4:4:4': 0, '4:2:0': 2}[cfg['jpeg']['subsampling']])
        sr = pil_resize(lr, hr.shape[:2], Image.BICUBIC)
    return lr, sr


@pytest.mark.parametrize('R, Lr, subsampling', [(128, 16, '4:2:0'), (40, 10, '4:2:0'), (40, 10, '4:4:4')])
def test_degrade_batch_with_jpeg_matches_the_composed_oracle(R, Lr, subsampling):
    from data.degrade import degrade_batch, degrade_config
    from test_gpu_degrade import _images
    n = 3
    cfg = degrade_config({'blur': {'kernel': 7, 'sigma': [0.3, 3], 'anisotropic': True}, 'noise': {'sigma': [1, 30]},
                          'jpeg': {'subsampling': subsampling}}, Lr)
    hr = _images(n, R, R, 3, seed=R + Lr)
    z = torch.randn(n, Lr, Lr, 3, generator=torch.Generator().manual_seed(5))
    # [blur_on, sigma_x, sigma_y, theta, noise_sigma, quality]: everything on; blur alone; noise and JPEG without blur -- then JPEG
    # alone, JPEG behind blur, nothing
    for rows in ([[1, 2.0, 0.6, 0.7, 12.5, 35], [1, 1.1, 1.1, 0.0, 0.0, 0], [0, 1.0, 1.0, 0.0, 20.0, 90]],
                 [[0, 1.0, 1.0, 0.0, 0.0, 10], [1, 0.5, 2.5, 2.0, 0.0, 75], [0, 1.0, 1.0, 0.0, 0.0, 0]]):
        deg = torch.tensor(rows, dtype=torch.float32)
        lr, sr = degrade_batch(torch.from_numpy(hr).cuda(), deg, cfg, z=z)
        d64 = deg.double().numpy()
        for i in range(n):
            ref_lr, ref_sr = _chain_oracle(hr[i], d64[i], cfg, z[i].numpy())
            assert np.array_equal(lr[i].cpu().numpy(), ref_lr), (rows[i], 'lr')
            assert np.array_equal(sr[i].cpu().numpy(), ref_sr), (rows[i], 'sr')
            plain_lr = degrade_oracle(hr[i], d64[i][:5], cfg, z[i].numpy())[0]
            assert np.array_equal(ref_lr, plain_lr) == (rows[i][5] == 0)             # JPEG changes the image it is on, no other
    # all qualities 0, and five numbers: the chain without the link, byte for byte
    deg = torch.tensor([[1, 2.0, 0.6, 0.7, 12.5, 0], [1, 1.1, 1.1, 0.0, 0.0, 0], [0, 1.0, 1.0, 0.0, 20.0, 0]], dtype=torch.float32)
    lr6, sr6 = degrade_batch(torch.from_numpy(hr).cuda(), deg, cfg, z=z)
    lr5, sr5 = degrade_batch(torch.from_numpy(hr).cuda(), deg[:, :5].contiguous(), cfg, z=z)
    assert torch.equal(lr6, lr5) and torch.equal(sr6, sr5)
    for i in range(n):
        ref_lr, ref_sr = degrade_oracle(hr[i], deg[i, :5].double().numpy(), cfg, z[i].numpy())
        assert np.array_equal(lr5[i].cpu().numpy(), ref_lr) and np.array_equal(sr5[i].cpu().numpy(), ref_sr)
    with pytest.raises(ValueError, match='deg'):
        degrade_batch(torch.from_numpy(hr).cuda(), torch.zeros(n, 7), cfg, z=z)


# ---- the loader, end to end ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def folder(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('hr_folder_jpeg'))
    return root, write_folder(root)


def _first_batch(root, seed, **kw):
    import data as Data
    opt = dataset_opt(root, **kw)
    torch.manual_seed(seed)
    return next(iter(Data.create_dataloader(Data.create_dataset(opt, 'train'), opt, 'train')))


def test_loader_with_a_jpeg_block_end_to_end(folder):
    root, _ = folder
    on = _first_batch(root, 5, degrade={'jpeg': {'quality': [20, 40]}}, mode='LRHR')
    off = _first_batch(root, 5, degrade={'jpeg': {'prob': 0, 'quality': [20, 40]}}, mode='LRHR')
    plain = _first_batch(root, 5, degrade={}, mode='LRHR')
    assert set(on) == {'HR', 'SR', 'LR', 'Index'} and tuple(on['SR'].shape) == (3, 3, 32, 32) and on['SR'].is_cuda
    assert torch.equal(on['HR'], off['HR']) and torch.equal(on['HR'], plain['HR'])              # the same crops and flips
    assert torch.equal(off['SR'], plain['SR']) and torch.equal(off['LR'], plain['LR'])          # prob 0: the chain without the link
    for j in range(3):
        assert not torch.equal(on['SR'][j], off['SR'][j]) and not torch.equal(on['LR'][j], off['LR'][j]), j
    # the validation split: the same images on every pass
    import data as Data
    opt = dataset_opt(root, degrade={'jpeg': {'quality': [20, 40]}, 'seed': 3})
    v1, v2 = ([b['SR'].clone() for b in Data.create_dataloader(Data.create_dataset(opt, 'val'), opt, 'val')] for _ in range(2))
    assert len(v1) == 3 and all(torch.equal(a, b) for a, b in zip(v1, v2))


def test_loader_jpeg_batch_trains_the_tiny_model(folder):
    import model as Model
    root, _ = folder
    batch = _first_batch(root, 7, degrade={'blur': {'kernel': 7, 'sigma': [0.5, 3]}, 'noise': {'sigma': [2, 20]},
                                           'jpeg': {'prob': 0.7, 'quality': [30, 95]}})
    m = Model.create_model(opt_for('sr3_tiny', phase='train', gpu=True))
    _, sd = load_golden('sr3_tiny')
    m.netG.load_state_dict(sd, strict=True)
    m.feed_data(batch)
    m.optimize_parameters()
    loss = m.get_current_log()['l_pix']
    assert np.isfinite(loss) and loss > 0
