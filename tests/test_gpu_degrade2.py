"""The second-order degradation on the GPU: the BOX resize against Pillow, sr3_noise_ex_u8 and the sinc blur against
the NumPy restatements of tests/test_degrade2_cpu.py / tests/test_degrade_cpu.py, the full two-round degrade_batch against the
composed NumPy + Pillow oracle, the loader end to end and one training step on the tiny model.  Every comparison is bit-exact: the
blur, the JPEG and the Poisson draw are integer arithmetic, the noise is one rounding per operation, the resizes are Pillow's."""
import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from helpers import load_golden, opt_for                                                     # noqa: E402
from test_degrade_cpu import blur_oracle, dataset_opt, degrade_oracle, pil_resize, write_folder          # noqa: E402
from test_degrade2_cpu import degrade2_oracle, noise_ex_oracle                               # noqa: E402


@pytest.fixture(autouse=True)
def _load_in_process(monkeypatch):
    """The validation loader forks one worker; forking a process with a live HIP context takes tens of seconds on the GPU box.  Load
    in-process here, as tests/test_gpu_degrade.py does: the batches are the same."""
    import torch.utils.data as _tud
    _DL = _tud.DataLoader
    monkeypatch.setattr(_tud, 'DataLoader', lambda *a, **k: _DL(*a, **dict(k, num_workers=0)))


def _images(n, H, W, C, seed, block=1):
    """random bytes; the top half of every image a 0 / 255 checkerboard of block x block squares (the extremes next to each other)"""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, size=(n, H, W, C)).astype(np.uint8)
    yy, xx = np.mgrid[0:H // 2, 0:W]
    a[:, :H // 2] = (((yy // block + xx // block) % 2) * 255).astype(np.uint8)[None, :, :, None]
    return a


# ---- the BOX resize --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C', [3, 1])
@pytest.mark.parametrize('hw, out', [((16, 16), (8, 8)), ((20, 37), (7, 13)), ((32, 32), (48, 40)), ((128, 128), (16, 16)), ((9, 9), (9, 9))])
def test_box_resize_is_pillows(hw, out, C):
    from data.prepare_data import resize_batch
    a = _images(3, hw[0], hw[1], C, seed=hw[0] + out[1] + C)
    got = resize_batch(torch.from_numpy(a), out, Image.BOX)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (3, out[0], out[1], C)
    for i in range(3):
        assert np.array_equal(got[i].cpu().numpy(), pil_resize(a[i], out, Image.BOX)), (hw, out, C, i)
    if hw != out:                                                             # the third filter is a third result
        assert not np.array_equal(got[0].cpu().numpy(), pil_resize(a[0], out, Image.BILINEAR))
    assert np.array_equal(resize_batch(torch.from_numpy(a), out, 4).cpu().numpy(), got.cpu().numpy())      # Pillow's number


# ---- sr3_noise_ex_u8 -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C', [3, 1])
def test_noise_ex_u8_matches_the_numpy_oracle(C):
    from data.degrade import noise_ex_batch, poisson_table
    T = poisson_table()
    rng = np.random.RandomState(5 + C)
    a = rng.randint(0, 256, size=(4, 16, 16, C)).astype(np.uint8)
    a[:, 0], a[:, 1] = 0, 255                                                 # lambda = 0: no change in the Poisson modes; lambda = 255
    a[:, 2, :8] = np.arange(8, dtype=np.uint8)[None, :, None]                 # the ties below meet both parities, and 0 from above
    a[:, 3, :8] = (255 - np.arange(8, dtype=np.uint8))[None, :, None]
    mode = np.array([0, 1, 2, 3], np.int32)                                   # one image per mode
    strength = np.array([0.5, 0.5, 1.3, 2.0], np.float32)
    z = rng.randn(4, 16, 16, C).astype(np.float32)
    z[:2, 2:6] = np.where(rng.rand(2, 4, 16, C) < 0.5, 1.0, -1.0)             # exact ties x.5 at sigma 0.5, colour and gray
    z[:2, 6] = 600.0                                                          # + 300 levels: clamps at 255
    z[:2, 7] = -600.0
    r = rng.randint(0, 2 ** 31 - 1, size=(4, 16, 16, C)).astype(np.int32)
    r[:, :, 0::5] = 0                                                         # the ends of r's range, in every row (v = 0 and 255 included)
    r[:, :, 1::5] = 2 ** 31 - 2
    ref = np.stack([noise_ex_oracle(a[i], int(mode[i]), strength[i], z[i], r[i], T) for i in range(4)])
    assert (ref[:2, 6] == 255).all() and (ref[:2, 7] == 0).all()
    assert ((ref[:2, 2:6] % 2 == 0) | (a[:2, 2:6] == 255)).all()              # every tie went to the even neighbour
    assert np.array_equal(ref[2:, 0], a[2:, 0]) and not np.array_equal(ref[2:, 1], a[2:, 1])       # lambda 0 stays; lambda 255 moves
    assert all(not np.array_equal(ref[i], a[i]) for i in range(4))
    if C == 3:                                                                # gray: one shift per pixel, up to the clamps
        d = ref[3].astype(int) - a[3].astype(int)
        inside = ((ref[3] > 0) & (ref[3] < 255)).all(-1)
        assert inside.any() and (d[inside] == d[inside][:, :1]).all()
    dev = torch.device('cuda')
    ad, md, sd, zd, rd = (torch.from_numpy(t).to(dev) for t in (a, mode, strength, z, r))
    out = noise_ex_batch(ad, md, sd, zd, rd)
    assert np.array_equal(out.cpu().numpy(), ref) and np.array_equal(ad.cpu().numpy(), a)
    # a batch permutation permutes the output
    perm = [2, 0, 3, 1]
    got_p = noise_ex_batch(*(torch.from_numpy(np.ascontiguousarray(t[perm])).to(dev) for t in (a, mode, strength, z, r)))
    assert np.array_equal(got_p.cpu().numpy(), ref[perm])
    # strength 0 copies its image whatever the draws hold; the others are untouched by it
    s0 = strength.copy()
    s0[[0, 3]] = 0.0
    zn = z.copy()
    zn[0] = np.nan
    out0 = noise_ex_batch(ad, md, torch.from_numpy(s0).to(dev), torch.from_numpy(zn).to(dev), rd).cpu().numpy()
    assert np.array_equal(out0[[0, 3]], a[[0, 3]]) and np.array_equal(out0[[1, 2]], ref[[1, 2]])
    # the draws a batch does not need may be absent
    gauss, pois = torch.tensor([0, 1, 0, 1], dtype=torch.int32, device=dev), torch.tensor([2, 3, 2, 3], dtype=torch.int32, device=dev)
    og = noise_ex_batch(ad, gauss, sd, zd, None).cpu().numpy()
    op = noise_ex_batch(ad, pois, sd, None, rd).cpu().numpy()
    for i in range(4):
        assert np.array_equal(og[i], noise_ex_oracle(a[i], i % 2, strength[i], z[i], None, T)), i
        assert np.array_equal(op[i], noise_ex_oracle(a[i], 2 + i % 2, strength[i], None, r[i], T)), i
    # in place
    same = noise_ex_batch(ad, md, sd, zd, rd, out=ad)
    assert same.data_ptr() == ad.data_ptr() and np.array_equal(ad.cpu().numpy(), ref)


# ---- the sinc kernel through sr3_blur_u8 -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('hw', [(20, 37), (16, 16)])
@pytest.mark.parametrize('k', [3, 7, 21])
def test_sinc_blur_matches_the_integer_oracle_and_rings(k, hw):
    """One image per cut-off.  The checkerboard half is made of 2 x 2 squares: its frequency (pi/2, pi/2) lies inside the pass band of
    omega = 3.14, so that image rings past both clamps (a one-pixel checkerboard sits at (pi, pi), outside every circular cut-off
    <= pi: it is averaged to grey and nothing overshoots)."""
    from data.degrade import blur_batch, sinc_weights
    omegas = (1.05, 2.0, 3.14)
    a = _images(3, hw[0], hw[1], 3, seed=k + hw[1], block=2)
    w = np.stack([sinc_weights(om, k) for om in omegas])
    got = blur_batch(torch.from_numpy(a).cuda(), torch.from_numpy(w).cuda()).cpu().numpy()
    for i in range(3):
        assert np.array_equal(got[i], blur_oracle(a[i], w[i])), (k, hw, omegas[i])
    top = got[2, :hw[0] // 2]                     # every k x k neighbourhood of these pixels (k >= 3) holds both 0 and 255
    assert (top == 0).any() and (top == 255).any() and ((top > 0) & (top < 255)).any()
    flat = np.full_like(a, 255)
    assert np.array_equal(blur_batch(torch.from_numpy(flat).cuda(), torch.from_numpy(w).cuda()).cpu().numpy(), flat)      # the taps sum to 1


# ---- the chain -------------------------------------------------------------------------------------------------------------------------

CHAIN = {'blur': {'kernel': 7, 'sigma': [0.3, 3], 'anisotropic': True}, 'sinc': {'prob': 0.5}, 'noise': {'sigma': [1, 30]},
         'shot': {'prob': 0.5}, 'gray_noise': 0.5, 'jpeg': {'quality': [30, 95]},
         'second': {'mid': [12, 40], 'resample': ['box', 'bilinear', 'bicubic'], 'blur': {'kernel': 5, 'sigma': [0.2, 1.5], 'anisotropic': True},
                    'sinc': {'prob': 0.5}, 'noise': {'sigma': [1, 20]}, 'shot': {'prob': 0.5}, 'gray_noise': 0.5,
                    'jpeg': {'quality': [30, 95], 'subsampling': '4:4:4'}, 'final_sinc': {'prob': 0.8, 'kernel': 7}}}
BOX, BIL = 4.0, 2.0


def _rows(M):
    """deg (6, 6) and deg2 (6, 20) by hand.  deg2: [sinc1, omega1, mode1, scale1, M, rs1, rs2, blur2, sx2, sy2, th2, sinc2, omega2,
    sigma2, mode2, scale2, q2, final_sinc, omega_f, jpeg_first]; rows 1.. carry other M / filters, which row 0 overrules."""
    deg = torch.tensor([[1, 2.0, 0.6, 0.7, 12.5, 60],        # 0: everything on, JPEG before the final sinc
                        [1, 1.1, 1.1, 0.0, 8.0, 35],         # 1: everything on, the final sinc before the JPEG
                        [1, 0.8, 2.0, 2.1, 20.0, 80],        # 2: round 2 wholly off
                        [1, 1.0, 1.0, 0.0, 0.0, 0],          # 3: a sinc kernel in round 1, nothing else
                        [0, 1.0, 1.0, 0.0, 1.0, 0],          # 4: Poisson gray in round 1, Gaussian colour in round 2
                        [0, 1.0, 1.0, 0.0, 0.0, 0]],         # 5: every switch 0
                       dtype=torch.float32)
    deg2 = torch.tensor([[0, 2.0, 2, 0.7, M, BOX, BIL, 1, 1.2, 0.4, 0.5, 1, 2.5, 6.0, 1, 1.0, 50, 1, 2.2, 1],
                         [1, 2.8, 0, 1.0, 99, 3, 3, 1, 0.9, 0.9, 0.0, 0, 2.0, 3.0, 3, 1.5, 75, 1, 3.14, 0],
                         [0, 2.0, 1, 1.0, 7, 2, 4, 0, 1.0, 1.0, 0.0, 1, 2.0, 0.0, 2, 1.0, 0, 0, 2.0, 1],
                         [1, 3.1415927, 3, 2.0, M, BOX, BIL, 0, 1.0, 1.0, 0.0, 0, 2.0, 0.0, 0, 1.0, 0, 0, 2.0, 0],
                         [0, 2.0, 3, 1.4, M, BOX, BIL, 0, 1.0, 1.0, 0.0, 0, 2.0, 9.0, 0, 1.0, 0, 0, 2.0, 0],
                         [0, 2.0, 0, 1.0, M, BOX, BIL, 0, 1.0, 1.0, 0.0, 0, 2.0, 0.0, 0, 1.0, 0, 0, 2.0, 1]], dtype=torch.float32)
    return deg, deg2


@pytest.mark.parametrize('M', [12, 40])
def test_degrade_batch_second_order_matches_the_composed_oracle(M):
    from data.degrade import degrade_batch, degrade_config
    R, Lr, n = 32, 8, 6
    cfg = degrade_config(CHAIN, Lr)
    hr = _images(n, R, R, 3, seed=11 + M, block=2)
    deg, deg2 = _rows(M)
    g = torch.Generator().manual_seed(3)
    z, z2 = torch.randn(n, M, M, 3, generator=g), torch.randn(n, Lr, Lr, 3, generator=g)
    r = torch.randint(0, 2 ** 31 - 1, (n, M, M, 3), dtype=torch.int32, generator=g)
    r2 = torch.randint(0, 2 ** 31 - 1, (n, Lr, Lr, 3), dtype=torch.int32, generator=g)
    lr, sr = degrade_batch(torch.from_numpy(hr).cuda(), deg, cfg, z=z, deg2=deg2, r=r, z2=z2, r2=r2)
    assert lr.is_cuda and lr.dtype == torch.uint8 and tuple(lr.shape) == (n, Lr, Lr, 3) and tuple(sr.shape) == (n, R, R, 3)
    d, d2 = deg.double().numpy(), deg2.double().numpy()
    refs = [degrade2_oracle(hr[i], d[i], d2[i], cfg, M, Image.BOX, Image.BILINEAR, z[i].numpy(), r[i].numpy(), z2[i].numpy(), r2[i].numpy())
            for i in range(n)]
    for i in range(n):
        assert np.array_equal(lr[i].cpu().numpy(), refs[i][0]), (M, i)
        assert np.array_equal(sr[i].cpu().numpy(), refs[i][1]), (M, i)
    # every switch 0: the two resizes alone, through the mid size, with row 0's filters
    plain = pil_resize(pil_resize(hr[5], (M, M), Image.BOX), (Lr, Lr), Image.BILINEAR)
    assert np.array_equal(lr[5].cpu().numpy(), plain) and np.array_equal(sr[5].cpu().numpy(), pil_resize(plain, (R, R), Image.BICUBIC))
    assert all(not np.array_equal(refs[i][0], pil_resize(pil_resize(hr[i], (M, M), Image.BOX), (Lr, Lr), Image.BILINEAR)) for i in range(5))
    # the order of the final stage matters to the oracle (so the test tells the two apart)
    swapped = d2[0].copy()
    swapped[19] = 0
    assert not np.array_equal(degrade2_oracle(hr[0], d[0], swapped, cfg, M, Image.BOX, Image.BILINEAR, z[0].numpy(), r[0].numpy(),
                                              z2[0].numpy(), r2[0].numpy())[0], refs[0][0])
    with pytest.raises(ValueError, match='shape'):
        degrade_batch(torch.from_numpy(hr), deg, cfg, z=z[:, :4], deg2=deg2, r=r, z2=z2, r2=r2)
    with pytest.raises(ValueError, match='deg2'):
        degrade_batch(torch.from_numpy(hr), deg, cfg, deg2=deg2[:, :19])


def test_degrade_batch_without_second_and_without_deg2():
    """no "second" block: round 1 lands on L with the top-level filter; deg2=None: today's chain, the first-order oracle"""
    from data.degrade import degrade_batch, degrade_config
    R, Lr, n = 32, 8, 4
    cfg = degrade_config({k: v for k, v in CHAIN.items() if k != 'second'}, Lr)
    assert cfg['extended'] and cfg['second'] is None
    hr = _images(n, R, R, 3, seed=21, block=2)
    deg = torch.tensor([[1, 2.0, 0.6, 0.7, 12.5, 60], [1, 1.1, 1.1, 0.0, 3.0, 0], [0, 1.0, 1.0, 0.0, 1.0, 40], [0, 1.0, 1.0, 0.0, 0.0, 0]],
                       dtype=torch.float32)
    tail = [Lr, 3, 3] + [0] * 13
    deg2 = torch.tensor([[1, 3.0, 1, 1.0] + tail, [0, 2.0, 2, 0.8] + tail, [0, 2.0, 3, 1.7] + tail, [1, 2.0, 3, 1.0] + tail], dtype=torch.float32)
    g = torch.Generator().manual_seed(4)
    z = torch.randn(n, Lr, Lr, 3, generator=g)
    r = torch.randint(0, 2 ** 31 - 1, (n, Lr, Lr, 3), dtype=torch.int32, generator=g)
    lr, sr = degrade_batch(torch.from_numpy(hr).cuda(), deg, cfg, z=z, deg2=deg2, r=r)
    d, d2 = deg.double().numpy(), deg2.double().numpy()
    for i in range(n):
        ref_lr, ref_sr = degrade2_oracle(hr[i], d[i], d2[i], cfg, Lr, Image.BICUBIC, Image.BICUBIC, z[i].numpy(), r[i].numpy())
        assert np.array_equal(lr[i].cpu().numpy(), ref_lr) and np.array_equal(sr[i].cpu().numpy(), ref_sr), i
    # deg2=None: the five numbers through the first-order oracle of tests/test_degrade_cpu.py
    lr1, sr1 = degrade_batch(torch.from_numpy(hr).cuda(), deg[:, :5], cfg, z=z)
    for i in range(n):
        ref_lr, ref_sr = degrade_oracle(hr[i], d[i, :5], cfg, z[i].numpy())
        assert np.array_equal(lr1[i].cpu().numpy(), ref_lr) and np.array_equal(sr1[i].cpu().numpy(), ref_sr), i
    # ... and with Gaussian colour noise and no sinc the second-order path gives those very bytes
    plain2 = torch.tensor([[0, 2.0, 0, 1.0] + tail] * n, dtype=torch.float32)
    lr2, sr2 = degrade_batch(torch.from_numpy(hr).cuda(), deg[:, :5], cfg, z=z, deg2=plain2)
    assert torch.equal(lr2, lr1) and torch.equal(sr2, sr1)


# ---- the loader, end to end ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def folder(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('hr_folder2'))
    return root, write_folder(root)


LOADER = dict(CHAIN, seed=1)


def _batches(root, phase, seed, **kw):
    import data as Data
    opt = dataset_opt(root, **kw)
    ds = Data.create_dataset(opt, phase)
    torch.manual_seed(seed)
    return [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()} for b in Data.create_dataloader(ds, opt, phase)]


def test_loader_second_order_seeds_govern_the_batches(folder):
    root, _ = folder
    a, b, c = (_batches(root, 'train', s, degrade=LOADER, mode='LRHR')[0] for s in (5, 5, 6))
    assert set(a) == {'HR', 'SR', 'LR', 'Index'} and tuple(a['SR'].shape) == (3, 3, 32, 32) and tuple(a['LR'].shape) == (3, 3, 8, 8)
    for k in ('HR', 'SR', 'LR'):
        assert a[k].is_cuda and a[k].dtype == torch.float32 and torch.equal(a[k], b[k]), k
    assert not torch.equal(a['SR'], c['SR'])
    first = {k: v for k, v in LOADER.items() if k in ('blur', 'noise', 'jpeg', 'seed')}
    plain = _batches(root, 'train', 5, degrade=first, mode='LRHR')[0]
    # the first item's crop does not move (draw_deg2 comes behind it); its second round (blur, noise, JPEG: all on) makes another image
    assert torch.equal(plain['HR'][0], a['HR'][0]) and not torch.equal(plain['SR'][0], a['SR'][0])
    # val: the same bytes on every pass, whatever the global generators do
    v1 = _batches(root, 'val', 1, degrade=LOADER)
    v2 = _batches(root, 'val', 2, degrade=LOADER)
    assert len(v1) == 3 and all(tuple(x['HR'].shape) == (1, 3, 32, 32) for x in v1)
    for x, y in zip(v1, v2):
        assert torch.equal(x['HR'], y['HR']) and torch.equal(x['SR'], y['SR'])
    assert not torch.equal(v1[0]['SR'], _batches(root, 'val', 1, degrade=dict(LOADER, seed=2))[0]['SR'])


def test_loader_second_order_batch_trains_the_tiny_model(folder):
    import data as Data
    import model as Model
    root, _ = folder
    opt = dataset_opt(root, degrade=LOADER)
    torch.manual_seed(7)
    batch = next(iter(Data.create_dataloader(Data.create_dataset(opt, 'train'), opt, 'train')))
    m = Model.create_model(opt_for('sr3_tiny', phase='train', gpu=True))
    _, sd = load_golden('sr3_tiny')
    m.netG.load_state_dict(sd, strict=True)
    m.netG.show_progress = False
    m.feed_data(batch)
    m.optimize_parameters()
    loss = m.get_current_log()['l_pix']
    assert np.isfinite(loss) and loss > 0
