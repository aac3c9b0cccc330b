"""Noise conditioning augmentation on the GPU (csrc/cond_augment.hip, the 7-channel input conv, EngineDiffusion.set_cond_augment): the
kernel bit for bit against the NumPy restatement of tests/condaug_ref.py, the 7-channel input conv against float64, and the model-level
paths -- forward, training step, sampling chains, the rules on x0, tiling, guidance -- against the oracle or against the chain without
the key.

Shapes: the kernel at 4 x 4 (16-byte accesses), 3 x 5 (the one-element form) and 4 x 4 one float off a 16-byte boundary (the alignment
fallback), three images so that the middle one can be dropped; the input conv at the four shapes that take each dispatch; the tiny
fixture (inner 8, 16 x 16) widened to in_channel 7 for training and sampling, and the inner-32 fixture at 16 x 32, the smallest model
whose input conv runs on the MFMA form."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

import condaug_ref as R                                                                   # noqa: E402
import gpu_util as G                                                                      # noqa: E402
from helpers import load_golden, opt_for                                                  # noqa: E402
from oracle import sr3_oracle as O                                                        # noqa: E402
from sr3_hip import lib as L                                                              # noqa: E402

F = np.float32
GUARD = 1024          # floats of sentinel around dst, in the same allocation
SENTINEL = 7.25
LEVELS = [0.0, 0.25, 0.9]
KEEP = [1, 0, 1]


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------------------

def _guarded(arr, d, mis=0):
    """arr on the device with GUARD sentinels on both sides in one allocation, `mis` floats off a 16-byte boundary: (view, buffer, offset)"""
    t = torch.as_tensor(arr)
    buf = torch.full((t.numel() + 2 * GUARD,), SENTINEL, device=d)
    assert buf.data_ptr() % 16 == 0
    off = GUARD + mis
    buf[off:off + t.numel()].copy_(t.reshape(-1))
    return buf[off:off + t.numel()].view(t.shape), buf, off


def _call(src, eps, a, s, keep, level_channel, dst, first):
    B, Cl, H, W = src.shape
    rc = L.load().sr3_cond_augment_f32(L.ptr(src), L.ptr(eps), L.ptr(a), L.ptr(s), L.ptr(keep), level_channel, L.ptr(dst), dst.shape[1], first,
                                       B, Cl, H, W, G.stream())
    torch.cuda.synchronize()
    return rc


def _inputs(hw):
    rng = np.random.default_rng(100 * hw[0] + hw[1])
    src, eps = (rng.standard_normal((3, 3) + hw).astype(F) for _ in range(2))
    src[0, 0, 0, 0] = -0.0                                                 # a level-0 image is a bit copy, the sign of a zero included
    return src, eps


@pytest.mark.parametrize('noise', [True, False], ids=['eps', 'no-eps'])
@pytest.mark.parametrize('level_channel', [1, 0], ids=['level', 'blind'])
@pytest.mark.parametrize('hw,mis', [((4, 4), 0), ((3, 5), 0), ((4, 4), 1)], ids=['4x4', '3x5', '4x4-misaligned'])
def test_kernel_is_bit_exact(hw, mis, level_channel, noise):
    d = G.dev()
    src, eps = _inputs(hw)
    a, s = R.level_coefs(LEVELS)
    sd_, ed = torch.from_numpy(src).to(d), (torch.from_numpy(eps).to(d) if noise else None)
    ad, sdv = torch.from_numpy(a).to(d), torch.from_numpy(s).to(d)
    written = 3 + level_channel
    for dst_channels, first in ((written + 3, 2), (written, 0)):
        for keep in (KEEP, None):
            rng = np.random.default_rng(5)
            dst0 = rng.standard_normal((3, dst_channels) + hw).astype(F)
            dst0[1] = np.nan                                               # a dropped image's old content does not matter either
            dst, buf, off = _guarded(dst0, d, mis)
            kd = None if keep is None else torch.tensor(keep, dtype=torch.int32, device=d)
            assert _call(sd_, ed, ad if noise else None, sdv, kd, level_channel, dst, first) == 0, L.load().sr3_last_error()
            want = R.augment(dst0, src, eps if noise else None, a, s, keep, level_channel, first)
            got = dst.cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (dst_channels, first, keep)
            # the level-0 image is src itself, whether noise is given or not
            assert np.array_equal(got[0, first:first + 3].view(np.uint32), src[0].view(np.uint32))
            if level_channel:
                assert (got[2, first + 3] == s[2]).all() and not got[0, first + 3].any()
            if keep is not None:
                z = got[1, first:first + written]
                assert not z.any() and not np.signbit(z).any()             # +0.0, the level plane too
            assert bool((buf[:off] == SENTINEL).all()) and bool((buf[off + dst.numel():] == SENTINEL).all()), 'wrote outside dst'
    assert torch.equal(sd_.cpu(), torch.from_numpy(src)) and (ed is None or torch.equal(ed.cpu(), torch.from_numpy(eps)))


def test_dropped_images_are_not_read():
    """src and eps of a dropped image may hold anything: its planes are +0.0, not 0 * NaN"""
    d = G.dev()
    src, eps = _inputs((4, 4))
    src[1], eps[1] = np.nan, np.inf
    a, s = (torch.from_numpy(t).to(d) for t in R.level_coefs(LEVELS))
    keep = torch.tensor(KEEP, dtype=torch.int32, device=d)
    dst = torch.full((3, 6, 4, 4), SENTINEL, device=d)
    assert _call(torch.from_numpy(src).to(d), torch.from_numpy(eps).to(d), a, s, keep, 1, dst, 1) == 0
    got = dst.cpu().numpy()
    assert not got[1, 1:5].any() and np.isfinite(got).all() and (got[:, 0] == SENTINEL).all() and (got[:, 5] == SENTINEL).all()


# ---- 2. the 7-channel input conv --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('B,Ca,Cb,H,W,Cout', [(2, 4, 3, 3, 32, 32), (2, 4, 3, 4, 64, 64), (2, 4, 3, 1, 32, 128), (2, 7, 0, 5, 24, 8)],
                         ids=['one-block-per-wave', 'four-per-wave', 'single-row', 'valu'])
def test_conv_in_7_channels(B, Ca, Cb, H, W, Cout):
    """sr3_conv_in_f32 against float64 F.conv2d at the tolerance of tests/test_gpu_ops.py::test_conv_in (2e-5 max(1, |ref|))"""
    d = G.dev()
    gen = torch.Generator().manual_seed(31 * H + W + Cout)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    a, b = rnd(B, Ca, H, W), (rnd(B, Cb, H, W) if Cb else None)
    w, bias = rnd(Cout, Ca + Cb, 3, 3) * 0.2, rnd(Cout)
    out = torch.full((B, H, W, Cout), float('nan'), device=d)
    ad, bd, wd, biasd = a.to(d), (None if b is None else b.to(d)), G.ohwi(w).to(d), bias.to(d)
    L.check(L.load().sr3_conv_in_f32(L.ptr(ad), Ca, L.ptr(bd), Cb, B, H, W, L.ptr(wd), L.ptr(biasd), Cout, L.ptr(out), G.stream()))
    torch.cuda.synchronize()
    x = a if b is None else torch.cat([a, b], 1)
    ref = TF.conv2d(x.double(), w.double(), bias.double(), padding=1)
    err = G.assert_close(G.nchw(out).cpu(), ref, what='conv_in 7')
    print('conv_in %s: max abs err %.3e' % ((B, Ca, Cb, H, W, Cout), err))


# ---- the models -------------------------------------------------------------------------------------------------------------------------

_models = {}
AUG = {'max_level': 0.5, 'sample_level': 0.3, 'level_channel': True}


def _model(name, phase, wide=True):
    """one model per (fixture, phase, width): the widened golden weights under the level channel, the golden ones as they are for the
    blind form: (netG, golden record, state dict)"""
    import model as Model
    key = (name, phase, wide)
    if key not in _models:
        if wide:
            m = Model.create_model(R.opt7(name, phase=phase, aug=AUG))
            g, sd = R.widened(name)
        else:
            m = Model.create_model(opt_for(name, phase=phase, gpu=True))
            g, sd = load_golden(name)
        m.netG.load_state_dict(sd, strict=True)
        m.netG.show_progress = False
        _models[key] = (m, g, sd)
    m, g, sd = _models[key]
    netG = m.netG
    # every test starts from the same settings
    netG.set_prediction('eps')
    netG.set_sampler(None)
    netG.set_tiling(None)
    netG.set_consistency(None)
    netG.set_guidance(None)
    netG.set_cond_drop(0.0)
    netG.set_cond_augment(**AUG) if wide else netG.set_cond_augment(None)
    netG.use_graph = True
    return netG, g, sd


def _last_state(netG):
    return next(reversed(netG._loop_cache.values()))


# ---- 3. the forward of a model whose input conv takes the MFMA form --------------------------------------------------------------------

def test_unet_forward_16x32_inner32():
    d = G.dev()
    netG, g, sd = _model('sr3_seam', 'val')
    gen = torch.Generator().manual_seed(3)
    x, cond = torch.randn(2, 3, 16, 32, generator=gen), torch.rand(2, 4, 16, 32, generator=gen) * 2 - 1
    level = torch.tensor([0.93, 0.41])
    eps = netG.denoise_fn(x.to(d), level.to(d), cond=cond.to(d)).cpu()
    with torch.no_grad():
        ref = O.unet_forward(sd, R.desc7('sr3_seam'), torch.cat([cond, x], 1), level.view(2, 1))
    err = (eps - ref).abs().max().item()
    tol = 2e-5 * max(1.0, ref.abs().max().item())
    print('unet forward 16 x 32: max abs err %.3e (tolerance %.3e)' % (err, tol))
    assert err <= tol
    ops = netG.denoise_fn.plan.op_list(2)
    ci = [i for i, o in enumerate(ops) if o['kind'] == 20]
    assert len(ci) == 1 and ops[ci[0]]['cin'] == 7 and (ops[ci[0]]['h_out'], ops[ci[0]]['w_out']) == (16, 32)
    print('input conv fused its statistics: %d; next op kind %d' % (ops[ci[0]]['fused_output_stats'], ops[ci[0] + 1]['kind']))
    if ops[ci[0]]['fused_output_stats']:
        assert ops[ci[0] + 1]['kind'] != 30, 'a stand-alone statistics pass follows an input conv that fused its statistics'


# ---- 4. the training step ---------------------------------------------------------------------------------------------------------------

T_LEVELS = [0.0, 0.3, 0.45, 0.1]
T_KEEP = [1, 1, 0, 1]


def _train_batch():
    gen = torch.Generator().manual_seed(41)
    hr, sr = (torch.rand(4, 3, 16, 16, generator=gen) * 2 - 1 for _ in range(2))
    z, ceps = (torch.randn(4, 3, 16, 16, generator=gen) for _ in range(2))
    gamma = torch.tensor([0.97, 0.85, 0.6, 0.35])
    return hr, sr, z, gamma, ceps


_oracle_steps = {}


def _oracle(sd, prediction):
    if prediction not in _oracle_steps:
        hr, sr, z, gamma, ceps = _train_batch()
        cond = R.network_cond(sr, ceps, T_LEVELS, T_KEEP, True)
        _oracle_steps[prediction] = R.p_losses(sd, R.desc7('sr3_tiny'), hr, cond, gamma, z, prediction) + (cond,)
    return _oracle_steps[prediction]


def _engine_step(netG, inject=True, **kw):
    d = G.dev()
    hr, sr, z, gamma, ceps = _train_batch()
    if inject:
        kw = dict(dict(cond_level=T_LEVELS, cond_noise=ceps.to(d), cond_keep=T_KEEP), **kw)
    loss = netG.p_losses({'HR': hr.to(d), 'SR': sr.to(d)}, noise=z.to(d), gamma=gamma, **kw)
    torch.cuda.synchronize()
    return float(loss), netG.denoise_fn.grad_arena.clone()


@pytest.mark.parametrize('prediction', ['eps', 'v'])
def test_training_step_matches_the_oracle(prediction):
    """tolerances of tests/test_gpu_train.py for this model size: loss relative 1e-5, gradients normwise relative 1e-4 where |ref| > 1e-6"""
    netG, g, sd = _model('sr3_tiny', 'train')
    netG.set_prediction(prediction)
    ref_loss, ref_grads, ref_cond = _oracle(sd, prediction)
    loss, arena = _engine_step(netG)
    print('%s: loss %.6f, oracle %.6f' % (prediction, loss, ref_loss))
    # what the network read: the kernel's tensor, bit for bit -- the dropped image all zeros, its level plane too
    buf = netG._cond_aug_buf.cpu()
    assert tuple(buf.shape) == (4, 4, 16, 16) and np.array_equal(buf.numpy().view(np.uint32), ref_cond.numpy().view(np.uint32))
    assert not buf[2].any() and bool((buf[1, 3] == np.float32(0.3)).all()) and torch.equal(buf[0, :3], _train_batch()[1][0])
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (loss, ref_loss)
    worst = []
    for key, grad in netG.denoise_fn.named_gradients():
        ref = ref_grads[key]
        num, den = (grad.cpu().double() - ref).norm().item(), max(ref.norm().item(), 1e-7)
        worst.append((num / den, key, den))
    worst.sort(reverse=True)
    print('%s: worst gradients (rel err, key, |ref|): %s' % (prediction, worst[:3]))
    bad = [w for w in worst if w[0] > 1e-4 and w[2] > 1e-6]
    assert not bad, bad[:8]
    # the new input plane's filters get a gradient of their own, and it is the oracle's
    gw = dict(netG.denoise_fn.named_gradients())['downs.0.weight']
    assert tuple(gw.shape) == (8, 7, 3, 3) and all(float(gw[:, c].abs().max()) > 0 for c in range(7))
    ref_plane = ref_grads['downs.0.weight'][:, 3]
    rel = (gw[:, 3].cpu().double() - ref_plane).norm().item() / ref_plane.norm().item()
    print('%s: level plane filters: gradient rel err %.3e (|ref| %.3e)' % (prediction, rel, ref_plane.norm().item()))
    assert rel <= 1e-4
    # the same step again: bitwise equal
    loss2, arena2 = _engine_step(netG)
    assert loss2 == loss and torch.equal(arena2, arena)


def test_the_draws_in_front_stay_where_they_were():
    """with the key set, a fixed seed draws the (t, gamma, z, keep) of the step without the key"""
    d = G.dev()
    netG, g, sd = _model('sr3_tiny', 'train')
    hr, sr = (t.to(d) for t in _train_batch()[:2])
    seen = []
    real = netG.denoise_fn.train_step
    netG.denoise_fn.train_step = lambda hr, cond, z, ca, cb, level, tstep, **kw: (seen.append((cond.clone(), z.clone(), level.clone())),
                                                                                 torch.tensor(0.0))[1]
    try:
        for drop, aug in ((0.5, AUG), (0.5, None), (0.0, AUG)):
            netG.set_cond_drop(drop)
            netG.set_cond_augment(**(aug or {'max_level': None}))
            np.random.seed(11)
            torch.manual_seed(12)
            netG.p_losses({'HR': hr, 'SR': sr})
    finally:
        netG.denoise_fn.train_step = real
    (c1, z1, l1), (c0, z0, l0), (c2, z2, l2) = seen
    assert tuple(c1.shape) == (4, 4, 16, 16) and tuple(c0.shape) == (4, 3, 16, 16)
    assert torch.equal(z1, z0) and torch.equal(l1, l0) and torch.equal(z2, z0) and torch.equal(l2, l0)
    keep1, keep0 = c1.flatten(1).any(1), c0.flatten(1).any(1)              # a dropped image is all zeros, under either setting
    print('kept under cond_drop 0.5: %s' % keep0.tolist())
    assert torch.equal(keep1, keep0)
    # without cond_drop: the drawn levels lie in [0, max_level) and differ between the images; every image's LR channels are noised
    lv = c2[:, 3, 0, 0]
    assert bool((lv >= 0).all()) and bool((lv < 0.5).all()) and len(set(lv.tolist())) == 4
    assert bool((c2[:, 3] == lv.view(4, 1, 1)).all()) and all(not torch.equal(c2[i, :3], sr[i]) for i in range(4))


def test_blind_at_level_zero_is_the_step_without_the_key():
    netG, g, sd = _model('sr3_tiny', 'train', wide=False)
    hr, sr, z, gamma, ceps = _train_batch()
    l0, g0 = _engine_step(netG, inject=False)
    netG.set_cond_augment(0.0, 0.0, False)
    l1, g1 = _engine_step(netG, inject=False)                              # levels and noise drawn: max_level 0 makes every level 0
    assert torch.equal(netG._cond_aug_buf.cpu(), sr)
    assert l1 == l0 and torch.equal(g1, g0)
    netG.set_cond_augment(0.5, 0.0, False)
    l2, g2 = _engine_step(netG, inject=False)
    assert l2 != l0 and not torch.equal(netG._cond_aug_buf.cpu(), sr)      # (and a level above 0 is not)
    netG.set_cond_augment(None)


# ---- 5. sampling --------------------------------------------------------------------------------------------------------------------------

def _tables(netG):
    tables, level, t_map, c3, noisy = netG._step_rule()
    tabs = {k: t.cpu().numpy() for k, t in zip(R.KEYS, tables)}
    if c3 is not None:
        tabs['c3'] = c3.cpu().numpy()
    return tabs, level.cpu().numpy(), noisy


def _close(got, want, what):
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    tol = 2e-5 * max(1.0, float(np.abs(want).max()))
    assert err <= tol, '%s: max abs err %.3e > %.3e' % (what, err, tol)
    return err


def _loop_inputs(g, d):
    cond, x_T = (torch.from_numpy(g['loop/' + n]).to(d) for n in ('sr', 'x_T'))
    ceps = torch.randn(cond.shape, generator=torch.Generator().manual_seed(77)).to(d)
    return cond, x_T, ceps


@pytest.mark.parametrize('rule', ['ancestral', 'ddim', 'dpmpp_2m'])
def test_replayed_chain_against_the_oracle(rule):
    """The replayed chain of p_sample_loop at sample_level 0.3 with the conditioning noise injected, then the same graph replayed by hand
    from the same start, every step checked against the oracle's step from the ENGINE's state before it (image, history, the z the
    graph drew) on the augmented conditioning tensor: the per-step tolerance 2e-5 max(1, |want|) applies to every step."""
    d = G.dev()
    netG, g, sd = _model('sr3_tiny', 'val')
    if rule != 'ancestral':
        netG.set_sampler(8 if rule == 'ddim' else 5, kind=rule)
    cond, x_T, ceps = _loop_inputs(g, d)
    B = cond.shape[0]
    netG.p_sample_loop(cond, continous=True, x_T=x_T, cond_noise=ceps)      # (captures)
    torch.manual_seed(17)
    out = netG.p_sample_loop(cond, continous=True, x_T=x_T, cond_noise=ceps).clone()
    st = _last_state(netG)
    assert st['graph'] is not None and st['cond_augment'] is True and tuple(st['cond'].shape) == (B, 4, 16, 16)
    # what the network reads: the kernel's tensor at level 0.3, bit for bit; what the caller gets first: the clean image
    want_cond = R.network_cond(cond.cpu(), ceps.cpu(), [0.3] * B)
    assert np.array_equal(st['cond'].cpu().numpy().view(np.uint32), want_cond.numpy().view(np.uint32))
    tabs, level, noisy = _tables(netG)
    T = len(tabs['a'])
    assert out.shape[0] == B * (T + 1) and torch.equal(out[:B], cond) and st['step'].tolist()[1] == -1
    st['img'].copy_(x_T)
    if st.get('hist') is not None:
        st['hist'].zero_()
    st['step'].fill_(T - 1)
    torch.manual_seed(17)
    desc = R.desc7('sr3_tiny')
    for k, j in enumerate(reversed(range(T))):
        x = st['img'].cpu()
        hist = st['hist'].cpu().numpy() if st.get('hist') is not None else None
        st['graph'].replay()
        torch.cuda.synchronize()
        assert torch.equal(st['img'], out[(k + 1) * B:(k + 2) * B]), 'the hand-replayed chain is not p_sample_loop\'s at step index %d' % j
        z = st['z'].cpu().numpy() if noisy else None
        new, h1 = R.sample_step(sd, desc, want_cond, x, level[j + 1], tabs, j, z, hist)
        e1 = _close(st['img'].cpu().numpy(), new, 'x after step index %d' % j)
        print('step index %d: max abs err x %.3e' % (j, e1))
    assert st['step'].tolist()[1] == -1 and bool(torch.isfinite(out).all())
    assert np.array_equal(st['cond'].cpu().numpy().view(np.uint32), want_cond.numpy().view(np.uint32))      # constant over the chain
    # replayed and eager chains are bitwise equal (the ancestral rule draws its noise: the same seed on both sides)
    netG.use_graph = False
    torch.manual_seed(17)
    eager = netG.p_sample_loop(cond, continous=True, x_T=x_T, cond_noise=ceps)
    assert torch.equal(eager, out)
    netG.use_graph = True
    # drawn, not injected: behind x_T, so the chain starts where the chain without the key starts
    torch.manual_seed(19)
    drawn = netG.p_sample_loop(cond, continous=True).clone()
    torch.manual_seed(19)
    x_T19 = torch.randn(cond.shape, device=d)
    ceps19 = torch.randn(cond.shape, device=d)
    torch.manual_seed(19)
    torch.randn(cond.shape, device=d), torch.randn(cond.shape, device=d)
    assert torch.equal(netG.p_sample_loop(cond, continous=True, x_T=x_T19, cond_noise=ceps19), drawn)


def test_blind_at_level_zero_is_the_chain_without_the_key():
    d = G.dev()
    netG, g, sd = _model('sr3_tiny', 'val', wide=False)
    cond, x_T, ceps = _loop_inputs(g, d)
    torch.manual_seed(23)
    plain = netG.p_sample_loop(cond, continous=True).clone()
    netG.set_cond_augment(0.5, 0.0, False)
    torch.manual_seed(23)
    blind = netG.p_sample_loop(cond, continous=True).clone()
    assert torch.equal(blind, plain)
    assert torch.equal(_last_state(netG)['cond'], cond)
    # and a level above zero is another chain from the same x_T, whose first snapshot is still the clean image
    netG.set_cond_augment(0.5, 0.3, False)
    torch.manual_seed(23)
    noisy = netG.p_sample_loop(cond, continous=True).clone()
    B = cond.shape[0]
    assert torch.equal(noisy[:B], cond) and not torch.equal(noisy[-B:], plain[-B:])
    st = _last_state(netG)
    assert tuple(st['cond'].shape) == tuple(cond.shape) and not torch.equal(st['cond'], cond)
    netG.set_cond_augment(None)


def test_rules_read_the_clean_image():
    """under "consistency": {"block": 8} and sample_level 0.5 the result's block means are the CLEAN conditioning image's within the bound
    of tests/test_gpu_consistency.py (1e-6 at strength 1) -- and the augmented image's block means are more than ten bounds away, so
    this cannot pass by accident"""
    from sr3_hip.diffusion import block_means
    d = G.dev()
    netG, g, sd = _model('sr3_tiny', 'val')
    netG.set_cond_augment(0.5, 0.5, True)
    netG.set_consistency(8)
    cond, x_T, ceps = _loop_inputs(g, d)
    B = cond.shape[0]
    out = netG.p_sample_loop(cond, continous=True, x_T=x_T, cond_noise=ceps)
    st = _last_state(netG)
    y = block_means(cond, 8)
    y_aug = block_means(st['cond'][:, :3].contiguous(), 8)
    assert torch.equal(st['ymean'], y) and torch.equal(out[:B], cond)
    err = float((block_means(out[-B:].contiguous(), 8) - y).abs().max())
    apart = float((y_aug - y).abs().max())
    print('consistency error against the clean image %.3e; clean and augmented block means differ by %.3e' % (err, apart))
    assert apart > 10 * 1e-6
    assert err <= 1e-6
    # back-projection makes its target from the clean image too
    from sr3_hip.diffusion import resample_f32
    netG.set_consistency(None)
    netG.set_backprojection(4)
    res = netG.p_sample_loop(cond, x_T=x_T, cond_noise=ceps)
    st = _last_state(netG)
    assert bool(torch.isfinite(res).all()) and torch.equal(st['y_lr'], resample_f32(cond, (4, 4), 'bicubic'))
    netG.set_backprojection(None)


def test_item_seeds_make_an_image_independent_of_its_batch():
    """An image's own generator draws x_T, then its conditioning noise, then every z: the augmented conditioning image of an image and its
    whole chain are the same bits alone and in a batch of 3 (at this model size the engine runs the same kernels at both batch sizes)."""
    d = G.dev()
    netG, g, sd = _model('sr3_tiny', 'val')
    gen = torch.Generator().manual_seed(5)
    cond = (torch.rand(3, 3, 16, 16, generator=gen) * 2 - 1).to(d)
    seeds = [101, 202, 303]
    three = netG.p_sample_loop(cond, continous=True, item_seeds=seeds).clone()
    cond3 = _last_state(netG)['cond'].clone()
    assert torch.equal(netG.p_sample_loop(cond, continous=True, item_seeds=seeds), three)
    assert bool((cond3[:, 3] == np.float32(0.3)).all()) and not torch.equal(cond3[:, :3], cond)
    for i, seed in enumerate(seeds):
        alone = netG.p_sample_loop(cond[i:i + 1].contiguous(), continous=True, item_seeds=[seed])
        assert torch.equal(_last_state(netG)['cond'][0], cond3[i]), i
        diff = float((three[i::3] - alone).abs().max())
        print('image %d alone against in a batch of 3: max abs diff %.3e' % (i, diff))
        assert torch.equal(three[i::3], alone), i
    assert float((three[-3] - three[-1]).abs().max()) > 1e-3


def test_tiling_cuts_the_augmented_tensor():
    from sr3_hip.tiling import TileGrid
    d = G.dev()
    netG, g, sd = _model('sr3_tiny', 'val')
    cond, x_T, ceps = _loop_inputs(g, d)
    torch.manual_seed(31)
    whole = netG.p_sample_loop(cond, continous=True, x_T=x_T, cond_noise=ceps).clone()
    # a tile that covers the image: the whole-image chain, bit for bit
    torch.manual_seed(31)
    assert torch.equal(netG.p_sample_loop_tiled(cond, continous=True, tile=16, overlap=0, x_T=x_T, cond_noise=ceps), whole)
    netG.set_tiling(32, 8)
    torch.manual_seed(31)
    assert torch.equal(netG.p_sample_loop(cond, continous=True, x_T=x_T, cond_noise=ceps), whole)
    netG.set_tiling(None)
    # two overlapping tiles per axis: the gathered conditioning tiles are slices of the augmented tensor, level plane included
    gen = torch.Generator().manual_seed(9)
    B, H, W = 2, 24, 24
    big = (torch.rand(B, 3, H, W, generator=gen) * 2 - 1).to(d)
    beps = torch.randn(B, 3, H, W, generator=gen).to(d)
    out = netG.p_sample_loop_tiled(big, continous=True, tile=16, overlap=8, cond_noise=beps)
    st = _last_state(netG)
    grid = st['grid']
    assert (grid.ny, grid.nx) == (2, 2) and tuple(st['cond_tiles'].shape) == (B * 4, 4, 16, 16)
    want = R.network_cond(big.cpu(), beps.cpu(), [0.3] * B)
    assert np.array_equal(st['cond'].cpu().numpy().view(np.uint32), want.numpy().view(np.uint32))
    for b in range(B):
        for iy in range(2):
            for ix in range(2):
                sy, sx = grid.slices(iy, ix)
                assert torch.equal(st['cond_tiles'][grid.tile_index(b, iy, ix)], st['cond'][b, :, sy, sx]), (b, iy, ix)
    assert torch.equal(out[:B], big) and bool(torch.isfinite(out).all())


def test_blind_form_goes_with_self_conditioning():
    """a 9-channel self-conditioned model under the blind form: the LR channels of the state's cond are the augmented image, the
    self-conditioning channels behind them are written by every step as before; the training step reads the augmented LR channels too"""
    import model as Model
    import selfcond_ref as SC
    d = G.dev()
    m = Model.create_model(SC.opt9('sr3_tiny', phase='train', prob=0.5, cond_augment={'max_level': 0.5, 'sample_level': 0.3, 'level_channel': False}))
    g, sd = SC.widened('sr3_tiny')
    m.netG.load_state_dict(sd, strict=True)
    netG = m.netG
    netG.show_progress = False
    cond, x_T, ceps = _loop_inputs(g, d)
    B = cond.shape[0]
    outs = []
    for use_graph in (False, True):
        netG.use_graph = use_graph
        torch.manual_seed(43)
        outs.append(netG.p_sample_loop(cond, continous=True, x_T=x_T, cond_noise=ceps).clone())
    st = _last_state(netG)
    want = R.network_cond(cond.cpu(), ceps.cpu(), [0.3] * B, level_channel=False)
    assert tuple(st['cond'].shape) == (B, 6, 16, 16) and st['self_condition'] and st['cond_augment']
    assert np.array_equal(st['cond'][:, :3].cpu().numpy().view(np.uint32), want.numpy().view(np.uint32)) and bool(st['cond'][:, 3:].any())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1][:B], cond) and bool(torch.isfinite(outs[1]).all())
    hr, sr, z, gamma, teps = _train_batch()
    loss = netG.p_losses({'HR': hr.to(d), 'SR': sr.to(d)}, noise=z.to(d), gamma=gamma, cond_level=T_LEVELS, cond_noise=teps.to(d),
                         cond_keep=T_KEEP, self_cond=[1, 0, 1, 1])
    twant = R.network_cond(sr, teps, T_LEVELS, T_KEEP, level_channel=False)
    buf = netG._self_cond_buf.cpu()
    assert bool(torch.isfinite(loss)) and np.array_equal(buf[:, :3].numpy().view(np.uint32), twant.numpy().view(np.uint32))
    assert bool(buf[0, 3:].any()) and not bool(buf[1, 3:].any())


def test_guided_chain_reads_an_all_zero_second_condition():
    d = G.dev()
    netG, g, sd = _model('sr3_tiny', 'val')
    netG.set_guidance(1.5, 'static')
    cond, x_T, ceps = _loop_inputs(g, d)
    B = cond.shape[0]
    outs = []
    for use_graph in (False, True):
        netG.use_graph = use_graph
        torch.manual_seed(37)
        outs.append(netG.p_sample_loop(cond, continous=True, x_T=x_T, cond_noise=ceps).clone())
    st = _last_state(netG)
    assert tuple(st['cond0'].shape) == (B, 4, 16, 16) and not bool(st['cond0'].any())      # the level plane too: a dropped training image
    assert bool((st['cond'][:, 3] == np.float32(0.3)).all())
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[1]).all()) and st['step'].tolist()[1] == -1
    assert torch.equal(outs[1][:B], cond)
    netG.set_guidance(None)
