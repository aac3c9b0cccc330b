"""EMA of the weights on the GPU: the fused Adam+EMA kernel (sr3_adam_ema_step, through the C ABI) against sr3_adam_step and a
float64 lerp, and the model-level behaviour -- the EMA trajectory over optimizer steps, validation on the EMA weights while training
goes on undisturbed, and learning-rate warm-up.

The bound of the lerp, for every element: w = fp32(1 - decay), r = e + (p_new - e) * double(w) in float64;
|ema_out - r| <= 2^-23 * max(|e|, |p_new|).  The rounding of w, the subtraction, the product and the sum are each within 2^-24
relative; their total is below 2^-24 * (1 + 8 w) * max(|e|, |p_new|) < 2^-23 for w <= 0.1; a fused multiply-add only lowers it."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_golden, opt_for                      # noqa: E402
import gpu_util as G                                             # noqa: E402
from sr3_hip import lib as L                                     # noqa: E402

HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
# 4: one vector; 1028: a ragged second block; 16 778 252 = 4 * (2 * 8192 * 256 + 259): the grid is capped at 8192 x 256 threads, so
# the grid-stride loop wraps twice and ends in a ragged tail
SIZES = [4, 1028, 16778252]


def f(v):
    return C.c_float(v)


def adam(p, g, m, v, step, n=None):
    return L.load().sr3_adam_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel() if n is None else n, f(HYPER['lr']),
                                  f(HYPER['b1']), f(HYPER['b2']), f(HYPER['eps']), step, G.stream())


def adam_ema(p, g, m, v, ema, step, decay, mode, n=None):
    return L.load().sr3_adam_ema_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(ema), p.numel() if n is None else n,
                                      f(HYPER['lr']), f(HYPER['b1']), f(HYPER['b2']), f(HYPER['eps']), step, f(decay), mode,
                                      G.stream())


def inputs(n, seed):
    gen = torch.Generator(device=G.dev()).manual_seed(seed)
    p = torch.randn(n, device=G.dev(), generator=gen)
    g = torch.randn(n, device=G.dev(), generator=gen) * 0.1
    m = torch.randn(n, device=G.dev(), generator=gen) * 0.1
    v = torch.rand(n, device=G.dev(), generator=gen) * 0.01
    ema = torch.randn(n, device=G.dev(), generator=gen)
    return p, g, m, v, ema


def lerp_bound_violations(ema_out, e, p_new, decay):
    """Elements outside |ema_out - r| <= 2^-23 max(|e|, |p_new|) (see the module docstring); float64 on the device."""
    w = float(np.float32(1.0 - decay))
    e64, p64 = e.double(), p_new.double()
    r = e64 + (p64 - e64) * w
    bound = 2.0 ** -23 * torch.maximum(e64.abs(), p64.abs())
    return int(((ema_out.double() - r).abs() > bound).sum().item())


@pytest.mark.parametrize('step', [1, 7])
@pytest.mark.parametrize('n', SIZES)
def test_fused_step_matches_adam_and_float64_lerp(n, step):
    p, g, m, v, ema = inputs(n, 1000 + n % 997 + step)
    # a slice with zero gradient and zero moments keeps its weights (p_new = p); with ema = p there, mode 2 must return it unchanged
    lo, hi = n // 4, n // 2
    g[lo:hi] = 0
    m[lo:hi] = 0
    v[lo:hi] = 0
    ema[lo:hi] = p[lo:hi]
    rp, rm, rv = p.clone(), m.clone(), v.clone()                 # the reference, once: sr3_adam_step on copies of the same inputs
    assert adam(rp, g, rm, rv, step) == 0
    assert torch.equal(rp[lo:hi], p[lo:hi]) and not torch.equal(rp, p)

    def run(mode, decay, with_ema=True):
        q, qm, qv, qe = p.clone(), m.clone(), v.clone(), (ema.clone() if with_ema else None)
        L.check(adam_ema(q, g, qm, qv, qe, step, decay, mode))
        assert torch.equal(q, rp) and torch.equal(qm, rm) and torch.equal(qv, rv), 'Adam outputs differ from sr3_adam_step (mode %d)' % mode
        return qe

    assert run(0, 0.9999, with_ema=False) is None               # mode 0: ema = NULL is accepted
    assert torch.equal(run(0, 0.9999), ema)                      # ... and a given one is untouched
    assert torch.equal(run(1, 0.9999), rp)                       # mode 1: an exact copy of the new weights
    for decay in (0.9999, 0.9):
        out = run(2, decay)
        print('n %d step %d decay %g: max |ema_out - ema| %.3e' % (n, step, decay, float((out - ema).abs().max())))
        assert lerp_bound_violations(out, ema, rp, decay) == 0
        assert torch.equal(out[lo:hi], ema[lo:hi])               # p_new == ema: unchanged exactly
        assert not torch.equal(out, ema)
    torch.cuda.synchronize()


def test_bad_arguments_are_refused_and_touch_nothing():
    n = 1028
    p, g, m, v, ema = inputs(n, 77)
    keep = [t.clone() for t in (p, g, m, v, ema)]
    lib = L.load()
    cases = [
        ('ema is NULL', dict(ema=None, mode=1)), ('ema is NULL', dict(ema=None, mode=2)),
        ('ema_mode', dict(mode=3)), ('ema_mode', dict(mode=-1)),
        ('ema_decay', dict(decay=1.0)), ('ema_decay', dict(decay=-0.1)), ('ema_decay', dict(decay=float('nan'))),
        ('n ', dict(n=n - 2)), ('step', dict(step=0)),
    ]
    for word, kw in cases:
        a = dict(ema=ema, step=3, decay=0.9, mode=2, n=n)
        a.update(kw)
        rc = adam_ema(p, g, m, v, a['ema'], a['step'], a['decay'], a['mode'], n=a['n'])
        msg = (lib.sr3_last_error() or b'').decode()
        assert rc == -1, (kw, rc)                                # SR3_E_BADARG
        assert 'sr3_adam_ema_step: ' + word in msg, (kw, msg)
        torch.cuda.synchronize()
        assert all(torch.equal(a_, b_) for a_, b_ in zip((p, g, m, v, ema), keep)), kw


# ---- model level: sr3_tiny, the draws of a training step injected as tests/test_gpu_train.py does ---------------------------------
def build(ema=None, warmup_steps=0, phase='train'):
    import model as Model
    opt = opt_for('sr3_tiny', phase=phase, gpu=True)
    if ema is not None:
        opt['train']['ema_scheduler'] = dict(ema)
    if warmup_steps:
        opt['train']['optimizer']['warmup_steps'] = warmup_steps
    m = Model.create_model(opt)
    g, sd = load_golden('sr3_tiny')
    m.netG.load_state_dict(sd, strict=True)
    un = m.netG.denoise_fn
    if un.ema_arena is not None:
        un.ema_from_weights()                                    # the EMA starts from the weights the model starts from
    m.netG.show_progress = False
    z, gamma = torch.from_numpy(g['train/z']).to(G.dev()), torch.from_numpy(g['train/gamma'])
    orig = m.netG.p_losses
    m.netG.p_losses = lambda x_in, noise=None: orig(x_in, noise=z, gamma=gamma)
    m.golden = g
    return m


def train_step(m):
    m.feed_data({'HR': torch.from_numpy(m.golden['loop/hr']), 'SR': torch.from_numpy(m.golden['loop/sr'])})
    m.optimize_parameters()


def weights(m):
    return {k: v for k, v in m.netG.state_dict().items() if k.startswith('denoise_fn.')}


def ema_weights(m):
    return m.netG.denoise_fn.ema_state_dict('denoise_fn.')


def same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def same_training_state(a, b):
    return (torch.equal(a.netG.denoise_fn.arena.data, b.netG.denoise_fn.arena.data) and torch.equal(a.optG.exp_avg, b.optG.exp_avg)
            and torch.equal(a.optG.exp_avg_sq, b.optG.exp_avg_sq) and a.optG.step_count == b.optG.step_count)


def test_ema_trajectory_over_four_steps():
    m = build(ema=dict(enabled=True, step_start_ema=3, update_ema_every=1, ema_decay=0.9))
    plain = build()
    assert plain.netG.denoise_fn.ema_arena is None
    ptr = m.netG.denoise_fn.ema_arena.data_ptr()
    for s in (1, 2, 3, 4):
        prev = ema_weights(m)
        train_step(m)
        train_step(plain)
        new, ema = weights(m), ema_weights(m)
        if s < 3:
            assert same(ema, new), 'step %d: the EMA is not a copy of the weights' % s
        else:
            bad = sum(lerp_bound_violations(ema[k], prev[k], new[k], 0.9) for k in ema)
            assert bad == 0, 'step %d: %d elements outside the lerp bound' % (s, bad)
            assert not same(ema, new) and not same(ema, prev)
    assert m.netG.denoise_fn.ema_arena.data_ptr() == ptr
    assert same_training_state(m, plain), 'EMA changed the training trajectory'


def test_update_ema_every_two_steps():
    m = build(ema=dict(enabled=True, step_start_ema=1, update_ema_every=2, ema_decay=0.9))
    for s in (1, 2, 3, 4):
        prev = ema_weights(m)
        train_step(m)
        assert same(ema_weights(m), prev) == (s % 2 == 1), 'step %d' % s


def test_validation_runs_on_ema_weights_and_leaves_training_alone():
    ema_opt = dict(enabled=True, step_start_ema=1, update_ema_every=1, ema_decay=0.9)
    a, b = build(ema=ema_opt), build(ema=ema_opt)
    g = a.golden
    val = {'HR': torch.from_numpy(g['loop/hr']), 'SR': torch.from_numpy(g['loop/sr'])}

    def sample(m):
        m.feed_data(dict(val))
        torch.manual_seed(5)
        m.test(continous=False)
        return m.SR.clone()

    for _ in range(2):
        train_step(a)
    ema_then, live_then = ema_weights(a), weights(a)
    assert not same(ema_then, live_then)
    img = sample(a)
    assert a.netG.training
    cache = a.netG._loop_cache
    assert len(cache) == 1
    key, graph = next(iter(cache.keys())), next(iter(cache.values()))['graph']
    assert graph is not None and key[4] == a.netG.denoise_fn.ema_arena.data_ptr()
    train_step(a)
    for _ in range(3):
        train_step(b)
    assert same_training_state(a, b), 'a validation pass changed the training trajectory'
    assert torch.equal(a.netG.denoise_fn.ema_arena, b.netG.denoise_fn.ema_arena)
    # the image is the one a val-phase model gives with the EMA weights of that moment -- and not the one the live weights gave
    v = build(phase='val')
    v.netG.load_state_dict(ema_then, strict=False)
    ref = sample(v)
    assert torch.isfinite(img).all() and torch.equal(img, ref)
    v.netG.load_state_dict(live_then, strict=False)
    assert not torch.equal(img, sample(v))
    # the next validation replays the graph captured by the first: the optimizer step in between moved no address
    img2 = sample(a)
    assert list(a.netG._loop_cache.keys()) == [key] and a.netG._loop_cache[key]['graph'] is graph
    assert not torch.equal(img2, img)                            # (the EMA moved with the third step)
    assert same_training_state(a, b)


def test_linear_warmup_scales_the_learning_rate():
    m, hand = build(warmup_steps=4), build()
    lr = hand.optG.defaults['lr']
    for s in (1, 2, 3):
        train_step(m)
        hand.optG.defaults['lr'] = lr * s / 4
        train_step(hand)
        assert same_training_state(m, hand), 'step %d' % s
    assert m.optG.defaults['lr'] == lr and m.optG.state_dict()['param_groups'][0]['lr'] == lr
    base = build()
    train_step(base)
    assert not torch.equal(base.netG.denoise_fn.arena.data, m.netG.denoise_fn.arena.data)      # (warm-up really changed the steps)
