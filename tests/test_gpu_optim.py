"""Gradient accumulation and global-norm clipping on the GPU (config train.optimizer.accumulate / clip_grad_norm): the three entry
points through the C ABI -- sr3_grad_norm, sr3_grad_accumulate, sr3_adam_ema_step_scaled -- and the model-level behaviour on the tiny
fixtures, the draws of a training step injected as tests/test_gpu_train.py does.

Bounds.  Norm: |norm - ref| <= 2^-22 ref against float64 numpy -- the result is rounded to fp32 once (2^-24); the double
accumulation of n <= 2.7e6 non-negative terms (squares of fp32 are exact in double) adds below n * 2^-53 < 1e-9.  coef: 2^-22
relative against what torch.nn.utils.clip_grad_norm_ does to a float64 copy, max_norm being an fp32 value on both sides: the fp32
norm, the sum with 1e-6f and the division round once each (3 * 2^-24).  Everything else is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import DESCS, load_golden, opt_for                  # noqa: E402
import gpu_util as G                                             # noqa: E402
from sr3_hip import lib as L                                     # noqa: E402

EPS22 = 2.0 ** -22
GRID_ROUND = 512 * 256 * 4          # floats one grid-stride round of the fixed norm / accumulate grid covers
# 4: one vector; 1020: under one block; one full round + 4: the ragged tail; 2^20 + 4: two rounds and a tail; five rounds + 4: the
# four-deep unrolled loop runs once and hands a round and a tail to the plain one
SIZES = [4, 1020, GRID_ROUND + 4, 2 ** 20 + 4, 5 * GRID_ROUND + 4]
HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


def f(v):
    return C.c_float(v)


def heavy(n, seed):
    """randn * 10^U(-6, 2): eight decades of magnitudes in one array."""
    gen = torch.Generator(device=G.dev()).manual_seed(seed)
    return torch.randn(n, device=G.dev(), generator=gen) * 10.0 ** (torch.rand(n, device=G.dev(), generator=gen) * 8 - 6)


def scratch_for(n):
    nb = int(L.load().sr3_grad_norm_scratch_bytes(n))
    return torch.empty(nb, dtype=torch.uint8, device=G.dev()), nb


def grad_norm(g, max_norm=0.0):
    out4 = torch.full((4,), float('nan'), device=G.dev())
    s, nb = scratch_for(g.numel())
    L.check(L.load().sr3_grad_norm(L.ptr(g), g.numel(), f(max_norm), L.ptr(s), nb, L.ptr(out4), G.stream()))
    return out4


def accumulate(acc, g, first, max_norm=0.0, with_norm=False):
    out4 = torch.full((4,), float('nan'), device=G.dev()) if with_norm else None
    s, nb = scratch_for(g.numel())
    L.check(L.load().sr3_grad_accumulate(L.ptr(acc), L.ptr(g), g.numel(), int(first), f(max_norm), L.ptr(s), nb, L.ptr(out4), G.stream()))
    return out4


def bits(t):
    return t.view(torch.int32)


def norm64(g):
    x = g.cpu().numpy().astype(np.float64)
    return float(np.sqrt(np.sum(x * x)))


@pytest.fixture(scope='module')
def arrays():
    """Per size: the heavy-tailed array and its float64 norm, computed once."""
    out = {}
    for n in SIZES:
        g = heavy(n, 100 + n % 1009)
        out[n] = (g, norm64(g))
    return out


@pytest.mark.parametrize('n', SIZES)
def test_norm_against_float64(n, arrays):
    g, ref = arrays[n]
    o = grad_norm(g).cpu()
    print('n %d: norm %.9g ref %.9g rel %.3e' % (n, o[0], ref, abs(float(o[0]) - ref) / ref))
    assert abs(float(o[0]) - ref) <= EPS22 * ref
    assert o[1] == 1.0 and o[2] == 1.0 and o[3] == 0.0          # max_norm <= 0: norm only
    z = grad_norm(torch.zeros(n, device=G.dev()), max_norm=1.0).cpu()
    assert z.tolist() == [0.0, 1.0, 1.0, 0.0]
    for bad in (float('inf'), float('nan')):
        h = g.clone()
        h[-1] = bad
        b = grad_norm(h, max_norm=1.0).cpu()
        assert b[2] == 0.0 and not np.isfinite(float(b[0])) and b[3] == 0.0, (bad, b)


@pytest.mark.parametrize('n', SIZES)
def test_coef_against_torch_clip_grad_norm(n, arrays):
    g, ref = arrays[n]
    g64 = g.cpu().double()
    k = int(g64.abs().argmax())
    for max_norm in (float(np.float32(0.5 * ref)), float(np.float32(2.0 * ref)), 1.0):
        p = torch.nn.Parameter(torch.zeros(n, dtype=torch.float64))
        p.grad = g64.clone()
        torch.nn.utils.clip_grad_norm_([p], max_norm)
        want = float(p.grad[k] / g64[k])                         # the factor torch applied
        o = grad_norm(g, max_norm=max_norm).cpu()
        print('n %d max_norm %.6g: coef %.9g torch %.9g' % (n, max_norm, o[1], want))
        assert abs(float(o[1]) - want) <= EPS22 * want
        assert o[2] == 1.0
        if max_norm > 1.001 * (ref + 1e-6):                      # (torch's coefficient carries the 1e-6 too)
            assert float(o[1]) == 1.0


@pytest.mark.parametrize('n', SIZES)
def test_accumulate_and_fused_norm_bits(n, arrays):
    g1 = arrays[n][0]
    g2, g3 = heavy(n, 7 + n % 13), heavy(n, 9 + n % 17)
    acc = torch.full((n,), float('nan'), device=G.dev())
    assert accumulate(acc, g1, first=True) is None
    assert torch.equal(acc, g1)
    accumulate(acc, g2, first=False)
    s12 = g1 + g2
    assert torch.equal(acc, s12)
    fused = accumulate(acc, g3, first=False, max_norm=1.0, with_norm=True)
    assert torch.equal(acc, s12 + g3)
    alone = grad_norm(acc, max_norm=1.0)
    assert torch.equal(bits(fused), bits(alone)) and torch.equal(bits(alone), bits(grad_norm(acc, max_norm=1.0)))
    assert abs(float(alone[0]) - norm64(acc)) <= EPS22 * norm64(acc)
    # first = 1 with the norm riding along; a NaN in the sum clears the flag in both forms, with the same bits
    acc2 = torch.full((n,), float('nan'), device=G.dev())
    assert torch.equal(bits(accumulate(acc2, g1, first=True, with_norm=True)), bits(grad_norm(g1))) and torch.equal(acc2, g1)
    g3[-1] = float('nan')
    fused = accumulate(acc2, g3, first=False, with_norm=True)
    assert float(fused[2]) == 0.0 and torch.equal(bits(fused), bits(grad_norm(acc2)))
    torch.cuda.synchronize()


# ---- the scaled, guarded Adam(+EMA) step ---------------------------------------------------------------------------------------
def adam_inputs(n, seed):
    gen = torch.Generator(device=G.dev()).manual_seed(seed)
    r = lambda s: torch.randn(n, device=G.dev(), generator=gen) * s
    return r(1.0), r(0.1), r(0.1), torch.rand(n, device=G.dev(), generator=gen) * 0.01, r(1.0)      # p, g, m, v, ema


def adam_ema(bufs, g, step, mode, scale4=None, decay=0.9, n=None):
    p, m, v, ema = bufs
    a = [L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(ema), p.numel() if n is None else n, f(HYPER['lr']), f(HYPER['b1']),
         f(HYPER['b2']), f(HYPER['eps']), step, f(decay), mode]
    if scale4 is None:
        return L.load().sr3_adam_ema_step(*a, G.stream())
    return L.load().sr3_adam_ema_step_scaled(*a, L.ptr(scale4), G.stream())


# 8 389 644 = 4 * (8192 * 256 + 259): the Adam grid is capped at 8192 x 256 threads: one wrap of the grid-stride loop and a ragged tail
@pytest.mark.parametrize('step', [1, 1000])
@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('n', [4, 1028, 8389644])
def test_scaled_adam_bits(n, mode, step):
    p, g, m, v, ema = adam_inputs(n, 31 + n % 101 + step)
    fresh = lambda: [t.clone() for t in (p, m, v, ema)]
    for coef in (1.0, 0.37109375, float(np.float32(1e-3 / 3))):
        scale4 = torch.tensor([123.0, coef, 1.0, 0.0], device=G.dev())
        want, got = fresh(), fresh()
        L.check(adam_ema(want, g * scale4[1], step, mode))          # torch's fp32 product, then the unscaled entry
        L.check(adam_ema(got, g, step, mode, scale4=scale4))
        assert all(torch.equal(a, b) for a, b in zip(got, want)), 'coef %g' % coef
        assert not torch.equal(got[0], p)
    off = torch.tensor([float('inf'), 0.5, 0.0, 0.0], device=G.dev())
    got = fresh()
    L.check(adam_ema(got, g, step, mode, scale4=off))
    assert all(torch.equal(a, b) for a, b in zip(got, (p, m, v, ema))), 'flag 0 wrote something'
    torch.cuda.synchronize()


def adam_plain(p, g, m, v, step, n=None):
    return L.load().sr3_adam_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel() if n is None else n, f(HYPER['lr']), f(HYPER['b1']),
                                  f(HYPER['b2']), f(HYPER['eps']), step, G.stream())


# 8 388 612 = 4 * (8192 * 256 + 1): the capped grid wraps once and thread 0 alone takes a second vector
@pytest.mark.parametrize('n', [4, 4 * (256 * 8192 + 1)])
def test_three_adam_entries_are_one_pass(n):
    """sr3_adam_step, sr3_adam_ema_step and sr3_adam_ema_step_scaled run one kernel template: the same bits in p / m / v through all
    three in every EMA mode, the unscaled entry's ema through the scaled one at coef 1, nothing written at flag 0, and the plain
    entry refuses a misaligned pointer as the other two do."""
    step = 7
    pad = adam_inputs(n + 4, 53 + n % 89)                        # four floats more: the views from element 1 are 4 bytes off
    p, g, m, v, ema = (t[:n] for t in pad)
    rp, rm, rv = p.clone(), m.clone(), v.clone()
    L.check(adam_plain(rp, g, rm, rv, step))
    assert not torch.equal(rp, p)
    on = torch.tensor([55.0, 1.0, 1.0, 0.0], device=G.dev())
    off = torch.tensor([55.0, 1.0, 0.0, 0.0], device=G.dev())
    for mode in (0, 1, 2):
        a, b, c = ([t.clone() for t in (p, m, v, ema)] for _ in range(3))
        L.check(adam_ema(a, g, step, mode))
        L.check(adam_ema(b, g, step, mode, scale4=on))
        L.check(adam_ema(c, g, step, mode, scale4=off))
        for got in (a, b):
            assert all(torch.equal(bits(x), bits(y)) for x, y in zip(got[:3], (rp, rm, rv))), 'mode %d' % mode
        assert torch.equal(bits(b[3]), bits(a[3])), 'ema, mode %d' % mode
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(c, (p, m, v, ema))), 'flag 0 wrote something (mode %d)' % mode
    keep = [t.clone() for t in pad]
    rc = adam_plain(pad[0][1:n + 1], g, m, v, step)
    assert rc == -3 and b'sr3_adam_step: misaligned' in L.load().sr3_last_error(), rc          # SR3_E_ALIGN
    torch.cuda.synchronize()
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(pad, keep)), 'a refused call wrote something'


def test_bad_arguments_are_refused_and_touch_nothing():
    n = 1028
    lib = L.load()
    p, g, m, v, ema = adam_inputs(n, 5)
    scale4 = torch.tensor([1.0, 0.5, 1.0, 0.0], device=G.dev())
    out4 = torch.full((4,), 7.0, device=G.dev())
    s, nb = scratch_for(n)
    s.zero_()
    live = (p, g, m, v, ema, scale4, out4, s)
    keep = [t.clone() for t in live]

    def refused(rc, entry, word, code=-1):
        msg = (lib.sr3_last_error() or b'').decode()
        assert rc == code, (entry, word, rc)
        assert entry + ': ' in msg and word in msg, (entry, word, msg)
        torch.cuda.synchronize()
        assert all(torch.equal(bits(a), bits(b)) if a.dtype == torch.float32 else torch.equal(a, b) for a, b in zip(live, keep)), (entry, word)

    bufs = (p, m, v, ema)
    E = 'sr3_adam_ema_step_scaled'
    refused(lib.sr3_adam_ema_step_scaled(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(ema), n, f(1e-3), f(0.9), f(0.999), f(1e-8), 3,
                                         f(0.9), 2, None, G.stream()), E, 'scale4_dev is NULL')
    refused(adam_ema((p, m, v, None), g, 3, 2, scale4=scale4), E, 'ema is NULL')
    refused(adam_ema(bufs, None, 3, 2, scale4=scale4), E, 'grads')
    refused(adam_ema(bufs, g, 3, 3, scale4=scale4), E, 'ema_mode')
    refused(adam_ema(bufs, g, 3, 2, scale4=scale4, decay=1.0), E, 'ema_decay')
    refused(adam_ema(bufs, g, 3, 2, scale4=scale4, n=n - 2), E, 'n ')
    refused(adam_ema(bufs, g, 0, 2, scale4=scale4), E, 'step')
    refused(adam_ema(bufs, g, 3, 2, scale4=out4[1:]), E, 'misaligned', code=-3)
    E = 'sr3_grad_norm'
    st = G.stream()
    refused(lib.sr3_grad_norm(None, n, f(1.0), L.ptr(s), nb, L.ptr(out4), st), E, 'grads is NULL')
    refused(lib.sr3_grad_norm(L.ptr(g), n, f(1.0), None, nb, L.ptr(out4), st), E, 'scratch is NULL')
    refused(lib.sr3_grad_norm(L.ptr(g), n, f(1.0), L.ptr(s), nb, None, st), E, 'out4_dev is NULL')
    refused(lib.sr3_grad_norm(L.ptr(g), n - 2, f(1.0), L.ptr(s), nb, L.ptr(out4), st), E, 'n ')
    refused(lib.sr3_grad_norm(L.ptr(g), n, f(float('nan')), L.ptr(s), nb, L.ptr(out4), st), E, 'max_norm')
    refused(lib.sr3_grad_norm(L.ptr(g), n, f(1.0), L.ptr(s), nb - 1, L.ptr(out4), st), E, 'scratch_bytes')
    refused(lib.sr3_grad_norm(L.ptr(g[1:]), n - 4, f(1.0), L.ptr(s), nb, L.ptr(out4), st), E, 'misaligned', code=-3)
    E = 'sr3_grad_accumulate'
    refused(lib.sr3_grad_accumulate(None, L.ptr(g), n, 0, f(1.0), L.ptr(s), nb, L.ptr(out4), st), E, 'acc is NULL')
    refused(lib.sr3_grad_accumulate(L.ptr(p), None, n, 0, f(1.0), L.ptr(s), nb, L.ptr(out4), st), E, 'g is NULL')
    refused(lib.sr3_grad_accumulate(L.ptr(p), L.ptr(g), n - 2, 0, f(1.0), L.ptr(s), nb, L.ptr(out4), st), E, 'n ')
    refused(lib.sr3_grad_accumulate(L.ptr(p), L.ptr(g), n, 0, f(1.0), None, nb, L.ptr(out4), st), E, 'scratch is NULL')
    refused(lib.sr3_grad_accumulate(L.ptr(p), L.ptr(g), n, 0, f(1.0), L.ptr(s), 0, L.ptr(out4), st), E, 'scratch_bytes')
    refused(lib.sr3_grad_accumulate(L.ptr(p), L.ptr(g), n, 0, f(float('nan')), L.ptr(s), nb, L.ptr(out4), st), E, 'max_norm')
    refused(lib.sr3_grad_accumulate(L.ptr(p), L.ptr(g[1:]), n - 4, 0, f(1.0), L.ptr(s), nb, L.ptr(out4), st), E, 'misaligned', code=-3)


# ---- model level: sr3_tiny / ddpm_tiny ----------------------------------------------------------------------------------------------
EMA = dict(enabled=True, step_start_ema=1, update_ema_every=1, ema_decay=0.9)


def build(name='sr3_tiny', ema=None, **optimizer_keys):
    """A train-phase model on the golden weights whose p_losses takes the recorded draws; `m.draws['z']` may be swapped between steps."""
    import model as Model
    opt = opt_for(name, phase='train', gpu=True)
    opt['train']['optimizer'].update(optimizer_keys)
    if ema is not None:
        opt['train']['ema_scheduler'] = dict(ema)
    m = Model.create_model(opt)
    g, sd = load_golden(name)
    m.netG.load_state_dict(sd, strict=True)
    if m.netG.denoise_fn.ema_arena is not None:
        m.netG.denoise_fn.ema_from_weights()
    d = G.dev()
    kw = dict(gamma=torch.from_numpy(g['train/gamma'])) if DESCS[name]['variant'] == 'sr3' else dict(t=torch.from_numpy(g['train/t']).to(d))
    m.draws = dict(z=torch.from_numpy(g['train/z']).to(d), kw=kw)
    orig = m.netG.p_losses
    m.netG.p_losses = lambda x_in, noise=None: orig(x_in, noise=m.draws['z'], **m.draws['kw'])
    m.golden = g
    return m


def second_draw(m):
    z = m.draws['z']
    return torch.randn(z.shape, generator=torch.Generator().manual_seed(11)).to(z.device)


def feed(m):
    m.feed_data({'HR': torch.from_numpy(m.golden['loop/hr']), 'SR': torch.from_numpy(m.golden['loop/sr'])})


def train_step(m, z=None):
    if z is not None:
        m.draws['z'] = z
    feed(m)
    m.optimize_parameters()


def state(m):
    un = m.netG.denoise_fn
    s = [un.arena.data, m.optG.exp_avg, m.optG.exp_avg_sq]
    return s + ([un.ema_arena] if un.ema_arena is not None else [])


def same_state(a, b):
    return a.optG.step_count == b.optG.step_count and all(torch.equal(x, y) for x, y in zip(state(a), state(b)))


def gradient_of(m, z=None, grad_scale_div=1):
    """grad_arena a stand-alone train_step leaves for the fixture batch (with grad_scale = 1 / (grad_scale_div * b c h w))."""
    un = m.netG.denoise_fn
    if z is not None:
        m.draws['z'] = z
    feed(m)
    b, c, h, w = m.data['HR'].shape
    orig = un.train_step
    un.train_step = lambda *a, grad_scale, **kw: orig(*a, grad_scale=1.0 / (grad_scale_div * b * c * h * w), **kw)
    try:
        m.netG(m.data)
    finally:
        un.train_step = orig
    return un.grad_arena.clone()


@pytest.mark.parametrize('name', ['sr3_tiny', 'ddpm_tiny'])
def test_two_micro_batches_against_separate_steps(name):
    m, ref = build(name, accumulate=2), build(name)
    un = m.netG.denoise_fn
    z1, z2 = m.draws['z'], second_draw(m)
    w0, epoch0 = un.arena.data.clone(), un._weights_epoch
    train_step(m, z1)
    assert torch.equal(un.arena.data, w0) and m.optG.step_count == 0 and m.optG.micro_count == 1 and un._weights_epoch == epoch0
    assert m.optG.exp_avg is None
    train_step(m, z2)
    g1, g2 = gradient_of(ref, z1, 2), gradient_of(ref, z2, 2)
    assert not torch.equal(g1, g2)
    want = g1 + g2
    assert torch.equal(m.optG.grad_acc, want)
    assert m.optG.step_count == 1 and un._weights_epoch == epoch0 + 1
    # exactly one Adam step, on that sum
    rp, rm, rv = w0.clone(), torch.zeros_like(w0), torch.zeros_like(w0)
    L.check(L.load().sr3_adam_step(L.ptr(rp), L.ptr(want), L.ptr(rm), L.ptr(rv), rp.numel(), f(1e-4), f(0.9), f(0.999), f(1e-8), 1, G.stream()))
    assert torch.equal(un.arena.data, rp) and torch.equal(m.optG.exp_avg, rm) and torch.equal(m.optG.exp_avg_sq, rv)
    assert not torch.equal(rp, w0)
    # the third micro-batch opens a new sum
    train_step(m, z1)
    assert m.optG.step_count == 1 and torch.equal(un.arena.data, rp) and not torch.equal(m.optG.grad_acc, want)


@pytest.mark.parametrize('name', ['sr3_tiny', 'ddpm_tiny'])
def test_same_micro_batch_twice_matches_golden_gradients(name):
    """The mean over two copies of the fixture batch is the fixture's gradient: the criterion of
    tests/test_gpu_train.py::test_loss_and_gradients_match_reference_autograd on the accumulated arena."""
    m = build(name, accumulate=2)
    train_step(m)
    train_step(m)
    un = m.netG.denoise_fn
    bad = []
    for e in un.plan.table:
        ref = torch.from_numpy(m.golden['grad/denoise_fn.' + e['name']])
        got = un.plan.view(m.optG.grad_acc, e).cpu()
        assert got.shape == ref.shape, e['name']
        num, den = (got - ref).norm().item(), max(ref.norm().item(), 1e-7)
        if num / den > 1e-4 and den > 1e-6:
            bad.append((num / den, e['name'], den))
    assert not bad, sorted(bad, reverse=True)[:8]


def test_clipping_matches_adam_on_the_scaled_gradient():
    plain = build(ema=EMA)
    g = gradient_of(plain)
    ref_norm = norm64(g)
    clip = float(np.float32(0.5 * ref_norm))
    m = build(ema=EMA, clip_grad_norm=clip)
    train_step(m)
    log = m.get_current_log()
    print('grad_norm %.9g ref %.9g' % (log['grad_norm'], ref_norm))
    assert abs(log['grad_norm'] - ref_norm) <= EPS22 * ref_norm
    assert abs(log['l_pix'] - float(m.golden['train/l_pix'])) <= 1e-5 * abs(float(m.golden['train/l_pix']))
    n4 = m.optG.norm4.cpu()
    want = clip / (ref_norm + 1e-6)
    assert float(n4[0]) == log['grad_norm'] and abs(float(n4[1]) - want) <= EPS22 * want and float(n4[2]) == 1.0
    assert torch.equal(m.netG.denoise_fn.grad_arena, g)
    un = plain.netG.denoise_fn
    plain.optG._moments(un.arena.data)
    plain.optG.step_count = 1
    L.check(adam_ema_model(plain, g * m.optG.norm4[1], 1, 2))
    assert same_state(m, plain)
    assert 'grad_norm' not in build().get_current_log()


def adam_ema_model(m, grads, step, mode):
    un = m.netG.denoise_fn
    return L.load().sr3_adam_ema_step(L.ptr(un.arena.data), L.ptr(grads), L.ptr(m.optG.exp_avg), L.ptr(m.optG.exp_avg_sq), L.ptr(un.ema_arena),
                                      grads.numel(), f(1e-4), f(0.9), f(0.999), f(1e-8), step, f(EMA['ema_decay']), mode, G.stream())


def test_a_clip_far_above_the_norm_changes_nothing():
    a, b = build(ema=EMA, clip_grad_norm=1e9), build(ema=EMA)
    z2 = second_draw(a)
    for z in (a.draws['z'], z2):
        train_step(a, z)
        train_step(b, z)
    assert same_state(a, b) and a.optG.step_count == 2
    assert float(a.optG.norm4[1]) == 1.0


def test_non_finite_gradient_skips_the_step_on_device():
    m, clean = build(ema=EMA, clip_grad_norm=1e9), build(ema=EMA, clip_grad_norm=1e9)
    train_step(m)
    train_step(clean)
    before = [t.clone() for t in state(m)]
    feed(m)
    m.netG(m.data)
    m.netG.denoise_fn.grad_arena[5] = float('inf')
    m.optG.step()
    torch.cuda.synchronize()
    assert float(m.optG.norm4[2]) == 0.0
    assert all(torch.equal(a, b) for a, b in zip(state(m), before)), 'a non-finite gradient reached the training state'
    assert m.optG.step_count == 2                                # the host count advances: nothing is read back
    train_step(m)                                                # the next clean step trains normally
    assert float(m.optG.norm4[2]) == 1.0
    assert all(bool(torch.isfinite(t).all()) for t in state(m)) and not torch.equal(state(m)[0], before[0])
    # ... exactly as the step a model that never saw the bad gradient takes with the same count
    clean.optG.step_count = 2
    train_step(clean)
    assert same_state(m, clean)


NEW_ENTRIES = ('sr3_grad_norm', 'sr3_grad_accumulate', 'sr3_adam_ema_step_scaled', 'sr3_grad_norm_scratch_bytes')


def test_defaults_make_no_call_to_the_new_entries(monkeypatch):
    lib = L.load()
    calls = {k: 0 for k in NEW_ENTRIES}

    def counted(name, fn):
        def call(*a):
            calls[name] += 1
            return fn(*a)
        return call
    for k in NEW_ENTRIES:
        monkeypatch.setattr(lib, k, counted(k, getattr(lib, k)))
    a, b = build(), build(accumulate=1)
    for _ in range(2):
        train_step(a)
        train_step(b)
    assert sum(calls.values()) == 0, calls
    assert a.optG.grad_acc is None and a.optG.norm4 is None and same_state(a, b) and a.optG.step_count == 2
    c = build(accumulate=2, clip_grad_norm=1.0)                  # (the counter does see the calls of a model that makes them)
    train_step(c)
    train_step(c)
    assert calls['sr3_grad_accumulate'] == 2 and calls['sr3_adam_ema_step_scaled'] == 1 and calls['sr3_grad_norm'] == 0


def test_forced_collectives_world1_reduce_the_accumulated_arena_once(monkeypatch):
    """K = 2 over RCCL with one rank: bit-equal to the plain K = 2 run (which takes the norm from the accumulate pass, while the
    data-parallel one takes it stand-alone after the reduce), with one arena all-reduce per optimizer step."""
    import os
    import torch.distributed as dist
    keys = dict(accumulate=2, clip_grad_norm=1e-4)
    a, b = build(**keys), build(**keys)
    z1, z2 = a.draws['z'], second_draw(a)
    train_step(a, z1)
    train_step(a, z2)
    assert float(a.optG.norm4[1]) < 1.0
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29541')
    dist.init_process_group('nccl', rank=0, world_size=1)
    try:
        un = b.netG.denoise_fn
        un.force_dp = True
        sizes = []
        real = dist.all_reduce

        def counted(t, *args, **kw):
            sizes.append(t.numel())
            return real(t, *args, **kw)
        monkeypatch.setattr(dist, 'all_reduce', counted)
        train_step(b, z1)
        assert sizes == [1]                                      # the loss scalar only
        train_step(b, z2)
        torch.cuda.synchronize()
        assert len(un._reducer.buckets) == 1
        assert sorted(sizes) == [1, 1, un.arena.numel()], sizes
        assert same_state(a, b) and torch.equal(bits(a.optG.norm4), bits(b.optG.norm4)) and torch.equal(a.optG.grad_acc, b.optG.grad_acc)
        assert a.get_current_log() == b.get_current_log()
    finally:
        b.netG.denoise_fn.force_dp = False
        dist.destroy_process_group()
