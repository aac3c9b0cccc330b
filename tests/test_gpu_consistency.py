"""LR-consistent sampling on the GPU (csrc/consistency.hip, EngineDiffusion.set_consistency): sr3_block_mean_f32 and sr3_consistent_step
through the C ABI against the NumPy restatement of tests/test_consistency_cpu.py (fp32 elementwise operations, the block sum in
float64, delta rounded once), and the chains of p_sample_loop under the "consistency" key against a loop written here from
denoise_fn forwards plus that restatement.

Shapes: the smallest that take each path -- r = 2 at a width that is no multiple of 4 (the one-element form), r = 4 (a quad is one
block row), r = 8 / 16 (2 / 4 lanes per block), r = 32 (8 lanes; 32 in the one-element form), 160 x 160 (29 workgroups, strips that
start inside a wavefront), r = 2 at 512 x 342 (525 312 one-element items), and the r = 4 case with every tensor off a 16-byte boundary."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_util as G                                                                      # noqa: E402
from helpers import load_golden, opt_for                                                  # noqa: E402
from sr3_hip import lib as L                                                              # noqa: E402
from test_consistency_cpu import F, KEYS, block_mean64, oracle_step                       # noqa: E402

GUARD = 1024      # floats of NaN around a tensor, in the same allocation

# (block, (B, C, H, W), misaligned)
SHAPES = [(2, (2, 3, 6, 10), False), (4, (2, 3, 8, 12), False), (8, (3, 4, 16, 24), False), (16, (2, 1, 32, 48), False),
          (32, (1, 3, 64, 32), False), (8, (3, 3, 160, 160), False), (4, (2, 3, 8, 12), True), (2, (2, 3, 512, 342), False)]
IDS = ['r%d-%s%s' % (r, 'x'.join(map(str, s)), '-misaligned' if mis else '') for r, s, mis in SHAPES]

# four rows that differ; row 2 is the a = 0.9, b = 0.43 row the step tests run at; |c1|, |c2|, |c3|, |sigma| <= 1
TABLES = dict(a=[1.1, 0.7, 0.9, 0.6], b=[0.2, 0.75, 0.43, 0.7], c1=[1.0, 0.45, 0.55, 0.4], c2=[0.0, 0.5, 0.45, -0.2],
              sigma=[0.0, 0.4, 0.5, 0.25], c3=[0.0, -0.35, 0.5, -0.45])
J = 2


def _tabs():
    return {k: np.asarray(v, dtype=F) for k, v in TABLES.items()}


def _dev(t, d, mis=0):
    """`t` (numpy or torch, fp32) on the device with GUARD NaNs in front of and behind it in ONE allocation, `mis` floats off a 16-byte
    boundary: (view, whole buffer, offset)"""
    t = torch.as_tensor(t)
    n = t.numel()
    buf = torch.full((n + 2 * GUARD,), float('nan'), device=d)
    off = GUARD + mis
    assert buf.data_ptr() % 16 == 0
    buf[off:off + n].copy_(t.reshape(-1))
    return buf[off:off + n].view(t.shape), buf, off


def _guard_intact(buf, off, n):
    return bool(torch.isnan(buf[:off]).all()) and bool(torch.isnan(buf[off + n:]).all())


def _ints(v, d):
    return torch.tensor(v, dtype=torch.int32, device=d)


def _inputs(r, shape, scale=1.0):
    g = np.random.default_rng(1000 * r + sum(shape))
    B, Cc, H, W = shape
    x = (scale * g.standard_normal(shape)).astype(F)
    eps, z, h = (g.standard_normal(shape).astype(F) for _ in range(3))
    y = g.uniform(-1.0, 1.0, (B, Cc, H // r, W // r)).astype(F)
    return x, eps, z, h, y


def _step(x, eps, z, y, r, lam, tabs, step2, clip, c3, hist):
    B, Cc, H, W = x.shape
    rc = L.load().sr3_consistent_step(L.ptr(x), L.ptr(eps), L.ptr(z), L.ptr(y), B, Cc, H, W, r, lam, *[L.ptr(tabs[k]) for k in KEYS],
                                      L.ptr(step2), clip, L.ptr(c3), L.ptr(hist), G.stream())
    torch.cuda.synchronize()
    return rc


def _run(case, d, clip, with_hist, with_z, lam, inputs, j=J):
    """one call on guarded (and, for the misaligned case, shifted) copies of the inputs -> (x', hist' or None, counter) on the host"""
    r, shape, mis = case
    x, eps, z, h, y = inputs
    dt = {k: torch.from_numpy(v).to(d) for k, v in _tabs().items()}
    xd, xbuf, xo = _dev(x, d, 1 if mis else 0)
    ed = _dev(eps, d, 2 if mis else 0)[0]
    zd = _dev(z, d, 3 if mis else 0)[0] if with_z else None
    hd, hbuf, ho = _dev(h, d, 1 if mis else 0) if with_hist else (None, None, 0)
    yd = torch.from_numpy(y).to(d)
    step2 = _ints([-7, j], d)
    assert _step(xd, ed, zd, yd, r, lam, dt, step2, clip, dt['c3'] if with_hist else None, hd) == 0, L.load().sr3_last_error()
    assert _guard_intact(xbuf, xo, xd.numel()), 'the kernel wrote outside x'
    assert hbuf is None or _guard_intact(hbuf, ho, hd.numel()), 'the kernel wrote outside hist'
    assert torch.equal(ed.cpu(), torch.from_numpy(eps)) and torch.equal(yd.cpu(), torch.from_numpy(y))
    return xd.cpu().numpy(), None if hd is None else hd.cpu().numpy(), step2.tolist()


def _check(got, want, what):
    """|got - oracle| <= 4 * 2^-23 * max(1, |oracle|) per element, and at most 1 % of the elements differ at all.  delta may be off by
    one fp32 ulp of a value <= 2 (2.4e-7) where the order of the double sum matters; |c1|, |c3| <~ 1 carry it through two more roundings."""
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    tol = 4.0 * 2.0 ** -23 * np.maximum(1.0, np.abs(want.astype(np.float64)))
    frac = float((got != want).mean())
    print('%s: max |diff| %.3e, %.4f %% of the elements differ' % (what, diff.max(), 100.0 * frac))
    assert np.all(diff <= tol), '%s: %g' % (what, diff.max())
    assert frac <= 0.01, '%s: %.3f %% of the elements differ from the oracle' % (what, 100.0 * frac)


# ---- 1. block means ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', SHAPES, ids=IDS)
def test_block_mean_against_float64(case):
    from sr3_hip.diffusion import block_means
    r, shape, mis = case
    d = G.dev()
    x = _inputs(r, shape, scale=3.0)[0]
    xd, xbuf, xo = _dev(x, d, 1 if mis else 0)
    B, Cc, H, W = shape
    out, obuf, oo = _dev(np.full((B, Cc, H // r, W // r), np.nan, dtype=F), d)
    L.check(L.load().sr3_block_mean_f32(L.ptr(xd), B, Cc, H, W, r, L.ptr(out), G.stream()))
    torch.cuda.synchronize()
    assert _guard_intact(obuf, oo, out.numel()) and torch.equal(xd.cpu(), torch.from_numpy(x))
    got = out.cpu().numpy()
    m64 = block_mean64(x, r)
    ulp = np.spacing(np.abs(m64).astype(F)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - m64)
    print('r = %d %s: max err %.3e (%.2f ulp)' % (r, shape, err.max(), (err / ulp).max()))
    assert np.all(err <= ulp)
    if not mis:      # the public helper is the same call
        assert torch.equal(block_means(torch.from_numpy(x).to(d), r).cpu(), out.cpu())


# ---- 2. the step against the oracle; 4. the counter -------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', SHAPES, ids=IDS)
def test_consistent_step_against_oracle(case):
    r, shape, mis = case
    d = G.dev()
    big = shape[2] * shape[3] > 100000
    inputs = _inputs(r, shape)
    x, eps, z, h, y = inputs
    tabs = _tabs()
    combos = [(clip, hi, wz, lam) for clip in (0, 1) for hi in (False, True) for wz in (False, True) for lam in (1.0, 0.5)]
    if big:
        combos = combos[::5]      # (the large one-element case: the paths are the small cases'; four combinations keep it quick)
    for clip, hi, wz, lam in combos:
        gx, gh, step2 = _run(case, d, clip, hi, wz, lam, inputs)
        assert step2 == [J, J - 1]
        wx, wh = oracle_step(x, eps, z if wz else None, y, r, lam, tabs, J, clip, h if hi else None)
        what = 'r %d %s clip %d hist %d z %d strength %g' % (r, shape, clip, hi, wz, lam)
        _check(gx, wx, what + ': x')
        if hi:
            _check(gh, wh, what + ': hist')
    # the tables are read at row j, not j - 1: the neighbouring row gives something else entirely
    other = oracle_step(x, eps, z, y, r, 1.0, tabs, J - 1, 1, h)[0]
    gx = _run(case, d, 1, True, True, 1.0, inputs)[0]
    assert np.abs(gx - other).max() > 0.1
    if not big:
        for j in (0, 3):
            gx, gh, step2 = _run(case, d, 1, True, True, 1.0, inputs, j=j)
            assert step2 == [j, j - 1]
            wx, wh = oracle_step(x, eps, z, y, r, 1.0, tabs, j, 1, h)
            _check(gx, wx, 'row %d: x' % j)
            _check(gh, wh, 'row %d: hist' % j)


@pytest.mark.parametrize('clip', [0, 1])
def test_consistent_step_heavy_tailed(clip):
    """x scaled by 3: with the clamp most of x0 sits at +-1, without it |x0| reaches 10"""
    case = SHAPES[2]
    r, shape, _ = case
    inputs = _inputs(r, shape, scale=3.0)
    x, eps, z, h, y = inputs
    for lam in (1.0, 0.5):
        gx, gh, _ = _run(case, G.dev(), clip, True, True, lam, inputs)
        wx, wh = oracle_step(x, eps, z, y, r, lam, _tabs(), J, clip, h)
        _check(gx, wx, 'heavy-tailed clip %d strength %g: x' % (clip, lam))
        _check(gh, wh, 'heavy-tailed clip %d strength %g: hist' % (clip, lam))
    if clip:
        x0 = np.clip(F(0.9) * x - F(0.43) * eps, -1, 1)
        assert 0.3 < float((np.abs(x0) == 1).mean()) < 0.9


# ---- 3. the projection property --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', SHAPES, ids=IDS)
def test_projection_property(case):
    """strength 1, clip on, targets in [-1, 1]: the history the step leaves is x0', and its block means are the target's.
    |mean_block(hist) - y| <= 3.6e-7: half an ulp(4) per element from the add (|x0'| <= 3) plus half an ulp(2) on delta."""
    r, shape, _ = case
    inputs = _inputs(r, shape)
    gx, gh, _ = _run(case, G.dev(), 1, True, True, 1.0, inputs)
    y = inputs[4]
    assert np.abs(y).max() <= 1.0
    err = np.abs(block_mean64(gh, r) - y.astype(np.float64)).max()
    print('r = %d %s: max |mean_block(x0\') - y| = %.3e' % (r, shape, err))
    assert err <= 3.6e-7
    assert np.abs(gh).max() <= 3.0


# ---- 5. reproducible -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', SHAPES, ids=IDS)
def test_two_runs_give_the_same_bits(case):
    r, shape, _ = case
    inputs = _inputs(r, shape)
    a = _run(case, G.dev(), 1, True, True, 0.5, inputs)
    b = _run(case, G.dev(), 1, True, True, 0.5, inputs)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_refusals_launch_nothing():
    d = G.dev()
    r, shape, _ = SHAPES[1]
    x, eps, z, h, y = (torch.from_numpy(t).to(d) for t in _inputs(r, shape))
    dt = {k: torch.from_numpy(v).to(d) for k, v in _tabs().items()}
    keep = x.clone()
    step2 = _ints([-7, J], d)
    lib = L.load()
    for kw, code, word in ((dict(r=3), -1, b'block'), (dict(lam=0.0), -1, b'strength'), (dict(lam=float('nan')), -1, b'strength'),
                           (dict(hist=x), -1, b'overlaps'), (dict(c3=None), -1, b'c3'), (dict(y=x), -1, b'target_means')):
        a = dict(r=r, lam=1.0, c3=dt['c3'], hist=h, y=y)
        a.update(kw)
        assert _step(x, eps, z, a['y'], a['r'], a['lam'], dt, step2, 1, a['c3'], a['hist']) == code, kw
        assert word in lib.sr3_last_error()
    assert torch.equal(x, keep) and step2.tolist() == [-7, J]


# ---- 6. the chains -----------------------------------------------------------------------------------------------------------------------

BLOCK = 4


def _model(consistency, sampler=None):
    import model as Model
    opt = opt_for('sr3_tiny', phase='val', gpu=True)
    val = opt['model']['beta_schedule']['val']
    if consistency is not None:
        val['consistency'] = consistency
    if sampler is not None:
        val['sampler'] = sampler
    m = Model.create_model(opt)
    g, sd = load_golden('sr3_tiny')
    m.netG.load_state_dict(sd, strict=True)
    m.netG.show_progress = False
    m.set_new_noise_schedule(val, schedule_phase='val')
    return m.netG, g


def _rule_tables(netG):
    """the rule's tables on the host, as the engine's own _step_rule hands them to the kernel: (dict of fp32 arrays, level table)"""
    tables, level, t_map, c3, noisy = netG._step_rule()
    tabs = {k: t.cpu().numpy() for k, t in zip(KEYS, tables)}
    if c3 is not None:
        tabs['c3'] = c3.cpu().numpy()
    return tabs, level.cpu().numpy(), c3 is not None, noisy


def _own_loop_check(netG, cond, x_T, zs, out, target=None):
    """The chain again, written here: per step one denoise_fn forward at the step's level on the ENGINE's image before the step (its
    previous snapshot: teacher forcing, so the per-step tolerance applies to every step) and the oracle tail; the history is carried
    by the oracle.  Every step of these chains is a snapshot (T = 8 or S = 5: stride 1)."""
    from sr3_hip.diffusion import block_means
    d = cond.device
    tabs, level, multistep, noisy = _rule_tables(netG)
    T = len(tabs['a'])
    B = cond.shape[0]
    assert out.shape[0] == B * (T + 1)
    y = (block_means(cond[:, :3].contiguous(), BLOCK) if target is None else target).cpu().numpy()
    hist = np.zeros(tuple(x_T.shape), dtype=F) if multistep else None
    for k, j in enumerate(reversed(range(T))):
        before = x_T if k == 0 else out[k * B:(k + 1) * B]
        lv = torch.full((B,), float(level[j + 1]), dtype=torch.float32, device=d)
        eps = netG.denoise_fn(before.contiguous(), lv, cond=cond).cpu().numpy()
        z = zs[j].cpu().numpy() if (noisy and zs is not None and j > 0) else None
        want, hist = oracle_step(before.cpu().numpy(), eps, z, y, BLOCK, netG.consistency['strength'], tabs, j, 1, hist)
        got = out[(k + 1) * B:(k + 2) * B].cpu().numpy()
        err = float(np.abs(got.astype(np.float64) - want).max())
        tol = 2e-5 * max(1.0, float(np.abs(want).max()))
        print('step index %d: max abs err %.3e (tolerance %.3e)' % (j, err, tol))
        assert err <= tol, (j, err, tol)
    return tabs


def _consistency_error(out_last, want_means):
    from sr3_hip.diffusion import block_means
    return float((block_means(out_last.contiguous(), BLOCK) - want_means).abs().max())


@pytest.mark.parametrize('rule', ['ancestral', 'ddim', 'dpmpp_2m'])
def test_chain_against_own_loop_graph_and_block_means(rule):
    from sr3_hip.diffusion import block_means
    d = G.dev()
    sampler = None if rule == 'ancestral' else {'type': rule, 'steps': 5}
    netG, g = _model({'block': BLOCK}, sampler)
    assert netG.consistency == dict(block=BLOCK, strength=1.0)
    cond, x_T, zs = (torch.from_numpy(g['loop/' + n]).to(d) for n in ('sr', 'x_T', 'zs'))
    B = cond.shape[0]
    # eager; the ancestral rule with its noise injected
    netG.use_graph = False
    eager = netG.p_sample_loop(cond, continous=True, x_T=x_T, noise_seq=zs if rule == 'ancestral' else None).clone()
    st = next(reversed(netG._loop_cache.values()))
    assert st['consistency'] == netG.consistency and tuple(st['ymean'].shape) == (B, 3, 16 // BLOCK, 16 // BLOCK)
    assert torch.equal(st['ymean'], block_means(cond, BLOCK)) and st['step'].tolist() == [0, -1]
    tabs = _own_loop_check(netG, cond, x_T, zs if rule == 'ancestral' else None, eager)
    # the last step's row makes the result x0' itself, so its block means are the target's
    assert tabs['c1'][0] + (tabs['c3'][0] if 'c3' in tabs else 0.0) == 1.0 and tabs['c2'][0] == 0.0 and tabs['sigma'][0] == 0.0
    err = _consistency_error(eager[-B:], block_means(cond, BLOCK))
    print('%s: consistency error of the result %.3e' % (rule, err))
    assert err <= 1e-6
    # graph replay equals the eager loop bit for bit (the ancestral rule draws its noise: same seed on both sides)
    outs = []
    for use_graph in (False, True):
        netG.use_graph = use_graph
        torch.manual_seed(17)
        outs.append(netG.p_sample_loop(cond, continous=True, x_T=x_T).clone())
    st = next(reversed(netG._loop_cache.values()))
    assert st['graph'] is not None and torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[1]).all())
    if rule != 'ancestral':
        assert torch.equal(outs[1], eager)
    assert _consistency_error(outs[1][-B:], block_means(cond, BLOCK)) <= 1e-6
    # without the key the same chain is not consistent: the projection is what did it
    netG.set_consistency(None)
    torch.manual_seed(17)
    plain = netG.p_sample_loop(cond, continous=True, x_T=x_T)
    assert _consistency_error(plain[-B:], block_means(cond, BLOCK)) > 1e-3


def test_consistency_target_is_honoured():
    from sr3_hip.diffusion import block_means
    d = G.dev()
    netG, g = _model({'block': BLOCK, 'strength': 1.0}, {'type': 'ddim', 'steps': 5})
    cond, x_T = (torch.from_numpy(g['loop/' + n]).to(d) for n in ('sr', 'x_T'))
    B = cond.shape[0]
    own = block_means(cond, BLOCK)
    target = (0.5 * own + 0.1).contiguous()
    assert float((target - own).abs().max()) > 0.05
    for use_graph in (False, True):
        netG.use_graph = use_graph
        out = netG.super_resolution(cond, continous=True, consistency_target=target)
        assert _consistency_error(out[-B:], target) <= 1e-6
        assert _consistency_error(out[-B:], own) > 0.05
    # back to the conditioning image's own means on the same cached state
    out = netG.super_resolution(cond, continous=True)
    assert _consistency_error(out[-B:], own) <= 1e-6
    # a strength below 1 goes part of the way at every step; the check against the loop written here covers it
    netG.set_consistency(BLOCK, 0.5)
    netG.use_graph = False
    half = netG.p_sample_loop(cond, continous=True, x_T=x_T, consistency_target=target)
    _own_loop_check(netG, cond, x_T, None, half, target=target)
    with pytest.raises(L.Sr3Error, match='consistency_target'):
        netG.p_sample_loop(cond, consistency_target=target[:, :, :2])
    netG.set_consistency(32)
    with pytest.raises(L.Sr3Error, match='32.*16 x 16'):
        netG.p_sample_loop(cond)


# ---- 7. off means off -------------------------------------------------------------------------------------------------------------------

def test_off_means_off():
    d = G.dev()
    netG, g = _model({'block': BLOCK})
    never, _ = _model(None)
    cond, x_T, zs = (torch.from_numpy(g['loop/' + n]).to(d) for n in ('sr', 'x_T', 'zs'))
    T = zs.shape[0]
    calls = []
    real = netG.denoise_fn.reverse_step

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    netG.denoise_fn.reverse_step = spy
    netG.use_graph = False
    netG.p_sample_loop(cond, x_T=x_T, noise_seq=zs)
    assert calls == []                                   # on: the third branch, not the fused step
    netG.set_consistency(None)
    assert netG.consistency is None and netG._loop_cache == {}
    off = netG.p_sample_loop(cond, continous=True, x_T=x_T, noise_seq=zs)
    assert len(calls) == T
    st = next(reversed(netG._loop_cache.values()))
    assert 'ymean' not in st and 'consistency' not in st and next(reversed(netG._loop_cache.keys()))[-2] is None
    never.use_graph = False
    assert never.consistency is None
    assert torch.equal(off, never.p_sample_loop(cond, continous=True, x_T=x_T, noise_seq=zs))
    # and replayed
    del netG.denoise_fn.reverse_step
    outs = []
    for n in (netG, never):
        n.use_graph = True
        torch.manual_seed(5)
        outs.append(n.p_sample_loop(cond, continous=True, x_T=x_T).clone())
    assert torch.equal(outs[0], outs[1])
