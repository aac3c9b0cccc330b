"""Guided sampling without a device: the C-ABI entries of csrc/guidance.hip (sr3_cond_drop_f32, sr3_abs_quantile_f32, sr3_guided_step) are
exported, declared, bound and refuse bad arguments before they launch anything; the config plumbing ("guidance" in a phase's
beta_schedule block / set_guidance, "cond_drop" in model.diffusion / set_cond_drop) and its refusals; and the NumPy restatements that
tests/test_gpu_guidance.py checks the kernels against.

`oracle_quantile` is the contract of the select: the two order statistics by np.partition on |v| (exact), the interpolation in float64,
one rounding to fp32.  `oracle_guided_step` is the contract of the step: fp32 elementwise operations, one rounding each."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from helpers import ROOT, SCHEDS, opt_for

F = np.float32
KEYS = ('a', 'b', 'c1', 'c2', 'sigma')
MODES = ('none', 'static', 'dynamic')      # sr3_guided_step's mode numbers, in order


# ---- the oracles --------------------------------------------------------------------------------------------------------------------

def oracle_quantile(v, rank_lo, frac):
    """v [B, n] fp32 -> [B] fp32: (float)(v_lo + frac (v_hi - v_lo)) over |v[b]|, v_lo / v_hi the rank_lo-th / (rank_lo + 1)-th smallest
    (v_hi = v_lo at the last rank); v_lo itself where v_hi == v_lo or frac == 0 (the formula's value for finite data; no inf - inf)."""
    a = np.abs(np.asarray(v, dtype=F))
    B, n = a.shape
    hi_rank = min(rank_lo + 1, n - 1)
    part = np.partition(a, sorted({rank_lo, hi_rank}), axis=1)
    lo, hi = part[:, rank_lo].astype(np.float64), part[:, hi_rank].astype(np.float64)
    with np.errstate(invalid='ignore'):
        q = lo + np.float64(frac) * (hi - lo)
    return np.where((hi == lo) | (frac == 0.0), lo, q).astype(F)


def oracle_guided_step(x, out_c, out_u, scale, z, tabs, j, mode, rank_lo=0, frac=0.0, hist=None):
    """One guided step in the kernel's operations and association.  tabs: fp32 arrays a, b, c1, c2, sigma (c3 with hist), read at row j;
    mode 0 / 1 / 2 = none / static / dynamic.  -> (x', hist' = x0' or None, thr [B])"""
    x, out_c = np.asarray(x, dtype=F), np.asarray(out_c, dtype=F)
    a, b, c1, c2, sg = (F(tabs[k][j]) for k in KEYS)
    out = out_c
    if out_u is not None:
        out_u = np.asarray(out_u, dtype=F)
        out = out_u + F(scale) * (out_c - out_u)
    x0 = a * x - b * out
    B = x.shape[0]
    thr = np.ones(B, dtype=F)
    if mode == 1:
        x0 = np.clip(x0, F(-1.0), F(1.0))
    elif mode == 2:
        thr = np.fmax(F(1.0), oracle_quantile(x0.reshape(B, -1), rank_lo, frac)).astype(F)
        s = thr.reshape(B, 1, 1, 1)
        x0 = np.minimum(np.maximum(x0, -s), s) / s
    mean = c1 * x0 + c2 * x
    if hist is not None:
        mean = mean + F(tabs['c3'][j]) * np.asarray(hist, dtype=F)
    zz = np.zeros_like(x) if z is None else np.asarray(z, dtype=F)
    res = mean + zz * sg
    assert res.dtype == F and x0.dtype == F
    return res, (x0 if hist is not None else None), thr


def test_quantile_rank_by_hand():
    from sr3_hip.diffusion import quantile_rank
    assert quantile_rank(1, 0) == (0, 0.0) and quantile_rank(1, 0.5) == (0, 0.0) and quantile_rank(1, 0.995) == (0, 0.0) and quantile_rank(1, 1) == (0, 0.0)
    assert quantile_rank(2, 0) == (0, 0.0) and quantile_rank(2, 0.5) == (0, 0.5) and quantile_rank(2, 1) == (1, 0.0)
    r, f = quantile_rank(2, 0.995)
    assert r == 0 and f == 0.995
    assert quantile_rank(105, 0) == (0, 0.0) and quantile_rank(105, 0.5) == (52, 0.0) and quantile_rank(105, 1) == (104, 0.0)
    r, f = quantile_rank(105, 0.995)                       # 0.995 * 104 = 103.48
    assert r == 103 and abs(f - 0.48) < 1e-12 and f == 0.995 * 104 - 103
    for n in (1, 2, 105, 768, 196608):
        for p in (0, 0.5, 0.995, 1, 1.0 / 3):
            r, f = quantile_rank(n, p)
            assert 0 <= r < n and 0.0 <= f < 1.0 and isinstance(r, int) and isinstance(f, float)
    for bad in ((0, 0.5), (-3, 0.5), (2.0, 0.5), (True, 0.5), (5, -0.1), (5, 1.01), (5, float('nan')), (5, 'p'), (5, None), (5, True)):
        with pytest.raises(ValueError):
            quantile_rank(*bad)


@pytest.mark.parametrize('n', [1, 2, 48, 105, 769])
def test_oracle_quantile_against_numpy(n):
    from sr3_hip.diffusion import quantile_rank
    g = np.random.default_rng(n)
    v = (g.standard_normal((3, n)) * np.exp(g.standard_normal((3, n)))).astype(F)
    v[1] = np.round(v[1])                                  # ties
    for p in (0, 0.5, 0.995, 1, 0.25):
        want = np.quantile(np.abs(v).astype(np.float64), p, axis=1).astype(F)
        got = oracle_quantile(v, *quantile_rank(n, p))
        assert got.dtype == F and np.array_equal(got, want), (n, p, got, want)
    # an infinite value comes out as itself, at any frac
    v[0, 0] = -np.inf
    assert oracle_quantile(v, n - 1, 0.0)[0] == np.inf
    if n > 1:
        assert np.isfinite(oracle_quantile(v, n - 2, 0.0)[0]) and oracle_quantile(v, n - 2, 0.5)[0] == np.inf


def _tabs(g, rows=3):
    return {k: g.uniform(-1.0, 1.0, rows).astype(F) for k in KEYS + ('c3',)}


def test_oracle_guided_step_is_the_existing_tail_without_guidance():
    """out_u = None, mode 1: the tail every loop runs today (its torch-fp32 restatement in tests/test_gpu_multistep.py), bit for bit,
    with and without history; and a few identities of the other modes"""
    from test_gpu_multistep import tail32
    g = np.random.default_rng(7)
    shape = (2, 3, 6, 10)
    x, oc, ou, z, h = ((2.0 * g.standard_normal(shape)).astype(F) for _ in range(5))
    tabs = _tabs(g)
    tt = {k: torch.from_numpy(v) for k, v in tabs.items()}
    for j in (0, 2):
        for with_h in (False, True):
            for zz in (None, z):
                got, gh, thr = oracle_guided_step(x, oc, None, 1.5, zz, tabs, j, 1, hist=h if with_h else None)
                want, wh = tail32(torch.from_numpy(x), torch.from_numpy(oc), None if zz is None else torch.from_numpy(zz),
                                  torch.from_numpy(h) if with_h else None, tt, j, True)
                assert got.tobytes() == want.numpy().tobytes() and np.all(thr == 1.0)
                if with_h:
                    assert gh.tobytes() == wh.numpy().tobytes()
                want0 = tail32(torch.from_numpy(x), torch.from_numpy(oc), None if zz is None else torch.from_numpy(zz),
                               torch.from_numpy(h) if with_h else None, tt, j, False)[0]
                assert oracle_guided_step(x, oc, None, 1.5, zz, tabs, j, 0, hist=h if with_h else None)[0].tobytes() == want0.numpy().tobytes()
    # scale 0 is the unconditional output, scale 1 the conditional one up to one rounding of (oc - ou) + ou
    assert np.array_equal(oracle_guided_step(x, oc, ou, 0.0, z, tabs, 1, 1)[0], oracle_guided_step(x, ou, None, 0.0, z, tabs, 1, 1)[0])
    # dynamic: |x0| <= 1 everywhere -> s = 1 and mode 2 is mode 1; a heavy image is scaled by its own quantile
    small = (0.1 * x).astype(F)
    t1 = dict(tabs, a=np.full(3, 0.5, F), b=np.full(3, 0.01, F))
    a1, _, thr1 = oracle_guided_step(small, oc * F(0.1), None, 1.0, z, t1, 0, 2, rank_lo=179, frac=0.0)
    assert np.all(thr1 == 1.0) and a1.tobytes() == oracle_guided_step(small, oc * F(0.1), None, 1.0, z, t1, 0, 1)[0].tobytes()
    t2 = dict(tabs, a=np.full(3, 0.9, F), b=np.full(3, 0.43, F))
    _, hh, thr2 = oracle_guided_step(x, oc, ou, 3.0, z, t2, 2, 2, rank_lo=170, frac=0.25, hist=h)
    assert np.all(thr2 > 1.0) and np.abs(hh).max() <= 1.0 and thr2[0] != thr2[1]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------

NEW = (('sr3_cond_drop_f32', 6, C.c_int), ('sr3_abs_quantile_scratch_bytes', 2, C.c_size_t), ('sr3_abs_quantile_f32', 9, C.c_int),
       ('sr3_guided_step', 25, C.c_int))


def test_symbols_are_exported_declared_and_bound():
    from sr3_hip import lib as L
    lib = L.load()
    src = open(ROOT + '/include/sr3_mi355x.h').read()
    assert 'guided sampling (engine extension; no reference counterpart)' in src
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name, nargs, res in NEW:
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES and L.SIGNATURES[name][0] is res and len(L.SIGNATURES[name][1]) == nargs
        decl = re.search(name + r'\s*\((.*?)\)\s*;', src, flags=re.S)
        assert decl is not None and len(decl.group(1).split(',')) == nargs, name
    assert L.SIGNATURES['sr3_abs_quantile_f32'][1][4] is C.c_double and L.SIGNATURES['sr3_guided_step'][1][19] is C.c_double
    assert lib.sr3_version() == 1


def _p(k, off=0):
    """a made-up, 16-byte aligned, non-NULL address: the entries below refuse before they touch memory"""
    return C.c_void_p((k << 24) + off)


def test_scratch_bytes():
    from sr3_hip import lib as L
    lib = L.load()
    assert lib.sr3_abs_quantile_scratch_bytes(0, 5) == 0 and lib.sr3_abs_quantile_scratch_bytes(2, 0) == 0
    assert lib.sr3_abs_quantile_scratch_bytes(1 << 12, 1 << 19) == 0
    a, b = lib.sr3_abs_quantile_scratch_bytes(1, 768), lib.sr3_abs_quantile_scratch_bytes(5, 1 << 20)
    assert 0 < a < b <= 5 * 3 * 2048 * 4 + 64 and a % 16 == 0 and b % 16 == 0


def _q_args(**kw):
    a = dict(src=_p(1), batch=2, n=105, rank_lo=103, frac=0.48, out=_p(2), scratch=_p(3), bytes=1 << 20)
    a.update(kw)
    return [a[k] for k in ('src', 'batch', 'n', 'rank_lo', 'frac', 'out', 'scratch', 'bytes')] + [None]


Q_REFUSALS = [
    (dict(src=None), -1, 'src'), (dict(out=None), -1, 'out_dev'), (dict(scratch=None), -1, 'scratch'), (dict(batch=0), -1, 'batch'),
    (dict(n=0), -1, 'values per image'), (dict(n=-5), -1, 'values per image'), (dict(rank_lo=-1), -1, 'rank_lo'), (dict(rank_lo=105), -1, 'rank_lo'),
    (dict(frac=1.0), -1, 'frac'), (dict(frac=-0.1), -1, 'frac'), (dict(frac=float('nan')), -1, 'frac'), (dict(bytes=64), -1, 'scratch_bytes'),
    (dict(scratch=_p(3, 2)), -3, 'scratch'), (dict(out=_p(1, 8)), -1, 'out_dev'), (dict(scratch=_p(1)), -1, 'scratch'),
    (dict(scratch=_p(2)), -1, 'scratch'), (dict(batch=1 << 12, n=1 << 19, rank_lo=0), -2, '2^31'),
]


@pytest.mark.parametrize('case', range(len(Q_REFUSALS)))
def test_abs_quantile_refusals_no_gpu(case):
    from sr3_hip import lib as L
    lib = L.load()
    kw, code, word = Q_REFUSALS[case]
    assert lib.sr3_abs_quantile_f32(*_q_args(**kw)) == code, kw
    msg = lib.sr3_last_error().decode()
    assert word in msg, (kw, msg)


def test_cond_drop_refusals_no_gpu():
    from sr3_hip import lib as L
    lib = L.load()
    ok = dict(src=_p(1), keep=_p(2), batch=3, per=48, dst=_p(3))
    for kw, code, word in ((dict(src=None), -1, 'src'), (dict(keep=None), -1, 'keep_dev'), (dict(dst=None), -1, 'dst'), (dict(batch=0), -1, 'batch'),
                           (dict(per=0), -1, 'elems_per_image'), (dict(dst=_p(1, 4)), -1, 'partially'), (dict(dst=_p(1, 3 * 48 * 4 - 4)), -1, 'partially'),
                           (dict(dst=_p(2)), -1, 'keep_dev'), (dict(batch=1 << 12, per=1 << 19), -2, '2^31')):
        a = dict(ok, **kw)
        assert lib.sr3_cond_drop_f32(a['src'], a['keep'], a['batch'], a['per'], a['dst'], None) == code, kw
        msg = lib.sr3_last_error().decode()
        assert msg.startswith('cond_drop') and word in msg, (kw, msg)


def _g_args(**kw):
    a = dict(x=_p(1), out_c=_p(2), out_u=_p(3), scale=1.5, z=None, batch=2, channels=3, height=8, width=12, ta=_p(4), tb=_p(5), tc1=_p(6),
             tc2=_p(7), tsig=_p(8), c3=None, hist=None, step2=_p(9), mode=2, rank_lo=100, frac=0.5, x0=_p(12), qs=_p(13), qbytes=1 << 20,
             thr=_p(14))
    a.update(kw)
    return [a[k] for k in ('x', 'out_c', 'out_u', 'scale', 'z', 'batch', 'channels', 'height', 'width', 'ta', 'tb', 'tc1', 'tc2', 'tsig',
                           'c3', 'hist', 'step2', 'mode', 'rank_lo', 'frac', 'x0', 'qs', 'qbytes', 'thr')] + [None]


NB = 2 * 3 * 8 * 12 * 4      # bytes of x in _g_args
G_REFUSALS = [
    (dict(x=None), -1, 'x_nchw'), (dict(out_c=None), -1, 'out_c'), (dict(ta=None), -1, 'tab_a'), (dict(tb=None), -1, 'tab_b'),
    (dict(tc1=None), -1, 'tab_c1'), (dict(tc2=None), -1, 'tab_c2'), (dict(tsig=None), -1, 'tab_sigma'), (dict(step2=None), -1, 'step2_dev'),
    (dict(batch=0), -1, 'batch'), (dict(channels=-1), -1, 'channels'), (dict(height=0), -1, 'height'), (dict(width=-4), -1, 'width'),
    (dict(mode=3), -1, 'mode'), (dict(mode=-1), -1, 'mode'),
    (dict(scale=float('nan')), -1, 'scale'), (dict(scale=float('inf')), -1, 'scale'), (dict(scale=float('-inf')), -1, 'scale'),
    (dict(rank_lo=-1), -1, 'rank_lo'), (dict(rank_lo=3 * 8 * 12), -1, 'rank_lo'), (dict(frac=1.0), -1, 'frac'), (dict(frac=-0.5), -1, 'frac'),
    (dict(frac=float('nan')), -1, 'frac'),
    (dict(x0=None), -1, 'x0_scratch'), (dict(qs=None), -1, 'scratch'), (dict(qbytes=16), -1, 'scratch_bytes'),
    (dict(c3=_p(10)), -1, 'c3'), (dict(hist=_p(11)), -1, 'c3'),
    (dict(c3=_p(10), hist=_p(1)), -1, 'history overlaps'), (dict(c3=_p(10), hist=_p(1, NB - 4)), -1, 'history overlaps'),
    (dict(c3=_p(10), hist=_p(2)), -1, 'history overlaps'), (dict(c3=_p(10), hist=_p(3)), -1, 'hist_nchw overlaps out_u'),
    (dict(c3=_p(10), hist=_p(12)), -1, 'hist_nchw overlaps x0_scratch'),
    (dict(x0=_p(1)), -1, 'x0_scratch overlaps x_nchw'), (dict(x0=_p(1, NB - 4)), -1, 'x0_scratch overlaps x_nchw'),
    (dict(x0=_p(1, -4)), -1, 'x0_scratch overlaps x_nchw'), (dict(x0=_p(3)), -1, 'x0_scratch overlaps out_u'),
    (dict(out_u=_p(1)), -1, 'out_u overlaps x_nchw'), (dict(out_u=_p(1, NB - 4)), -1, 'out_u overlaps x_nchw'),
    (dict(out_c=_p(1)), -1, 'out_c overlaps x_nchw'), (dict(z=_p(1)), -1, 'z_nchw overlaps x_nchw'),
    (dict(qs=_p(1)), -1, 'q_scratch overlaps x_nchw'), (dict(thr=_p(1)), -1, 'thr_out_dev overlaps x_nchw'),
    (dict(batch=1 << 12, channels=2, height=1 << 9, width=1 << 9), -2, '2^31'),
]


@pytest.mark.parametrize('case', range(len(G_REFUSALS)))
def test_guided_step_refusals_no_gpu(case):
    """every refusal of sr3_guided_step returns its code and names the argument, before any launch: no device is present here"""
    from sr3_hip import lib as L
    lib = L.load()
    kw, code, word = G_REFUSALS[case]
    assert lib.sr3_guided_step(*_g_args(**kw)) == code, kw
    msg = lib.sr3_last_error().decode()
    assert msg.startswith('guided_step') and word in msg, (kw, msg)


def test_guided_step_scratch_is_mode_2_only():
    """modes 0 and 1 take no scratch and read no ranks: with those bad, a later check (c3 without a history) is what refuses"""
    from sr3_hip import lib as L
    lib = L.load()
    for mode in (0, 1):
        assert lib.sr3_guided_step(*_g_args(mode=mode, x0=None, qs=None, qbytes=0, rank_lo=-5, frac=7.0, c3=_p(10))) == -1
        assert 'c3' in lib.sr3_last_error().decode()


# ---- the config keys and the setters ----------------------------------------------------------------------------------------------------

def _netG(name, **unet_diff):
    import model as Model
    opt = opt_for(name, gpu=False)
    if unet_diff.get('conditional'):
        opt['model']['unet']['in_channel'] = 6
        opt['model']['diffusion']['conditional'] = True
    return Model.create_model(opt), opt


def test_config_key_and_set_guidance():
    m, opt = _netG('sr3_tiny')
    netG = m.netG
    from sr3_hip.diffusion import THRESHOLDS
    assert THRESHOLDS == MODES
    assert netG.guidance is None and netG.cond_drop == 0.0                  # absent keys: off
    keys = set(netG.state_dict().keys())
    val = opt['model']['beta_schedule']['val']
    val['guidance'] = {'scale': 1.5, 'threshold': 'dynamic', 'percentile': 0.995}
    m.set_new_noise_schedule(val, schedule_phase='val')
    assert netG.guidance == dict(scale=1.5, threshold='dynamic', percentile=0.995) and netG._loop_cache == {}
    assert set(netG.state_dict().keys()) == keys
    m.set_new_noise_schedule(opt['model']['beta_schedule']['train'], schedule_phase='train')      # the other phase has no key
    assert netG.guidance is None
    for spec, want in (({'scale': 2}, dict(scale=2.0, threshold='static', percentile=None)),
                       ({'threshold': 'dynamic'}, dict(scale=1.0, threshold='dynamic', percentile=0.995)),
                       ({'scale': 0.0, 'threshold': 'none', 'percentile': 0.5}, dict(scale=0.0, threshold='none', percentile=None)),
                       ({'scale': 3.0, 'threshold': 'dynamic', 'percentile': 1}, dict(scale=3.0, threshold='dynamic', percentile=1.0))):
        val['guidance'] = spec
        m.set_new_noise_schedule(val, schedule_phase='val')
        assert netG.guidance == want, spec
        m.set_new_noise_schedule(opt['model']['beta_schedule']['train'], schedule_phase='train')      # (a phase is set once per change)
    val['guidance'] = None                                                   # "guidance": null
    m.set_new_noise_schedule(val, schedule_phase='val')
    assert netG.guidance is None
    for bad, word in (({'scale': 'big'}, 'scale'), ({'scale': True}, 'scale'), ({'scale': float('nan')}, 'scale'), ({'scale': float('inf')}, 'scale'),
                      ({'scale': [1.5]}, 'scale'), ({'scale': 1.5, 'threshold': 'soft'}, 'threshold'), ({'scale': 1.5, 'threshold': 2}, 'threshold'),
                      ({'threshold': 'dynamic', 'percentile': 1.01}, 'percentile'), ({'threshold': 'dynamic', 'percentile': -0.1}, 'percentile'),
                      ({'threshold': 'dynamic', 'percentile': 'high'}, 'percentile'), ({'threshold': 'dynamic', 'percentile': None}, 'percentile'),
                      ('on', 'dict')):
        with pytest.raises(ValueError, match=word):
            netG.set_new_noise_schedule(dict(SCHEDS['sr3_tiny'], guidance=bad), torch.device('cpu'))
        assert netG.guidance is None
    # programmatic form; the state is unchanged after a refusal
    netG._loop_cache['stale'] = object()
    netG.set_guidance(1.5, 'dynamic', 0.9)
    assert netG.guidance == dict(scale=1.5, threshold='dynamic', percentile=0.9) and netG._loop_cache == {}
    for args in (('x',), (True,), (1.5, 'soft'), (1.5, 'dynamic', 2.0), (float('nan'),)):
        with pytest.raises(ValueError):
            netG.set_guidance(*args)
    assert netG.guidance == dict(scale=1.5, threshold='dynamic', percentile=0.9)
    netG.set_guidance(None, 'dynamic')
    assert netG.guidance == dict(scale=1.0, threshold='dynamic', percentile=0.995)
    netG.set_guidance(2.0)
    assert netG.guidance == dict(scale=2.0, threshold='static', percentile=None)
    netG._loop_cache['stale'] = object()
    netG.set_guidance(None)
    assert netG.guidance is None and netG._loop_cache == {}


def test_cond_drop_key_and_setter():
    import model as Model
    opt = opt_for('sr3_tiny', gpu=False)
    for v, want in ((0.1, 0.1), (0, 0.0), (None, 0.0)):
        opt['model']['diffusion']['cond_drop'] = v
        netG = Model.create_model(opt).netG
        assert netG.cond_drop == want and not any('cond_drop' in k for k in netG.state_dict())
    del opt['model']['diffusion']['cond_drop']
    netG = Model.create_model(opt).netG
    assert netG.cond_drop == 0.0
    for bad in (1.0, -0.1, 1.5, float('nan'), 'half', True):
        opt['model']['diffusion']['cond_drop'] = bad
        with pytest.raises(ValueError, match='cond_drop'):
            Model.create_model(opt)
        with pytest.raises(ValueError, match='cond_drop'):
            netG.set_cond_drop(bad)
        assert netG.cond_drop == 0.0
    netG.set_cond_drop(0.25)
    assert netG.cond_drop == 0.25
    netG.set_cond_drop(0)
    assert netG.cond_drop == 0.0
    # an unconditional model has nothing to drop
    for name in ('ddpm_tiny', 'sr3_uncond'):
        opt = opt_for(name, gpu=False)
        opt['model']['diffusion']['cond_drop'] = 0.1
        with pytest.raises(ValueError, match='unconditional'):
            Model.create_model(opt)


@pytest.mark.parametrize('name', ['ddpm_tiny', 'sr3_uncond'])
def test_guidance_on_an_unconditional_model_is_refused(name):
    m, opt = _netG(name)
    with pytest.raises(ValueError, match='unconditional'):
        m.netG.set_guidance(1.5)
    with pytest.raises(ValueError, match='unconditional'):
        m.netG.set_new_noise_schedule(dict(SCHEDS[name], guidance={'scale': 1.0, 'threshold': 'dynamic'}), torch.device('cpu'))
    assert m.netG.guidance is None
    from sr3_hip import lib as L
    with pytest.raises(L.Sr3Error):          # off: today's refusal of a CPU model
        m.netG.p_sample_loop((1, 3, 16, 16))


def test_guidance_with_tiling_or_consistency_is_not_implemented():
    s = SCHEDS['sr3_tiny']
    netG = _netG('sr3_tiny')[0].netG
    cpu = torch.device('cpu')
    with pytest.raises(NotImplementedError, match='guidance with tiling'):
        netG.set_new_noise_schedule(dict(s, tiling={'tile': 16, 'overlap': 4}, guidance={'scale': 1.5}), cpu)
    with pytest.raises(NotImplementedError, match='guidance with consistency'):
        netG.set_new_noise_schedule(dict(s, consistency={'block': 4}, guidance={'scale': 1.5}), cpu)
    netG.set_new_noise_schedule(dict(s), cpu)
    # tiling first, then guidance -- and the other way round
    netG.set_tiling(16, 4)
    with pytest.raises(NotImplementedError, match='guidance with tiling'):
        netG.set_guidance(1.5)
    assert netG.guidance is None and netG.tiling is not None
    netG.set_tiling(None)
    netG.set_guidance(1.5, 'dynamic')
    with pytest.raises(NotImplementedError, match='guidance with tiling'):
        netG.set_tiling(16, 4)
    assert netG.tiling is None and netG.guidance == dict(scale=1.5, threshold='dynamic', percentile=0.995)
    with pytest.raises(NotImplementedError, match='guidance with tiling'):      # the explicit tiled loop, whatever set_tiling says
        netG.p_sample_loop_tiled(torch.zeros(1, 3, 32, 32), tile=16, overlap=4)
    # consistency, both orders
    with pytest.raises(NotImplementedError, match='guidance with consistency'):
        netG.set_consistency(4)
    assert netG.consistency is None
    netG.set_guidance(None)
    netG.set_consistency(4)
    with pytest.raises(NotImplementedError, match='guidance with consistency'):
        netG.set_guidance(None, 'dynamic')
    assert netG.guidance is None and netG.consistency == dict(block=4, strength=1.0)
    # the existing refusal keeps its text
    with pytest.raises(NotImplementedError, match='consistency with tiling'):
        netG.set_tiling(16, 4)
    # a sampler and guidance go together on the SR3 variant
    netG.set_consistency(None)
    netG.set_guidance(1.5)
    netG.set_sampler(4, kind='dpmpp_2m')
    assert netG.sampler['steps'] == 4 and netG.guidance is not None
    netG.set_new_noise_schedule(dict(s, sampler={'type': 'ddim', 'steps': 4}, guidance={'scale': 2.0, 'threshold': 'none'}), cpu)
    assert netG.sampler['steps'] == 4 and netG.guidance == dict(scale=2.0, threshold='none', percentile=None)


def test_ddpm_guidance_under_a_sampler_is_not_implemented():
    s = SCHEDS['ddpm_tiny']
    netG = _netG('ddpm_tiny', conditional=True)[0].netG
    assert netG.conditional and netG.variant == 'ddpm'
    cpu = torch.device('cpu')
    with pytest.raises(NotImplementedError, match='guidance.*t_map'):
        netG.set_new_noise_schedule(dict(s, sampler={'type': 'ddim', 'steps': 3}, guidance={'scale': 1.5}), cpu)
    netG.set_new_noise_schedule(dict(s), cpu)
    netG.set_sampler(3, 0.0)
    with pytest.raises(NotImplementedError, match='guidance.*t_map'):
        netG.set_guidance(1.5)
    assert netG.guidance is None
    netG.set_sampler(None)
    netG.set_guidance(1.5)                                   # the ancestral rule is fine
    with pytest.raises(NotImplementedError, match='guidance.*t_map'):
        netG.set_sampler(3, 0.0)
    assert netG.sampler is None and netG.guidance == dict(scale=1.5, threshold='static', percentile=None)
    with pytest.raises(NotImplementedError, match='guidance.*t_map'):
        netG.set_sampler(3, kind='dpmpp_2m')


def test_keys_absent_the_loop_state_key_has_none():
    """with every new key absent the loop-state key's guidance component is None and the tiling entry stays last (built without a
    device: the key is formed before any tensor is made, so a meta device shows it)"""
    netG = _netG('sr3_tiny')[0].netG
    assert netG.guidance is None

    seen = []

    class Stop(Exception):
        pass

    class Cache(dict):
        def get(self, key, default=None):
            seen.append(key)
            raise Stop

    for gd, want in ((None, None), (dict(scale=1.5, threshold='dynamic', percentile=0.995), (1.5, 'dynamic', 0.995))):
        netG._loop_cache = Cache()
        with pytest.raises(Stop):
            netG._loop_state((2, 3, 16, 16), (2, 3, 16, 16), torch.device('cpu'), guidance=gd)
        key = seen[-1]
        assert key[-3] == want and key[-2] is None and key[-1] is None
    netG._loop_cache = {}
