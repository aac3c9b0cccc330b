"""LR-consistent sampling without a device: the two C-ABI entries (sr3_block_mean_f32, sr3_consistent_step) are exported, declared and
refuse bad arguments before they launch anything; the config plumbing ("consistency" in a phase's beta_schedule block /
set_consistency); and the NumPy restatement of the step that tests/test_gpu_consistency.py checks the kernel against.

The restatement (`oracle_step`) is the contract of csrc/consistency.hip: fp32 elementwise operations, one rounding each (np.float32
arithmetic), the block sum in float64, delta rounded to fp32 once."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from helpers import ROOT, SCHEDS, opt_for

F = np.float32
KEYS = ('a', 'b', 'c1', 'c2', 'sigma')


# ---- the oracle -------------------------------------------------------------------------------------------------------------------

def block_sum64(x, r):
    """float64 sums of the r x r blocks of x [B, C, H, W] -> [B, C, H / r, W / r]"""
    B, Cc, H, W = x.shape
    return np.asarray(x, dtype=np.float64).reshape(B, Cc, H // r, r, W // r, r).sum(axis=(3, 5))


def block_mean64(x, r):
    return block_sum64(x, r) / np.float64(r * r)


def project(x0, y, r, lam):
    """x0' = x0 + (float)(lam * (y - mean_block(x0))): the double block sum, delta rounded once, one fp32 add per element"""
    x0 = np.asarray(x0, dtype=F)
    delta = (np.float64(F(lam)) * (np.asarray(y, dtype=F).astype(np.float64) - block_sum64(x0, r) / np.float64(r * r))).astype(F)
    return x0 + np.repeat(np.repeat(delta, r, axis=2), r, axis=3)


def oracle_step(x, eps, z, y, r, lam, tabs, j, clip, hist=None):
    """One consistent step in the kernel's operations and association.  tabs: dict of fp32 arrays a, b, c1, c2, sigma (and c3 when hist
    is given), read at row j.  -> (x', hist') with hist' = x0' (None without history)"""
    x, eps = np.asarray(x, dtype=F), np.asarray(eps, dtype=F)
    a, b, c1, c2, sg = (F(tabs[k][j]) for k in KEYS)
    x0 = a * x - b * eps
    if clip:
        x0 = np.clip(x0, F(-1.0), F(1.0))
    x0p = project(x0, y, r, lam)
    mean = c1 * x0p + c2 * x
    if hist is not None:
        mean = mean + F(tabs['c3'][j]) * np.asarray(hist, dtype=F)
    zz = np.zeros_like(x) if z is None else np.asarray(z, dtype=F)
    out = mean + zz * sg
    assert out.dtype == F and x0p.dtype == F
    return out, (x0p if hist is not None else None)


@pytest.mark.parametrize('r', [2, 4, 8, 16, 32])
def test_oracle_projection_sanity(r):
    """The projection is idempotent, and with strength 1 it lands on the target.

    Twice against once: the second pass sees a residual y - mean(x0') of at most the bound below and adds it to every element, so an
    element moves by at most one ulp at the data's scale -- ulp(max(1, |x0'|)); an element near zero moves by that residual, which is
    many of ITS ulps, so the comparison is not relative to the element.
    The residual: each of the r^2 adds rounds by at most half an ulp of a value below 4 (|x0'| <= 3 for targets and x0 in [-1, 1]:
    2^-22 / 2 = 1.2e-7), delta by half an ulp of a value <= 2 (1.2e-7): |mean_block(x0') - y| <= 3.6e-7."""
    rng = np.random.default_rng(100 + r)
    shape = (2, 3, 2 * r, 3 * r)
    x0 = np.clip(rng.standard_normal(shape), -1, 1).astype(F)
    y = rng.uniform(-1, 1, (2, 3, 2, 3)).astype(F)
    once = project(x0, y, r, 1.0)
    twice = project(once, y, r, 1.0)
    ulp = np.spacing(np.maximum(np.abs(once), F(1.0)))
    assert np.all(np.abs(twice.astype(np.float64) - once.astype(np.float64)) <= ulp)
    resid = np.abs(block_mean64(once, r) - y.astype(np.float64)).max()
    print('r = %d: residual %.2e' % (r, resid))
    assert resid <= 3.6e-7
    # strength 0.5 goes half the way
    half = project(x0, y, r, 0.5)
    want = 0.5 * (block_mean64(x0, r) + y.astype(np.float64))
    assert np.abs(block_mean64(half, r) - want).max() <= 3.6e-7


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------

def test_symbols_are_exported_and_declared():
    from sr3_hip import lib as L
    lib = L.load()
    src = open(ROOT + '/include/sr3_mi355x.h').read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name, nargs in (('sr3_block_mean_f32', 8), ('sr3_consistent_step', 20)):
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES and L.SIGNATURES[name][0] is C.c_int and len(L.SIGNATURES[name][1]) == nargs
        decl = re.search(name + r'\s*\((.*?)\)\s*;', src, flags=re.S)
        assert decl is not None and len(decl.group(1).split(',')) == nargs, name
    assert lib.sr3_version() == 1


def _p(k):
    """a made-up, 16-byte aligned, non-NULL address: the entries below refuse before they touch memory"""
    return C.c_void_p(k << 24)


def _step_args(**kw):
    a = dict(x=_p(1), eps=_p(2), z=None, y=_p(3), batch=2, channels=3, height=8, width=12, block=4, strength=1.0, ta=_p(4), tb=_p(5),
             tc1=_p(6), tc2=_p(7), tsig=_p(8), step2=_p(9), clip=1, c3=None, hist=None)
    a.update(kw)
    return [a[k] for k in ('x', 'eps', 'z', 'y', 'batch', 'channels', 'height', 'width', 'block', 'strength', 'ta', 'tb', 'tc1', 'tc2',
                           'tsig', 'step2', 'clip', 'c3', 'hist')] + [None]


STEP_REFUSALS = [
    (dict(x=None), -1, 'x_nchw'), (dict(eps=None), -1, 'eps_nchw'), (dict(y=None), -1, 'target_means'), (dict(ta=None), -1, 'tab_a'),
    (dict(tb=None), -1, 'tab_b'), (dict(tc1=None), -1, 'tab_c1'), (dict(tc2=None), -1, 'tab_c2'), (dict(tsig=None), -1, 'tab_sigma'),
    (dict(step2=None), -1, 'step2_dev'),
    (dict(batch=0), -1, 'batch'), (dict(channels=-1), -1, 'channels'), (dict(height=0), -1, 'height'), (dict(width=-4), -1, 'width'),
    (dict(block=3), -1, 'block'), (dict(block=1), -1, 'block'), (dict(block=64, height=64, width=64), -1, 'block'), (dict(block=0), -1, 'block'),
    (dict(block=8), -1, 'width'), (dict(height=6), -1, 'height'),
    (dict(strength=float('nan')), -1, 'strength'), (dict(strength=0.0), -1, 'strength'), (dict(strength=-0.5), -1, 'strength'),
    (dict(strength=1.5), -1, 'strength'), (dict(strength=float('inf')), -1, 'strength'),
    (dict(c3=_p(10)), -1, 'c3'), (dict(hist=_p(11)), -1, 'c3'),
    (dict(c3=_p(10), hist=_p(1)), -1, 'history overlaps'), (dict(c3=_p(10), hist=_p(2)), -1, 'history overlaps'),
    (dict(c3=_p(10), hist=C.c_void_p((1 << 24) + 2 * 3 * 8 * 12 * 4 - 4)), -1, 'history overlaps'),
    (dict(y=_p(1)), -1, 'target_means'), (dict(y=C.c_void_p((1 << 24) + 2 * 3 * 8 * 12 * 4 - 4)), -1, 'target_means'),
    (dict(y=C.c_void_p((1 << 24) - 4)), -1, 'target_means'),
    (dict(batch=1 << 12, channels=2, height=1 << 9, width=1 << 9), -2, '2^31'),
]


@pytest.mark.parametrize('case', range(len(STEP_REFUSALS)))
def test_consistent_step_refusals_no_gpu(case):
    """every refusal of sr3_consistent_step returns its code and names the argument, before any launch: no device is present here"""
    from sr3_hip import lib as L
    lib = L.load()
    kw, code, word = STEP_REFUSALS[case]
    assert lib.sr3_consistent_step(*_step_args(**kw)) == code, kw
    msg = lib.sr3_last_error().decode()
    assert msg.startswith('consistent_step') and word in msg, (kw, msg)


def test_block_mean_refusals_no_gpu():
    from sr3_hip import lib as L
    lib = L.load()
    ok = dict(src=_p(1), batch=2, channels=3, height=8, width=12, block=4, dst=_p(2))
    for kw, code, word in ((dict(src=None), -1, 'src_nchw'), (dict(dst=None), -1, 'dst_means'), (dict(batch=0), -1, 'batch'),
                           (dict(width=0), -1, 'width'), (dict(block=5), -1, 'block'), (dict(block=64, height=64, width=64), -1, 'block'),
                           (dict(block=8), -1, 'width'), (dict(height=10), -1, 'height'), (dict(dst=_p(1)), -1, 'dst_means'),
                           (dict(batch=1 << 12, channels=2, height=1 << 9, width=1 << 9), -2, '2^31')):
        a = dict(ok, **kw)
        assert lib.sr3_block_mean_f32(a['src'], a['batch'], a['channels'], a['height'], a['width'], a['block'], a['dst'], None) == code, kw
        msg = lib.sr3_last_error().decode()
        assert msg.startswith('block_mean') and word in msg, (kw, msg)


# ---- the config key and set_consistency ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['sr3_tiny', 'ddpm_tiny'])
def test_config_key_and_set_consistency(name):
    import model as Model
    opt = opt_for(name, gpu=False)
    m = Model.create_model(opt)
    netG = m.netG
    assert netG.consistency is None                                        # absent key: off
    keys = set(netG.state_dict().keys())
    val = opt['model']['beta_schedule']['val']
    val['consistency'] = {'block': 8, 'strength': 0.5}
    m.set_new_noise_schedule(val, schedule_phase='val')
    assert netG.consistency == dict(block=8, strength=0.5) and netG._loop_cache == {}
    assert set(netG.state_dict().keys()) == keys
    m.set_new_noise_schedule(opt['model']['beta_schedule']['train'], schedule_phase='train')      # the other phase has no key
    assert netG.consistency is None
    val['consistency'] = {'block': 4}
    m.set_new_noise_schedule(val, schedule_phase='val')
    assert netG.consistency == dict(block=4, strength=1.0)
    m.set_new_noise_schedule(opt['model']['beta_schedule']['train'], schedule_phase='train')
    val['consistency'] = None                                              # "consistency": null
    m.set_new_noise_schedule(val, schedule_phase='val')
    assert netG.consistency is None
    for bad, word in (({'block': 3}, 'block'), ({'block': 64}, 'block'), ({'block': 8.0}, 'block'), ({'block': True}, 'block'),
                      ({'block': '8'}, 'block'), ({'strength': 0.5}, 'block'), ({'block': 8, 'strength': 0}, 'strength'),
                      ({'block': 8, 'strength': 1.01}, 'strength'), ({'block': 8, 'strength': -1}, 'strength'),
                      ({'block': 8, 'strength': float('nan')}, 'strength'), ({'block': 8, 'strength': 'strong'}, 'strength'),
                      ({'block': 8, 'strength': None}, 'strength')):
        with pytest.raises(ValueError, match=word) as e:
            netG.set_new_noise_schedule(dict(SCHEDS[name], consistency=bad), torch.device('cpu'))
        assert repr(list(bad.values())[-1]) in str(e.value) or 'required' in str(e.value)
        assert netG.consistency is None
    # programmatic form
    netG._loop_cache['stale'] = object()
    netG.set_consistency(16, 0.25)
    assert netG.consistency == dict(block=16, strength=0.25) and netG._loop_cache == {}
    for args in ((5,), (8, 2.0), (8, 0.0)):
        with pytest.raises(ValueError):
            netG.set_consistency(*args)
    assert netG.consistency == dict(block=16, strength=0.25)
    netG._loop_cache['stale'] = object()
    netG.set_consistency(None)
    assert netG.consistency is None and netG._loop_cache == {}
    with pytest.raises(ValueError, match='consistency is off'):
        netG.p_sample_loop((1, 3, 16, 16), consistency_target=torch.zeros(1, 3, 4, 4))


def test_consistency_with_tiling_is_not_implemented():
    import model as Model
    s = SCHEDS['sr3_tiny']
    netG = Model.create_model(opt_for('sr3_tiny', gpu=False)).netG
    with pytest.raises(NotImplementedError, match='tiling'):
        netG.set_new_noise_schedule(dict(s, tiling={'tile': 16, 'overlap': 4}, consistency={'block': 4}), torch.device('cpu'))
    netG.set_new_noise_schedule(dict(s), torch.device('cpu'))
    netG.set_tiling(16, 4)
    with pytest.raises(NotImplementedError, match='tiling'):
        netG.set_consistency(4)
    assert netG.consistency is None and netG.tiling is not None
    netG.set_tiling(None)
    netG.set_consistency(4)
    with pytest.raises(NotImplementedError, match='tiling'):
        netG.set_tiling(16, 4)
    assert netG.tiling is None and netG.consistency == dict(block=4, strength=1.0)
    with pytest.raises(NotImplementedError, match='tiling'):      # the explicit tiled loop, whatever set_tiling says
        netG.p_sample_loop_tiled(torch.zeros(1, 3, 32, 32), tile=16, overlap=4)
    # a sampler and consistency go together on the SR3 variant
    netG.set_sampler(4, kind='dpmpp_2m')
    assert netG.sampler['steps'] == 4 and netG.consistency is not None
    netG.set_new_noise_schedule(dict(s, sampler={'type': 'ddim', 'steps': 4}, consistency={'block': 8}), torch.device('cpu'))
    assert netG.sampler['steps'] == 4 and netG.consistency == dict(block=8, strength=1.0)


def test_ddpm_consistency_under_a_sampler_is_not_implemented():
    import model as Model
    s = SCHEDS['ddpm_tiny']
    netG = Model.create_model(opt_for('ddpm_tiny', gpu=False)).netG
    with pytest.raises(NotImplementedError, match='t_map'):
        netG.set_new_noise_schedule(dict(s, sampler={'type': 'ddim', 'steps': 3}, consistency={'block': 4}), torch.device('cpu'))
    netG.set_new_noise_schedule(dict(s), torch.device('cpu'))
    netG.set_sampler(3, 0.0)
    with pytest.raises(NotImplementedError, match='t_map'):
        netG.set_consistency(4)
    assert netG.consistency is None
    netG.set_sampler(None)
    netG.set_consistency(4)
    with pytest.raises(NotImplementedError, match='t_map'):
        netG.set_sampler(3, 0.0)
    assert netG.sampler is None and netG.consistency == dict(block=4, strength=1.0)
    with pytest.raises(NotImplementedError, match='t_map'):
        netG.set_sampler(3, kind='dpmpp_2m')


@pytest.mark.parametrize('name', ['ddpm_tiny', 'sr3_uncond'])
def test_unconditional_consistency_needs_a_target(name):
    """an unconditional model has no conditioning image to take block means from: the chain is refused unless the caller brings the
    target (the refusal comes before anything touches a device)"""
    import model as Model
    netG = Model.create_model(opt_for(name, gpu=False)).netG
    netG.set_consistency(4)
    with pytest.raises(NotImplementedError, match='consistency_target'):
        netG.p_sample_loop((1, 3, 16, 16))
    with pytest.raises(NotImplementedError, match='consistency_target'):
        netG.sample(1)
    netG.set_consistency(None)
    from sr3_hip import lib as L
    with pytest.raises(L.Sr3Error):          # off again: today's refusal of a CPU model
        netG.p_sample_loop((1, 3, 16, 16))
