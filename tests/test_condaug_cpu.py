"""Noise conditioning augmentation without a GPU: the config key and the setter, every ValueError and every refusal by its text, the
float64 -> fp32 coefficients, the new export's declaration against its ctypes binding, its argument refusals byte for byte
(tests/golden/cond_augment_refusals.json), and that a model without the key draws and keys its loop states as before.

Record the refusals again (only from a library whose refusals are the wanted ones):  python tests/test_condaug_cpu.py"""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'cond_augment_refusals.json')
AUG = {'max_level': 0.5, 'sample_level': 0.1, 'level_channel': True}
BLIND = {'max_level': 0.5, 'sample_level': 0.1, 'level_channel': False}


def _netG(name='sr3_tiny', aug=AUG, phase='val', in_channel=7, **diffusion):
    import model as Model
    from condaug_ref import opt7
    return Model.create_model(opt7(name, phase=phase, aug=aug, gpu=False, in_channel=in_channel, **diffusion)).netG


# ---- the key and the setter -----------------------------------------------------------------------------------------------------------

def test_parse_cond_augment():
    from sr3_hip.diffusion import parse_cond_augment
    assert parse_cond_augment(None) == {'max_level': None}
    assert parse_cond_augment(AUG) == AUG
    assert parse_cond_augment({'max_level': 0.25}) == {'max_level': 0.25, 'sample_level': 0.0, 'level_channel': True}
    with pytest.raises(ValueError, match=r'cond_augment: a dict with "max_level" is expected \(got 0\.5\)'):
        parse_cond_augment(0.5)
    with pytest.raises(ValueError, match=r'cond_augment: a dict with "max_level" is expected \(got True\)'):
        parse_cond_augment(True)
    for k in ('level', 'max', 'prob', 'Max_level'):
        with pytest.raises(ValueError, match=r"cond_augment: unknown key '%s' \(known: \"max_level\", \"sample_level\", \"level_channel\"\)" % k):
            parse_cond_augment({'max_level': 0.5, k: 0.1})
    for spec in ({}, {'sample_level': 0.1}, {'max_level': None}):
        with pytest.raises(ValueError, match=r'cond_augment: "max_level" is required'):
            parse_cond_augment(spec)


def test_config_key_switches_it_on():
    assert _netG().cond_augment == AUG
    assert _netG(aug=BLIND, in_channel=6).cond_augment == BLIND
    assert _netG(aug={'max_level': 0}).cond_augment == {'max_level': 0.0, 'sample_level': 0.0, 'level_channel': True}
    assert _netG(aug=None, in_channel=6).cond_augment is None                              # key absent
    assert _netG(aug=None, in_channel=6, cond_augment=None).cond_augment is None           # null
    with pytest.raises(ValueError, match=r"cond_augment: unknown key 'levels'"):
        _netG(aug={'max_level': 0.5, 'levels': 3})
    with pytest.raises(ValueError, match=r'in_channel 7 .* in_channel 6'):
        _netG(in_channel=6)                                                                # the config key goes through the setter's check


def test_setter_and_its_value_errors():
    netG = _netG(aug=None)
    netG._loop_cache = {'stale': 1}
    netG.set_cond_augment(0.5, 0.1)
    assert netG.cond_augment == AUG and netG._loop_cache == {}
    netG.set_cond_augment(0)
    assert netG.cond_augment == {'max_level': 0.0, 'sample_level': 0.0, 'level_channel': True}
    netG.set_cond_augment()
    assert netG.cond_augment is None
    netG.set_cond_augment(0.25, 0.5, True)
    netG.set_cond_augment(None)
    assert netG.cond_augment is None
    for bad in (-0.1, 1.0, 1.5, float('nan'), float('inf'), True):
        with pytest.raises(ValueError, match=r'cond_augment max_level must lie in \[0, 1\)'):
            netG.set_cond_augment(bad)
        with pytest.raises(ValueError, match=r'cond_augment sample_level must lie in \[0, 1\)'):
            netG.set_cond_augment(0.5, bad)
    with pytest.raises(ValueError, match=r"cond_augment max_level must be a number \(got 'half'\)"):
        netG.set_cond_augment('half')
    with pytest.raises(ValueError, match=r'cond_augment sample_level must be a number \(got \[0\.1\]\)'):
        netG.set_cond_augment(0.5, [0.1])
    for bad in (1, 0, 'yes', None):
        with pytest.raises(ValueError, match=r'cond_augment level_channel must be true or false'):
            netG.set_cond_augment(0.5, 0.1, bad)
    assert netG.cond_augment is None
    # the UNet's in_channel: both numbers are stated; the blind form takes the UNet as it is
    plain = _netG(aug=None, in_channel=6)
    with pytest.raises(ValueError, match=r'in_channel 7 \(3 conditioning \+ 1 level \+ 3 image channels\); this one has in_channel 6'):
        plain.set_cond_augment(0.5)
    assert plain.cond_augment is None
    plain.set_cond_augment(0.5, 0.1, False)
    assert plain.cond_augment == BLIND
    # an unconditional model has nothing to augment, in either form
    for lc in (True, False):
        with pytest.raises(ValueError, match=r'cond_augment on an unconditional model: there is no conditioning image to augment'):
            _netG('sr3_uncond', aug=None, in_channel=3).set_cond_augment(0.5, 0.1, lc)
    with pytest.raises(ValueError, match=r'cond_augment on an unconditional model'):
        _netG('sr3_uncond', aug=BLIND, in_channel=3)


# ---- what it does not go with -----------------------------------------------------------------------------------------------------------

SELFCOND = r'cond_augment with the level channel together with self-conditioning: a 10-channel input'
DISTILL = r'cond_augment with train\.distill: .* on the %s'


def test_level_channel_with_self_conditioning_is_refused_in_either_order():
    netG = _netG(aug=None, in_channel=9)
    netG.set_self_condition(0.5)
    with pytest.raises(NotImplementedError, match=SELFCOND):
        netG.set_cond_augment(0.5, 0.1, True)
    assert netG.cond_augment is None
    netG = _netG(in_channel=7)
    with pytest.raises(NotImplementedError, match=SELFCOND):
        netG.set_self_condition(0.5)
    assert netG.self_condition is None
    # and again when the loop starts, whatever put the two settings there
    netG.self_condition = {'prob': 0.5}
    with pytest.raises(NotImplementedError, match=SELFCOND):
        netG.p_sample_loop(torch.zeros(1, 3, 16, 16))
    # the blind form goes with self-conditioning, in either order
    netG = _netG(aug=None, in_channel=9)
    netG.set_self_condition(0.5)
    netG.set_cond_augment(0.5, 0.1, False)
    netG.set_self_condition(None)
    netG.set_self_condition(0.25)
    assert netG.cond_augment == BLIND and netG.self_condition == {'prob': 0.25}


def test_distillation_is_refused():
    from sr3_hip.distill import Distiller
    s, t = _netG(phase='train'), _netG(aug=None)
    with pytest.raises(NotImplementedError, match=DISTILL % 'student'):
        Distiller(s, t, steps=4)
    with pytest.raises(NotImplementedError, match=DISTILL % 'teacher'):
        Distiller(t, s, steps=4)
    # switched on behind a Distiller: refused when its step starts
    d = Distiller.__new__(Distiller)
    d.student, d.teacher = t, s
    with pytest.raises(NotImplementedError, match=DISTILL % 'teacher'):
        d.step({'HR': torch.zeros(1, 3, 16, 16), 'SR': torch.zeros(1, 3, 16, 16)})


def test_injected_values_need_the_setting():
    netG = _netG(aug=None, in_channel=6)
    data = {'HR': torch.zeros(2, 3, 16, 16), 'SR': torch.zeros(2, 3, 16, 16)}
    kw = dict(noise=torch.zeros(2, 3, 16, 16), gamma=torch.tensor([0.9, 0.8]))
    with pytest.raises(ValueError, match=r'cond_level / cond_noise is given but noise conditioning augmentation is off'):
        netG.p_losses(data, cond_level=[0.1, 0.2], **kw)
    with pytest.raises(ValueError, match=r'cond_level / cond_noise is given but noise conditioning augmentation is off'):
        netG.p_losses(data, cond_noise=torch.zeros(2, 3, 16, 16), **kw)
    with pytest.raises(ValueError, match=r'cond_noise is given but noise conditioning augmentation is off'):
        netG.p_sample_loop(data['SR'], cond_noise=torch.zeros(2, 3, 16, 16))
    netG.set_cond_augment(0.5, 0.1, False)
    with pytest.raises(ValueError, match=r'cond_level must lie in \[0, 1\)'):
        netG.p_losses(data, cond_level=[0.1, 1.0], **kw)
    # with nothing in the way the loop gets as far as asking for a GPU
    from sr3_hip import lib as L
    with pytest.raises(L.Sr3Error, match='GPU'):
        netG.p_sample_loop(data['SR'])


# ---- the coefficients -------------------------------------------------------------------------------------------------------------------

def test_level_coefficients():
    from condaug_ref import level_coefs
    from sr3_hip.diffusion import cond_level_coefs
    levels = np.concatenate([[0.0, 1e-4, 0.1, 0.25, 0.3, 0.5, 0.9, 0.999, np.nextafter(np.float32(1), np.float32(0))],
                             np.random.default_rng(0).uniform(0, 1, 2000)])
    a, s = cond_level_coefs(levels.tolist())
    assert a.dtype == torch.float32 and s.dtype == torch.float32
    ra, rs = level_coefs(levels)
    assert np.array_equal(a.numpy(), ra) and np.array_equal(s.numpy(), rs)
    assert a[0].item() == 1.0 and s[0].item() == 0.0                                     # s = 0 gives a == 1 exactly
    # a^2 + s^2 is within one fp32 ulp of 1 (in exact arithmetic on the two fp32 values)
    err = np.abs(a.numpy().astype(np.float64) ** 2 + s.numpy().astype(np.float64) ** 2 - 1.0)
    assert err.max() <= np.spacing(np.float32(1.0)), err.max()
    # a tensor of drawn levels takes the same road
    a2, s2 = cond_level_coefs(torch.tensor(levels, dtype=torch.float32))
    assert torch.equal(a2, a) and torch.equal(s2, s)


def test_restatement_sanity():
    from condaug_ref import augment, augment_f32, level_coefs
    rng = np.random.default_rng(3)
    src, eps = (rng.standard_normal((3, 3, 3, 5)).astype(np.float32) for _ in range(2))
    src[0, 0, 0, 0] = -0.0
    a, s = level_coefs([0.0, 0.25, 0.9])
    out = augment_f32(src, eps, a, s)
    assert np.array_equal(out[0].view(np.uint32), src[0].view(np.uint32))                # level 0: a bit copy, the -0.0 included
    assert np.array_equal(out[2], a[2] * src[2] + s[2] * eps[2]) and not np.array_equal(out[1], src[1])
    dst = np.full((3, 6, 3, 5), 7.0, np.float32)
    got = augment(dst, src, eps, a, s, [1, 0, 1], True, 1)
    assert np.all(got[:, 0] == 7.0) and np.all(got[:, 5] == 7.0) and np.array_equal(got[2, 1:4], out[2])
    assert not got[1, 1:5].any() and np.all(got[2, 4] == s[2]) and np.all(got[0, 4] == 0.0)
    blind = augment(dst, src, None, a, s, None, False, 0)
    assert np.array_equal(blind[:, :3], src) and np.all(blind[:, 3:] == 7.0)
    # the variance of the augmented image of a unit-variance source stays 1
    big = rng.standard_normal((1, 1, 256, 256)).astype(np.float32)
    v = augment_f32(big, rng.standard_normal(big.shape).astype(np.float32), *level_coefs([0.6])).var()
    assert abs(v - 1.0) < 0.02


# ---- the export ---------------------------------------------------------------------------------------------------------------------------

NAMES = ['src_nchw', 'eps_nchw', 'a_dev', 's_dev', 'keep_dev', 'level_channel', 'dst_nchw', 'dst_channels', 'dst_first_channel', 'batch',
         'channels', 'height', 'width', 'stream']


def test_export_is_declared_and_bound_with_the_headers_signature():
    from helpers import ROOT
    from sr3_hip import lib as L
    src = open(os.path.join(ROOT, 'include', 'sr3_mi355x.h')).read()
    m = re.search(r'\bint\s+sr3_cond_augment_f32\s*\(([^)]*)\)\s*;', src)
    assert m, 'sr3_cond_augment_f32 is not declared in include/sr3_mi355x.h'
    params = [' '.join(p.split()) for p in m.group(1).split(',')]
    assert [p.split()[-1].lstrip('*') for p in params] == NAMES
    want = [C.c_void_p if '*' in p else {'int': C.c_int}[p.split()[0]] for p in params]
    res, args = L.SIGNATURES['sr3_cond_augment_f32']
    assert res is C.c_int and args == want
    assert L.load().sr3_cond_augment_f32.argtypes == want
    # the comment in front of it is the contract: both forms, the order of the checks and what is left untouched are stated
    doc = src[:m.start()].rsplit('/*', 1)[1]
    for word in ('eps_nchw NULL', 'keep_dev', 'level_channel', 'SR3_E_BADARG', 'SR3_E_UNSUPPORTED', 'in this order', 'untouched', 'bit copy'):
        assert word in doc, word
    assert 'cond_augment' in open(os.path.join(ROOT, 'image-super-resolution-via-iterative-refinement_amd', 'csrc', 'build.sh')).read()
    assert '`sr3_cond_augment_f32`' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def _p(k, off=0):
    """a made-up, 16-byte aligned, non-NULL address: the entry refuses before it touches memory"""
    return C.c_void_p((k << 24) + off)


IMG = 2 * 3 * 4 * 4 * 4      # bytes of the default source batch
HUGE = dict(batch=1 << 10, channels=3, height=1 << 10, width=1 << 10, dc=3)      # 3 x 2^30 elements


def _args(**kw):
    a = dict(src=_p(1), eps=_p(2), a=_p(3), s=_p(4), keep=_p(5), level=1, dst=_p(6), dc=7, first=0, batch=2, channels=3, height=4, width=4,
             stream=None)
    a.update(kw)
    return [a[k] for k in ('src', 'eps', 'a', 's', 'keep', 'level', 'dst', 'dc', 'first', 'batch', 'channels', 'height', 'width', 'stream')]


# (arguments, code, a word of the message); the fixture pins the whole text.  The last rows hold two faults each: the one reported is the
# one the checks meet first -- required pointers, a_dev, the image's sizes, dst's channels, the 2^31 limit, the overlaps
REFUSALS = [
    (dict(src=None), -1, 'src_nchw is NULL'), (dict(s=None), -1, 's_dev is NULL'), (dict(dst=None), -1, 'dst_nchw is NULL'),
    (dict(a=None), -1, 'a_dev is NULL'),
    (dict(batch=0), -1, 'positive'), (dict(channels=-3), -1, 'positive'), (dict(height=0), -1, 'positive'), (dict(width=-1), -1, 'positive'),
    (dict(dc=0), -1, 'dst_channels must be positive'), (dict(first=-1), -1, 'must not be negative'),
    (dict(first=4), -1, 'dst_first_channel 4 + channels 3 + the level channel exceeds dst_channels 7'),
    (dict(first=5, level=0), -1, 'dst_first_channel 5 + channels 3 exceeds dst_channels 7'),
    (dict(dc=3), -1, 'exceeds dst_channels 3'),
    (dict(HUGE, level=0), -2, '2^31'), (dict(batch=1 << 16, channels=1, height=1 << 7, width=1 << 7, dc=2), -2, '2^31'),
    (dict(dst=_p(1)), -1, 'dst_nchw overlaps src_nchw'), (dict(dst=_p(1, IMG - 4)), -1, 'dst_nchw overlaps src_nchw'),
    (dict(dst=_p(2)), -1, 'dst_nchw overlaps eps_nchw'), (dict(dst=_p(3)), -1, 'dst_nchw overlaps a_dev'),
    (dict(s=_p(6, 16)), -1, 'dst_nchw overlaps s_dev'), (dict(keep=_p(6, 2 * 7 * 16 * 4 - 4)), -1, 'dst_nchw overlaps keep_dev'),
    (dict(src=None, a=None), -1, 'src_nchw is NULL'), (dict(a=None, batch=0), -1, 'a_dev is NULL'), (dict(batch=0, dc=0), -1, 'positive (got 0, 3'),
    (dict(dc=0, first=-1), -1, 'dst_channels must be positive'), (dict(HUGE, first=1, level=0), -1, 'exceeds dst_channels 3'),
    (dict(HUGE, level=0, dst=_p(1)), -2, '2^31'), (dict(dst=_p(1), s=_p(1)), -1, 'dst_nchw overlaps src_nchw'),
]


def _call(lib, case):
    rc = lib.sr3_cond_augment_f32(*_args(**REFUSALS[case][0]))
    return [int(rc), lib.sr3_last_error().decode()]


@pytest.fixture(scope='module')
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_every_case(recorded):
    assert sorted(recorded) == sorted('REFUSALS[%d]' % i for i in range(len(REFUSALS)))


@pytest.mark.parametrize('case', range(len(REFUSALS)))
def test_refusal_is_the_recorded_one(recorded, case):
    """every argument check comes before any launch: the codes and texts come back with made-up pointers and no device"""
    from sr3_hip import lib as L
    kw, code, word = REFUSALS[case]
    got = _call(L.load(), case)
    assert got[0] == code and word in got[1] and got[1].startswith('cond_augment: '), (kw, got)
    assert got == recorded['REFUSALS[%d]' % case], kw


# ---- off means off ------------------------------------------------------------------------------------------------------------------------

def test_without_the_key_the_draws_and_the_loop_state_key_are_unchanged():
    netG = _netG(aug=None, in_channel=6, phase='train')
    assert netG.cond_augment is None
    seen = []
    netG.denoise_fn.train_step = lambda hr, cond, z, ca, cb, level, tstep, **kw: (seen.append((cond, z, level)), torch.tensor(0.0))[1]
    data = {'HR': torch.zeros(2, 3, 16, 16), 'SR': torch.ones(2, 3, 16, 16)}
    np.random.seed(11)
    torch.manual_seed(12)
    netG.p_losses(data)
    after = (np.random.get_state()[1].copy(), torch.get_rng_state().clone())
    # the reference's draws, restated: the level's interval, the levels, z -- and nothing after them
    np.random.seed(11)
    torch.manual_seed(12)
    tt = np.random.randint(1, netG.num_timesteps + 1)
    gamma = torch.FloatTensor(np.random.uniform(netG.sqrt_alphas_cumprod_prev[tt - 1], netG.sqrt_alphas_cumprod_prev[tt], size=2))
    z = torch.randn_like(data['HR'])
    cond, got_z, level = seen[0]
    assert cond is data['SR'] and torch.equal(got_z, z) and torch.equal(level, gamma)
    assert np.array_equal(np.random.get_state()[1], after[0]) and torch.equal(torch.get_rng_state(), after[1])
    # the loop-state key of a plain model, component by component; an augmented state appends its marker, behind self-conditioning's
    un = netG.denoise_fn
    shape = (2, 3, 16, 16)
    netG._loop_state(shape, shape, torch.device('cpu'))
    want = (shape, shape, 'cpu', netG.num_timesteps, un.weights().data_ptr(), un.freq.data_ptr(), un.plan.generation, False, None,
            None, None, None, None)
    assert list(netG._loop_cache.keys()) == [want]
    st = netG._loop_cache[want]
    assert st['cond_augment'] is False and st['self_condition'] is False and tuple(st['cond'].shape) == shape
    wide = (2, 4, 16, 16)
    netG._loop_state(shape, wide, torch.device('cpu'), cond_augment=True)
    assert list(netG._loop_cache.keys())[-1] == want[:1] + (wide,) + want[2:] + ('cond_augment',)
    assert netG._loop_cache[list(netG._loop_cache.keys())[-1]]['cond_augment'] is True
    netG._loop_state(shape, (2, 6, 16, 16), torch.device('cpu'), self_condition=True, cond_augment=True)
    assert list(netG._loop_cache.keys())[-1][-2:] == ('self_condition', 'cond_augment')


if __name__ == '__main__':
    root = os.path.dirname(HERE)
    sys.path[:0] = [root, os.path.join(root, 'image-super-resolution-via-iterative-refinement_amd'), HERE]
    from sr3_hip import lib as L
    lib = L.load()
    out = {'REFUSALS[%d]' % i: _call(lib, i) for i in range(len(REFUSALS))}
    bad = [k for k, v in out.items() if v[0] >= 0]
    assert not bad, 'not refused (a launch was attempted): %s' % bad
    with open(FIXTURE, 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write('\n')
    print('recorded %d refusals from %s' % (len(out), L.LIB_PATH))
