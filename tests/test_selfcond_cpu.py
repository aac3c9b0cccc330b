"""Self-conditioning without a GPU: the config key and the setter, every ValueError and every refusal by its text, the new export's
declaration against its ctypes binding, and that a model without the key draws and keys its loop states as before."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from helpers import ROOT, SCHEDS, opt_for
from selfcond_ref import opt9, write_back, x0_coefs, x0_f32


def _netG(name='sr3_tiny', prob=0.5, phase='val', in_channel=9, **diffusion):
    import model as Model
    opt = opt9(name, phase=phase, prob=prob, gpu=False, **diffusion)
    opt['model']['unet']['in_channel'] = in_channel
    return Model.create_model(opt).netG


# ---- the key and the setter -----------------------------------------------------------------------------------------------------------

def test_parse_self_condition():
    from sr3_hip.diffusion import SELF_CONDITION_PROB, parse_self_condition
    assert SELF_CONDITION_PROB == 0.5
    assert parse_self_condition(None) is None and parse_self_condition(False) is None
    assert parse_self_condition(True) == 0.5 and parse_self_condition({}) == 0.5 and parse_self_condition({'prob': None}) == 0.5
    assert parse_self_condition({'prob': 0.25}) == 0.25 and parse_self_condition({'prob': 0}) == 0
    with pytest.raises(ValueError, match=r'self_condition: true or a dict with "prob" is expected \(got 0\.5\)'):
        parse_self_condition(0.5)
    with pytest.raises(ValueError, match=r"self_condition: unknown key 'p' \(known: \"prob\"\)"):
        parse_self_condition({'p': 0.5})


def test_config_key_switches_it_on():
    assert _netG(prob=0.25).self_condition == {'prob': 0.25}
    assert _netG(prob=None, self_condition=True).self_condition == {'prob': 0.5}
    assert _netG(prob=None, self_condition={}).self_condition == {'prob': 0.5}
    for off in (None, False):
        assert _netG(prob=None, self_condition=off).self_condition is None
    assert _netG(prob=None).self_condition is None                     # key absent
    # an unconditional model: no conditioning channels, 2 x 3 image channels
    assert _netG('sr3_uncond', prob=1.0, in_channel=6).self_condition == {'prob': 1.0}


def test_setter_and_its_value_errors():
    netG = _netG(prob=None)
    netG._loop_cache = {'stale': 1}
    netG.set_self_condition(0.75)
    assert netG.self_condition == {'prob': 0.75} and netG._loop_cache == {}
    netG.set_self_condition(0)
    assert netG.self_condition == {'prob': 0.0}
    netG.set_self_condition(1)
    assert netG.self_condition == {'prob': 1.0}
    netG.set_self_condition()
    assert netG.self_condition is None
    for bad in (-0.1, 1.5, float('nan'), True):
        with pytest.raises(ValueError, match=r'self_condition prob must lie in \[0, 1\]'):
            netG.set_self_condition(bad)
    with pytest.raises(ValueError, match=r"self_condition prob must be a number \(got 'half'\)"):
        netG.set_self_condition('half')
    assert netG.self_condition is None
    # the UNet's in_channel: both numbers are stated
    plain = _netG(prob=None, in_channel=6)
    with pytest.raises(ValueError, match=r'in_channel 9 \(3 conditioning \+ 2 x 3 image channels\); this one has in_channel 6'):
        plain.set_self_condition(0.5)
    assert plain.self_condition is None
    with pytest.raises(ValueError, match=r'in_channel 6 \(0 conditioning \+ 2 x 3 image channels\); this one has in_channel 3'):
        _netG('sr3_uncond', prob=None, in_channel=3).set_self_condition(0.5)
    with pytest.raises(ValueError, match=r'in_channel 9 .* in_channel 6'):
        _netG(prob=0.5, in_channel=6)                                  # the config key goes through the same check


# ---- what it does not go with -----------------------------------------------------------------------------------------------------------

TILING = r'self-conditioning with tiling: the conditioning tiles are gathered once per chain'
GUIDANCE = r'self-conditioning with guidance: the second forward and the guided x0 live inside sr3_guided_step'
DDPM = r'self-conditioning of the DDPM variant under a sampler \(DDIM, DPM-Solver\+\+\): .* sr3_unet_forward, which has no step-index -> timestep map'
DISTILL = r'self-conditioning with train\.distill: .* on the student'


def test_refused_when_set():
    netG = _netG()
    with pytest.raises(NotImplementedError, match=TILING):
        netG.set_tiling(8, 2)
    assert netG.tiling is None
    with pytest.raises(NotImplementedError, match=GUIDANCE):
        netG.set_guidance(1.5)
    assert netG.guidance is None
    # the other order
    other = _netG(prob=None)
    other.set_tiling(8, 2)
    with pytest.raises(NotImplementedError, match=TILING):
        other.set_self_condition(0.5)
    other.set_tiling(None)
    other.set_guidance(1.5)
    with pytest.raises(NotImplementedError, match=GUIDANCE):
        other.set_self_condition(0.5)
    assert other.self_condition is None
    other.set_guidance(None)
    other.set_self_condition(0.5)
    # what does work is not refused: the samplers and the other two rules on the SR3 variant, every prediction, cond_drop
    for kind in ('ddim', 'dpmpp_2m'):
        netG.set_sampler(4, kind=kind)
    netG.set_consistency(4)
    netG.set_consistency(None)
    netG.set_backprojection(4)
    netG.set_backprojection(None)
    for p in ('v', 'x0', 'eps'):
        netG.set_prediction(p)
    netG.set_cond_drop(0.1)
    assert netG.self_condition == {'prob': 0.5}


def test_ddpm_variant_under_a_sampler_is_refused():
    ddpm = _netG('ddpm_tiny', prob=0.5, in_channel=6)                  # the ancestral sampler: fine
    assert ddpm.variant == 'ddpm' and ddpm.self_condition == {'prob': 0.5} and ddpm.sampler is None
    with pytest.raises(NotImplementedError, match=DDPM):
        ddpm.set_sampler(3)
    assert ddpm.sampler is None
    other = _netG('ddpm_tiny', prob=None, in_channel=6)
    other.set_sampler(3)
    with pytest.raises(NotImplementedError, match=DDPM):
        other.set_self_condition(0.5)
    # the schedule's own key goes through set_sampler
    with pytest.raises(NotImplementedError, match=DDPM):
        ddpm.set_new_noise_schedule(dict(SCHEDS['ddpm_tiny'], sampler={'type': 'ddim', 'steps': 3}), torch.device('cpu'))


def test_refused_when_the_loop_starts():
    """settings that got past the setters (attributes written directly, the tiled loop's own arguments) stop the loop before any launch"""
    netG = _netG()
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(NotImplementedError, match=TILING):
        netG.p_sample_loop_tiled(x, tile=8, overlap=2)
    netG.guidance = dict(scale=1.5, threshold='static', percentile=None)
    with pytest.raises(NotImplementedError, match=GUIDANCE):
        netG.p_sample_loop(x)
    netG.guidance = None
    ddpm = _netG('ddpm_tiny', prob=0.5, in_channel=6)
    ddpm.sampler = dict(type='ddim', steps=3, eta=0.0)
    with pytest.raises(NotImplementedError, match=DDPM):
        ddpm.p_sample_loop((1, 3, 16, 16))
    # with nothing in the way the loop gets as far as asking for a GPU
    from sr3_hip import lib as L
    with pytest.raises(L.Sr3Error, match='GPU'):
        netG.p_sample_loop(x)


def test_distillation_is_refused():
    from sr3_hip.distill import Distiller
    s, t = _netG(phase='train'), _netG(prob=None)
    with pytest.raises(NotImplementedError, match=DISTILL):
        Distiller(s, t, steps=4)
    with pytest.raises(NotImplementedError, match=r'self-conditioning with train\.distill: .* on the teacher'):
        Distiller(t, s, steps=4)


def test_self_cond_flags_need_the_setting():
    netG = _netG(prob=None)
    data = {'HR': torch.zeros(2, 3, 16, 16), 'SR': torch.zeros(2, 6, 16, 16)}
    with pytest.raises(ValueError, match=r'self_cond is given but self-conditioning is off'):
        netG.p_losses(data, noise=torch.zeros(2, 3, 16, 16), gamma=torch.tensor([0.9, 0.8]), self_cond=[1, 0])


# ---- the export ---------------------------------------------------------------------------------------------------------------------------

def test_export_is_declared_and_bound_with_the_headers_signature():
    from sr3_hip import lib as L
    src = open(os.path.join(ROOT, 'include', 'sr3_mi355x.h')).read()
    m = re.search(r'\bint\s+sr3_selfcond_x0_f32\s*\(([^)]*)\)\s*;', src)
    assert m, 'sr3_selfcond_x0_f32 is not declared in include/sr3_mi355x.h'
    params = [' '.join(p.split()) for p in m.group(1).split(',')]
    names = [p.split()[-1].lstrip('*') for p in params]
    assert names == ['x_nchw', 'out_nchw', 'tab_a', 'tab_b', 'step_dev', 'keep_dev', 'clip', 'batch', 'channels', 'height', 'width',
                     'dst_nchw', 'dst_channels', 'dst_first_channel', 'stream']
    want = [C.c_void_p if '*' in p else {'int': C.c_int}[p.split()[0]] for p in params]
    res, args = L.SIGNATURES['sr3_selfcond_x0_f32']
    assert res is C.c_int and args == want
    lib = L.load()
    assert lib.sr3_selfcond_x0_f32.argtypes == want
    # the comment in front of it is the contract: both forms and the refusals are stated
    doc = src[:m.start()].rsplit('/*', 1)[1]
    for word in ('step_dev', 'keep_dev', 'SR3_E_BADARG', 'dst_first_channel + channels > dst_channels', 'untouched'):
        assert word in doc, word
    assert 'selfcond' in open(os.path.join(ROOT, 'image-super-resolution-via-iterative-refinement_amd', 'csrc', 'build.sh')).read()
    assert '`sr3_selfcond_x0_f32`' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_refusals_need_no_gpu():
    """every argument check comes before any launch, so each refusal can be provoked with host pointers"""
    from sr3_hip import lib as L
    lib = L.load()
    x, out, dst = np.zeros((2, 3, 4, 4), np.float32), np.zeros((2, 3, 4, 4), np.float32), np.zeros((2, 6, 4, 4), np.float32)
    a, b = np.ones(2, np.float32), np.ones(2, np.float32)
    p = lambda t: None if t is None else C.c_void_p(t.ctypes.data)

    def call(x=x, out=out, a=a, b=b, dims=(2, 3, 4, 4), dst=dst, dc=6, first=3):
        rc = lib.sr3_selfcond_x0_f32(p(x), p(out), p(a), p(b), None, None, 1, *dims, p(dst), dc, first, None)
        return rc, (lib.sr3_last_error() or b'').decode()
    BAD, UNSUP = -1, None
    for kw, text in ((dict(x=None), 'selfcond_x0: x_nchw is NULL'), (dict(out=None), 'selfcond_x0: out_nchw is NULL'),
                     (dict(a=None), 'selfcond_x0: tab_a is NULL'), (dict(b=None), 'selfcond_x0: tab_b is NULL'),
                     (dict(dst=None), 'selfcond_x0: dst_nchw is NULL'),
                     (dict(dims=(0, 3, 4, 4)), 'selfcond_x0: batch, channels, height and width must be positive (got 0, 3, 4, 4)'),
                     (dict(dims=(2, 3, 4, -1)), 'selfcond_x0: batch, channels, height and width must be positive (got 2, 3, 4, -1)'),
                     (dict(dc=0), 'selfcond_x0: dst_channels must be positive (got 0)'),
                     (dict(first=-1), 'selfcond_x0: dst_first_channel must not be negative (got -1)'),
                     (dict(first=4), 'selfcond_x0: dst_first_channel 4 + channels 3 exceeds dst_channels 6'),
                     (dict(dst=x, dc=3, first=0), 'selfcond_x0: dst_nchw overlaps x_nchw'),
                     (dict(dst=out, dc=3, first=0), 'selfcond_x0: dst_nchw overlaps out_nchw')):
        rc, msg = call(**kw)
        assert rc < 0 and msg == text, (kw, rc, msg)
    rc, msg = call(dims=(1 << 10, 3, 1 << 10, 1 << 10), dc=3, first=0)
    assert rc < 0 and msg == 'selfcond_x0: image batch too large (batch * channels * height * width >= 2^31)', (rc, msg)
    assert not x.any() and not dst.any()


# ---- the restatement the GPU tests compare against ------------------------------------------------------------------------------------

def test_restatement_sanity():
    rng = np.random.default_rng(3)
    x, out = (rng.standard_normal((3, 3, 3, 5)).astype(np.float32) for _ in range(2))
    a, b = np.float32([1.1, 0.7, 0.9]), np.float32([0.2, 0.75, 0.43])
    x0 = x0_f32(a, b, x, out, True)
    assert x0.dtype == np.float32 and np.abs(x0).max() <= 1.0 and (np.abs(x0) == 1.0).any()
    raw = x0_f32(a, b, x, out, False)
    assert np.abs(raw).max() > 1.0 and np.array_equal(np.clip(raw, -1, 1), x0)
    assert np.array_equal(raw[1], np.float32(0.7) * x[1] - np.float32(0.75) * out[1])
    dst = np.full((3, 6, 3, 5), 7.0, np.float32)
    got = write_back(dst, x, out, a, b, [1, 0, 1], True, 3)
    assert np.all(got[:, :3] == 7.0) and np.array_equal(got[0, 3:], x0[0]) and not got[1, 3:].any() and np.array_equal(got[2, 3:], x0[2])
    # x0 = a x - b out inverts each parameterisation on exact data
    ca = np.float64([0.9, 0.5])
    cb = np.sqrt(1 - ca ** 2)
    x0t, z = rng.uniform(-1, 1, (2, 1, 1, 1)), rng.standard_normal((2, 1, 1, 1))
    xt = ca.reshape(-1, 1, 1, 1) * x0t + cb.reshape(-1, 1, 1, 1) * z
    outs = {'eps': z, 'v': ca.reshape(-1, 1, 1, 1) * z - cb.reshape(-1, 1, 1, 1) * x0t, 'x0': x0t}
    for kind, o in outs.items():
        ka, kb = x0_coefs(kind, ca)
        assert np.abs(x0_f32(ka, kb, xt, o, False) - x0t).max() < 1e-5, kind


# ---- off means off ------------------------------------------------------------------------------------------------------------------------

def test_without_the_key_the_draws_and_the_loop_state_key_are_unchanged():
    netG = _netG(prob=None, in_channel=6, phase='train')
    assert netG.self_condition is None
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
    # the loop-state key of a plain model, component by component; a self-conditioned state appends its marker
    un = netG.denoise_fn
    shape = (2, 3, 16, 16)
    netG._loop_state(shape, shape, torch.device('cpu'))
    want = (shape, shape, 'cpu', netG.num_timesteps, un.weights().data_ptr(), un.freq.data_ptr(), un.plan.generation, False, None,
            None, None, None, None)
    assert list(netG._loop_cache.keys()) == [want]
    st = netG._loop_cache[want]
    assert st['self_condition'] is False and tuple(st['cond'].shape) == shape
    wide = (2, 6, 16, 16)
    netG._loop_state(shape, wide, torch.device('cpu'), self_condition=True)
    assert list(netG._loop_cache.keys())[-1] == want[:1] + (wide,) + want[2:] + ('self_condition',)
