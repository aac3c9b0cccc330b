"""Training objective, CPU side (no GPU): the coefficient functions behind v- / x0-prediction and Min-SNR weights (pure numpy), what
`sampler_tables` changes with the prediction, every refusal of the Python setters and of the two C entries (sr3_train_step_ex,
sr3_loss_grad_f32: argument checks launch nothing, so they run without a device), and the checkpoint's `engine` key."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from helpers import SCHEDS, opt_for
from oracle import sr3_oracle as O
from sr3_hip import diffusion as D          # (prediction_coefs / loss_weights: an ImportError here is the feature missing)
from sr3_hip.diffusion import loss_weights, prediction_coefs, sampler_tables

NAMES = ('sr3_tiny', 'ddpm_tiny')


def _ac(name):
    s = SCHEDS[name]
    return np.cumprod(1.0 - D.make_beta_schedule(s['schedule'], s['n_timestep'], s['linear_start'], s['linear_end']))


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('kind', D.PREDICTIONS)
def test_prediction_coefs_recover_x0(name, kind):
    """x0_a x - x0_b target == x0 for x = ca x0 + cb z: the step tail's a, b invert the training target, in float64."""
    ac = _ac(name)
    ca, cb = np.sqrt(ac)[:, None], np.sqrt(1.0 - ac)[:, None]
    rng = np.random.default_rng(5)
    x0, z = rng.uniform(-1, 1, (1, 64)), rng.standard_normal((1, 64))
    a, b, tz, tx = prediction_coefs(kind, ca, cb)
    assert a.shape == b.shape == tz.shape == tx.shape == ca.shape and a.dtype == np.float64
    got = a * (ca * x0 + cb * z) - b * (tz * z + tx * x0)
    # (eps amplifies by 1 / ca <= 1.03 on these schedules: 1e-12 absolute is > 1000 ulp of the terms)
    assert np.abs(got - x0).max() <= 1e-12, np.abs(got - x0).max()


@pytest.mark.parametrize('name', NAMES)
def test_eps_coefs_are_todays_tables(name):
    """eps: the fp32 tables the engine holds today (the reference's sqrt_recip / sqrt_recipm1 buffers), bit for bit; v: the buffers
    sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod; x0: the constants."""
    ac, tab = _ac(name), O.schedule_tables(SCHEDS[name])
    f = lambda v: np.asarray(v, dtype=np.float32)
    a, b, tz, tx = prediction_coefs('eps', np.sqrt(ac), np.sqrt(1.0 - ac))
    assert np.array_equal(f(a), tab['sqrt_recip_alphas_cumprod']) and np.array_equal(f(b), tab['sqrt_recipm1_alphas_cumprod'])
    assert np.all(tz == 1.0) and np.all(tx == 0.0)
    a, b, tz, tx = prediction_coefs('v', np.sqrt(ac), np.sqrt(1.0 - ac))
    assert np.array_equal(f(a), tab['sqrt_alphas_cumprod']) and np.array_equal(f(b), tab['sqrt_one_minus_alphas_cumprod'])
    assert np.array_equal(tz, a) and np.array_equal(tx, -b)
    a, b, tz, tx = prediction_coefs('x0', np.sqrt(ac), np.sqrt(1.0 - ac))
    assert np.all(a == 0.0) and np.all(b == -1.0) and np.all(tz == 0.0) and np.all(tx == 1.0)


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('gamma', [5.0, 0.5, 1e3])
def test_loss_weights_are_min_snr(name, gamma):
    ac = _ac(name)
    ca = np.sqrt(ac)
    snr = ac / (1.0 - ac)
    div = {'eps': snr, 'v': snr + 1.0, 'x0': np.ones_like(snr)}
    for kind in D.PREDICTIONS:
        w = loss_weights(kind, 'min_snr', gamma, ca)
        ref = np.minimum(snr, gamma) / div[kind]
        assert w.dtype == np.float64 and np.allclose(w, ref, rtol=1e-9, atol=0.0), (kind, w, ref)
        assert np.array_equal(loss_weights(kind, 'uniform', None, ca), np.ones_like(ca))
    # (the tiny schedules' SNR runs from 1e4 .. 1e6 down to about 20: gamma = 1e3 takes both branches of the min)
    if gamma == 1e3:
        assert (snr > gamma).any() and (snr < gamma).any()


def test_loss_weights_at_infinite_snr():
    """ca = 1 (the first entry of SR3's level table: SNR infinite): finite, and the limit of min(SNR, gamma) / {SNR, SNR + 1, 1}."""
    one = np.array([1.0, np.sqrt(0.5)])
    assert np.array_equal(loss_weights('eps', 'min_snr', 5.0, one), [0.0, 1.0])
    assert np.array_equal(loss_weights('v', 'min_snr', 5.0, one)[:1], [0.0])
    assert np.array_equal(loss_weights('x0', 'min_snr', 5.0, one)[:1], [5.0])
    for kind in D.PREDICTIONS:
        assert np.all(np.isfinite(loss_weights(kind, 'min_snr', 5.0, one)))
    assert abs(loss_weights('v', 'min_snr', 5.0, one)[1] - 0.5) < 1e-15 and abs(loss_weights('x0', 'min_snr', 5.0, one)[1] - 1.0) < 1e-15


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('kind,walk,eta', [('ddim', 'time', 0.0), ('ddim', 'time', 1.0), ('dpmpp_2m', 'logsnr', 0.0)])
def test_sampler_tables_change_a_and_b_only(name, kind, walk, eta):
    ac = _ac(name)
    base = sampler_tables(ac, 4, eta, kind=kind, walk=walk)
    dflt = sampler_tables(ac, 4, eta, kind=kind, walk=walk, prediction='eps')
    assert set(base) == set(dflt) and all(np.array_equal(base[k], dflt[k]) for k in base)
    ab = ac[base['tau']]
    for p in ('v', 'x0'):
        t = sampler_tables(ac, 4, eta, kind=kind, walk=walk, prediction=p)
        assert set(t) == set(base)
        for k in base:
            assert np.array_equal(t[k], base[k]) == (k not in ('a', 'b')), (p, k)
        a, b = prediction_coefs(p, np.sqrt(ab), np.sqrt(1.0 - ab))[:2]
        assert np.array_equal(t['a'], a) and np.array_equal(t['b'], b)
    with pytest.raises(ValueError, match='prediction'):
        sampler_tables(ac, 4, eta, kind=kind, walk=walk, prediction='score')


def _model(name='sr3_tiny', phase='val', **diffusion):
    import model as Model
    opt = opt_for(name, phase=phase, gpu=False)
    opt['model']['diffusion'].update(diffusion)
    return Model.create_model(opt), opt


def test_setters_refuse_before_any_device():
    nan, inf = float('nan'), float('inf')
    with pytest.raises(ValueError, match='prediction'):
        prediction_coefs('score', 1.0, 0.0)
    with pytest.raises(ValueError, match='weight'):
        loss_weights('v', 'snr', 5.0, 0.5)
    for bad in (0.0, -1.0, nan, inf, 'x'):
        with pytest.raises(ValueError, match='gamma'):
            loss_weights('v', 'min_snr', bad, 0.5)
    m, _ = _model()
    n = m.netG
    assert n.prediction == 'eps' and n.objective is None
    with pytest.raises(ValueError, match="'score'"):
        n.set_prediction('score')
    with pytest.raises(ValueError, match='loss type'):
        n.set_objective('l3')
    with pytest.raises(ValueError, match='loss weight'):
        n.set_objective('l1', weight='snr')
    with pytest.raises(ValueError, match='delta'):
        n.set_objective('l2', delta=1.0)
    with pytest.raises(ValueError, match='gamma'):
        n.set_objective('l2', gamma=5.0)
    for bad in (0.0, -2.0, nan, inf):
        with pytest.raises(ValueError, match='delta'):
            n.set_objective('huber', delta=bad)
        with pytest.raises(ValueError, match='gamma'):
            n.set_objective('l1', weight='min_snr', gamma=bad)
    assert n.prediction == 'eps' and n.objective is None          # a refused call changes nothing
    n.set_objective('huber', weight='min_snr')
    assert n.objective == dict(type='huber', delta=1.0, weight='min_snr', gamma=5.0)
    # the config keys reach the same setters, and refuse the same way
    m, _ = _model(prediction='v', loss={'type': 'huber', 'delta': 0.25, 'weight': 'min_snr', 'gamma': 3.0})
    assert m.netG.prediction == 'v' and m.netG.objective == dict(type='huber', delta=0.25, weight='min_snr', gamma=3.0)
    with pytest.raises(ValueError, match='prediction'):
        _model(prediction='score')
    with pytest.raises(ValueError, match='delta'):
        _model(loss={'type': 'l1', 'delta': 1.0})


def test_set_prediction_switches_tables_and_keeps_the_state_dict():
    m, _ = _model()
    n = m.netG
    keys = set(n.state_dict())
    n._loop_cache['stale'] = object()
    n.set_prediction('v')
    assert not n._loop_cache
    a, b = n._x0_tables()
    assert a is n.sqrt_alphas_cumprod and b is n.sqrt_one_minus_alphas_cumprod and n._step_rule()[0][:2] == (a, b)
    n.set_sampler(4, 0.0, kind='dpmpp_2m')
    ref = sampler_tables(n._alphas_cumprod64, 4, 0.0, kind='dpmpp_2m', walk='logsnr', prediction='v')
    assert torch.equal(n._sampler_a, torch.tensor(ref['a'], dtype=torch.float32))
    n._loop_cache['stale'] = object()
    n.set_prediction('x0')                     # a configured sampler's tables follow
    assert not n._loop_cache and n.sampler == dict(type='dpmpp_2m', steps=4, eta=0.0, walk='logsnr')
    assert torch.equal(n._sampler_a, torch.zeros(4)) and torch.equal(n._sampler_b, -torch.ones(4))
    assert torch.equal(n._sampler_c1, torch.tensor(ref['c1'], dtype=torch.float32))
    n.set_sampler(None)
    a, b = n._x0_tables()
    assert torch.equal(a, torch.zeros(8)) and torch.equal(b, -torch.ones(8))
    n._loop_cache['stale'] = object()
    n.set_objective('l2')
    assert not n._loop_cache
    n.set_prediction('eps')
    assert n._x0_tables() == (n.sqrt_recip_alphas_cumprod, n.sqrt_recipm1_alphas_cumprod)
    assert set(n.state_dict()) == keys


def _fake():
    return C.cast(C.create_string_buffer(64), C.c_void_p)          # a non-NULL pointer nothing may read: the refusals launch nothing


def test_c_entries_refuse_bad_objective_arguments():
    from sr3_hip import engine as E, lib as L
    lib = L.load()
    f, p = C.c_float, _fake()
    plan = E.Plan('sr3', 6, 3, 8, 4, [1, 2], [8], 1, 16)

    def step(tz, tx, w, kind, delta):
        return lib.sr3_train_step_ex(plan.handle, p, p, 3, p, p, p, p, None, p, p, p, p, 1 << 30, p, f(1.0), f(0.0), 0, 0, None, None, 2,
                                     tz, tx, w, kind, f(delta), None)

    def op(tz, tx, w, kind, delta, channels=3, batch=2, pixels=16, hr=p, scratch=p):
        return lib.sr3_loss_grad_f32(p, p, hr, tz, tx, w, batch, channels, pixels, kind, f(delta), f(1.0), p, p, scratch, None)

    assert lib.sr3_loss_grad_scratch_bytes() == 256 * 8
    for call, who, lo in ((step, b'sr3_train_step_ex', -1), (op, b'sr3_loss_grad_f32', 0)):
        for some in ((p, None, None), (None, p, None), (None, None, p), (p, p, None), (p, None, p), (None, p, p)):
            assert call(*some, 0, 1.0) == -1, some                      # SR3_E_BADARG
            msg = lib.sr3_last_error()
            assert who in msg and b'tgt_z' in msg and b'tgt_x0' in msg and b'weight' in msg, msg
        for kind in (lo - 1, 3, 100):
            assert call(p, p, p, kind, 1.0) == -1 and call(None, None, None, kind, 1.0) == -1
            assert who in lib.sr3_last_error() and b'loss_kind' in lib.sr3_last_error()
        for delta in (0.0, -1.0, float('nan'), float('inf')):
            assert call(p, p, p, 2, delta) == -1 and call(None, None, None, 2, delta) == -1
            assert who in lib.sr3_last_error() and b'huber_delta' in lib.sr3_last_error()
    # the op's own arguments
    assert op(p, p, p, 0, 1.0, channels=5) == -1 and b'channels' in lib.sr3_last_error()
    assert op(p, p, p, 0, 1.0, channels=0) == -1 and b'channels' in lib.sr3_last_error()
    assert op(p, p, p, 0, 1.0, batch=0) == -1 and b'batch' in lib.sr3_last_error()
    assert op(p, p, p, 0, 1.0, pixels=0) == -1 and b'pixels' in lib.sr3_last_error()
    assert op(p, p, p, 0, 1.0, hr=None) == -1 and b'hr_nchw' in lib.sr3_last_error()
    assert op(p, p, p, 0, 1.0, scratch=None) == -1 and b'scratch' in lib.sr3_last_error()
    assert op(p, p, p, 0, 1.0, scratch=C.c_void_p(p.value + 4)) == -3 and b'scratch' in lib.sr3_last_error()      # SR3_E_ALIGN
    assert lib.sr3_version() == 1                                         # additive: the ABI version does not move


def test_opt_checkpoint_records_a_non_eps_prediction(tmp_path):
    def run(sub, **diffusion):
        m, opt = _model(phase='train', **diffusion)
        os.makedirs(tmp_path / sub)
        m.opt['path']['checkpoint'] = str(tmp_path / sub)
        m.save_network(epoch=1, iter_step=3)
        return torch.load(tmp_path / sub / 'I3_E1_opt.pth', map_location='cpu'), torch.load(tmp_path / sub / 'I3_E1_gen.pth', map_location='cpu')

    ck, gen = run('eps')
    assert set(ck) == {'epoch', 'iter', 'scheduler', 'optimizer'}
    ckx, _ = run('eps_explicit', prediction='eps', loss={'type': 'l2'})
    assert set(ckx) == set(ck)
    ckv, genv = run('v', prediction='v')
    assert set(ckv) == set(ck) | {'engine'} and ckv['engine'] == {'prediction': 'v'}
    assert set(genv) == set(gen)                                          # *_gen.pth keeps the reference's format

    def resume(sub, **diffusion):
        import model as Model
        opt = opt_for('sr3_tiny', phase='train', gpu=False)
        opt['model']['diffusion'].update(diffusion)
        opt['path']['resume_state'] = str(tmp_path / sub / 'I3_E1')
        return Model.create_model(opt)

    assert resume('v', prediction='v').begin_step == 3 and resume('eps').begin_step == 3
    for sub, cfg, names in (('v', {}, ("'v'", "'eps'")), ('v', {'prediction': 'x0'}, ("'v'", "'x0'")), ('eps', {'prediction': 'v'}, ("'eps'", "'v'"))):
        with pytest.raises(ValueError) as e:
            resume(sub, **cfg)
        assert all(n in str(e.value) for n in names), str(e.value)
    # a validation-phase load reads no training state: the config alone says what the weights predict
    import model as Model
    opt = opt_for('sr3_tiny', phase='val', gpu=False)
    opt['path']['resume_state'] = str(tmp_path / 'v' / 'I3_E1')
    assert Model.create_model(opt).netG.prediction == 'eps'
