"""Progressive distillation without a device: the C-ABI entries of csrc/distill.hip (sr3_teacher_step_f32, sr3_distill_target_f32) are
exported, declared, bound and refuse bad arguments before they launch anything; explicit sampler walks; the walks and coefficients of
sr3_hip/distill.py in float64; the config plumbing (train.distill, engine.distill of *_opt.pth); and the NumPy float32 restatements
that tests/test_gpu_distill.py checks the kernels against.

`np_teacher_step` / `np_distill_target` are the contract of the kernels: fp32 elementwise operations, one rounding each (NumPy rounds
every float32 product, sum and difference on its own; it fuses nothing)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from helpers import ROOT, SCHEDS, opt_for

F = np.float32
FIXTURES = ('sr3_tiny', 'ddpm_tiny')      # T = 8 and T = 6


# ---- the restatements ---------------------------------------------------------------------------------------------------------------

def _col(v, like):
    return np.asarray(v, dtype=F).reshape((-1,) + (1,) * (like.ndim - 1))


def _np_x0(x, out_c, out_u, scale, a, b, clip):
    out = out_c
    if out_u is not None:
        out = out_u + F(scale) * (out_c - out_u)
    x0 = _col(a, x) * x - _col(b, x) * out
    if clip:
        x0 = np.minimum(np.maximum(x0, F(-1.0)), F(1.0))
    assert x0.dtype == F
    return x0


def np_teacher_step(x, out_c, out_u, scale, a, b, c1, c2, clip):
    """sr3_teacher_step_f32 on float32 arrays [B, ...] and per-image float32 coefficients [B] -> (x_next, x0)."""
    x0 = _np_x0(x, out_c, out_u, scale, a, b, clip)
    x_next = _col(c1, x) * x0 + _col(c2, x) * x
    assert x_next.dtype == F
    return x_next, x0


def np_distill_target(z_t, x_mid, out_c, out_u, scale, x0_first, a, b, w1, w2, s1, s2, clip):
    """sr3_distill_target_f32 -> (x_tgt, eps_tgt)."""
    x0b = _np_x0(x_mid, out_c, out_u, scale, a, b, clip)
    x_tgt = _col(w1, z_t) * x0_first + _col(w2, z_t) * x0b
    eps_tgt = _col(s1, z_t) * z_t - _col(s2, z_t) * x_tgt
    assert x_tgt.dtype == F and eps_tgt.dtype == F
    return x_tgt, eps_tgt


def alphas_cumprod(name):
    from sr3_hip.diffusion import make_beta_schedule
    s = SCHEDS[name]
    return np.cumprod(1.0 - make_beta_schedule(s['schedule'], s['n_timestep'], s['linear_start'], s['linear_end']))


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------

NEW = (('sr3_teacher_step_f32', 14), ('sr3_distill_target_f32', 18))


def test_symbols_are_exported_declared_and_bound():
    from sr3_hip import lib as L
    lib = L.load()
    src = open(ROOT + '/include/sr3_mi355x.h').read()
    assert 'progressive distillation (engine extension; no reference counterpart)' in src
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name, nargs in NEW:
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES and L.SIGNATURES[name][0] is C.c_int and len(L.SIGNATURES[name][1]) == nargs
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
        decl = re.search(name + r'\s*\((.*?)\)\s*;', src, flags=re.S)
        assert decl is not None and len(decl.group(1).split(',')) == nargs, name
    assert L.SIGNATURES['sr3_teacher_step_f32'][1][3] is C.c_float and L.SIGNATURES['sr3_distill_target_f32'][1][4] is C.c_float
    assert lib.sr3_version() == 1
    assert 'distill' in open(ROOT + '/image-super-resolution-via-iterative-refinement_amd/csrc/build.sh').read().split('SRCS="')[1].split('"')[0].split()
    doc = open(ROOT + '/INTEGRATION.md').read()
    assert all(name in doc for name, _ in NEW)


def _p(k, off=0):
    """a made-up, 16-byte aligned, non-NULL address: the entries below refuse before they touch memory"""
    return C.c_void_p((k << 24) + off)


NB = 2 * 96 * 4      # bytes of an image batch in the calls below

T_KEYS = ('x', 'out_c', 'out_u', 'scale', 'a', 'b', 'c1', 'c2', 'batch', 'per', 'clip', 'x_next', 'x0_out')


def _t_args(**kw):
    a = dict(x=_p(1), out_c=_p(2), out_u=_p(3), scale=1.5, a=_p(4), b=_p(5), c1=_p(6), c2=_p(7), batch=2, per=96, clip=1, x_next=_p(8),
             x0_out=_p(9))
    a.update(kw)
    return [a[k] for k in T_KEYS] + [None]


T_REFUSALS = [
    (dict(x=None), -1, 'x is NULL'), (dict(out_c=None), -1, 'out_c'), (dict(a=None), -1, 'a is NULL'), (dict(b=None), -1, 'b is NULL'),
    (dict(c1=None), -1, 'c1'), (dict(c2=None), -1, 'c2'), (dict(x_next=None), -1, 'x_next'), (dict(x0_out=None), -1, 'x0_out'),
    (dict(batch=0), -1, 'batch'), (dict(batch=-2), -1, 'batch'), (dict(per=0), -1, 'elems_per_image'), (dict(per=-96), -1, 'elems_per_image'),
    (dict(scale=float('nan')), -1, 'scale'), (dict(scale=float('inf')), -1, 'scale'), (dict(scale=float('-inf')), -1, 'scale'),
    (dict(x_next=_p(1, 4)), -1, 'x_next overlaps x partially'), (dict(x_next=_p(1, NB - 4)), -1, 'x_next overlaps x partially'),
    (dict(x0_out=_p(1)), -1, 'x0_out overlaps x'), (dict(x_next=_p(1), x0_out=_p(1, NB - 16)), -1, 'x_next overlaps x0_out'),
    (dict(x_next=_p(2)), -1, 'x_next overlaps out_c'), (dict(x0_out=_p(3, 16)), -1, 'x0_out overlaps out_u'),
    (dict(x0_out=_p(8)), -1, 'x_next overlaps x0_out'), (dict(x_next=_p(4)), -1, 'x_next overlaps a'),
    (dict(x0_out=_p(5, 4)), -1, 'x0_out overlaps b'), (dict(x_next=_p(6)), -1, 'x_next overlaps c1'), (dict(x0_out=_p(7)), -1, 'x0_out overlaps c2'),
    (dict(batch=1 << 12, per=1 << 19), -2, '2^31'), (dict(batch=1, per=(1 << 31) - 1, x0_out=_p(40)), -1, 'overlaps'),
]


@pytest.mark.parametrize('case', range(len(T_REFUSALS)))
def test_teacher_step_refusals_no_gpu(case):
    from sr3_hip import lib as L
    lib = L.load()
    kw, code, word = T_REFUSALS[case]
    assert lib.sr3_teacher_step_f32(*_t_args(**kw)) == code, kw
    msg = lib.sr3_last_error().decode()
    assert msg.startswith('teacher_step') and word in msg, (kw, msg)


D_KEYS = ('z_t', 'x_mid', 'out_c', 'out_u', 'scale', 'x0_first', 'a', 'b', 'w1', 'w2', 's1', 's2', 'batch', 'per', 'clip', 'x_tgt', 'eps_tgt')


def _d_args(**kw):
    a = dict(z_t=_p(1), x_mid=_p(2), out_c=_p(3), out_u=_p(4), scale=1.5, x0_first=_p(5), a=_p(6), b=_p(7), w1=_p(8), w2=_p(9), s1=_p(10),
             s2=_p(11), batch=2, per=96, clip=1, x_tgt=_p(12), eps_tgt=_p(13))
    a.update(kw)
    return [a[k] for k in D_KEYS] + [None]


D_REFUSALS = [(dict(**{k: None}), -1, k + ' is NULL') for k in ('z_t', 'x_mid', 'out_c', 'x0_first', 'a', 'b', 'w1', 'w2', 's1', 's2', 'x_tgt', 'eps_tgt')] + [
    (dict(batch=0), -1, 'batch'), (dict(per=0), -1, 'elems_per_image'), (dict(per=-1), -1, 'elems_per_image'),
    (dict(scale=float('nan')), -1, 'scale'), (dict(scale=float('inf')), -1, 'scale'),
    (dict(x_tgt=_p(1)), -1, 'x_tgt overlaps z_t'), (dict(eps_tgt=_p(1, NB - 4)), -1, 'eps_tgt overlaps z_t'),
    (dict(x_tgt=_p(2)), -1, 'x_tgt overlaps x_mid'), (dict(eps_tgt=_p(3)), -1, 'eps_tgt overlaps out_c'),
    (dict(x_tgt=_p(4, 32)), -1, 'x_tgt overlaps out_u'), (dict(eps_tgt=_p(5)), -1, 'eps_tgt overlaps x0_first'),
    (dict(eps_tgt=_p(12)), -1, 'x_tgt overlaps eps_tgt'), (dict(eps_tgt=_p(12, 4)), -1, 'x_tgt overlaps eps_tgt'),
] + [(dict(x_tgt=_p(6 + i)), -1, 'x_tgt overlaps ' + k) for i, k in enumerate(('a', 'b', 'w1', 'w2', 's1', 's2'))] + [
    (dict(eps_tgt=_p(10, 4)), -1, 'eps_tgt overlaps s1'), (dict(batch=1 << 12, per=1 << 19), -2, '2^31'),
]


@pytest.mark.parametrize('case', range(len(D_REFUSALS)))
def test_distill_target_refusals_no_gpu(case):
    from sr3_hip import lib as L
    lib = L.load()
    kw, code, word = D_REFUSALS[case]
    assert lib.sr3_distill_target_f32(*_d_args(**kw)) == code, kw
    msg = lib.sr3_last_error().decode()
    assert msg.startswith('distill_target') and word in msg, (kw, msg)


# ---- walks --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', FIXTURES)
def test_distill_walks_and_halving(name):
    from sr3_hip.distill import distill_walks, halve_walk
    ac = alphas_cumprod(name)
    T = ac.shape[0]
    for walk in ('logsnr', 'time'):
        for N in range(1, T // 2 + 1):
            tau2, tau_s = distill_walks(ac, N, walk)
            assert tau2.shape == (2 * N,) and tau2[-1] == T - 1 and np.all(np.diff(tau2) > 0)
            assert tau_s.dtype == np.int64 and np.array_equal(tau_s, tau2[1::2]) and tau_s[-1] == T - 1
            assert np.array_equal(halve_walk(tau2), tau_s)
            # the student's walk is next round's teacher walk
            if N % 2 == 0:
                t2, ts = distill_walks(ac, N // 2, [int(v) for v in tau_s])
                assert np.array_equal(t2, tau_s) and np.array_equal(ts, tau_s[1::2])
    with pytest.raises(ValueError, match='more than the schedule'):
        distill_walks(ac, T // 2 + 1, 'logsnr')
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            distill_walks(ac, bad, 'logsnr')
    with pytest.raises(ValueError):
        halve_walk([0, 3, T - 1])
    with pytest.raises(ValueError, match='has 2 timesteps but steps is 4'):
        distill_walks(ac, 2, [1, T - 1])


def test_halve_walk_chains_8_4_2():
    from sr3_hip.distill import distill_walks, halve_walk
    ac = alphas_cumprod('sr3_tiny')
    tau8 = distill_walks(ac, 4, 'logsnr')[0]
    assert tau8.tolist() == list(range(8))
    tau4 = halve_walk(tau8)
    tau2 = halve_walk(tau4)
    assert tau4.tolist() == [1, 3, 5, 7] and tau2.tolist() == [3, 7] and halve_walk(tau2).tolist() == [7]
    with pytest.raises(ValueError):
        halve_walk([7])


@pytest.mark.parametrize('name', FIXTURES)
def test_explicit_walks(name):
    from sr3_hip.diffusion import sampler_tables, sampler_walk
    ac = alphas_cumprod(name)
    T = ac.shape[0]
    for walk in ('time', 'logsnr'):
        for S in (1, 2, 3, T):
            tau = sampler_walk(ac, S, walk)
            for given in (list(map(int, tau)), tau, tuple(map(int, tau)), tau.astype(np.int32)):
                for steps in (S, None):
                    got = sampler_walk(ac, steps, given)
                    assert got.dtype == np.int64 and np.array_equal(got, tau)
            for kind, eta in (('ddim', 0.0), ('ddim', 0.5), ('dpmpp_2m', 0.0)):
                for pred in ('eps', 'v'):
                    want = sampler_tables(ac, S, eta, kind=kind, walk=walk, prediction=pred)
                    got = sampler_tables(ac, S, eta, kind=kind, walk=list(tau), prediction=pred)
                    assert set(got) == set(want)
                    for k in want:
                        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (walk, S, kind, k)
    # a student's walk does not start at 0: allowed for a list
    tau = sampler_walk(ac, None, [1, 3, T - 1])
    assert tau.tolist() == [1, 3, T - 1]
    assert sampler_tables(ac, None, 0.0, walk=[1, 3, T - 1])['tau'].tolist() == [1, 3, T - 1]
    for bad, word in (([0, 2, 2, T - 1], 'strictly increasing'), ([3, 1, T - 1], 'strictly increasing'), ([0, 1, T - 2], 'must end at T - 1'),
                      ([0, T], 'must lie in'), ([-1, T - 1], 'must lie in'), ([], 'list of integer'), ([0.0, float(T - 1)], 'list of integer'),
                      ([[0, T - 1]], 'list of integer'), ([0.5, T - 1], 'list of integer'),
                      (None, 'list of integer'), (3, 'list of integer')):
        with pytest.raises(ValueError, match=word):
            sampler_walk(ac, None, bad)
        with pytest.raises(ValueError, match=word):
            sampler_tables(ac, None, 0.0, walk=bad)
    with pytest.raises(ValueError, match='has 3 timesteps but steps is 4'):
        sampler_walk(ac, 4, [0, 2, T - 1])
    with pytest.raises(ValueError, match='has 3 timesteps but steps is 2'):
        sampler_tables(ac, 2, 0.0, walk=[0, 2, T - 1])
    with pytest.raises(ValueError, match='one of'):
        sampler_walk(ac, 2, 'cosine')


def test_set_sampler_carries_an_explicit_walk():
    import model as Model
    from sr3_hip.diffusion import sampler_tables
    name = 'sr3_tiny'
    opt = opt_for(name, phase='val', gpu=False)
    opt['model']['beta_schedule']['val']['sampler'] = {'type': 'ddim', 'steps': 4, 'walk': [1, 3, 5, 7]}
    m = Model.create_model(opt)
    netG = m.netG
    assert netG.sampler is None
    ac = netG._alphas_cumprod64
    netG.set_sampler(4, walk=np.array([1, 3, 5, 7]))
    assert netG.sampler == dict(type='ddim', steps=4, eta=0.0, walk=[1, 3, 5, 7]) and all(type(v) is int for v in netG.sampler['walk'])
    want = sampler_tables(ac, 4, 0.0, walk=[1, 3, 5, 7])
    assert netG._sampler_tau.tolist() == [1, 3, 5, 7] and netG._sampler_tau.dtype == torch.int32
    for k in ('a', 'b', 'c1', 'c2', 'sigma', 'level'):
        assert np.array_equal(getattr(netG, '_sampler_' + k).numpy(), want[k].astype(F)), k
    netG.set_prediction('v')              # rebuilds the tables on the same walk
    assert netG.sampler['walk'] == [1, 3, 5, 7]
    assert np.array_equal(netG._sampler_a.numpy(), sampler_tables(ac, 4, 0.0, walk=[1, 3, 5, 7], prediction='v')['a'].astype(F))
    netG.set_prediction('eps')
    with pytest.raises(ValueError, match='has 4 timesteps but steps is 3'):
        netG.set_sampler(3, walk=[1, 3, 5, 7])
    assert netG.sampler['steps'] == 4      # a refused call changes nothing
    netG.set_sampler(None)
    m.set_new_noise_schedule(opt['model']['beta_schedule']['val'], schedule_phase='val')      # the config key
    assert netG.sampler == dict(type='ddim', steps=4, eta=0.0, walk=[1, 3, 5, 7])
    # named walks keep their form
    netG.set_sampler(4)
    assert netG.sampler == dict(type='ddim', steps=4, eta=0.0)
    netG.set_sampler(4, walk='logsnr')
    assert netG.sampler == dict(type='ddim', steps=4, eta=0.0, walk='logsnr')


# ---- coefficients, float64 ------------------------------------------------------------------------------------------------------------

def _ddim(ac_from, ac_to):
    d = np.sqrt(1.0 - ac_to)
    return np.sqrt(ac_to) - d * np.sqrt(ac_from) / np.sqrt(1.0 - ac_from), d / np.sqrt(1.0 - ac_from)


CASES = [(n, N, w) for n in FIXTURES for w in ('logsnr', 'time') for N in range(1, SCHEDS[n]['n_timestep'] // 2 + 1)]


@pytest.mark.parametrize('name,N,walk', CASES)
def test_weights_are_convex(name, N, walk):
    from sr3_hip.distill import distill_coefs, distill_walks
    ac = alphas_cumprod(name)
    tau2, _ = distill_walks(ac, N, walk)
    k = np.arange(1, N + 1)
    for pred in ('eps', 'v', 'x0'):
        co = distill_coefs(ac, tau2, k, pred)
        assert np.all(np.abs(co['w1'] + co['w2'] - 1.0) <= 1e-12)
        assert np.all((co['w1'] >= 0.0) & (co['w1'] <= 1.0) & (co['w2'] >= 0.0) & (co['w2'] <= 1.0))
        assert co['w1'][0] == 0.0 and co['w2'][0] == 1.0                       # k = 1 ends on the clean node
        assert np.all(co['sigma_t'] > 0.0) and np.array_equal(co['t_node'], tau2[1::2]) and np.array_equal(co['t_mid'], tau2[0::2])
        node = np.append(1.0, ac[tau2])
        assert np.allclose(co['alpha_t'] ** 2, node[2 * k], rtol=1e-15) and np.allclose(co['alpha_m'] ** 2, node[2 * k - 1], rtol=1e-15)
    one = distill_coefs(ac, tau2, N, 'v')                                      # a scalar k
    assert one['w1'].shape == () and one['w1'] == distill_coefs(ac, tau2, k, 'v')['w1'][-1]
    for bad in (0, N + 1, [1, N + 1], 1.0, True):
        with pytest.raises(ValueError):
            distill_coefs(ac, tau2, bad, 'eps')
    with pytest.raises(ValueError):
        distill_coefs(ac, tau2[1:], 1, 'eps') if N > 1 else distill_coefs(ac, [ac.shape[0] - 1], 1, 'eps')


def _teacher_two_steps(co, z_t, out1, out2):
    """the teacher's two unclipped DDIM steps in float64 -> (x1, z_m, x2, z_e); the coefficient arrays broadcast over [K, n]"""
    c = {k: np.asarray(v)[:, None] for k, v in co.items()}
    x1 = c['a1'] * z_t - c['b1'] * out1
    z_m = c['c1'] * x1 + c['c2'] * z_t
    x2 = c['a2'] * z_m - c['b2'] * out2
    return x1, z_m, x2, c['c1b'] * x2 + c['c2b'] * z_m


@pytest.mark.parametrize('name,N,walk', CASES)
def test_one_student_step_is_the_teachers_two(name, N, walk):
    """random data, no clipping: a DDIM step of the student's own tables from z_t with x0 = x~ lands on the teacher's z_e"""
    from sr3_hip.diffusion import sampler_tables
    from sr3_hip.distill import distill_coefs, distill_walks
    ac = alphas_cumprod(name)
    tau2, tau_s = distill_walks(ac, N, walk)
    k = np.arange(1, N + 1)
    g = np.random.default_rng(N)
    z_t, out1, out2 = (g.standard_normal((N, 257)) for _ in range(3))
    tabs = sampler_tables(ac, N, 0.0, walk=list(tau_s))
    full = sampler_tables(ac, 2 * N, 0.0, walk=list(tau2))
    for pred in ('eps', 'v', 'x0'):
        co = distill_coefs(ac, tau2, k, pred)
        # the teacher's steps are rows of its own sampler tables (a, b by prediction_coefs; the eps tables' sqrt(1 / ab - 1) cancels
        # where ab is near 1: 1 - ab >= 1e-6 on these schedules leaves it ten digits, hence 1e-9 for b)
        tp = sampler_tables(ac, 2 * N, 0.0, walk=list(tau2), prediction=pred)
        assert np.allclose(co['a1'], tp['a'][2 * k - 1], rtol=1e-14) and np.allclose(co['b1'], tp['b'][2 * k - 1], rtol=1e-9)
        assert np.allclose(co['a2'], tp['a'][2 * k - 2], rtol=1e-14) and np.allclose(co['b2'], tp['b'][2 * k - 2], rtol=1e-9)
        assert np.array_equal(co['c1'], full['c1'][2 * k - 1]) and np.array_equal(co['c2'], full['c2'][2 * k - 1])
        assert np.array_equal(co['c1b'], full['c1'][2 * k - 2]) and np.array_equal(co['c2b'], full['c2'][2 * k - 2])
        x1, z_m, x2, z_e = _teacher_two_steps(co, z_t, out1, out2)
        x_t = co['w1'][:, None] * x1 + co['w2'][:, None] * x2
        got = tabs['c1'][k - 1][:, None] * x_t + tabs['c2'][k - 1][:, None] * z_t
        err = np.abs(got - z_e).max() / max(1.0, np.abs(z_e).max())
        assert err <= 1e-12, (pred, err)
        eps_t = co['s1'][:, None] * z_t - co['s2'][:, None] * x_t
        assert np.abs(co['alpha_t'][:, None] * x_t + co['sigma_t'][:, None] * eps_t - z_t).max() <= 1e-12 * max(1.0, np.abs(z_t).max())


@pytest.mark.parametrize('name,N,walk', CASES)
def test_perfect_teacher_and_prediction_kinds(name, N, walk):
    from sr3_hip.distill import distill_coefs, distill_walks
    ac = alphas_cumprod(name)
    tau2, _ = distill_walks(ac, N, walk)
    k = np.arange(1, N + 1)
    g = np.random.default_rng(100 + N)
    x, noise, X1, X2 = (g.standard_normal((N, 129)) for _ in range(4))
    x_tilde = {}
    for pred in ('eps', 'v', 'x0'):
        co = distill_coefs(ac, tau2, k, pred)
        al_t, sg_t, al_m, sg_m = (co[n][:, None] for n in ('alpha_t', 'sigma_t', 'alpha_m', 'sigma_m'))
        z_t = al_t * x + sg_t * noise

        def output(pred_x0, z, al, sg):      # what a network of this kind puts out when its x0 prediction is pred_x0
            eps = (z - al * pred_x0) / sg
            return {'eps': eps, 'v': al * eps - sg * pred_x0, 'x0': pred_x0}[pred]
        # a perfect teacher: x1 = x2 = x
        x1, z_m, _, _ = _teacher_two_steps(co, z_t, output(x, z_t, al_t, sg_t), np.zeros_like(x))
        x1, z_m, x2, _ = _teacher_two_steps(co, z_t, output(x, z_t, al_t, sg_t), output(x, z_m, al_m, sg_m))
        x_t = co['w1'][:, None] * x1 + co['w2'][:, None] * x2
        eps_t = co['s1'][:, None] * z_t - co['s2'][:, None] * x_t
        assert np.abs(x_t - x).max() <= 1e-9 and np.abs(eps_t - noise).max() <= 1e-9, (pred, np.abs(x_t - x).max(), np.abs(eps_t - noise).max())
        # any teacher: fed the outputs that stand for the same x0 predictions X1, X2, every kind gives the same x~
        x1, z_m, _, _ = _teacher_two_steps(co, z_t, output(X1, z_t, al_t, sg_t), np.zeros_like(x))
        x1, z_m, x2, _ = _teacher_two_steps(co, z_t, output(X1, z_t, al_t, sg_t), output(X2, z_m, al_m, sg_m))
        assert np.abs(x1 - X1).max() <= 1e-9 and np.abs(x2 - X2).max() <= 1e-9
        x_tilde[pred] = co['w1'][:, None] * x1 + co['w2'][:, None] * x2
    assert np.abs(x_tilde['eps'] - x_tilde['v']).max() <= 1e-9 and np.abs(x_tilde['x0'] - x_tilde['v']).max() <= 1e-9


def test_restatements_against_float64():
    """the float32 restatements follow the float64 arithmetic to fp32 rounding, clamp on both branches, k = 1 rows and guidance included"""
    from sr3_hip.distill import distill_coefs, distill_walks
    ac = alphas_cumprod('sr3_tiny')
    tau2, _ = distill_walks(ac, 4, 'logsnr')
    k = np.array([1, 4, 2])
    co = distill_coefs(ac, tau2, k, 'v')
    g = np.random.default_rng(5)
    shape = (3, 3, 4, 6)
    z_t, oc, ou, oc2, ou2 = ((1.5 * g.standard_normal(shape)).astype(F) for _ in range(5))
    c32 = {n: v.astype(F) for n, v in co.items()}
    for out_u, out_u2, scale in ((None, None, 1.0), (ou, ou2, 1.5)):
        for clip in (False, True):
            x_mid, x0a = np_teacher_step(z_t, oc, out_u, scale, c32['a1'], c32['b1'], c32['c1'], c32['c2'], clip)
            x_tgt, eps_tgt = np_distill_target(z_t, x_mid, oc2, out_u2, scale, x0a, c32['a2'], c32['b2'], c32['w1'], c32['w2'], c32['s1'], c32['s2'], clip)
            c = {n: v.reshape(-1, 1, 1, 1) for n, v in co.items()}
            o1 = oc.astype(np.float64) if out_u is None else out_u + scale * (oc.astype(np.float64) - out_u)
            o2 = oc2.astype(np.float64) if out_u is None else out_u2 + scale * (oc2.astype(np.float64) - out_u2)
            r1 = c['a1'] * z_t - c['b1'] * o1
            assert (np.abs(r1) < 1).any() and (np.abs(r1) > 1).any()
            r1 = np.clip(r1, -1, 1) if clip else r1
            rm = c['c1'] * r1 + c['c2'] * z_t
            r2 = c['a2'] * rm - c['b2'] * o2
            assert (np.abs(r2) < 1).any() and (np.abs(r2) > 1).any()
            r2 = np.clip(r2, -1, 1) if clip else r2
            rt = c['w1'] * r1 + c['w2'] * r2
            re = c['s1'] * z_t - c['s2'] * rt
            for got, want in ((x0a, r1), (x_mid, rm), (x_tgt, rt), (eps_tgt, re)):
                assert np.abs(got - want).max() <= 2e-5 * max(1.0, np.abs(want).max())
            assert np.array_equal(x_tgt[0], _np_x0(x_mid, oc2, out_u2, scale, c32['a2'], c32['b2'], clip)[0])      # k = 1: w1 = 0, w2 = 1


# ---- config -------------------------------------------------------------------------------------------------------------------------

class _StubOptimizer(object):
    def __init__(self):
        self.calls = []

    def zero_grad(self):
        self.calls.append('zero_grad')

    def step(self):
        self.calls.append('step')

    def last_grad_norm(self):
        return None


def test_key_absent_is_the_old_path():
    import model as Model
    m = Model.create_model(opt_for('sr3_tiny', phase='train', gpu=False))
    assert m.distiller is None and m._distill_state is None
    seen = []
    m.netG.p_losses = lambda x_in, noise=None: (seen.append(x_in), torch.tensor(1536.0))[1]
    m.optG = _StubOptimizer()
    m.feed_data({'HR': torch.zeros(2, 3, 16, 16), 'SR': torch.zeros(2, 3, 16, 16)})
    m.optimize_parameters()
    assert len(seen) == 1 and seen[0] is m.data and m.optG.calls == ['zero_grad', 'step']
    assert m.get_current_log()['l_pix'] == 1.0
    m2 = Model.create_model(opt_for('sr3_tiny', phase='val', gpu=False))
    assert m2.distiller is None and m2.netG.sampler is None


def test_key_on_a_cpu_model_is_refused(tmp_path):
    import model as Model
    from sr3_hip import lib as L
    opt = opt_for('sr3_tiny', phase='train', gpu=False)
    opt['train']['distill'] = {'teacher': str(tmp_path / 'no_such_teacher'), 'steps': 4, 'walk': 'logsnr', 'guidance_scale': None}
    with pytest.raises(L.Sr3Error, match='GPU'):
        Model.create_model(opt)
    for bad in ({'steps': 4}, {'teacher': 'x'}, 'teacher'):
        opt['train']['distill'] = bad
        with pytest.raises(ValueError, match='train.distill'):
            Model.create_model(opt)
    # the val phase does not read the key
    opt = opt_for('sr3_tiny', phase='val', gpu=False)
    opt['train']['distill'] = {'teacher': str(tmp_path / 'no_such_teacher'), 'steps': 4}
    assert Model.create_model(opt).distiller is None


def test_distiller_refuses_cpu_models():
    import model as Model
    from sr3_hip import lib as L
    from sr3_hip.distill import Distiller
    s = Model.create_model(opt_for('sr3_tiny', phase='train', gpu=False)).netG
    t = Model.create_model(opt_for('sr3_tiny', phase='val', gpu=False)).netG
    with pytest.raises(L.Sr3Error, match='GPU'):
        Distiller(s, t, steps=4)


def test_engine_distill_round_trip(tmp_path):
    """*_opt.pth of a distilled student records its chain; a val-phase model that resumes from it samples on that walk unless the
    config names a sampler; a model without the state writes the file it wrote before"""
    import model as Model
    opt = opt_for('sr3_tiny', phase='train', gpu=False)
    opt['path']['checkpoint'] = str(tmp_path)
    m = Model.create_model(opt)
    m.save_network(1, 10)
    ck = torch.load(str(tmp_path / 'I10_E1_opt.pth'), map_location='cpu')
    assert 'engine' not in ck
    m._distill_state = {'steps': 4, 'walk': np.array([1, 3, 5, 7])}          # what train.distill leaves behind (Distiller.state())
    m.save_network(1, 20)
    ck = torch.load(str(tmp_path / 'I20_E1_opt.pth'), map_location='cpu')
    assert ck['engine'] == {'distill': {'steps': 4, 'walk': [1, 3, 5, 7]}} and all(type(v) is int for v in ck['engine']['distill']['walk'])
    m.netG.set_prediction('v')
    m.save_network(1, 30)
    ck = torch.load(str(tmp_path / 'I30_E1_opt.pth'), map_location='cpu')
    assert ck['engine'] == {'prediction': 'v', 'distill': {'steps': 4, 'walk': [1, 3, 5, 7]}}
    # val phase: the walk becomes the sampler, on this schedule and on the val schedule set afterwards
    opt = opt_for('sr3_tiny', phase='val', gpu=False)
    opt['path']['resume_state'] = str(tmp_path / 'I20_E1')
    m2 = Model.create_model(opt)
    want = dict(type='ddim', steps=4, eta=0.0, walk=[1, 3, 5, 7])
    assert m2._distill_state == {'steps': 4, 'walk': [1, 3, 5, 7]} and m2.netG.sampler == want
    m2.set_new_noise_schedule(opt['model']['beta_schedule']['val'], schedule_phase='val')
    assert m2.netG.sampler == want and m2.netG._sampler_tau.tolist() == [1, 3, 5, 7]
    for k, v in m.netG.state_dict().items():
        assert torch.equal(m2.netG.state_dict()[k], v), k
    # ... unless the config names one
    opt = opt_for('sr3_tiny', phase='val', gpu=False)
    opt['path']['resume_state'] = str(tmp_path / 'I20_E1')
    opt['model']['beta_schedule']['val']['sampler'] = {'type': 'ddim', 'steps': 3}
    m3 = Model.create_model(opt)
    m3.set_new_noise_schedule(opt['model']['beta_schedule']['val'], schedule_phase='val')
    assert m3.netG.sampler == dict(type='ddim', steps=3, eta=0.0)
    # a checkpoint without the record: no sampler
    opt = opt_for('sr3_tiny', phase='val', gpu=False)
    opt['path']['resume_state'] = str(tmp_path / 'I10_E1')
    m4 = Model.create_model(opt)
    assert m4._distill_state is None and m4.netG.sampler is None
    # a train-phase resume goes on as before and keeps the file's other keys
    opt = opt_for('sr3_tiny', phase='train', gpu=False)
    opt['path']['resume_state'] = str(tmp_path / 'I20_E1')
    m5 = Model.create_model(opt)
    assert m5.begin_step == 20 and m5.distiller is None and m5.netG.sampler is None
