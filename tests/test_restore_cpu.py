"""Zero-shot restoration without a device (csrc/restore.hip, sr3_hip/x0_rules.py's Restore, EngineDiffusion.set_restore): the travelled
walk and its tables, the properties of the NumPy restatement tests/restore_ref.py (what tests/test_gpu_restore.py checks the kernels
against, bit for bit), the config plumbing with every refusal, and the refusals of the three C-ABI entries -- code and whole text, as
tests/golden/restore_refusals.json recorded them.

Record again (only from a library whose refusals are the wanted ones):  python tests/test_restore_cpu.py
"""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import restore_ref as R
from helpers import ROOT, SCHEDS, opt_for

F = np.float32
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'restore_refusals.json')


# ---- the travelled walk ----------------------------------------------------------------------------------------------------------------

def _visits(walk):
    """(the indices in the order they are stepped, the counter the walk ends on)"""
    seq = [i for top, n in walk for i in range(top, top - n, -1)]
    return seq, walk[-1][0] - walk[-1][1]


@pytest.mark.parametrize('S,length,repeats', [(8, 2, 3), (8, 3, 2), (7, 3, 4), (5, 1, 2), (6, 5, 3), (2, 1, 5), (9, 4, 2)])
def test_travel_walk_visits_every_index_repeats_times(S, length, repeats):
    """length < S (a segment as long as the walk is the plain walk: test_travel_walk_plain_and_ragged)"""
    from sr3_hip.x0_rules import travel_walk, walk_jumps
    walk = travel_walk(S, length, repeats)
    seq, end = _visits(walk)
    assert end == -1 and len(seq) == S * repeats
    assert sorted(seq) == sorted(list(range(S)) * repeats)
    # segment k covers top_k = S - 1 - k length down to max(top_k - length + 1, 0), and runs `repeats` times before the next starts
    tops = list(range(S - 1, -1, -length))
    assert [t for t, _ in walk] == [t for t in tops for _ in range(repeats)] or length >= S
    for top, n in walk:
        assert top - n + 1 == max(top - length + 1, 0) or length >= S
    # one jump between two runs of a segment, from the counter below it back to its top; none between two segments
    jumps = walk_jumps(walk)
    assert len(jumps) == (0 if length >= S else len(tops) * (repeats - 1))
    assert all(to > c >= -1 for c, to in jumps)
    # an index's visits are its segment's runs: nothing below the segment is stepped before its last run ends
    first_seen = {}
    for pos, i in enumerate(seq):
        first_seen.setdefault(i, pos)
    assert all(first_seen[i] > first_seen[i + 1] for i in range(S - 1))


def test_travel_walk_plain_and_ragged():
    from sr3_hip.x0_rules import travel_walk, walk_jumps
    for S, length, repeats in ((8, 8, 3), (8, 20, 3), (8, 2, 1), (8, 1, 1), (1, 1, 1)):
        assert travel_walk(S, length, repeats) == [(S - 1, S)] and walk_jumps(travel_walk(S, length, repeats)) == []
    # 7 steps in segments of 3: the last segment is the one index 0
    assert travel_walk(7, 3, 2) == [(6, 3), (6, 3), (3, 3), (3, 3), (0, 1), (0, 1)]
    assert walk_jumps(travel_walk(7, 3, 2)) == [(3, 6), (0, 3), (-1, 0)]
    assert travel_walk(8, 2, 3)[:4] == [(7, 2), (7, 2), (7, 2), (5, 2)]
    for bad in ((0, 1, 1), (4, 0, 2), (4, 2, 0), (4.0, 2, 2), (4, True, 2)):
        with pytest.raises(ValueError, match='travel_walk'):
            travel_walk(*bad)


def test_travel_tables_match_float64():
    from sr3_hip.x0_rules import travel_tables, travel_walk, walk_jumps
    betas = np.linspace(1e-4, 2e-2, 8)
    abar = np.cumprod(1.0 - betas)
    walk = travel_walk(8, 3, 3)
    ra, rs, to = travel_tables(walk, abar)
    assert ra.dtype == F and rs.dtype == F and to.dtype == np.int32 and ra.shape == rs.shape == to.shape == (8,)
    jumps = dict(walk_jumps(walk))
    assert jumps == {4: 7, 1: 4, -1: 1}
    for r in range(8):
        c = r - 1
        if c in jumps:
            q = abar[jumps[c]] / (1.0 if c < 0 else abar[c])
            assert ra[r] == F(np.sqrt(q)) and rs[r] == F(np.sqrt(1.0 - q)) and to[r] == jumps[c]
            # ra^2 + rs^2 = 1 within one rounding of each factor: |fl(v)^2 - v^2| <= (2 u + u^2) v^2
            assert abs(float(ra[r]) ** 2 + float(rs[r]) ** 2 - 1.0) <= 2.0 * R.EPS * (1.0 + R.EPS)
        else:      # no jump is defined here: a launch would change nothing
            assert ra[r] == 1.0 and rs[r] == 0.0 and to[r] == c
    # the plain walk: every row the identity
    ra, rs, to = travel_tables(travel_walk(8, 8, 3), abar)
    assert np.all(ra == 1.0) and np.all(rs == 0.0) and to.tolist() == list(range(-1, 7))
    with pytest.raises(ValueError, match='does not fit'):
        travel_tables(walk, abar[:5])


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------

def test_mask_is_exact_at_zero_and_one():
    g = np.random.default_rng(3)
    x0, y = (g.standard_normal((2, 3, 5, 7)).astype(F) for _ in range(2))
    for mshape in ((2, 1, 5, 7), (2, 3, 5, 7)):
        m = (g.uniform(size=mshape) < 0.5).astype(F)
        out = R.project_mask(x0, y, m, 1.0)
        mb = np.broadcast_to(m, x0.shape)
        assert np.array_equal(out[mb == 1], y[mb == 1]) and np.array_equal(out[mb == 0], x0[mb == 0])
        # a strength below 1 touches the known pixels only, and goes part of the way
        half = R.project_mask(x0, y, m, 0.5)
        assert np.array_equal(half[mb == 0], x0[mb == 0])
        assert np.allclose(half[mb == 1], 0.5 * (x0[mb == 1] + y[mb == 1]), atol=1e-6)
    # the form x0 + w (y - x0) would NOT give y at w = 1: the lerp form is the contract
    alt = x0 + F(1.0) * (y - x0)
    assert not np.array_equal(alt, y)


WEIGHTS = [('mean', 3), ('rec601', 3), ([0.5, 0.25], 2), ([1.0], 1), ([0.4, -0.2, 0.3, 0.1], 4)]


@pytest.mark.parametrize('weights,channels', WEIGHTS, ids=[str(w) for w, _ in WEIGHTS])
def test_gray_projection_lands_on_the_target(weights, channels):
    from sr3_hip.x0_rules import gray_weights
    a, p = gray_weights(weights, channels)
    assert a.dtype == F and p.dtype == F and np.array_equal(p, R.pinv(a))
    g = np.random.default_rng(11 + channels)
    x0 = np.clip(g.standard_normal((2, channels, 6, 10)), -2, 2).astype(F)      # magnitude <= 2
    y = g.uniform(-1, 1, (2, 1, 6, 10)).astype(F)
    bound = R.gray_bound(a, p, 2.0, 1.0)
    once = R.project_gray(x0, y, a, p, 1.0)
    resid = np.abs((a.astype(np.float64)[None, :, None, None] * once.astype(np.float64)).sum(1, keepdims=True) - y.astype(np.float64))
    print('weights %s: residual %.3e, bound %.3e' % (weights, resid.max(), bound))
    assert 0.0 < bound < 1e-5 and resid.max() <= bound
    # applying it twice moves nothing beyond that bound: the second pass sees a residual within it, times |p_c| <= 1 / |a| ...
    twice = R.project_gray(once, y, a, p, 1.0)
    move = np.abs(twice.astype(np.float64) - once.astype(np.float64))
    pmax = np.abs(p.astype(np.float64))[None, :, None, None]
    # ... |x0''_c - x0'_c| <= |p_c| (residual + its own rounding, within the bound again) + half an ulp of the sum
    assert np.all(move <= pmax * 2.0 * bound + R.EPS * np.abs(once.astype(np.float64)) * 2.0)
    # strength 0.5 goes half the way
    half = R.project_gray(x0, y, a, p, 0.5)
    g0 = (a.astype(np.float64)[None, :, None, None] * x0.astype(np.float64)).sum(1, keepdims=True)
    gh = (a.astype(np.float64)[None, :, None, None] * half.astype(np.float64)).sum(1, keepdims=True)
    assert np.abs(gh - 0.5 * (g0 + y.astype(np.float64))).max() <= bound


def test_restatement_of_the_step_and_the_jump():
    """the tail around the projection is the shared one: with an all-zero mask the step is the plain p_sample update"""
    g = np.random.default_rng(5)
    shape = (2, 3, 4, 6)
    x, eps, z, h, y = (g.standard_normal(shape).astype(F) for _ in range(5))
    tabs = {k: np.asarray(v, dtype=F) for k, v in dict(a=[1.1, 0.9], b=[0.2, 0.43], c1=[1.0, 0.55], c2=[0.0, 0.45], sigma=[0.0, 0.5],
                                                         c3=[0.0, 0.5]).items()}
    out, hist = R.restore_step(x, eps, z, 0, y, np.zeros((2, 1, 4, 6), dtype=F), None, None, 1.0, tabs, 1, 1, h)
    x0 = np.clip(F(0.9) * x - F(0.43) * eps, F(-1), F(1))
    assert np.array_equal(hist, x0)
    assert np.array_equal(out, ((F(0.55) * x0 + F(0.45) * x) + F(0.5) * h) + z * F(0.5))
    out1, _ = R.restore_step(x, eps, None, 0, y, np.ones((2, 3, 4, 6), dtype=F), None, None, 1.0, tabs, 0, 1)
    assert np.array_equal(out1, y)                     # row 0: c1 = 1, c2 = 0, sigma = 0 -- the known image itself
    xj, c = R.travel_back(x, z, np.asarray([1.0, 0.8], dtype=F), np.asarray([0.0, 0.6], dtype=F), np.asarray([-1, 5]), 0)
    assert c == 5 and np.array_equal(xj, F(0.8) * x + F(0.6) * z)
    xi, c = R.travel_back(x, z, np.asarray([1.0, 0.8], dtype=F), np.asarray([0.0, 0.6], dtype=F), np.asarray([-1, 5]), -1)
    assert c == -1 and np.array_equal(xi, x)


# ---- the config key and set_restore ------------------------------------------------------------------------------------------------------

def _netG(name):
    import model as Model
    opt = opt_for(name, gpu=False)
    m = Model.create_model(opt)
    return m, m.netG, opt


@pytest.mark.parametrize('name', ['sr3_tiny', 'ddpm_tiny', 'sr3_uncond'])
def test_config_key_and_set_restore(name):
    from sr3_hip.x0_rules import RULES, gray_weights
    m, netG, opt = _netG(name)
    assert netG.restore is None and [r.name for r in RULES] == ['consistency', 'guidance', 'backprojection', 'restore']
    keys = set(netG.state_dict().keys())
    val = opt['model']['beta_schedule']['val']
    val['restore'] = {'operator': 'mask', 'strength': 0.5}
    m.set_new_noise_schedule(val, schedule_phase='val')
    assert netG.restore == dict(operator='mask', strength=0.5, weights=None, pinv=None, travel=None) and netG._loop_cache == {}
    assert set(netG.state_dict().keys()) == keys
    m.set_new_noise_schedule(opt['model']['beta_schedule']['train'], schedule_phase='train')      # the other phase has no key
    assert netG.restore is None
    val['restore'] = {'operator': 'gray', 'weights': 'rec601', 'travel': {'length': 2, 'repeats': 3}}
    m.set_new_noise_schedule(val, schedule_phase='val')
    a, p = gray_weights('rec601', 3)
    assert netG.restore == dict(operator='gray', strength=1.0, weights=tuple(float(v) for v in a), pinv=tuple(float(v) for v in p),
                                travel=(2, 3))
    assert np.array_equal(a, np.asarray([0.299, 0.587, 0.114], dtype=F))
    a64 = a.astype(np.float64)
    assert np.array_equal(p, (a64 / (a64 ** 2).sum()).astype(F))
    m.set_new_noise_schedule(opt['model']['beta_schedule']['train'], schedule_phase='train')
    val['restore'] = None                                                  # "restore": null
    m.set_new_noise_schedule(val, schedule_phase='val')
    assert netG.restore is None
    for bad, word in (({'strength': 0.5}, '"operator" is required'), ({'operator': 'blur'}, 'operator must be one of'),
                      ({'operator': 3}, 'operator must be one of'), ({'operator': 'mask', 'power': 2}, 'unknown key'),
                      ({'operator': 'mask', 'strength': 0}, 'strength must lie in'), ({'operator': 'mask', 'strength': 1.01}, 'strength must lie in'),
                      ({'operator': 'gray', 'strength': float('nan')}, 'strength must lie in'),
                      ({'operator': 'gray', 'strength': 'strong'}, 'strength must be a number'),
                      ({'operator': 'mask', 'strength': True}, 'strength must lie in'),
                      ({'operator': 'mask', 'weights': 'rec601'}, 'the operator is \'mask\''),
                      ({'operator': 'gray', 'weights': 'luma'}, 'weights must be'), ({'operator': 'gray', 'weights': [1, 2]}, '2 weights for 3 channels'),
                      ({'operator': 'gray', 'weights': [0, 0, 0]}, 'not all be zero'), ({'operator': 'gray', 'weights': [1, 'x', 2]}, 'must be a number'),
                      ({'operator': 'gray', 'weights': [1, float('inf'), 2]}, 'be finite'), ({'operator': 'gray', 'weights': 7}, 'weights must be'),
                      ({'operator': 'mask', 'travel': 3}, 'travel: a dict'), ({'operator': 'mask', 'travel': {'jump': 3}}, 'travel: a dict'),
                      ({'operator': 'mask', 'travel': {'length': 0, 'repeats': 2}}, 'travel length'),
                      ({'operator': 'mask', 'travel': {'length': 2.5, 'repeats': 2}}, 'travel length'),
                      ({'operator': 'mask', 'travel': {'length': 2, 'repeats': 0}}, 'travel repeats'),
                      ({'operator': 'mask', 'travel': {'length': 2, 'repeats': 65}}, 'travel repeats'), ('mask', 'a dict of')):
        with pytest.raises(ValueError, match=re.escape(word)):
            netG.set_new_noise_schedule(dict(SCHEDS[name], restore=bad), torch.device('cpu'))
        assert netG.restore is None
    # programmatic form; repeats 1 is the plain walk
    netG._loop_cache['stale'] = object()
    netG.set_restore('mask', 0.25, travel={'length': 4, 'repeats': 1})
    assert netG.restore == dict(operator='mask', strength=0.25, weights=None, pinv=None, travel=None) and netG._loop_cache == {}
    with pytest.raises(ValueError):
        netG.set_restore('gray', 2.0)
    assert netG.restore['operator'] == 'mask'
    netG._loop_cache['stale'] = object()
    netG.set_restore(None)
    assert netG.restore is None and netG._loop_cache == {}
    with pytest.raises(ValueError, match='restore is off'):
        netG.p_sample_loop(torch.zeros(1, 3, 16, 16) if netG.conditional else (1, 3, 16, 16), restore_target=torch.zeros(1, 1, 16, 16))


def test_restore_excludes_tiling_and_the_other_rules():
    _, netG, _ = _netG('sr3_tiny')
    s = SCHEDS['sr3_tiny']
    with pytest.raises(NotImplementedError, match='restore with tiling: sr3_tiled_step owns the tail'):
        netG.set_new_noise_schedule(dict(s, tiling={'tile': 16, 'overlap': 4}, restore={'operator': 'mask'}), torch.device('cpu'))
    netG.set_new_noise_schedule(dict(s), torch.device('cpu'))
    netG.set_tiling(16, 4)
    with pytest.raises(NotImplementedError, match='restore with tiling'):
        netG.set_restore('gray')
    assert netG.restore is None
    netG.set_tiling(None)
    netG.set_restore('gray')
    with pytest.raises(NotImplementedError, match='restore with tiling'):
        netG.set_tiling(16, 4)
    with pytest.raises(NotImplementedError, match='restore with tiling'):      # the explicit tiled loop, whatever set_tiling says
        netG.p_sample_loop_tiled(torch.zeros(1, 3, 32, 32), tile=16, overlap=4)
    for setter, args, noun, entry in (('set_consistency', (4,), 'consistency', 'sr3_consistent_step'),
                                      ('set_guidance', (1.5,), 'guidance', 'sr3_guided_step'),
                                      ('set_backprojection', (4,), 'back-projection', 'sr3_backproject_step')):
        with pytest.raises(NotImplementedError, match='restore with %s: sr3_restore_step and %s each own the whole tail' % (noun, entry)):
            getattr(netG, setter)(*args)
        netG.set_restore(None)
        getattr(netG, setter)(*args)
        with pytest.raises(NotImplementedError, match='restore with %s' % noun):
            netG.set_restore('mask')
        assert netG.restore is None
        getattr(netG, setter)(None)
        netG.set_restore('gray')
    # mask and gray together: one key, one operator
    assert netG.restore['operator'] == 'gray'


def test_restore_new_refusals():
    from sr3_hip import lib as L
    _, netG, _ = _netG('sr3_tiny')
    s = SCHEDS['sr3_tiny']
    # travel under the multistep solver, in both orders; without travel the two go together
    netG.set_restore('mask', travel={'length': 2, 'repeats': 2})
    with pytest.raises(NotImplementedError, match='travel under dpmpp_2m.*stale'):
        netG.set_sampler(4, kind='dpmpp_2m')
    assert netG.sampler is None
    netG.set_sampler(4, 0.0)
    assert netG.sampler['type'] == 'ddim'
    netG.set_restore(None)
    netG.set_sampler(4, kind='dpmpp_2m')
    with pytest.raises(NotImplementedError, match='travel under dpmpp_2m'):
        netG.set_restore('mask', travel={'length': 2, 'repeats': 2})
    netG.set_restore('mask')
    assert netG.restore is not None and netG.sampler['type'] == 'dpmpp_2m'
    with pytest.raises(NotImplementedError, match='travel under dpmpp_2m'):
        netG.set_new_noise_schedule(dict(s, sampler={'type': 'dpmpp_2m', 'steps': 4},
                                         restore={'operator': 'gray', 'travel': {'length': 2, 'repeats': 2}}), torch.device('cpu'))
    # noise_seq with travel: an index is visited more than once
    netG.set_new_noise_schedule(dict(s, restore={'operator': 'gray', 'travel': {'length': 2, 'repeats': 2}}), torch.device('cpu'))
    with pytest.raises(L.Sr3Error, match='noise_seq with restore travel.*item_seeds'):
        netG.p_sample_loop(torch.zeros(1, 3, 16, 16), noise_seq=torch.zeros(8, 1, 3, 16, 16))
    # the mask operator has no default target, and says so; the gray operator takes the conditioning image's (then: no GPU here)
    netG.set_restore('mask')
    with pytest.raises(NotImplementedError, match=r'restore_target=\(known, mask\).*no default'):
        netG.p_sample_loop(torch.zeros(1, 3, 16, 16))
    netG.set_restore('gray')
    with pytest.raises(L.Sr3Error, match='needs the model on a GPU'):
        netG.p_sample_loop(torch.zeros(1, 3, 16, 16))
    # self-conditioning (a 9-channel network), in both orders
    import model as Model
    opt = opt_for('sr3_tiny', gpu=False)
    opt['model']['unet']['in_channel'] = 9
    n9 = Model.create_model(opt).netG
    n9.set_self_condition(0.5)
    with pytest.raises(NotImplementedError, match='restore with self-conditioning'):
        n9.set_restore('mask')
    n9.set_self_condition(None)
    n9.set_restore('mask')
    with pytest.raises(NotImplementedError, match='restore with self-conditioning'):
        n9.set_self_condition(0.5)
    # the learned-variance tail
    opt = opt_for('sr3_tiny', gpu=False)
    opt['model']['unet']['out_channel'] = 6
    opt['model']['diffusion']['learned_variance'] = {'lambda': 0.001}
    nv = Model.create_model(opt).netG
    nv.set_new_noise_schedule(dict(s), torch.device('cpu'))
    assert nv.sampler['type'] == 'ancestral'
    with pytest.raises(NotImplementedError, match='learned-variance ancestral sampler with restore'):
        nv.set_restore('gray')
    nv.set_sampler(4, 0.0)                       # on the prediction rows with the table sigma it runs
    nv.set_restore('gray')
    with pytest.raises(NotImplementedError, match='learned-variance ancestral sampler with restore'):
        nv.set_sampler(4, kind='ancestral')


def test_ddpm_under_a_sampler_takes_restore_and_still_refuses_consistency():
    _, netG, _ = _netG('ddpm_tiny')
    s = SCHEDS['ddpm_tiny']
    netG.set_new_noise_schedule(dict(s, sampler={'type': 'ddim', 'steps': 3}, restore={'operator': 'mask'}), torch.device('cpu'))
    assert netG.sampler['steps'] == 3 and netG.restore['operator'] == 'mask'
    netG.set_restore('gray', travel={'length': 1, 'repeats': 2})
    netG.set_sampler(3, 1.0)
    assert netG.restore['travel'] == (1, 2)
    with pytest.raises(NotImplementedError, match='consistency of the DDPM variant under a sampler.*t_map'):
        netG.set_consistency(4)
    netG.set_restore(None)
    with pytest.raises(NotImplementedError, match='t_map'):
        netG.set_consistency(4)
    assert netG.consistency is None
    with pytest.raises(NotImplementedError, match='t_map'):
        netG.set_new_noise_schedule(dict(s, sampler={'type': 'ddim', 'steps': 3}, consistency={'block': 4}), torch.device('cpu'))
    # an unconditional model has no conditioning image to take the gray from
    netG.set_new_noise_schedule(dict(s, restore={'operator': 'gray'}), torch.device('cpu'))
    with pytest.raises(NotImplementedError, match='restore on an unconditional model needs restore_target='):
        netG.sample(1)


def test_model_reads_the_batch_targets():
    """DDPM.test() / DDPM.sample() hand data['known'] + data['mask'] (mask) or data['gray'] (gray) on as restore_target"""
    m, netG, _ = _netG('sr3_tiny')
    known, mask, gray = torch.zeros(1, 3, 16, 16), torch.ones(1, 1, 16, 16), torch.zeros(1, 1, 16, 16)
    m.feed_data({'HR': known, 'SR': known, 'known': known, 'mask': mask, 'gray': gray})
    assert m._restore_target() is None                      # the key is off
    netG.set_restore('mask')
    got = m._restore_target()
    assert got[0].shape == known.shape and got[1].shape == mask.shape
    netG.set_restore('gray')
    assert m._restore_target().shape == gray.shape
    seen = {}
    netG.super_resolution = lambda x, continous=False, **kw: seen.update(kw) or x
    m.test()
    assert seen['restore_target'].shape == gray.shape
    m.feed_data({'HR': known, 'SR': known})
    assert m._restore_target() is None                      # the gray operator's default; the mask operator then says what it needs
    netG.set_restore('mask')
    assert m._restore_target() is None


def test_loop_state_key_is_unchanged_without_restore():
    """the key of a state without the rule is what it was: the rule's component is appended, and only where the rule is on"""
    _, netG, _ = _netG('sr3_tiny')
    keys = []
    netG._cached = lambda key, new=None: keys.append(key) or (new if new is not None else {})
    netG.denoise_fn.weights = lambda: torch.zeros(1)
    shape = (1, 3, 16, 16)
    netG._loop_state(shape, shape, torch.device('cpu'))
    assert len(keys[0]) == 13 and keys[0][-4:] == (None, None, None, None)      # back-projection, guidance, consistency, tiles
    netG.set_restore('mask', 0.5)
    keys.clear()
    netG._loop_state(shape, shape, torch.device('cpu'), restore=netG.restore)
    assert keys[0][:13][-4:] == (None, None, None, None) and keys[0][13:] == (('restore', 'mask', 0.5, None, None),)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------

def test_symbols_are_exported_and_declared():
    from sr3_hip import lib as L
    lib = L.load()
    src = open(ROOT + '/include/sr3_mi355x.h').read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name, nargs in (('sr3_restore_step', 24), ('sr3_travel_back_f32', 10), ('sr3_gray_f32', 8)):
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES and L.SIGNATURES[name][0] is C.c_int and len(L.SIGNATURES[name][1]) == nargs
        decl = re.search(name + r'\s*\((.*?)\)\s*;', src, flags=re.S)
        assert decl is not None and len(decl.group(1).split(',')) == nargs, name


def _p(k, off=0):
    """a made-up, 16-byte aligned, non-NULL address (+ off bytes): the entries below refuse before they touch memory"""
    return C.c_void_p((k << 24) + off)


IMG = 2 * 3 * 8 * 12 * 4      # bytes of the default image batch
W3 = (C.c_float * 4)(0.25, 0.5, 0.25, 0.0)
WNAN = (C.c_float * 4)(0.25, float('nan'), 0.25, 0.0)
HUGE = dict(batch=1 << 12, channels=2, height=1 << 9, width=1 << 9)      # 2^31 elements

RS_KEYS = ('x', 'eps', 'z', 'op', 'target', 'mask', 'mc', 'ga', 'gp', 'batch', 'channels', 'height', 'width', 'strength', 'ta', 'tb', 'tc1',
           'tc2', 'tsig', 'step2', 'clip', 'c3', 'hist', 'stream')


def _rs_args(**kw):
    a = dict(x=_p(1), eps=_p(2), z=None, op=0, target=_p(3), mask=_p(4), mc=1, ga=None, gp=None, batch=2, channels=3, height=8, width=12,
             strength=1.0, ta=_p(5), tb=_p(6), tc1=_p(7), tc2=_p(8), tsig=_p(9), step2=_p(10), clip=1, c3=None, hist=None, stream=None)
    a.update(kw)
    return [a[k] for k in RS_KEYS]


GRAY = dict(op=1, mask=None, mc=0, ga=W3, gp=W3)

RS_REFUSALS = [
    (dict(x=None), -1, 'x_nchw'), (dict(eps=None), -1, 'eps_nchw'), (dict(target=None), -1, 'target'), (dict(ta=None), -1, 'tab_a'),
    (dict(tb=None), -1, 'tab_b'), (dict(tc1=None), -1, 'tab_c1'), (dict(tc2=None), -1, 'tab_c2'), (dict(tsig=None), -1, 'tab_sigma'),
    (dict(step2=None), -1, 'step2_dev'),
    (dict(op=2), -1, 'op must be'), (dict(op=-1), -1, 'op must be'),
    (dict(mask=None), -1, 'mask is NULL'), (dict(GRAY, ga=None), -1, 'gray_a_host'), (dict(GRAY, gp=None), -1, 'gray_p_host'),
    (dict(batch=0), -1, 'batch'), (dict(channels=-1), -1, 'channels'), (dict(height=0), -1, 'height'), (dict(width=-4), -1, 'width'),
    (dict(mc=2), -1, 'mask_channels'), (dict(mc=0), -1, 'mask_channels'), (dict(mc=4), -1, 'mask_channels'),
    (dict(GRAY, channels=5), -1, 'at most 4 channels'),
    (dict(HUGE), -2, '2^31'), (dict(GRAY, **HUGE), -2, '2^31'),
    (dict(strength=float('nan')), -1, 'strength'), (dict(strength=0.0), -1, 'strength'), (dict(strength=-0.5), -1, 'strength'),
    (dict(strength=1.5), -1, 'strength'), (dict(GRAY, strength=float('inf')), -1, 'strength'),
    (dict(c3=_p(11)), -1, 'c3'), (dict(hist=_p(12)), -1, 'c3'),
    (dict(c3=_p(11), hist=_p(1)), -1, 'history overlaps'), (dict(c3=_p(11), hist=_p(2)), -1, 'history overlaps'),
    (dict(c3=_p(11), hist=_p(1, IMG - 4)), -1, 'history overlaps'),
    (dict(target=_p(1)), -1, 'x_nchw overlaps target'), (dict(target=_p(1, IMG - 4)), -1, 'x_nchw overlaps target'),
    (dict(GRAY, target=_p(1, IMG // 3)), -1, 'x_nchw overlaps target'),
    (dict(mask=_p(1, -4)), -1, 'x_nchw overlaps mask'), (dict(mc=3, mask=_p(1, -IMG + 4)), -1, 'x_nchw overlaps mask'),
    (dict(z=_p(1)), -1, 'x_nchw overlaps z_nchw'), (dict(eps=_p(1, 16)), -1, 'x_nchw overlaps eps_nchw'),
    (dict(step2=_p(1, 4)), -1, 'x_nchw overlaps step2_dev'), (dict(step2=_p(3, 4)), -1, 'step2_dev overlaps target'),
    (dict(ta=_p(1, 8)), -1, 'x_nchw overlaps tab_a'), (dict(tsig=_p(10, 4)), -1, 'step2_dev overlaps tab_sigma'),
    (dict(c3=_p(11), hist=_p(3)), -1, 'hist_nchw overlaps target'), (dict(c3=_p(11), hist=_p(12), mask=_p(12, IMG - 4)), -1, 'hist_nchw overlaps mask'),
    (dict(c3=_p(10), hist=_p(12)), -1, 'step2_dev overlaps tab_c3'),
    (dict(GRAY, ga=WNAN), -1, 'not finite'), (dict(GRAY, gp=WNAN), -1, 'not finite'),
    # two faults at once: the one reported is the one the checks meet first
    (dict(x=None, op=7), -1, 'x_nchw'), (dict(op=7, batch=0), -1, 'op must be'), (dict(mask=None, batch=0), -1, 'mask is NULL'),
    (dict(batch=0, mc=2), -1, 'batch'), (dict(HUGE, mc=4), -1, 'mask_channels'), (dict(HUGE, strength=0.0), -2, '2^31'),
    (dict(strength=0.0, c3=_p(11)), -1, 'strength'), (dict(c3=_p(11), target=_p(1)), -1, 'c3'), (dict(GRAY, ga=WNAN, target=_p(1)), -1, 'overlaps'),
]

TB_KEYS = ('x', 'z', 'ra', 'rs', 'to', 'rows', 'step2', 'batch', 'per', 'stream')


def _tb_args(**kw):
    a = dict(x=_p(1), z=_p(2), ra=_p(3), rs=_p(4), to=_p(5), rows=8, step2=_p(6), batch=2, per=288, stream=None)
    a.update(kw)
    return [a[k] for k in TB_KEYS]


TB_REFUSALS = [
    (dict(x=None), -1, 'x is NULL'), (dict(z=None), -1, 'z is NULL'), (dict(ra=None), -1, 'tab_ra'), (dict(rs=None), -1, 'tab_rs'),
    (dict(to=None), -1, 'tab_to'), (dict(step2=None), -1, 'step2_dev'),
    (dict(rows=0), -1, 'rows'), (dict(batch=0), -1, 'batch'), (dict(per=-1), -1, 'elems_per_image'),
    (dict(batch=1 << 12, per=1 << 19), -2, '2^31'),
    (dict(z=_p(1)), -1, 'x overlaps z'), (dict(z=_p(1, 2 * 288 * 4 - 4)), -1, 'x overlaps z'), (dict(ra=_p(1, 16)), -1, 'x overlaps tab_ra'),
    (dict(rs=_p(1, -4)), -1, 'x overlaps tab_rs'), (dict(to=_p(1, -28)), -1, 'x overlaps tab_to'), (dict(step2=_p(1)), -1, 'x overlaps step2_dev'),
    (dict(step2=_p(2, 4)), -1, 'step2_dev overlaps z'), (dict(step2=_p(5, 28)), -1, 'step2_dev overlaps tab_to'),
    (dict(x=None, rows=0), -1, 'x is NULL'), (dict(rows=0, z=_p(1)), -1, 'rows'),
]

G_KEYS = ('src', 'batch', 'channels', 'height', 'width', 'ga', 'dst', 'stream')


def _g_args(**kw):
    a = dict(src=_p(1), batch=2, channels=3, height=8, width=12, ga=W3, dst=_p(2), stream=None)
    a.update(kw)
    return [a[k] for k in G_KEYS]


G_REFUSALS = [
    (dict(src=None), -1, 'src_nchw'), (dict(ga=None), -1, 'gray_a_host'), (dict(dst=None), -1, 'dst_nchw'),
    (dict(batch=0), -1, 'batch'), (dict(width=0), -1, 'width'), (dict(channels=5), -1, 'at most 4 channels'), (dict(HUGE), -2, '2^31'),
    (dict(dst=_p(1)), -1, 'dst_nchw overlaps src_nchw'), (dict(dst=_p(1, IMG - 4)), -1, 'dst_nchw overlaps src_nchw'),
    (dict(dst=_p(1, -4)), -1, 'dst_nchw overlaps src_nchw'), (dict(ga=WNAN), -1, 'not finite'),
]

ENTRIES = {
    'RS_REFUSALS': ('sr3_restore_step', 'restore_step', _rs_args, RS_REFUSALS),
    'TB_REFUSALS': ('sr3_travel_back_f32', 'travel_back', _tb_args, TB_REFUSALS),
    'G_REFUSALS': ('sr3_gray_f32', 'gray', _g_args, G_REFUSALS),
}
CASES = [(t, i) for t in ENTRIES for i in range(len(ENTRIES[t][3]))]


def _call(lib, table, case):
    entry, _, build, rows = ENTRIES[table]
    rc = getattr(lib, entry)(*build(**rows[case][0]))
    return [int(rc), lib.sr3_last_error().decode()]


@pytest.fixture(scope='module')
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_every_case(recorded):
    assert sorted(recorded) == sorted('%s[%d]' % c for c in CASES)


@pytest.mark.parametrize('table,case', CASES, ids=['%s-%d' % c for c in CASES])
def test_entry_refusals_no_gpu(recorded, table, case):
    """every refusal returns its code, is prefixed with the entry's name and names the argument, before any launch (no device is
    present here); code and text are the recorded ones"""
    from sr3_hip import lib as L
    _, who, _, rows = ENTRIES[table]
    kw, code, word = rows[case]
    got = _call(L.load(), table, case)
    assert got[0] == code and got[1].startswith(who + ': ') and word in got[1], (kw, got)
    assert got == recorded['%s[%d]' % (table, case)], (table, case)


if __name__ == '__main__':
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    sys.path[:0] = [root, os.path.join(root, 'image-super-resolution-via-iterative-refinement_amd'), here]
    from sr3_hip import lib as L
    lib = L.load()
    out = {'%s[%d]' % c: _call(lib, *c) for c in CASES}
    bad = [k for k, v in out.items() if v[0] >= 0]
    assert not bad, 'not refused (a launch was attempted): %s' % bad
    with open(FIXTURE, 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write('\n')
    print('recorded %d refusals from %s' % (len(out), L.LIB_PATH))
