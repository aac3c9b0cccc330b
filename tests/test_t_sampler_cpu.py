"""The loss-aware timestep sampler and the surface of calc_bpd_loop without a GPU: the resampler against its restatement, the config
key and its refusals, that a model without the key draws exactly what it drew, that one with it hands the training step the restated
draw and weight, the checkpoint round trip of the history, and calc_bpd_loop's refusals before anything is launched."""
import copy
import os

import numpy as np
import pytest
import torch

from helpers import opt_for
from test_learned_var_cpu import lv_opt
import vlb_eval_ref as V

from sr3_hip import t_sampler as TS


# ---- the resampler ----------------------------------------------------------------------------------------------------------------------

def _fill(rs, ref, T, rounds, seed=0, skip=None):
    rng = np.random.RandomState(seed)
    for r in range(rounds):
        t = np.array([k for k in range(T) if not (skip is not None and k == skip and r == rounds - 1)])
        losses = rng.rand(t.shape[0]) * (1.0 + t)
        rs.update(t, losses)
        ref.update(t, losses)


def test_uniform_until_every_step_has_its_history():
    T, H = 7, 3
    rs, ref = TS.LossSecondMomentResampler(T, H, 0.01), V.Resampler(T, H, 0.01)
    _fill(rs, ref, T, H, skip=4)                 # step 4 is one entry short
    assert not rs.warmed_up()
    np.testing.assert_array_equal(rs.probabilities(), np.full(T, 1.0 / T))
    np.testing.assert_array_equal(rs.weights(np.arange(T)), np.ones(T))
    rs.update([4], [2.5])
    ref.update([4], [2.5])
    assert rs.warmed_up()
    p = rs.probabilities()
    np.testing.assert_allclose(p, ref.probabilities(), rtol=1e-12)
    assert p.max() > 1.5 / T                    # (no longer uniform: the losses grow with t)


def test_ring_overwrites_the_oldest_entry():
    T, H = 3, 2
    rs, ref = TS.LossSecondMomentResampler(T, H, 0.0), V.Resampler(T, H, 0.0)
    seq = [(0, 1.0), (1, 1.0), (2, 1.0), (0, 2.0), (1, 1.0), (2, 1.0), (0, 4.0), (0, 8.0), (2, 3.0)]
    for t, v in seq:
        rs.update([t], [v])
        ref.update([t], [v])
    assert rs.counts.tolist() == [4, 2, 3]
    assert sorted(rs.losses[0].tolist()) == [4.0, 8.0] and sorted(rs.losses[2].tolist()) == [1.0, 3.0]
    w = np.sqrt(np.array([(16.0 + 64.0) / 2, 1.0, (1.0 + 9.0) / 2]))
    np.testing.assert_allclose(rs.probabilities(), w / w.sum(), rtol=1e-12)
    np.testing.assert_allclose(rs.probabilities(), ref.probabilities(), rtol=1e-12)
    rs.update([1], [float('nan')])              # a non-finite loss does not enter the history
    assert rs.counts.tolist() == [4, 2, 3]


@pytest.mark.parametrize('u', [0.0, 0.001, 0.5, 1.0])
def test_uniform_mix_sums_to_one_and_weights_average_to_one(u):
    T, H = 11, 4
    rs, ref = TS.LossSecondMomentResampler(T, H, u), V.Resampler(T, H, u)
    _fill(rs, ref, T, H + 2, seed=5)
    p = rs.probabilities()
    np.testing.assert_allclose(p, ref.probabilities(), rtol=1e-12)
    assert abs(p.sum() - 1.0) <= 1e-14 and p.min() >= u / T - 1e-15
    if u == 1.0:
        np.testing.assert_allclose(p, np.full(T, 1.0 / T), rtol=1e-12)
    w = rs.weights(np.arange(T))
    np.testing.assert_allclose(w, ref.weights(np.arange(T)), rtol=1e-12)
    assert abs(float((p * w).sum()) - 1.0) <= 1e-13                 # E_p[1 / (T p)] = 1: the objective's expectation is kept


def test_state_round_trip_and_shape_check():
    rs = TS.LossSecondMomentResampler(5, 3, 0.01)
    _fill(rs, V.Resampler(5, 3, 0.01), 5, 4, seed=2)
    other = TS.LossSecondMomentResampler(5, 3, 0.01)
    other.load_state_dict(copy.deepcopy(rs.state_dict()))
    np.testing.assert_array_equal(other.probabilities(), rs.probabilities())
    assert other.counts.tolist() == rs.counts.tolist()
    with pytest.raises(ValueError, match='does not fit'):
        TS.LossSecondMomentResampler(6, 3).load_state_dict(rs.state_dict())


# ---- the key ----------------------------------------------------------------------------------------------------------------------------

def test_parse_t_sampler():
    assert TS.parse_t_sampler(None) is None and TS.parse_t_sampler(False) is None
    assert TS.parse_t_sampler({'type': 'loss_second_moment'}) == dict(type='loss_second_moment', history=10, uniform=0.001)
    assert TS.parse_t_sampler({'type': 'loss_second_moment', 'history': 4, 'uniform': 0}) == dict(type='loss_second_moment', history=4, uniform=0.0)
    for spec, text in ((True, 'a dict'), ({'typ': 'x'}, "unknown key 'typ'"), ({'type': 'importance'}, "unknown type 'importance'"),
                       ({'history': 0}, 'history must be an integer >= 1'), ({'history': 2.5}, 'history must be'), ({'history': True}, 'history must be'),
                       ({'uniform': -0.1}, 'uniform must be a number in'), ({'uniform': 1.5}, 'uniform must be'), ({'uniform': 'a'}, 'uniform must be')):
        with pytest.raises(ValueError, match=text):
            TS.parse_t_sampler(spec)


def _build(opt):
    import model as Model
    return Model.create_model(copy.deepcopy(opt))


def _ts_opt(name, phase='train', learned=False, key=True, **kw):
    if learned:
        opt = lv_opt(name)
        opt['phase'] = phase
    else:
        opt = opt_for(name, phase=phase, gpu=False)
    if key:
        opt['model']['diffusion']['t_sampler'] = dict({'type': 'loss_second_moment', 'history': 2, 'uniform': 0.01}, **kw)
    return opt


def test_plain_sr3_is_refused_and_says_why():
    with pytest.raises(ValueError, match='x_t between two grid levels has no posterior'):
        _build(_ts_opt('sr3_tiny'))
    m = _build(_ts_opt('sr3_tiny', key=False))
    assert m.netG.t_sampler is None
    with pytest.raises(ValueError, match='plain SR3 model'):
        m.netG.set_t_sampler('loss_second_moment')
    with pytest.raises(ValueError, match="unknown key 'decay'"):
        _build(_ts_opt('ddpm_tiny', decay=0.9))


def test_key_builds_the_sampler_per_schedule():
    for name, learned in (('ddpm_tiny', False), ('sr3_tiny', True)):
        m = _build(_ts_opt(name, learned=learned))
        ts = m.netG.t_sampler
        assert isinstance(ts, TS.LossSecondMomentResampler) and (ts.T, ts.history, ts.uniform) == (m.netG.num_timesteps, 2, 0.01)
        ts.update([0], [1.0])
        m.netG.set_new_noise_schedule(m.opt['model']['beta_schedule']['train'], torch.device('cpu'))
        assert m.netG.t_sampler is ts                      # the same schedule length: the same history
        m.netG.set_t_sampler(None)
        assert m.netG.t_sampler is None
    with pytest.raises(ValueError, match='needs learned_variance'):
        _build(_ts_opt('sr3_tiny', learned=True)).netG.set_learned_variance(None)


# ---- off means off; on means the restated draw --------------------------------------------------------------------------------------------

def _stub(netG, seen):
    def train_step(hr, cond, z, ca, cb, level, tstep, **kw):
        seen.append(dict(kw, z=z, level=level, tstep=tstep))
        netG.denoise_fn.last_vlb = torch.tensor(0.0)
        netG.denoise_fn.last_per_image = torch.arange(2.0 * hr.shape[0]).reshape(hr.shape[0], 2) + 1.0
        return torch.tensor(0.0)
    netG.denoise_fn.train_step = train_step


DATA = {'HR': torch.zeros(3, 3, 16, 16), 'SR': torch.ones(3, 3, 16, 16)}


def test_without_the_key_the_draws_are_unchanged():
    # SR3 under learned_variance: one randint on the grid, then z
    netG = _build(_ts_opt('sr3_tiny', learned=True, key=False)).netG
    seen = []
    _stub(netG, seen)
    np.random.seed(11)
    torch.manual_seed(12)
    netG.p_losses(DATA)
    after = (np.random.get_state()[1].copy(), torch.get_rng_state().clone())
    np.random.seed(11)
    torch.manual_seed(12)
    tt = np.random.randint(1, netG.num_timesteps + 1)
    z = torch.randn_like(DATA['HR'])
    assert torch.equal(seen[0]['z'], z) and torch.equal(seen[0]['level'], torch.FloatTensor(np.full(3, netG.sqrt_alphas_cumprod_prev[tt])))
    assert np.array_equal(np.random.get_state()[1], after[0]) and torch.equal(torch.get_rng_state(), after[1])
    assert set(seen[0]) == {'z', 'level', 'tstep', 'grad_scale', 'drop_seed', 'objective', 'hybrid'} and seen[0]['objective'] is None
    # DDPM: randint per image, then z; the plain step's keywords
    netG = _build(_ts_opt('ddpm_tiny', key=False)).netG
    seen = []
    _stub(netG, seen)
    torch.manual_seed(13)
    netG.p_losses(DATA)
    after = torch.get_rng_state().clone()
    torch.manual_seed(13)
    t = torch.randint(0, netG.num_timesteps, (3,)).long()
    z = torch.randn_like(DATA['HR'])
    assert torch.equal(seen[0]['tstep'], t) and torch.equal(seen[0]['z'], z) and torch.equal(torch.get_rng_state(), after)
    assert set(seen[0]) == {'z', 'level', 'tstep', 'grad_scale', 'drop_seed', 'objective'} and seen[0]['objective'] is None


def _warm(ts, seed=4):
    rng = np.random.RandomState(seed)
    for _ in range(ts.history):
        ts.update(np.arange(ts.T), rng.rand(ts.T) * (1.0 + np.arange(ts.T)))
    assert ts.warmed_up()


def test_with_the_key_sr3_draws_one_step_from_p_and_weights_it():
    netG = _build(_ts_opt('sr3_tiny', learned=True)).netG
    ts, T = netG.t_sampler, netG.num_timesteps
    _warm(ts)
    ref = V.Resampler(T, ts.history, ts.uniform)
    for k in range(ts.history):
        ref.update(np.arange(T), ts.losses[:, k])
    seen = []
    _stub(netG, seen)
    np.random.seed(21)
    torch.manual_seed(22)
    netG.p_losses(DATA)
    np.random.seed(21)
    torch.manual_seed(22)
    p = ref.probabilities()
    j = int(np.random.choice(T, p=p))
    z = torch.randn_like(DATA['HR'])
    kw = seen[0]
    assert torch.equal(kw['z'], z) and torch.equal(kw['level'], torch.FloatTensor(np.full(3, netG.sqrt_alphas_cumprod_prev[j + 1])))
    tgt_z, tgt_x0, weight, kind, delta = kw['objective']
    assert tgt_z.tolist() == [1.0] * 3 and tgt_x0.tolist() == [0.0] * 3 and kind == -1
    np.testing.assert_array_equal(weight.numpy(), np.full(3, 1.0 / (T * p[j])).astype(np.float32))
    assert kw['per_image'] is kw['hybrid'][0] and tuple(kw['per_image'].shape) == (3, 8)
    assert torch.equal(kw['vlb_weight'], weight)                    # L_vlb is weighted too: `weight` reaches L_simple alone
    # the step's terms enter the history of the drawn step on the next flush, in order
    before = ts.counts.copy()
    netG.flush_t_sampler()
    assert (ts.counts - before).tolist() == [3 if k == j else 0 for k in range(T)]
    assert sorted(ts.losses[j].tolist()) == sorted([1.0, 3.0, 5.0][-ts.history:])
    netG.flush_t_sampler()                                          # (nothing pending: a no-op)
    assert (ts.counts - before).sum() == 3


def test_with_the_key_ddpm_draws_per_image_from_p_and_weights_them():
    netG = _build(_ts_opt('ddpm_tiny')).netG
    ts, T = netG.t_sampler, netG.num_timesteps
    seen = []
    _stub(netG, seen)
    torch.manual_seed(31)
    netG.p_losses(DATA)                                             # not warmed up: uniform p, weight 1
    torch.manual_seed(31)
    t = torch.multinomial(torch.full((T,), 1.0 / T, dtype=torch.float64), 3, replacement=True)
    z = torch.randn_like(DATA['HR'])
    assert torch.equal(seen[0]['tstep'], t) and torch.equal(seen[0]['z'], z)
    assert seen[0]['objective'][2].tolist() == [1.0] * 3 and 'hybrid' not in seen[0] and tuple(seen[0]['per_image'].shape) == (3, 8)
    netG.flush_t_sampler()
    _warm(ts)
    p = ts.probabilities()
    torch.manual_seed(32)
    netG.p_losses(DATA)
    torch.manual_seed(32)
    t = torch.multinomial(torch.tensor(p, dtype=torch.float64), 3, replacement=True)
    assert torch.equal(seen[1]['tstep'], t)
    np.testing.assert_array_equal(seen[1]['objective'][2].numpy(), (1.0 / (T * p)).astype(np.float32)[t.numpy()])
    rows = netG._hyb_table[t]
    assert torch.equal(seen[1]['per_image'], rows) and 'vlb_weight' not in seen[1]      # (no variance head: no L_vlb to weight)
    # with a variance head the per-image weights go into L_vlb's table as well
    netG = _build(_ts_opt('ddpm_tiny', learned=True)).netG
    _warm(netG.t_sampler)
    p = netG.t_sampler.probabilities()
    seen = []
    _stub(netG, seen)
    torch.manual_seed(33)
    netG.p_losses(DATA)
    want = torch.tensor((1.0 / (T * p)).astype(np.float32))[seen[0]['tstep']]
    assert torch.equal(seen[0]['vlb_weight'], want) and torch.equal(seen[0]['objective'][2], want) and len(set(want.tolist())) > 1


def test_weight_multiplies_an_objective_that_has_one():
    opt = _ts_opt('ddpm_tiny')
    opt['model']['diffusion']['prediction'] = 'v'
    netG = _build(opt).netG
    _warm(netG.t_sampler)
    seen = []
    _stub(netG, seen)
    torch.manual_seed(5)
    netG.p_losses(DATA)
    p = netG.t_sampler.probabilities()
    t = seen[0]['tstep']
    plain = netG._train_objective(t, None, torch.device('cpu'))
    tgt_z, tgt_x0, weight, _, _ = seen[0]['objective']
    assert torch.equal(tgt_z, plain[0]) and torch.equal(tgt_x0, plain[1])
    assert torch.equal(weight, plain[2] * torch.tensor((1.0 / (netG.num_timesteps * p)).astype(np.float32))[t])


# ---- the checkpoint ---------------------------------------------------------------------------------------------------------------------

class _Opt:
    def state_dict(self):
        return {'step': 3}

    def load_state_dict(self, sd):
        self.loaded = sd


@pytest.mark.parametrize('key', [True, False])
def test_opt_pth_round_trip(tmp_path, key):
    opt = _ts_opt('ddpm_tiny', key=key)
    opt['path']['checkpoint'] = str(tmp_path)
    m = _build(opt)
    m.optG = _Opt()
    if key:
        _warm(m.netG.t_sampler)
        m.netG.t_sampler.update([1], [9.0])
    m.save_network(2, 7)
    ck = torch.load(os.path.join(str(tmp_path), 'I7_E2_opt.pth'), map_location='cpu', weights_only=False)
    if not key:
        assert set(ck) == {'epoch', 'iter', 'scheduler', 'optimizer'}          # the checkpoint keys of a model without the key
        return
    assert set(ck) == {'epoch', 'iter', 'scheduler', 'optimizer', 't_sampler'}
    assert all(torch.is_tensor(v) or isinstance(v, (int, float, str)) for v in ck['t_sampler'].values())      # (loads under weights_only)
    m2 = _build(opt)
    m2.optG = _Opt()
    m2.opt['path']['resume_state'] = os.path.join(str(tmp_path), 'I7_E2')
    m2.load_network()
    ts, ts2 = m.netG.t_sampler, m2.netG.t_sampler
    np.testing.assert_array_equal(ts2.losses, ts.losses)
    np.testing.assert_array_equal(ts2.counts, ts.counts)
    np.testing.assert_array_equal(ts2.probabilities(), ts.probabilities())
    assert m2.begin_step == 7 and m2.optG.loaded == {'step': 3}


# ---- calc_bpd_loop's refusals, before anything is launched -------------------------------------------------------------------------------

def test_calc_bpd_loop_refuses_self_conditioning_and_tiling_on_a_cpu_model():
    from test_selfcond_cpu import _netG
    netG = _netG()
    with pytest.raises(NotImplementedError, match='self-conditioned model'):
        netG.calc_bpd_loop({'HR': DATA['HR'], 'SR': DATA['SR']})
    netG = _build(_ts_opt('sr3_tiny', phase='val', key=False)).netG
    netG.set_tiling(16, 0)
    with pytest.raises(NotImplementedError, match='calc_bpd_loop with tiling'):
        netG.calc_bpd_loop({'HR': DATA['HR'], 'SR': DATA['SR']})
    netG.set_tiling(None)
    from sr3_hip import lib as L
    with pytest.raises(L.Sr3Error, match='needs the model on a GPU'):            # and past the refusals: no CPU fallback
        netG.calc_bpd_loop({'HR': DATA['HR'], 'SR': DATA['SR']})
    assert not any(k[0] == 'bpd' for k in netG._loop_cache)


# ---- tools/image_nll.py: the config reader and the arguments -----------------------------------------------------------------------------

def test_image_nll_reads_a_commented_config_and_its_arguments(tmp_path, monkeypatch):
    import importlib.util
    import json
    import sys
    from helpers import ROOT
    spec = importlib.util.spec_from_file_location('image_nll', os.path.join(ROOT, 'tools', 'image_nll.py'))
    tool = importlib.util.module_from_spec(spec)
    monkeypatch.setattr(sys, 'path', list(sys.path))
    spec.loader.exec_module(tool)
    opt = opt_for('sr3_tiny', phase='train', gpu=False)
    del opt['path']['resume_state']
    opt['note'] = 'http://example.org/a//b'                       # (a // inside a string is not a comment)
    cfg = tmp_path / 'c.json'
    cfg.write_text('// a comment line\n' + json.dumps(opt, indent=1).replace('"distributed": false,', '"distributed": false, // trailing'))
    got = tool.load_config(str(cfg))
    assert got['phase'] == 'val' and got['gpu_ids'] == [0] and got['path']['resume_state'] is None and got['note'] == opt['note']
    assert got['model'] == opt['model'] and got['distributed'] is False
    monkeypatch.setattr(sys, 'argv', ['image_nll.py'])
    with pytest.raises(SystemExit):                                 # -c is required
        tool.main()
