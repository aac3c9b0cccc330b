"""`EngineDiffusion._capture` leaves a state as it found it, for every step it captures (sr3_tiny shapes, 16 x 16, B = 2, T = 8; S = 4
for the evaluation step): the warm-up step runs for real, so whatever it writes that a chain reads again -- the tensors the state
declares in st['dirty'] -- and every random stream it draws from have to be put back, bit for bit; and what was captured has to be the
step: one replay equals one eager step from the same start on a second state built and filled the same way."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import opt_for             # noqa: E402
import gpu_util as G                     # noqa: E402

SEEDS = [11, 22]
FILLED = ('img', 'z', 'eps', 'cond', 'hist', 'out2', 'x_tiles', 'eps_tiles', 'ymean',      # a sampling state's data
          'x0', 'xt', 'out', 'vb', 'mse', 'prior')                                         # the evaluation state's
# form -> (unet keys, diffusion keys, what switches the form on)
FORMS = {
    'fused': ({}, {}, lambda n: None),
    'fused_dpmpp_2m': ({}, {}, lambda n: n.set_sampler(4, 0.0, kind='dpmpp_2m')),
    'tiled': ({}, {}, lambda n: n.set_tiling(8, 4)),
    'rule_tail': ({}, {}, lambda n: n.set_consistency(4)),
    'selfcond': (dict(in_channel=9), {}, lambda n: n.set_self_condition(0.5)),
    'learned_var': (dict(out_channel=6), dict(learned_variance={'lambda': 0.001}), lambda n: None),
    'bpd': (dict(out_channel=6), dict(learned_variance={'lambda': 0.001}), lambda n: None),
}


@functools.lru_cache(maxsize=None)
def _model(unet, diffusion):
    import model as Model
    opt = opt_for('sr3_tiny', phase='val', gpu=True)
    opt['model']['unet'].update(dict(unet))
    opt['model']['diffusion'].update({k: dict(v) for k, v in diffusion})
    torch.manual_seed(1234)
    netG = Model.create_model(opt).netG
    netG.show_progress = False
    return netG


def _rand(shape, seed):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * 0.5).clamp(-1, 1)


def _state(netG, form):
    """a fresh state of the form, as the loop builds it (one eager chain), taken out of the cache; filled with known values"""
    dev = G.dev()
    netG._loop_cache = {}
    netG.use_graph = False
    sr = _rand((2, 3, 16, 16), 5).to(dev)
    if form == 'bpd':
        netG.calc_bpd_loop({'HR': _rand((2, 3, 16, 16), 6).to(dev), 'SR': sr}, steps=4, item_seeds=SEEDS)
    else:
        netG.super_resolution(sr, item_seeds=SEEDS)
    (key, st), = netG._loop_cache.items()
    assert (key[0] == 'bpd') == (form == 'bpd') and st['graph'] is None and len(st['gens']) == 2
    netG._loop_cache = {}
    for i, k in enumerate(FILLED):
        if st.get(k) is not None:
            st[k].copy_(_rand(tuple(st[k].shape), 100 + i))
    if st.get('cond_tiles') is not None:      # (cut from the state's cond once per chain)
        netG._gather_tiles(st, st['cond'], st['cond_tiles'], 0, st['cond_tiles'].shape[0])
    st['step'].copy_(torch.tensor([123, 2], dtype=torch.int32))      # the next step is 2; slot 0 is the step's scratch
    for g, v in zip(st['gens'], SEEDS):
        g.manual_seed(v)
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize('form', list(FORMS))
def test_capture_leaves_the_state_clean_and_captures_the_step(form):
    dev = G.dev()
    unet, diffusion, switch = FORMS[form]
    netG = _model(tuple(sorted(unet.items())), tuple((k, tuple(sorted(v.items()))) for k, v in diffusion.items()))
    netG.set_sampler(None) if netG.learned_variance is None else netG.set_sampler(netG.num_timesteps, kind='ancestral')
    for off in (netG.set_tiling, netG.set_consistency, netG.set_self_condition):
        off(None)
    switch(netG)
    step = netG._bpd_step if form == 'bpd' else netG._one_step
    want_dirty = {'fused': ('img', 'step'), 'fused_dpmpp_2m': ('img', 'step', 'hist'), 'tiled': ('img', 'step'), 'rule_tail': ('img', 'step'),
                  'selfcond': ('img', 'step', 'cond'), 'learned_var': ('img', 'step'), 'bpd': ('step',)}[form]
    st, st2 = _state(netG, form), _state(netG, form)
    assert tuple(st['dirty']) == want_dirty and st is not st2
    before = {k: st[k].clone() for k in st['dirty']}
    torch.cuda.manual_seed(99)
    rng = torch.cuda.get_rng_state(dev)
    gstate = [g.get_state() for g in st['gens']]

    netG._capture(st) if form != 'bpd' else netG._capture(st, step)
    torch.cuda.synchronize()
    assert st['graph'] is not None
    for k, v in before.items():
        assert torch.equal(st[k], v), k
    assert torch.equal(torch.cuda.get_rng_state(dev), rng)
    assert all(torch.equal(g.get_state(), s) for g, s in zip(st['gens'], gstate))

    st['graph'].replay()
    step(st2)
    torch.cuda.synchronize()
    out = 'vb' if form == 'bpd' else 'img'
    assert torch.equal(st[out], st2[out]) and not torch.equal(st[out], _rand(tuple(st[out].shape), 100 + FILLED.index(out)).to(dev))
    assert st['step'].tolist() == st2['step'].tolist() and st['step'].tolist()[1] == 1      # (slot 0: the forms that copy the counter leave 2 there)
