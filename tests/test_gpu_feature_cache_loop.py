"""Feature-cached sampling loops (set_feature_cache / the "feature_cache" config key): two captured graphs, one schedule."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'image-super-resolution-via-iterative-refinement_amd')
for p in (ROOT, PKG, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import gpu_util as G                                            # noqa: E402
from helpers import CONDITIONAL, SCHEDS, load_golden, opt_for   # noqa: E402

pytestmark = pytest.mark.gpu


def make(name, feature_cache=None):
    import model as Model
    opt = opt_for(name, phase='val', gpu=True)
    if feature_cache is not None:
        opt['model']['beta_schedule']['val']['feature_cache'] = feature_cache
    m = Model.create_model(opt)
    g, sd = load_golden(name)
    m.netG.load_state_dict(sd, strict=True)
    m.set_new_noise_schedule(opt['model']['beta_schedule']['val'], schedule_phase='val')
    m.netG.show_progress = False
    return m, g


def chain_input(name, g):
    d = G.dev()
    x_T = torch.from_numpy(g['loop/x_T']).to(d)
    return (torch.from_numpy(g['loop/sr']).to(d) if CONDITIONAL[name] else tuple(x_T.shape)), x_T


def run(netG, arg, x_T, seed=41):
    """the whole batch at the end of one chain (p_sample_loop itself returns the last image alone for a conditional model)"""
    torch.manual_seed(seed)
    last = netG.p_sample_loop(arg, continous=False, x_T=x_T)
    st = next(iter(netG._loop_cache.values()))
    assert len(netG._loop_cache) == 1 and torch.equal(last, st['img'] if last.dim() == 4 else st['img'][-1])
    return st['img'].clone()


def counts(n, interval, full_last=0):
    from sr3_hip.schedules import feature_cache_refresh
    full = sum(feature_cache_refresh(k, n, interval, full_last) for k in range(n))
    return [full, n - full]


@pytest.mark.parametrize('sampler', [None, 'ddim'])
@pytest.mark.parametrize('name', ['sr3_tiny', 'ddpm_tiny'])
def test_interval_one_is_the_uncached_chain(name, sampler):
    m, g = make(name)
    netG = m.netG
    arg, x_T = chain_input(name, g)
    if sampler is not None:
        netG.set_sampler(4, 0.5, kind=sampler)
    n = SCHEDS[name]['n_timestep'] if sampler is None else 4
    base = run(netG, arg, x_T)
    netG.set_feature_cache(interval=1, depth=1)
    got = run(netG, arg, x_T)
    st = next(iter(netG._loop_cache.values()))
    assert st['graph'] is not None and st['graph_cached'] is None and st['fc_replays'] == [n, 0]      # (no schedule named the cached graph)
    assert torch.equal(got, base)
    netG.set_feature_cache(None)
    assert torch.equal(run(netG, arg, x_T), base)


@pytest.mark.parametrize('name,depth', [('sr3_tiny', 2), ('ddpm_tiny', 3)])
def test_graph_chain_is_the_eager_chain(name, depth):
    m, g = make(name)
    netG = m.netG
    arg, x_T = chain_input(name, g)
    n = SCHEDS[name]['n_timestep']
    base = run(netG, arg, x_T)
    netG.set_feature_cache(interval=3, depth=depth, full_last=1)
    netG.use_graph = False
    eager = run(netG, arg, x_T)
    netG.use_graph = True
    got = run(netG, arg, x_T)
    st = next(iter(netG._loop_cache.values()))
    assert st['graph'] is not None and st['graph_cached'] is not None
    assert st['fc_replays'] == counts(n, 3, 1) and st['fc_replays'][1] > 0
    assert torch.equal(got, eager) and torch.isfinite(got).all()
    assert not torch.equal(got, base), 'the cached chain is the uncached one: no cached step ran'
    again = run(netG, arg, x_T)            # a second chain on the same state: the stale cache of the first is never read
    assert torch.equal(again, got) and st['fc_replays'] == [2 * c for c in counts(n, 3, 1)]
    # another schedule at the same depth: the same state, the same two graphs, only the order of the replays moves
    graphs = (st['graph'], st['graph_cached'])
    netG.set_feature_cache(interval=2, depth=depth)
    other = run(netG, arg, x_T)
    assert next(iter(netG._loop_cache.values())) is st and (st['graph'], st['graph_cached']) == graphs
    netG.use_graph = False
    assert torch.equal(run(netG, arg, x_T), other) and not torch.equal(other, got)


@pytest.mark.parametrize('name', ['sr3_tiny', 'ddpm_tiny'])
def test_dpmpp_chain_against_the_two_entries(name):
    """dpmpp_2m, interval 2: the loop's result is the chain made of direct calls of engine.reverse_step (sr3_reverse_step_cached)."""
    from sr3_hip import engine as E
    from sr3_hip.schedules import feature_cache_refresh
    m, g = make(name)
    netG = m.netG
    arg, x_T = chain_input(name, g)
    S = 4
    netG.set_sampler(S, 0.0, kind='dpmpp_2m')
    netG.set_feature_cache(interval=2, depth=1)
    got = run(netG, arg, x_T)
    st = next(iter(netG._loop_cache.values()))
    assert st['fc_replays'] == [2, 2]
    un, d = netG.denoise_fn, G.dev()
    tables, level, t_map, c3, noisy = netG._step_rule()
    assert not noisy and c3 is not None
    img, hist, eps = x_T.clone(), torch.zeros_like(x_T), torch.empty_like(x_T)
    step2 = torch.full((2,), S - 1, dtype=torch.int32, device=d)
    cache, ws = un.plan.new_feature_cache(img.shape[0], d), E.Workspace()
    cond = arg if CONDITIONAL[name] else None
    un.ensure_derived()
    for k in range(S):
        E.reverse_step(un.plan, un.weights(), un.freq, ws, img, None, tables, step2, cond=cond, level_table=level, eps_out=eps,
                       t_map=t_map, c3=c3, hist=hist, feat_cache=cache, refresh=feature_cache_refresh(k, S, 2))
    assert step2.tolist()[1] == -1
    assert torch.equal(got, img)


def test_through_the_model_with_the_config_key():
    m, g = make('sr3_tiny', feature_cache={'interval': 3, 'depth': 1, 'full_last': 0})
    assert m.netG.feature_cache == dict(interval=3, depth=1, full_last=0) and m.netG.denoise_fn.plan.options['feat_cache'] == 1
    m.feed_data({'HR': torch.from_numpy(g['loop/hr']), 'SR': torch.from_numpy(g['loop/sr'])})
    m.test(continous=False)
    assert tuple(m.SR.shape[-3:]) == (3, 16, 16) and bool(torch.isfinite(m.SR).all())
    st = next(iter(m.netG._loop_cache.values()))
    assert st['fc_replays'] == counts(SCHEDS['sr3_tiny']['n_timestep'], 3)
