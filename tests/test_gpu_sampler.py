"""The strided DDIM sampler on the GPU (tiny fixtures, batch 2, S <= 8): the step-index -> timestep map of sr3_reverse_step_ex, every
step of a sampler chain against the float64 textbook update fed with the oracle UNet's eps, graph replay against eager launches, the
noise-free eta = 0 chain, S = T / eta = 1 against the ancestral chain, and the config key through the drop-in `model` package.

Tolerances are the project's: one step 2e-5 * max(1, |ref|_inf), a whole chain 1e-4."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import DESCS, SCHEDS, CONDITIONAL, load_golden, opt_for      # noqa: E402
import gpu_util as G                                                     # noqa: E402

NAMES = ['sr3_tiny', 'ddpm_tiny']


def build(name, sampler=None):
    import model as Model
    opt = opt_for(name, phase='val', gpu=True)
    if sampler is not None:
        opt['model']['beta_schedule']['val']['sampler'] = sampler
    m = Model.create_model(opt)
    g, sd = load_golden(name)
    m.netG.load_state_dict(sd, strict=True)
    m.netG.show_progress = False
    return m, g, sd, opt


def _alphas_cumprod(name):
    s = SCHEDS[name]
    assert s['schedule'] == 'linear'
    return np.cumprod(1.0 - np.linspace(s['linear_start'], s['linear_end'], s['n_timestep'], dtype=np.float64))


def _walk(T, S):
    return np.round(np.linspace(0, T - 1, S)).astype(int) if S > 1 else np.array([T - 1])


def _textbook_step(ac, tau, j, eta, x, eps, z):
    """DDIM (Song et al. 2021, eq. 12 / 16) with the reference's clip_denoised: x0 is clipped and eps re-derived from it.  float64."""
    ab = float(ac[tau[j]])
    ap = float(ac[tau[j - 1]]) if j >= 1 else 1.0
    sigma = eta * float(np.sqrt((1 - ap) / (1 - ab)) * np.sqrt(1 - ab / ap))
    d = float(np.sqrt(max(1 - ap - sigma ** 2, 0.0)))
    x, eps = x.double(), eps.double()
    x0c = (float(np.sqrt(1 / ab)) * x - float(np.sqrt(1 / ab - 1)) * eps).clamp(-1.0, 1.0)
    out = float(np.sqrt(ap)) * x0c + d * (x - float(np.sqrt(ab)) * x0c) / float(np.sqrt(1 - ab))
    return out if z is None or sigma == 0.0 else out + sigma * z.double()


def _oracle_eps(sd, name, ac, tau, j, x, cond):
    from oracle import sr3_oracle as O
    b = x.shape[0]
    if DESCS[name]['variant'] == 'sr3':
        level = torch.FloatTensor([np.sqrt(ac[tau[j]])]).repeat(b, 1)       # = sqrt_alphas_cumprod_prev[tau[j] + 1]
    else:
        level = torch.full((b,), int(tau[j]), dtype=torch.long)
    with torch.no_grad():
        return O.unet_forward(sd, DESCS[name], torch.cat([cond, x], 1) if cond is not None else x, level)


def _loop_inputs(name, g, d):
    cond = torch.from_numpy(g['loop/sr']).to(d) if CONDITIONAL[name] else None
    x_T = torch.from_numpy(g['loop/x_T']).to(d)
    zs = torch.from_numpy(g['loop/zs']).to(d)
    assert x_T.shape[0] == 2
    return cond, x_T, zs, (cond if cond is not None else tuple(x_T.shape))


def test_ddpm_step_index_to_timestep_map_is_honoured():
    """sr3_reverse_step_ex conditions the DDPM UNet on t_map[counter] -- eps bit-equal to sr3_unet_forward at that timestep (same
    kernels) -- while the tail's tables stay indexed by the counter; with t_map = NULL it is sr3_reverse_step, bit for bit."""
    from sr3_hip import engine as E, lib as L
    m, g, sd, _ = build('ddpm_tiny')
    d = G.dev()
    netG, un = m.netG, m.netG.denoise_fn
    lib = L.load()
    xs = torch.from_numpy(g['step/x']).to(d)
    zs = torch.from_numpy(g['loop/zs']).to(d)
    B = xs.shape[0]
    tables = (netG.sqrt_recip_alphas_cumprod, netG.sqrt_recipm1_alphas_cumprod, netG.posterior_mean_coef1,
              netG.posterior_mean_coef2, netG._sigma)
    walk = [0, 3, 7, 12]                                   # (12 is past this fixture's T = 6: the map is all the embedding sees)
    t_map = torch.tensor(walk, dtype=torch.int32, device=d)
    for k, t in enumerate(walk):
        step2 = torch.tensor([-77, k], dtype=torch.int32, device=d)
        x1, eps1 = xs.clone(), torch.full_like(xs, float('nan'))
        un.reverse_step(x1, zs[k], tables, step2, eps_out=eps1, t_map=t_map)
        eps_ref = un(xs, torch.full((B,), t, dtype=torch.long, device=d))
        assert torch.equal(eps1, eps_ref), 'eps at index %d is not the forward at timestep %d' % (k, t)
        if t != k:
            assert not torch.equal(eps1, un(xs, torch.full((B,), k, dtype=torch.long, device=d)))
        x3 = xs.clone()
        netG._step_update(x3, eps_ref, zs[k], step_host=k)          # the tail reads row k of the tables, not row t
        assert torch.equal(x1, x3) and step2.tolist() == [k, k - 1]
    # NULL map: the forwarder and the entry it forwards to, through the C ABI
    ws = E.Workspace()
    un.ensure_derived()
    wsbuf, need = ws.get(un.plan, B, d)
    outs = []
    for fn, extra in ((lib.sr3_reverse_step, ()), (lib.sr3_reverse_step_ex, (None,))):
        for k in (5, 2, 0):
            step2 = torch.tensor([-77, k], dtype=torch.int32, device=d)
            x1, eps1 = xs.clone(), torch.full_like(xs, float('nan'))
            L.check(fn(un.plan.handle, L.ptr(x1), None, 0, L.ptr(un.freq), None, L.ptr(step2), L.ptr(un.weights()), L.ptr(wsbuf), need,
                       L.ptr(zs[k]), *[L.ptr(t) for t in tables], 1, L.ptr(eps1), B, G.stream(), *extra))
            torch.cuda.synchronize()
            assert step2.tolist() == [k, k - 1]
            outs.append((x1, eps1))
    for (xa, ea), (xb, eb) in zip(outs[:3], outs[3:]):
        assert torch.equal(xa, xb) and torch.equal(ea, eb) and bool(torch.isfinite(xa).all())
    with pytest.raises(L.Sr3Error):
        un.reverse_step(xs.clone(), None, tables, torch.zeros(2, dtype=torch.int32, device=d), t_map=t_map.long())


@pytest.mark.parametrize('eta', [0.0, 0.5])
@pytest.mark.parametrize('S', [6, 4])
@pytest.mark.parametrize('name', NAMES)
def test_sampler_steps_match_the_textbook_update(name, S, eta):
    """Every step of an S-step chain: the engine's new x against the float64 textbook update of the engine's own incoming x with
    the oracle UNet's eps (how test_gpu_trajectory.py compares single steps); then the free-running chain of p_sample_loop against
    the free-running oracle chain."""
    m, g, sd, _ = build(name)
    d = G.dev()
    netG = m.netG
    cond, x_T, zs, arg = _loop_inputs(name, g, d)
    T = SCHEDS[name]['n_timestep']
    ac, tau = _alphas_cumprod(name), _walk(T, S)
    netG.set_sampler(steps=S, eta=eta)
    assert netG._sampler_tau.tolist() == tau.tolist()
    st = netG._loop_state(tuple(x_T.shape), None if cond is None else tuple(x_T.shape), d)
    netG.denoise_fn.ensure_derived()
    st['img'].copy_(x_T)
    if cond is not None:
        st['cond'].copy_(cond)
    st['step'].fill_(S - 1)
    cc = None if cond is None else cond.cpu()
    xo = x_T.cpu()                                          # the oracle's own chain
    worst = 0.0
    for j in reversed(range(S)):
        x_in = st['img'].cpu()
        st['z'].copy_(zs[j])
        netG._one_step(st, draw_noise=False)
        assert st['z_used'] == (eta > 0)
        z = zs[j].cpu() if eta > 0 else None
        eps = _oracle_eps(sd, name, ac, tau, j, x_in, cc)
        G.assert_close(st['eps'].cpu(), eps, what='%s eps at step index %d' % (name, j))
        ref = _textbook_step(ac, tau, j, eta, x_in, eps, z)
        worst = max(worst, G.assert_close(st['img'].cpu(), ref, what='%s S=%d eta=%g step index %d' % (name, S, eta, j)))
        xo = _textbook_step(ac, tau, j, eta, xo, _oracle_eps(sd, name, ac, tau, j, xo, cc), z).float()
    assert st['step'].tolist() == [0, -1]
    stepped = st['img'].clone()
    out = netG.p_sample_loop(arg, continous=True, x_T=x_T, noise_seq=zs)
    last = out if (cond is None and DESCS[name]['variant'] == 'ddpm') else out[-2:]
    assert torch.equal(last, stepped)                       # the loop is those S steps
    err = float((last.cpu().double() - xo.double()).abs().max())
    print('%s S=%d eta=%g: worst step error %.2e, chain error %.2e' % (name, S, eta, worst, err))
    assert err <= 1e-4, err


@pytest.mark.parametrize('eta', [0.0, 0.5])
@pytest.mark.parametrize('name', NAMES)
def test_sampler_graph_replay_equals_eager(name, eta):
    m, g, sd, _ = build(name)
    d = G.dev()
    netG = m.netG
    cond, x_T, zs, arg = _loop_inputs(name, g, d)
    netG.set_sampler(steps=5, eta=eta)
    outs = []
    for use_graph in (False, True):
        netG.use_graph = use_graph
        torch.manual_seed(7)
        outs.append(netG.p_sample_loop(arg, continous=True).clone())
    st = next(iter(netG._loop_cache.values()))
    assert len(netG._loop_cache) == 1 and st['graph'] is not None and st['step'].tolist() == [0, -1]
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[1]).all())


@pytest.mark.parametrize('name', NAMES)
def test_eta_zero_chain_draws_no_noise(name):
    """eta = 0: the chain is a function of x_T alone -- the generator's state after x_T does not matter, `_draw` is never called and
    the step gets no z; with eta > 0 the same two seeds give two different images."""
    m, g, sd, _ = build(name)
    d = G.dev()
    netG = m.netG
    cond, x_T, zs, arg = _loop_inputs(name, g, d)
    calls = []
    draw = netG._draw
    netG._draw = lambda t, gens: (calls.append(1), draw(t, gens))[1]

    def chains(eta):
        netG.set_sampler(steps=6, eta=eta)
        outs = []
        for seed in (1, 2):
            torch.manual_seed(seed)
            outs.append(netG.p_sample_loop(arg, continous=False, x_T=x_T).clone())
        st = next(iter(netG._loop_cache.values()))
        assert st['graph'] is not None                      # the production path: captured and replayed
        return outs, st
    (a, b), st = chains(0.0)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert st['z_used'] is False and calls == []
    (a5, b5), st = chains(0.5)
    assert st['z_used'] is True and len(calls) > 0
    assert not torch.equal(a5, b5) and not torch.equal(a5, a)


@pytest.mark.parametrize('name', NAMES)
def test_full_walk_eta_one_is_the_ancestral_chain(name):
    """S = T, eta = 1: the sampler's tables are the ancestral ones up to one fp32 rounding, so the same x_T and noise give the same
    chain within the loop tolerance."""
    m, g, sd, _ = build(name)
    d = G.dev()
    netG = m.netG
    cond, x_T, zs, arg = _loop_inputs(name, g, d)
    T = SCHEDS[name]['n_timestep']
    ref = netG.p_sample_loop(arg, continous=True, x_T=x_T, noise_seq=zs).clone()
    netG.set_sampler(steps=T, eta=1.0)
    assert netG._sampler_tau.tolist() == list(range(T))
    out = netG.p_sample_loop(arg, continous=True, x_T=x_T, noise_seq=zs)
    assert out.shape == ref.shape
    err = float((out - ref).abs().max())
    print('%s: S = T = %d, eta = 1 against the ancestral chain: %.2e' % (name, T, err))
    assert err <= 1e-4, err


class _CountingGraph(object):
    def __init__(self, graph):
        self.graph, self.replays = graph, 0

    def replay(self):
        self.replays += 1
        self.graph.replay()


@pytest.mark.parametrize('S', [5, 8])
def test_config_key_drops_into_the_model_package(S):
    """`"sampler"` under model.beta_schedule.val: the phase switch of the reference's sr.py selects it, `test()` runs S replays of
    the captured step, `continous=True` returns 1 + #{j : j % (1 | S // 10) == 0} images per item, and set_sampler(None) gives the
    T-step chain back."""
    m, g, sd, opt = build('sr3_tiny', sampler={'type': 'ddim', 'steps': S, 'eta': 0.0})
    netG = m.netG
    T = SCHEDS['sr3_tiny']['n_timestep']
    assert netG.sampler is None                             # (the constructor sets the train schedule, as in the reference)
    m.set_new_noise_schedule(opt['model']['beta_schedule']['val'], schedule_phase='val')
    assert netG.sampler == dict(type='ddim', steps=S, eta=0.0) and netG.num_timesteps == T
    m.feed_data({'HR': torch.from_numpy(g['loop/hr'][:1]), 'SR': torch.from_numpy(g['loop/sr'][:1])})

    def run(steps):
        m.test(continous=True)                              # captures
        st = next(iter(netG._loop_cache.values()))
        assert len(netG._loop_cache) == 1 and st['step'].tolist() == [0, -1]
        first = m.SR.clone()
        st['graph'] = _CountingGraph(st['graph'])
        m.test(continous=True)
        assert st['graph'].replays == steps and st['step'].tolist() == [0, -1]
        n_snap = sum(1 for j in range(steps) if j % (1 | (steps // 10)) == 0)
        assert tuple(m.SR.shape) == (1 + n_snap, 3, 16, 16) and bool(torch.isfinite(m.SR).all())
        assert torch.equal(m.SR[0].cpu(), torch.from_numpy(g['loop/sr'][0]))
        return first, m.SR.clone()
    a, b = run(S)
    assert torch.equal(a[0], b[0]) and not torch.equal(a[-1], b[-1])         # (each chain draws its own x_T)
    m.test(continous=False)
    assert tuple(m.SR.shape) == (3, 16, 16)
    netG.set_sampler(None)
    assert netG.sampler is None and netG._loop_cache == {}
    run(T)
