"""Sampling a v- or x0-predicting model: every loop reads other a, b tables for x0c = clip(a x - b out) and nothing else.  The ancestral
chain, p_sample and p_mean_variance against the oracle on a table dict whose two x0 tables are replaced by `prediction_coefs`' x0_a,
x0_b; DDIM and DPM-Solver++(2M) under v against the textbook updates restated here in float64 with x0 = sqrt(abar) x - sqrt(1 - abar) v;
graph replay, the tiled loop and the switch of an existing model.

Tolerances are the project's (tests/test_gpu_sampler.py): one step 2e-5 * max(1, |ref|_inf), a whole chain 1e-4."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import DESCS, SCHEDS, CONDITIONAL, load_golden, opt_for      # noqa: E402
import gpu_util as G                                                     # noqa: E402
from oracle import sr3_oracle as O                                       # noqa: E402
from sr3_hip.diffusion import prediction_coefs, sampler_walk             # noqa: E402

NAMES = ['sr3_tiny', 'ddpm_tiny']


def build(name, prediction=None, sampler=None):
    import model as Model
    opt = opt_for(name, phase='val', gpu=True)
    if prediction is not None:
        opt['model']['diffusion']['prediction'] = prediction
    if sampler is not None:
        opt['model']['beta_schedule']['val']['sampler'] = sampler
    m = Model.create_model(opt)
    g, sd = load_golden(name)
    m.netG.load_state_dict(sd, strict=True)
    m.netG.show_progress = False
    return m, g, sd


def tables_for(name, pred):
    """The oracle's table dict with the two x0 tables replaced: fp32 of `prediction_coefs` on the fp64 schedule."""
    tab = O.schedule_tables(SCHEDS[name])
    ac = _alphas_cumprod(name)
    a, b = prediction_coefs(pred, np.sqrt(ac), np.sqrt(1.0 - ac))[:2]
    return dict(tab, sqrt_recip_alphas_cumprod=a.astype(np.float32), sqrt_recipm1_alphas_cumprod=b.astype(np.float32))


def _alphas_cumprod(name):
    s = SCHEDS[name]
    assert s['schedule'] == 'linear'
    return np.cumprod(1.0 - np.linspace(s['linear_start'], s['linear_end'], s['n_timestep'], dtype=np.float64))


def _loop_inputs(name, g, d):
    cond = torch.from_numpy(g['loop/sr']).to(d) if CONDITIONAL[name] else None
    x_T = torch.from_numpy(g['loop/x_T']).to(d)
    zs = torch.from_numpy(g['loop/zs']).to(d)
    return cond, x_T, zs, (cond if cond is not None else tuple(x_T.shape))


def _whole(name, out):
    return out if (not CONDITIONAL[name] and DESCS[name]['variant'] == 'ddpm') else out[-2:]


def _oracle_out(sd, name, level_or_t, x, cond):
    """The oracle UNet's output at one noise level (SR3: sqrt(abar), in x's dtype) / timestep (DDPM)."""
    b = x.shape[0]
    if DESCS[name]['variant'] == 'sr3':
        time = torch.full((b, 1), float(np.float32(level_or_t)), dtype=x.dtype)
    else:
        time = torch.full((b,), int(level_or_t), dtype=torch.long)
    with torch.no_grad():
        return O.unet_forward(sd, DESCS[name], torch.cat([cond, x], 1) if cond is not None else x, time)


def _ancestral_chain(sd, name, tab, cond, x_T, zs):
    """O.p_sample_loop's chain (its result only) in the dtype of its inputs: the oracle's own fp32 and float64 evaluations."""
    x = x_T
    for i in reversed(range(tab['num_timesteps'])):
        lv = tab['sqrt_alphas_cumprod_prev'][i + 1] if DESCS[name]['variant'] == 'sr3' else i
        x = O.p_sample_update(tab, x, _oracle_out(sd, name, lv, x, cond), i, zs[i] if i > 0 else None)
    return x


@pytest.mark.parametrize('pred', ['v', 'x0'])
@pytest.mark.parametrize('name', NAMES)
def test_ancestral_chain_matches_the_oracle_on_substituted_tables(name, pred):
    m, g, sd = build(name, prediction=pred)
    d = G.dev()
    cond, x_T, zs, arg = _loop_inputs(name, g, d)
    tab = tables_for(name, pred)
    cc = None if cond is None else cond.cpu()
    with torch.no_grad():
        ref = O.p_sample_loop(sd, DESCS[name], tab, cc, x_T.cpu(), zs.cpu(), conditional=CONDITIONAL[name], continous=True)
    # the gate below is only as good as the reference: its own fp32 and float64 evaluations must agree well inside it
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    r64 = _ancestral_chain(sd64, name, tab, None if cc is None else cc.double(), x_T.cpu().double(), zs.cpu().double())
    r32 = _ancestral_chain(sd, name, tab, cc, x_T.cpu(), zs.cpu())
    assert torch.equal(r32, _whole(name, ref))
    own = (r32.double() - r64).abs().max().item()
    assert own <= 1e-5, own
    out = m.netG.p_sample_loop(arg, continous=True, x_T=x_T, noise_seq=zs).cpu()
    err = (out - ref).abs().max().item()
    print('%s %s: chain error %.2e (oracle fp32 vs float64 %.2e)' % (name, pred, err, own))
    assert out.shape == ref.shape and err <= 1e-4, err
    eps_tab = O.schedule_tables(SCHEDS[name])
    with torch.no_grad():
        other = O.p_sample_loop(sd, DESCS[name], eps_tab, cc, x_T.cpu(), zs.cpu(), conditional=CONDITIONAL[name], continous=True)
    assert (other - ref).abs().max().item() > 1e-2          # the substituted tables matter: the eps chain ends elsewhere


@pytest.mark.parametrize('name', NAMES)
def test_graph_replay_equals_eager_under_v(name):
    m, g, sd = build(name, prediction='v')
    d = G.dev()
    netG = m.netG
    cond, x_T, zs, arg = _loop_inputs(name, g, d)
    outs = []
    for use_graph in (False, True):
        netG.use_graph = use_graph
        torch.manual_seed(7)
        outs.append(netG.p_sample_loop(arg, continous=True).clone())
    st = next(iter(netG._loop_cache.values()))
    assert len(netG._loop_cache) == 1 and st['graph'] is not None and st['step'].tolist() == [0, -1]
    assert st['tables'][0][0] is netG.sqrt_alphas_cumprod and st['tables'][0][1] is netG.sqrt_one_minus_alphas_cumprod
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[1]).all())


def _half_logsnr(ac):
    return 0.5 * np.log(ac / (1.0 - ac))


def _textbook_v_step(kind, ac, tau, j, eta, x, v, z, prev):
    """One sampler step of a v-predicting model, float64.  x0c = clip(sqrt(ab) x - sqrt(1 - ab) v) (Salimans & Ho 2022), then
    DDIM (Song et al. 2021, eq. 12 / 16; eps re-derived from the clipped x0), or DPM-Solver++(2M) (Lu et al. 2022, Algorithm 2) with
    prev = (the previous step's x0c, its h) or None at the first step.  Returns (x_new, (x0c, h))."""
    S = len(tau)
    ab = float(ac[tau[j]])
    ap = float(ac[tau[j - 1]]) if j >= 1 else 1.0
    x, v = x.double(), v.double()
    x0c = (np.sqrt(ab) * x - np.sqrt(1.0 - ab) * v).clamp(-1.0, 1.0)
    if kind == 'ddim':
        sigma = eta * float(np.sqrt((1 - ap) / (1 - ab)) * np.sqrt(1 - ab / ap))
        dd = float(np.sqrt(max(1 - ap - sigma ** 2, 0.0)))
        out = np.sqrt(ap) * x0c + dd * (x - np.sqrt(ab) * x0c) / np.sqrt(1 - ab)
        return (out if z is None or sigma == 0.0 else out + sigma * z.double()), (x0c, None)
    if j == 0:                                   # the last step goes to abar = 1
        return x0c.clone(), (x0c, None)
    h = float(_half_logsnr(ap) - _half_logsnr(ab))
    D = x0c
    if j < S - 1:
        r = prev[1] / h
        D = (1.0 + 1.0 / (2.0 * r)) * x0c - 1.0 / (2.0 * r) * prev[0]
    return np.sqrt(1.0 - ap) / np.sqrt(1.0 - ab) * x - np.sqrt(ap) * np.expm1(-h) * D, (x0c, h)


@pytest.mark.parametrize('kind,eta', [('ddim', 0.0), ('ddim', 1.0), ('dpmpp_2m', 0.0)])
@pytest.mark.parametrize('name', NAMES)
def test_sampler_steps_under_v_match_the_textbook(name, kind, eta):
    """Every step of a 4-step chain: the engine's new x against the float64 textbook update of the engine's own incoming x (and its own
    previous x0c, for the multistep solver) with the oracle UNet's output read as v; then p_sample_loop against the free-running
    float64 chain."""
    S = 4
    m, g, sd = build(name, prediction='v')
    d = G.dev()
    netG = m.netG
    cond, x_T, zs, arg = _loop_inputs(name, g, d)
    ac = _alphas_cumprod(name)
    netG.set_sampler(steps=S, eta=eta, kind=kind)
    tau = sampler_walk(ac, S, 'logsnr' if kind == 'dpmpp_2m' else 'time')
    assert netG._sampler_tau.tolist() == tau.tolist() and (netG._sampler_c3 is not None) == (kind == 'dpmpp_2m')
    assert torch.equal(netG._sampler_a.cpu(), torch.tensor(np.sqrt(ac[tau]), dtype=torch.float32))
    st = netG._loop_state(tuple(x_T.shape), None if cond is None else tuple(x_T.shape), d)
    netG.denoise_fn.ensure_derived()
    st['img'].copy_(x_T)
    if cond is not None:
        st['cond'].copy_(cond)
    if st.get('hist') is not None:
        st['hist'].zero_()
    st['step'].fill_(S - 1)
    cc = None if cond is None else cond.cpu()
    lv = lambda j: np.sqrt(ac[tau[j]]) if DESCS[name]['variant'] == 'sr3' else tau[j]
    xo, prev_o, prev_e, worst = x_T.cpu().double(), None, None, 0.0
    for j in reversed(range(S)):
        x_in = st['img'].cpu()
        st['z'].copy_(zs[j])
        netG._one_step(st, draw_noise=False)
        assert st['z_used'] == (eta > 0)
        z = zs[j].cpu() if eta > 0 else None
        v = _oracle_out(sd, name, lv(j), x_in, cc)
        G.assert_close(st['eps'].cpu(), v, what='%s output at step index %d' % (name, j))
        ref, prev_e = _textbook_v_step(kind, ac, tau, j, eta, x_in, v, z, prev_e)
        worst = max(worst, G.assert_close(st['img'].cpu(), ref, what='%s %s eta=%g step index %d' % (name, kind, eta, j)))
        if kind == 'dpmpp_2m':
            G.assert_close(st['hist'].cpu(), prev_e[0], what='%s history after step index %d' % (name, j))
            prev_e = (st['hist'].cpu().double(), prev_e[1])      # the next step's reference extrapolates from the engine's own history
        xo, prev_o = _textbook_v_step(kind, ac, tau, j, eta, xo, _oracle_out(sd, name, lv(j), xo.float(), cc), z, prev_o)
    assert st['step'].tolist() == [0, -1]
    stepped = st['img'].clone()
    out = netG.p_sample_loop(arg, continous=True, x_T=x_T, noise_seq=zs)
    assert torch.equal(_whole(name, out), stepped)          # the loop is those S steps
    err = float((stepped.cpu().double() - xo).abs().max())
    print('%s %s eta=%g under v: worst step error %.2e, chain error %.2e' % (name, kind, eta, worst, err))
    assert err <= 1e-4, err


@pytest.mark.parametrize('pred', ['v', 'x0'])
@pytest.mark.parametrize('name', NAMES)
def test_p_sample_and_p_mean_variance_one_step(name, pred):
    m, g, sd = build(name, prediction=pred)
    d = G.dev()
    netG = m.netG
    cond, x_T, zs, _ = _loop_inputs(name, g, d)
    tab = tables_for(name, pred)
    cc = None if cond is None else cond.cpu()
    T = SCHEDS[name]['n_timestep']
    for t in (T - 1, 2):
        tt = torch.full((x_T.shape[0],), t, dtype=torch.long, device=d) if DESCS[name]['variant'] == 'ddpm' else t
        with torch.no_grad():
            ref = O.p_sample(sd, DESCS[name], tab, x_T.cpu(), t, zs[t].cpu(), condition_x=cc)
            ref_mean = O.p_sample(sd, DESCS[name], tab, x_T.cpu(), t, torch.zeros_like(zs[t].cpu()), condition_x=cc)
        got = netG.p_sample(x_T, tt, condition_x=cond, noise=zs[t])
        G.assert_close(got.cpu(), ref, what='%s %s p_sample at t = %d' % (name, pred, t))
        mean = netG.p_mean_variance(x_T, tt, True, condition_x=cond)[0]
        G.assert_close(mean.cpu(), ref_mean, what='%s %s p_mean_variance at t = %d' % (name, pred, t))


def test_tiled_loop_under_v_with_one_tile_is_the_whole_image_loop():
    m, g, sd = build('sr3_tiny', prediction='v')
    d = G.dev()
    netG = m.netG
    cond, x_T, zs, arg = _loop_inputs('sr3_tiny', g, d)
    plain = netG.p_sample_loop(arg, continous=True, x_T=x_T, noise_seq=zs).clone()
    tiled = netG.p_sample_loop_tiled(arg, continous=True, tile=16, overlap=0, x_T=x_T, noise_seq=zs)
    assert torch.equal(tiled, plain) and bool(torch.isfinite(plain).all())
    tab = tables_for('sr3_tiny', 'v')
    with torch.no_grad():
        ref = O.p_sample_loop(sd, DESCS['sr3_tiny'], tab, cond.cpu(), x_T.cpu(), zs.cpu(), conditional=True, continous=True)
    assert (tiled.cpu() - ref).abs().max().item() <= 1e-4


@pytest.mark.parametrize('name', NAMES)
def test_set_prediction_drops_the_captured_loop(name):
    """One model, a deterministic 4-step DDIM chain replayed from its graph: after set_prediction('v') the next loop captures again, on
    the v tables, and ends where the float64 textbook chain of a v-model ends."""
    S = 4
    m, g, sd = build(name)
    d = G.dev()
    netG = m.netG
    netG.set_sampler(steps=S, eta=0.0)
    cond, x_T, zs, arg = _loop_inputs(name, g, d)
    as_eps = netG.p_sample_loop(arg, continous=True, x_T=x_T).clone()
    old = next(iter(netG._loop_cache.values()))
    assert old['graph'] is not None
    netG.set_prediction('v')
    assert not netG._loop_cache and netG.sampler == dict(type='ddim', steps=S, eta=0.0)
    as_v = netG.p_sample_loop(arg, continous=True, x_T=x_T).clone()
    new = next(iter(netG._loop_cache.values()))
    assert len(netG._loop_cache) == 1 and new is not old and new['graph'] is not None and new['graph'] is not old['graph']
    assert new['tables'][0][0] is netG._sampler_a and not torch.equal(as_v, as_eps)
    ac = _alphas_cumprod(name)
    tau = sampler_walk(ac, S, 'time')
    cc = None if cond is None else cond.cpu()
    xo = x_T.cpu().double()
    for j in reversed(range(S)):
        lv = np.sqrt(ac[tau[j]]) if DESCS[name]['variant'] == 'sr3' else tau[j]
        xo, _ = _textbook_v_step('ddim', ac, tau, j, 0.0, xo, _oracle_out(sd, name, lv, xo.float(), cc), None, None)
    err = float((_whole(name, as_v).cpu().double() - xo).abs().max())
    print('%s: chain after the switch, error %.2e' % (name, err))
    assert err <= 1e-4, err
