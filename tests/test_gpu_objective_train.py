"""Training under v- / x0-prediction, Min-SNR weights and the Huber loss: `p_losses` (sr3_train_step_ex behind it) against CPU autograd of
the oracle's UNet with the target, rho and weight written out here.  Tolerances are the project's for these fixtures
(tests/test_gpu_train.py): loss relative 1e-5, gradients normwise relative 1e-4 for entries with |ref| > 1e-6."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import DESCS, SCHEDS, CONDITIONAL, load_golden, opt_for      # noqa: E402
import gpu_util as G                                             # noqa: E402
from oracle import sr3_oracle as O                               # noqa: E402

NAMES = ['sr3_tiny', 'ddpm_tiny', 'sr3_uncond']
DELTA = 0.5
# Min-SNR gamma between the SNR of the fixture's two recorded noise levels (126 / 130, 81 / 40, 27.0 / 27.2): one image on each branch
# of min(SNR, gamma)
GAMMA = {'sr3_tiny': 128.0, 'ddpm_tiny': 60.0, 'sr3_uncond': 27.1}
CASES = [(p, l, w) for p in ('v', 'x0') for l in ('l2', 'huber') for w in ('uniform', 'min_snr')] + [('v', 'l1', 'uniform'), ('x0', 'l1', 'uniform')]

_models = {}


def model(name, **diffusion):
    """One train-phase model per fixture (and per set of config keys), with the golden weights."""
    import model as Model
    key = (name, repr(sorted(diffusion.items())))
    if key not in _models:
        opt = opt_for(name, phase='train', gpu=True)
        opt['model']['diffusion'].update(diffusion)
        m = Model.create_model(opt)
        g, sd = load_golden(name)
        m.netG.load_state_dict(sd, strict=True)
        _models[key] = (m, g, sd)
    return _models[key]


def engine_step(m, g, name, **kw):
    d = G.dev()
    data = {'HR': torch.from_numpy(g['loop/hr']).to(d), 'SR': torch.from_numpy(g['loop/sr']).to(d)}
    z = torch.from_numpy(g['train/z']).to(d)
    if DESCS[name]['variant'] == 'sr3':
        loss = m.netG.p_losses(data, noise=z, gamma=torch.from_numpy(g['train/gamma']), **kw)
    else:
        loss = m.netG.p_losses(data, noise=z, t=torch.from_numpy(g['train/t']).to(d), **kw)
    torch.cuda.synchronize()
    return float(loss)


_forwards = {}


def oracle_forward(name, g, sd):
    """The oracle's forward on the recorded draws, once per fixture: (parameters, network output with its autograd graph, ca [B])."""
    if name in _forwards:
        return _forwards[name]
    desc = DESCS[name]
    hr, sr, z = torch.from_numpy(g['loop/hr']), torch.from_numpy(g['loop/sr']), torch.from_numpy(g['train/z'])
    b = hr.shape[0]
    sdr = {k: v.clone().requires_grad_(v.is_floating_point() and k.startswith('denoise_fn.')) for k, v in sd.items()}
    if desc['variant'] == 'sr3':
        gamma = torch.from_numpy(g['train/gamma'])
        x_noisy = O.q_sample_sr3(hr, gamma.view(-1, 1, 1, 1), z)
        time, ca = gamma.view(b, -1), gamma.double()
    else:
        t = torch.from_numpy(g['train/t'])
        tab = O.schedule_tables(SCHEDS[name])
        a = torch.from_numpy(tab['sqrt_alphas_cumprod'])[t].view(-1, 1, 1, 1)
        s = torch.from_numpy(tab['sqrt_one_minus_alphas_cumprod'])[t].view(-1, 1, 1, 1)
        x_noisy = a * hr + s * z
        time, ca = t, a.double().view(-1)
    inp = torch.cat([sr, x_noisy], dim=1) if CONDITIONAL[name] else x_noisy
    _forwards[name] = (sdr, O.unet_forward(sdr, desc, inp, time).double(), ca)
    return _forwards[name]


def oracle_step(name, g, sd, pred, ltype, weight):
    """(loss, residual d [float64], {key: gradient of loss / numel}) -- the objective restated on the oracle's output: target
    v = ca z - cb x0 | x0, weight min(SNR, gamma) / {SNR + 1, 1}, rho = |d| | d^2 | Huber; torch autograd through the oracle's UNet."""
    hr, z = torch.from_numpy(g['loop/hr']), torch.from_numpy(g['train/z'])
    sdr, out, ca = oracle_forward(name, g, sd)
    ca = ca.view(-1, 1, 1, 1)
    cb = (1 - ca ** 2).sqrt()
    target = ca * z.double() - cb * hr.double() if pred == 'v' else hr.double()
    d = target - out
    snr = (ca ** 2 / (1 - ca ** 2)).view(-1)
    if weight == 'min_snr':
        assert snr.min().item() < GAMMA[name] < snr.max().item(), snr
        w = torch.minimum(snr, torch.tensor(GAMMA[name], dtype=torch.float64)) / (snr + 1 if pred == 'v' else torch.ones_like(snr))
    else:
        w = torch.ones_like(snr)
    if ltype == 'l1':
        rho = d.abs()
    elif ltype == 'l2':
        rho = d * d
    else:
        inside = d.abs() <= DELTA
        assert 0 < inside.sum().item() < inside.numel()          # both branches of the Huber loss occur
        rho = torch.where(inside, 0.5 * d * d, DELTA * (d.abs() - 0.5 * DELTA))
    loss = (w.view(-1, 1, 1, 1) * rho).sum()
    params = {k: v for k, v in sdr.items() if v.requires_grad}
    grads = torch.autograd.grad(loss / hr.numel(), list(params.values()), retain_graph=True)
    return float(loss.detach()), d.detach(), dict(zip(params, grads))


def configure(m, name, pred, ltype, weight):
    m.netG.set_prediction(pred)
    m.netG.set_objective(ltype, DELTA if ltype == 'huber' else None, weight, GAMMA[name] if weight == 'min_snr' else None)


def restore(m):
    m.netG.set_prediction('eps')
    m.netG.objective = None


@pytest.mark.parametrize('pred,ltype,weight', CASES)
@pytest.mark.parametrize('name', NAMES)
def test_p_losses_match_oracle_autograd(name, pred, ltype, weight):
    m, g, sd = model(name)
    ref_loss, d, ref_grads = oracle_step(name, g, sd, pred, ltype, weight)
    if ltype == 'l1':
        # L1 gradients are step functions of d: the recorded draws must keep every element away from the step
        assert d.abs().min().item() > 1e-5, d.abs().min().item()
    configure(m, name, pred, ltype, weight)
    try:
        loss = engine_step(m, g, name)
        grads = [(k, v.cpu().clone()) for k, v in m.netG.denoise_fn.named_gradients()]
    finally:
        restore(m)
    bad, worst = [], 0.0
    for key, grad in grads:
        ref = ref_grads['denoise_fn.' + key]
        num, den = (grad - ref).norm().item(), max(ref.norm().item(), 1e-7)
        if den > 1e-6:
            worst = max(worst, num / den)
            if num / den > 1e-4:
                bad.append((num / den, key))
    print('%s %s/%s/%s: loss %.9g ref %.9g (rel %.2e), worst gradient rel %.2e' % (name, pred, ltype, weight, loss, ref_loss, abs(loss - ref_loss) / abs(ref_loss), worst))
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (loss, ref_loss)
    assert abs(loss - float(g['train/loss_sum'])) > 1e-3 * float(g['train/loss_sum'])      # not the eps / L1 value
    assert not bad, sorted(bad, reverse=True)[:8]


@pytest.mark.parametrize('name', ['sr3_tiny', 'ddpm_tiny'])
def test_explicit_default_keys_are_the_keyless_step(name):
    """"prediction": "eps" with "loss": {"type": "l1", "weight": "uniform"} is the step of a config without the keys: same loss, same
    gradient arena, bit for bit (it passes no tables and runs k_l1_loss_grad)."""
    m, g, sd = model(name)
    base = engine_step(m, g, name)
    arena = m.netG.denoise_fn.grad_arena.clone()
    assert abs(base - float(g['train/loss_sum'])) <= 1e-5 * float(g['train/loss_sum'])
    m2, _, _ = model(name, prediction='eps', loss={'type': 'l1', 'weight': 'uniform'})
    assert m2.netG.objective == dict(type='l1', delta=None, weight='uniform', gamma=None) and m2.netG._train_objective(None, None, G.dev())[:3] == (None, None, None)
    assert engine_step(m2, g, name) == base
    assert torch.equal(m2.netG.denoise_fn.grad_arena, arena)


@pytest.mark.parametrize('name', ['sr3_tiny', 'ddpm_tiny'])
def test_objective_step_is_bitwise_reproducible(name):
    m, g, sd = model(name)
    configure(m, name, 'v', 'huber', 'min_snr')
    try:
        outs = []
        for _ in range(3):
            loss = engine_step(m, g, name, drop_seed=1234)
            outs.append((loss, m.netG.denoise_fn.grad_arena.clone()))
    finally:
        restore(m)
    for l, ga in outs[1:]:
        assert l == outs[0][0] and torch.equal(ga, outs[0][1])


@pytest.mark.parametrize('name,pred,ltype', [('sr3_tiny', 'v', 'huber'), ('ddpm_tiny', 'x0', 'l2')])
def test_config_keys_to_one_adam_step(name, pred, ltype):
    """config keys -> create_model -> feed_data -> optimize_parameters (draws patched to the recorded ones): l_pix and the update of
    every weight against torch.optim.Adam on the oracle's gradients, with the masks and bounds of
    tests/test_gpu_train.py::test_optimize_parameters_one_adam_step."""
    import model as Model
    loss_cfg = {'type': ltype, 'weight': 'min_snr', 'gamma': GAMMA[name]}
    if ltype == 'huber':
        loss_cfg['delta'] = DELTA
    opt = opt_for(name, phase='train', gpu=True)
    opt['model']['diffusion'].update(prediction=pred, loss=loss_cfg)
    m = Model.create_model(opt)
    g, sd = load_golden(name)
    m.netG.load_state_dict(sd, strict=True)
    d = G.dev()
    netG = m.netG
    z = torch.from_numpy(g['train/z']).to(d)
    orig = netG.p_losses
    if DESCS[name]['variant'] == 'sr3':
        netG.p_losses = lambda x_in, noise=None: orig(x_in, noise=z, gamma=torch.from_numpy(g['train/gamma']))
    else:
        netG.p_losses = lambda x_in, noise=None: orig(x_in, noise=z, t=torch.from_numpy(g['train/t']).to(d))
    m.feed_data({'HR': torch.from_numpy(g['loop/hr']), 'SR': torch.from_numpy(g['loop/sr'])})
    m.optimize_parameters()
    ref_loss, _, grads = oracle_step(name, g, sd, pred, ltype, 'min_snr')
    ref_lpix = ref_loss / g['loop/hr'].size
    assert abs(m.get_current_log()['l_pix'] - ref_lpix) <= 1e-5 * abs(ref_lpix), (m.get_current_log()['l_pix'], ref_lpix)
    params = {k: torch.nn.Parameter(sd[k].clone()) for k in grads}
    for k, v in params.items():
        v.grad = grads[k].clone()
    torch.optim.Adam(list(params.values()), lr=opt['train']['optimizer']['lr']).step()
    out = netG.state_dict()
    tot = bad = 0
    for key, ref_new in params.items():
        old, grad = sd[key], grads[key]
        mask = grad.abs() > 1e-6 * max(grad.abs().max().item(), 1e-12) + 1e-9
        upd = (out[key].cpu() - old)[mask]
        ref_upd = (ref_new.detach() - old)[mask]
        tot += mask.sum().item()
        bad += ((upd - ref_upd).abs() > 2e-6).sum().item()
    print('%s %s/%s: %d of %d updates off by more than 2e-6' % (name, pred, ltype, bad, tot))
    assert tot > 1000 and bad <= 1e-4 * tot, (bad, tot)
