"""Multi-head attention through whole networks (config keys model.unet.n_head / head_dim): forward against the CPU oracle with its
self_attention replaced by the reference module's multi-head forward (tests/mha_ref.py; unet_forward resolves self_attention as a module
global, so a monkeypatch gives the whole-UNet reference), the captured reverse step against the eager one, and one training step against
float64 autograd through the same patched oracle.

The network: inner_channel 32, channel_mults [1, 2, 4], attn_res [8], image 16 -- attention at 8 x 8 with 64 channels and in the middle
block at 4 x 4 with 128; n_head = 2 gives head widths 32 and 64, head_dim = 32 gives 2 and 4 heads."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_util as G                      # noqa: E402
import mha_ref                            # noqa: E402
from helpers import opt_for               # noqa: E402
from oracle import sr3_oracle as O        # noqa: E402

HEADS = [dict(n_head=2), dict(head_dim=32)]
IDS = ['n_head2', 'head_dim32']


def _opt(base, phase, heads):
    opt = copy.deepcopy(opt_for(base, phase=phase, gpu=True))
    u = opt['model']['unet']
    u.update(inner_channel=32, norm_groups=32, **heads)
    if base == 'sr3_tiny':
        u.update(channel_multiplier=[1, 2, 4], attn_res=[8], res_blocks=1)
    return opt


def _net(base, heads, phase='val', seed=21):
    import model.networks as networks
    opt = _opt(base, phase, heads)
    torch.manual_seed(seed)
    netG = networks.define_G(opt)
    netG.denoise_fn.reset_parameters()
    sd = {k: v.clone() for k, v in netG.state_dict().items()}
    d = G.dev()
    netG = netG.to(d)
    netG.set_loss(d)
    netG.set_new_noise_schedule(opt['model']['beta_schedule'][phase], d)
    netG.show_progress = False
    return netG, sd, O.desc_from_opt(opt), opt


def _inputs(desc, B=2):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, desc['in_channel'], 16, 16, generator=g)
    lvl = torch.tensor([3, 1][:B], dtype=torch.long) if desc['variant'] == 'ddpm' else torch.linspace(0.2, 0.95, B).view(B, 1)
    return x, lvl


@pytest.mark.parametrize('base', ['sr3_tiny', 'ddpm_tiny'])
@pytest.mark.parametrize('heads', HEADS, ids=IDS)
def test_forward_against_the_multi_head_oracle(monkeypatch, base, heads):
    d = G.dev()
    netG, sd, desc, opt = _net(base, heads)
    x, lvl = _inputs(desc)
    un = netG.denoise_fn
    got = un(x.to(d), lvl.to(d)).cpu()
    attn = [o for o in un.plan.op_list(2) if o['kind'] == 60]
    assert attn and {o['cin'] for o in attn} >= {64}
    with torch.no_grad():
        one = O.unet_forward(sd, desc, x, lvl)
        monkeypatch.setattr(O, 'self_attention', mha_ref.patched(**heads))
        ref = O.unet_forward(sd, desc, x, lvl)
    err = G.assert_close(got, ref, what='%s %s eps' % (base, heads))
    tol = 2e-5 * max(1.0, ref.abs().max().item())
    gap = (ref - one).abs().max().item()
    print('%s %s: eps max abs err %.2e (tolerance %.2e); multi-head against single-head oracle %.2e' % (base, heads, err, tol, gap))
    assert gap > tol, 'the head count does not show in this network: the comparison proves nothing'
    # the same weights without the key: the single-head forward, which the multi-head one must differ from
    netG1, _, _, _ = _net(base, {})
    got1 = netG1.denoise_fn(x.to(d), lvl.to(d)).cpu()
    G.assert_close(got1, one, what='%s single-head eps' % base)
    assert (got - got1).abs().max().item() > tol


@pytest.mark.parametrize('heads', HEADS, ids=IDS)
def test_three_captured_reverse_steps_equal_the_eager_ones(heads):
    d = G.dev()
    netG, sd, desc, opt = _net('sr3_tiny', heads)
    B = 2
    shape = (B, 3, 16, 16)
    g = torch.Generator().manual_seed(8)
    x0 = torch.randn(shape, generator=g)
    cond = torch.rand(shape, generator=g) * 2 - 1
    un = netG.denoise_fn
    st = netG._loop_state(shape, shape, d)
    un.ensure_derived()
    netG._capture(st)
    t0 = netG.num_timesteps - 1
    st['img'].copy_(x0); st['cond'].copy_(cond); st['step'].fill_(t0)
    zs, imgs = [], []
    for _ in range(3):
        st['graph'].replay()
        torch.cuda.synchronize()
        zs.append(st['z'].clone())
        imgs.append(st['img'].clone())
    assert int(st['step'][1].item()) == t0 - 3
    tab = O.schedule_tables(opt['model']['beta_schedule']['val'])
    x = x0.to(d)
    for i in range(3):
        t = t0 - i
        lvl = torch.full((B,), float(tab['sqrt_alphas_cumprod_prev'][t + 1]), dtype=torch.float32, device=d)
        eps = un(x, lvl, cond=cond.to(d))
        netG._step_update(x, eps, zs[i], step_host=t)
        assert torch.equal(x, imgs[i]), 'captured reverse step %d != forward + p_sample update' % i


@pytest.mark.parametrize('heads', HEADS, ids=IDS)
def test_training_step_against_float64_autograd(monkeypatch, heads):
    d = G.dev()
    netG, sd, desc, opt = _net('sr3_tiny', heads, phase='train')
    B = 2
    g = torch.Generator().manual_seed(9)
    hr = torch.rand(B, 3, 16, 16, generator=g) * 2 - 1
    sr = torch.rand(B, 3, 16, 16, generator=g) * 2 - 1
    z = torch.randn(B, 3, 16, 16, generator=g)
    gamma = torch.tensor([0.35, 0.85])
    un = netG.denoise_fn
    assert un.dropout == 0.0
    netG.train()
    runs = []
    for _ in range(2):
        loss = netG.p_losses({'HR': hr.to(d), 'SR': sr.to(d)}, noise=z.to(d), gamma=gamma, drop_seed=77)
        torch.cuda.synchronize()
        runs.append((float(loss), un.grad_arena.clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]), 'two runs of the training step differ'
    monkeypatch.setattr(O, 'self_attention', mha_ref.patched(**heads))
    sdr = {k: (v.double().clone().requires_grad_(k.startswith('denoise_fn.')) if v.is_floating_point() else v) for k, v in sd.items()}
    ref_loss = O.p_losses_sr3(sdr, desc, hr.double(), sr.double(), gamma.double(), z.double(), conditional=True)
    (ref_loss / hr.numel()).backward()
    ref_loss = float(ref_loss.detach())
    assert abs(runs[0][0] - ref_loss) <= 1e-5 * abs(ref_loss), (runs[0][0], ref_loss)
    rows = []
    for key, grad in un.named_gradients():
        ref = sdr['denoise_fn.' + key].grad
        den = max(ref.norm().item(), 1e-7)
        rows.append(((grad.cpu().double() - ref).norm().item() / den, key, den))
    rows.sort(reverse=True)
    print('%s: loss %.6f (float64 %.6f); worst gradients (rel err, key, |ref|): %s' % (heads, runs[0][0], ref_loss, rows[:4]))
    assert any('attn.qkv' in k for _, k, _ in rows)
    bad = [r for r in rows if r[0] > 1e-4 and r[2] > 1e-6]
    assert not bad, bad[:8]
