"""Training at an image size other than the config's image_size (plan option train_geom, set by EngineUNet when such a batch arrives):
the engine's fused forward + backward + Adam against the reference's autograd step recorded in tests/golden/train_rect.part*.npz
(tools/make_golden_train_rect.py; dropout 0, injected t / gamma / z), and the 9-tap weight-gradient kernel on the maps whose width
is not a power of two.  Bounds are those of tests/test_gpu_train.py (loss rel 1e-5, gradients normwise rel 1e-4 where |ref| > 1e-6)
and of tests/test_gpu_ops.py's weight-gradient cases (normwise 2e-6 against float64)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import CONDITIONAL, DESCS, SCHEDS, load_golden, opt_for      # noqa: E402
import gpu_util as G                                                       # noqa: E402
from sr3_hip import lib as L                                               # noqa: E402

CASES = [('sr3_tiny', 16, 24, False), ('sr3_tiny', 24, 16, False), ('ddpm_tiny', 16, 24, False), ('sr3_tiny', 80, 64, True)]
IDS = ['%s_%dx%d' % c[:3] for c in CASES]
_FIXTURE = []


def fixture():
    if not _FIXTURE:
        _FIXTURE.append(load_golden('train_rect')[0])
    return _FIXTURE[0]


def build_train(name, long_attention=False, dropout=0.0):
    import model as Model
    opt = opt_for(name, phase='train', gpu=True)
    if long_attention:
        opt['model']['unet']['long_attention'] = True
    opt['model']['unet']['dropout'] = dropout
    m = Model.create_model(opt)
    _, sd = load_golden(name)
    m.netG.load_state_dict(sd, strict=True)
    return m, sd


def case_data(name, H, W):
    g, k, d = fixture(), '%s/%dx%d/' % (name, H, W), G.dev()
    data = {'HR': torch.from_numpy(g[k + 'hr']).to(d), 'SR': torch.from_numpy(g[k + 'sr']).to(d)}
    kw = {'noise': torch.from_numpy(g[k + 'z']).to(d)}
    if DESCS[name]['variant'] == 'sr3':
        kw['gamma'] = torch.from_numpy(g[k + 'gamma'])
    else:
        kw['t'] = torch.from_numpy(g[k + 't']).to(d)
    return g, k, data, kw


def gradient_mismatches(un, ref_of):
    bad = []
    for key, grad in un.named_gradients():
        ref = ref_of(key)
        got = grad.cpu()
        assert got.shape == ref.shape, key
        num, den = (got - ref).norm().item(), max(ref.norm().item(), 1e-7)
        if num / den > 1e-4 and den > 1e-6:
            bad.append((num / den, key, den))
    return sorted(bad, reverse=True)


@pytest.mark.parametrize('name,H,W,long_attention', CASES, ids=IDS)
def test_loss_and_gradients_match_reference_autograd(name, H, W, long_attention):
    m, _ = build_train(name, long_attention)
    g, k, data, kw = case_data(name, H, W)
    loss = m.netG.p_losses(data, **kw)
    torch.cuda.synchronize()
    ref_loss = float(g[k + 'loss_sum'])
    print('%s %dx%d: loss %.9g, reference %.9g' % (name, H, W, float(loss), ref_loss))
    assert abs(float(loss) - ref_loss) <= 1e-5 * abs(ref_loss), (float(loss), ref_loss)
    bad = gradient_mismatches(m.netG.denoise_fn, lambda key: torch.from_numpy(g[k + 'grad/denoise_fn.' + key]))
    assert not bad, 'gradient mismatch (rel err, key, |ref|): %s' % bad[:8]


def test_long_attention_level_is_refused_without_the_option():
    m, _ = build_train('sr3_tiny')
    g, k, data, kw = case_data('sr3_tiny', 80, 64)
    with pytest.raises(L.Sr3Error) as ei:
        m.netG.p_losses(data, **kw)
    assert '1280 tokens' in str(ei.value) and 'long_attention' in str(ei.value)
    # ... and the model still trains at a size its attention kernels hold
    g, k, data, kw = case_data('sr3_tiny', 16, 24)
    loss = m.netG.p_losses(data, **kw)
    torch.cuda.synchronize()
    assert abs(float(loss) - float(g[k + 'loss_sum'])) <= 1e-5 * abs(float(g[k + 'loss_sum']))


def test_rectangular_training_step_is_bitwise_reproducible():
    m, _ = build_train('sr3_tiny')
    un = m.netG.denoise_fn
    g, k, data, kw = case_data('sr3_tiny', 16, 24)
    m.netG.train()
    outs = []
    for _ in range(3):
        loss = m.netG.p_losses(data, drop_seed=1234, **kw)
        torch.cuda.synchronize()
        outs.append((float(loss), un.grad_arena.clone()))
    assert un.plan.geometry == (16, 24)
    assert any(o['kind'] == 60 for o in un.plan.op_list(2)), 'no attention op in this network: nothing to test'
    for l, ga in outs[1:]:
        assert l == outs[0][0]
        assert torch.equal(ga, outs[0][1]), 'gradient arenas differ between two runs of the same step: max |diff| %.3g' % float((ga - outs[0][1]).abs().max())


def test_native_step_is_unchanged_by_a_rectangular_step_in_between():
    m, _ = build_train('sr3_tiny')
    un = m.netG.denoise_fn
    gn, _ = load_golden('sr3_tiny')
    d = G.dev()
    native = {'HR': torch.from_numpy(gn['loop/hr']).to(d), 'SR': torch.from_numpy(gn['loop/sr']).to(d)}
    nkw = {'noise': torch.from_numpy(gn['train/z']).to(d), 'gamma': torch.from_numpy(gn['train/gamma'])}
    l0 = float(m.netG.p_losses(native, **nkw))
    a0 = un.grad_arena.clone()
    ws0 = un._train_ws.numel()
    # a validation pass at a third size in between, as sr.py runs one every val_freq steps
    m.netG.eval()
    m.netG.show_progress = False
    with torch.no_grad():
        m.netG.super_resolution(torch.zeros(1, 3, 32, 16, device=d))
    m.netG.train()
    g, k, data, kw = case_data('sr3_tiny', 24, 16)
    lr = float(m.netG.p_losses(data, **kw))
    assert abs(lr - float(g[k + 'loss_sum'])) <= 1e-5 * abs(float(g[k + 'loss_sum']))
    assert un._train_ws.numel() >= ws0            # (24 x 16 needs more than 16 x 16: regrown)
    l1 = float(m.netG.p_losses(native, **nkw))
    torch.cuda.synchronize()
    assert abs(l0 - float(gn['train/loss_sum'])) <= 1e-5 * abs(float(gn['train/loss_sum']))
    assert l1 == l0 and torch.equal(un.grad_arena, a0)


def test_optimize_parameters_one_adam_step_rectangular():
    """feed_data -> optimize_parameters (RNG draws patched to the recorded ones) -> weights after Adam, at 16 x 24."""
    name = 'sr3_tiny'
    m, sd = build_train(name)
    g, k, data, kw = case_data(name, 16, 24)
    netG = m.netG
    orig = netG.p_losses
    netG.p_losses = lambda x_in, noise=None: orig(x_in, **kw)
    m.feed_data({'HR': data['HR'].cpu(), 'SR': data['SR'].cpu()})
    m.optimize_parameters()
    assert abs(m.get_current_log()['l_pix'] - float(g[k + 'l_pix'])) <= 1e-5 * abs(float(g[k + 'l_pix']))
    out = netG.state_dict()
    tot = bad = 0
    for key in g:
        if not key.startswith(k + 'adam1/'):
            continue
        name_ = key[len(k + 'adam1/'):]
        ref_new = torch.from_numpy(g[key])
        old = sd[name_]
        grad = torch.from_numpy(g[k + 'grad/' + name_])
        mask = grad.abs() > 1e-6 * max(grad.abs().max().item(), 1e-12) + 1e-9
        upd = (out[name_].cpu() - old)[mask]
        ref_upd = (ref_new - old)[mask]
        tot += mask.sum().item()
        bad += ((upd - ref_upd).abs() > 2e-6).sum().item()
    assert tot > 1000 and bad <= 1e-4 * tot, (bad, tot)


def test_dropout_training_step_matches_oracle_autograd_rectangular():
    from oracle import sr3_oracle as O
    name = 'sr3_tiny'
    m, sd = build_train(name, dropout=0.2)
    m.netG.train()
    g, k, data, kw = case_data(name, 16, 24)
    seed = 987654321
    loss = m.netG.p_losses(data, drop_seed=seed, **kw)
    torch.cuda.synchronize()
    sdr = {n: v.clone().requires_grad_(v.is_floating_point() and n.startswith('denoise_fn.')) for n, v in sd.items()}
    hr, sr = data['HR'].cpu(), data['SR'].cpu()
    ref_loss = O.p_losses_sr3(sdr, DESCS[name], hr, sr, kw['gamma'], kw['noise'].cpu(), conditional=True, dropout=(0.2, seed))
    (ref_loss / hr.numel()).backward()
    ref_loss = float(ref_loss.detach())
    assert abs(float(loss) - ref_loss) <= 1e-5 * abs(ref_loss), (float(loss), ref_loss)
    nodrop = float(g[k + 'loss_sum'])
    assert abs(float(loss) - nodrop) > 1e-3 * nodrop          # the mask really changed the forward
    bad = gradient_mismatches(m.netG.denoise_fn, lambda key: sdr['denoise_fn.' + key].grad)
    assert not bad, bad[:8]


# the 9-tap weight-gradient kernel (k_conv_wgrad9) off the power-of-two maps: chunk = 32 / Wc rows x Wc columns
WGRAD9_MAPS = [(8, 24), (16, 48), (12, 40), (16, 96)]          # Wc 8, 16, 8 (H % 4 == 0), 32
WGRAD9_CHANNELS = [(64, 64), (64, 4), (8, 64)]                # (Cin, Cout)


@pytest.mark.parametrize('cin,cout', WGRAD9_CHANNELS, ids=['%dto%d' % c for c in WGRAD9_CHANNELS])
@pytest.mark.parametrize('H,W', WGRAD9_MAPS, ids=['%dx%d' % s for s in WGRAD9_MAPS])
def test_weight_gradient_on_non_power_of_two_maps(H, W, cin, cout):
    """sr3_conv_wgrad_f32 on 3x3 stride-1 layers against float64 autograd of F.conv2d; inputs drawn as tests/test_gpu_ops.py draws
    them (standard normal: every one of the B * H * W >= 384 terms of a sum has the same scale, so the reference is well conditioned)."""
    import torch.nn.functional as F
    B = 2
    lib, d = L.load(), G.dev()
    gen = lambda *shape, seed: torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    x = gen(B, cin, H, W, seed=31)
    dy = gen(B, cout, H, W, seed=35)
    w = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, None, stride=1, padding=1).backward(dy.double())
    ref = w.grad
    xd, dyd = G.nhwc(x).to(d), G.nhwc(dy).to(d)
    nb = int(lib.sr3_conv_wgrad_scratch_bytes(B, H, W, 0, 1, 3, cin, 0, cout, 1))
    # the layer runs on the 9-tap kernel, not on the one-tap fallback: its pixel split is that kernel's row of wgrad_pick (csrc/wgrad.hip:
    # 512 workgroups aimed at, at least two 32-pixel chunks per split; the fallback's rule gives half as many splits on these shapes)
    tiles, nchunks = -(-cout // 64) * -(-cin // 64), B * H * W // 32
    per = -(-nchunks // min(-(-512 // tiles), max(nchunks // 2, 1)))
    assert nb == -(-nchunks // per) * cout * 9 * cin * 4, (nb, nchunks, per)
    scratch = torch.empty(max(nb, 16), dtype=torch.uint8, device=d)
    dw = torch.full((cout, 9, cin), float('nan'), device=d)
    L.check(lib.sr3_conv_wgrad_f32(L.ptr(xd), cin, None, 0, B, H, W, 0, 1, 3, cout, None, 0, L.ptr(dyd), L.ptr(dw), 1,
                                   L.ptr(scratch), nb, G.stream()))
    torch.cuda.synchronize()
    got = dw.cpu().view(cout, 3, 3, cin).permute(0, 3, 1, 2).double()
    e = (got - ref).norm().item() / ref.norm().item()
    print('%dx%d %d->%d: weight-gradient rel err vs float64 %.2e' % (H, W, cin, cout, e))
    assert e < 2e-6, (H, W, cin, cout, e)
