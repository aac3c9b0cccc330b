"""Scale-shift time conditioning through whole networks (config key model.unet.scale_shift_norm): forward against the CPU oracle with
its resnet_block replaced by tests/adagn_ref.py's (unet_forward resolves resnet_block as a module global, so a monkeypatch gives the
whole-UNet reference), plan option fold_fuse 0 against 1 bit for bit, the captured reverse step against the eager one, and training
steps against float64 autograd through the same patched oracle -- with dropout against the oracle's mask, and with two attention heads.

The networks are those of tests/test_gpu_attn_heads_unet.py: sr3_tiny / ddpm_tiny widened to inner_channel 32 (SR3: channel_mults
[1, 2, 4], attn_res [8], one res block per level), image 16, batch 2.  The FiLM projections are scaled up by 4 after the default
initialisation, so that the scale rows move the output by far more than the tolerance (asserted)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_util as G                      # noqa: E402
import adagn_ref                          # noqa: E402
import mha_ref                            # noqa: E402
from helpers import opt_for               # noqa: E402
from oracle import sr3_oracle as O        # noqa: E402

FILM = {'sr3': '.noise_func.noise_func.0.', 'ddpm': '.mlp.1.'}
B = 2


def _opt(base, phase, dropout=0, **extra):
    opt = copy.deepcopy(opt_for(base, phase=phase, gpu=True))
    u = opt['model']['unet']
    u.update(inner_channel=32, norm_groups=32, scale_shift_norm=True, dropout=dropout, **extra)
    if base == 'sr3_tiny':
        u.update(channel_multiplier=[1, 2, 4], attn_res=[8], res_blocks=1)
    return opt


def _net(base, phase='val', seed=21, ssn=True, **kw):
    import model.networks as networks
    opt = _opt(base, phase, **kw)
    if not ssn:
        del opt['model']['unet']['scale_shift_norm']
    netG = networks.define_G(opt)
    un = netG.denoise_fn
    torch.manual_seed(seed)
    un.reset_parameters()
    film = FILM[un.variant]
    for name, p in un.named_parameters():          # (views of the arena: writes go through)
        if film in name:
            p.mul_(4.0)
    sd = {k: v.clone() for k, v in netG.state_dict().items()}
    d = G.dev()
    netG = netG.to(d)
    netG.set_loss(d)
    netG.set_new_noise_schedule(opt['model']['beta_schedule'][phase], d)
    netG.show_progress = False
    return netG, sd, O.desc_from_opt(opt), opt


def _inputs(desc):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, desc['in_channel'], 16, 16, generator=g)
    lvl = torch.tensor([3, 1][:B], dtype=torch.long) if desc['variant'] == 'ddpm' else torch.linspace(0.2, 0.95, B).view(B, 1)
    return x, lvl


def _without_scale_rows(sd, variant):
    """the state dict with every block's scale rows -- the first half of the projection's weight and bias -- zeroed: GN2(h) + shift"""
    out = {k: v.clone() for k, v in sd.items()}
    for k, v in out.items():
        if FILM[variant] in k:
            v[:v.shape[0] // 2] = 0
    return out


@pytest.mark.parametrize('base', ['sr3_tiny', 'ddpm_tiny'])
def test_forward_against_the_scale_shift_oracle(monkeypatch, base):
    d = G.dev()
    netG, sd, desc, opt = _net(base)
    x, lvl = _inputs(desc)
    un = netG.denoise_fn
    got = un(x.to(d), lvl.to(d)).cpu()
    folds = un.plan.fold_list(B)
    kinds = {kind for kind, row in folds if row >= 0}
    n_blocks = sum(1 for e in un.plan.table if e['name'].endswith('.res_block.block1.block.3.weight'))
    assert sum(1 for _, row in folds if row >= 0) == n_blocks
    if base == 'sr3_tiny':          # a fold launch of its own AND a fold in the reduce of a split-K conv are both on this list
        ops = un.plan.op_list(B)
        assert 1 in kinds and any(kind == 2 and row >= 0 and ops[i]['kind'] == 50 and ops[i]['ksplit'] > 1 for i, (kind, row) in enumerate(folds)), folds
    monkeypatch.setattr(O, 'resnet_block', adagn_ref.resnet_block)
    with torch.no_grad():
        ref = O.unet_forward(sd, desc, x, lvl)
        shift_only = O.unet_forward(_without_scale_rows(sd, desc['variant']), desc, x, lvl)
    err = G.assert_close(got, ref, what='%s scale-shift eps' % base)
    tol = 2e-5 * max(1.0, ref.abs().max().item())
    gap = (ref - shift_only).abs().max().item()
    print('%s: eps max abs err %.2e (tolerance %.2e); the oracle without the scale rows differs by %.2e' % (base, err, tol, gap))
    assert gap > tol, 'the scale rows do not show in this network: the comparison proves nothing'


def _raw_calls(netG, sd_unused, desc, fold_fuse, fuse_stats=1):
    """forward eps, one reverse step and one training step (dropout 0.1) of a fresh plan under the options -> tensors to compare bitwise"""
    d = G.dev()
    un = netG.denoise_fn
    un.plan.set_option('fold_fuse', fold_fuse)
    un.plan.set_option('fuse_stats', fuse_stats)
    x, lvl = _inputs(desc)
    out = {'eps': un(x.to(d), lvl.to(d)).clone()}
    g = torch.Generator().manual_seed(12)
    hr, sr, z = (torch.rand(B, 3, 16, 16, generator=g) * 2 - 1 for _ in range(3))
    netG.train()
    un.dropout = 0.1
    loss = netG.p_losses({'HR': hr.to(d), 'SR': sr.to(d)}, noise=z.to(d), gamma=torch.tensor([0.35, 0.85]), drop_seed=20241021)
    torch.cuda.synchronize()
    out['loss'], out['grads'] = loss.clone(), un.grad_arena.clone()
    netG.eval()
    return out, un.plan.fold_list(B)


@pytest.mark.parametrize('fuse_stats', [1, 0])
def test_fold_fuse_0_and_1_give_the_same_bits(fuse_stats):
    """As the additive network's recorded bits are the same under fold_fuse 0 and 1 (tests/golden/plan_run_bits.json), so are this
    network's: the pairs the fused folds write -- in a split-K conv's reduce, and (fuse_stats 0) in the stand-alone statistics pass --
    are sr3_groupnorm_fold_mod_f32's bit for bit, in the inference forward and in the training step."""
    netG, sd, desc, opt = _net('sr3_tiny', phase='train')
    fused, folds1 = _raw_calls(netG, sd, desc, 1, fuse_stats)
    plain, folds0 = _raw_calls(netG, sd, desc, 0, fuse_stats)
    assert {kind for kind, row in folds0 if row >= 0} == {1}
    want = 2 if fuse_stats else 3
    assert any(kind == want and row >= 0 for kind, row in folds1), folds1
    for k in fused:
        assert torch.equal(fused[k], plain[k]), k
    assert bool(torch.isfinite(fused['grads']).all())


def test_three_captured_reverse_steps_equal_the_eager_ones():
    d = G.dev()
    netG, sd, desc, opt = _net('sr3_tiny')
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


def test_fork_side_joins_the_embed_op_before_the_first_modulated_fold():
    """plan option fork_side: the embed op runs on the side stream beside the input conv; the forward's bits are those of one stream."""
    d = G.dev()
    netG, sd, desc, opt = _net('sr3_tiny')
    x, lvl = _inputs(desc)
    un = netG.denoise_fn
    one = un(x.to(d), lvl.to(d)).clone()
    un.plan.set_option('fork_side', 1)
    ops = un.plan.op_list(B)
    assert ops[0].get('side_id', -1) >= 0 and any(o.get('wait_id', -1) == ops[0]['side_id'] for o in ops)
    for _ in range(3):
        assert torch.equal(un(x.to(d), lvl.to(d)), one)


def _train_against_autograd(monkeypatch, base, dropout=0.0, **extra):
    d = G.dev()
    netG, sd, desc, opt = _net(base, phase='train', dropout=dropout, **extra)
    g = torch.Generator().manual_seed(9)
    hr = torch.rand(B, 3, 16, 16, generator=g) * 2 - 1
    sr = torch.rand(B, 3, 16, 16, generator=g) * 2 - 1
    z = torch.randn(B, 3, 16, 16, generator=g)
    gamma, t = torch.tensor([0.35, 0.85]), torch.tensor([4, 1], dtype=torch.long)
    un = netG.denoise_fn
    assert un.dropout == dropout
    netG.train()
    sr3 = desc['variant'] == 'sr3'
    step = dict(gamma=gamma) if sr3 else dict(t=t.to(d))
    seed = 77
    runs = []
    for _ in range(2):
        loss = netG.p_losses({'HR': hr.to(d), 'SR': sr.to(d)}, noise=z.to(d), drop_seed=seed, **step)
        torch.cuda.synchronize()
        runs.append((float(loss), un.grad_arena.clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]), 'two runs of the training step differ'
    monkeypatch.setattr(O, 'resnet_block', adagn_ref.resnet_block)
    if 'n_head' in extra:
        monkeypatch.setattr(O, 'self_attention', mha_ref.patched(n_head=extra['n_head']))
    sdr = {k: (v.double().clone().requires_grad_(k.startswith('denoise_fn.')) if v.is_floating_point() else v) for k, v in sd.items()}
    drop = (dropout, seed) if dropout else None
    if sr3:
        ref_loss = O.p_losses_sr3(sdr, desc, hr.double(), sr.double(), gamma.double(), z.double(), conditional=True, dropout=drop)
    else:
        tab = O.schedule_tables(opt['model']['beta_schedule']['train'])
        ref_loss = O.p_losses_ddpm(sdr, desc, tab, hr.double(), sr.double(), t, z.double(), conditional=False, dropout=drop)
    (ref_loss / hr.numel()).backward()
    ref_loss = float(ref_loss.detach())
    assert abs(runs[0][0] - ref_loss) <= 1e-5 * abs(ref_loss), (runs[0][0], ref_loss)
    rows = []
    for key, grad in un.named_gradients():
        ref = sdr['denoise_fn.' + key].grad
        den = max(ref.norm().item(), 1e-7)
        rows.append(((grad.cpu().double() - ref).norm().item() / den, key, den))
    rows.sort(reverse=True)
    film = [r for r in rows if FILM[desc['variant']] in r[1]]
    print('%s dropout %g %s: loss %.6f (float64 %.6f); worst gradients (rel err, key, |ref|): %s; worst projection: %s'
          % (base, dropout, extra, runs[0][0], ref_loss, rows[:4], film[:2]))
    assert film and all(r[2] > 1e-6 for r in film), 'a projection has no gradient to compare'
    bad = [r for r in rows if r[0] > 1e-4 and r[2] > 1e-6]
    assert not bad, bad[:8]
    return runs[0][0]


@pytest.mark.parametrize('base', ['sr3_tiny', 'ddpm_tiny'])
def test_training_step_against_float64_autograd(monkeypatch, base):
    _train_against_autograd(monkeypatch, base)


def test_training_step_with_dropout_against_the_oracles_mask(monkeypatch):
    """dropout 0.2: the oracle keys a block's mask by the cumulative Cout of the blocks in front of it -- the key did not move to an
    offset into the widened table."""
    dropped = _train_against_autograd(monkeypatch, 'sr3_tiny', dropout=0.2)
    monkeypatch.undo()
    plain = _train_against_autograd(monkeypatch, 'sr3_tiny')
    assert abs(dropped - plain) > 1e-3 * abs(plain), 'the mask did not change the forward'


def test_two_heads_with_the_flag(monkeypatch):
    d = G.dev()
    netG, sd, desc, opt = _net('sr3_tiny', n_head=2)
    x, lvl = _inputs(desc)
    got = netG.denoise_fn(x.to(d), lvl.to(d)).cpu()
    monkeypatch.setattr(O, 'resnet_block', adagn_ref.resnet_block)
    with torch.no_grad():
        one = O.unet_forward(sd, desc, x, lvl)
        monkeypatch.setattr(O, 'self_attention', mha_ref.patched(n_head=2))
        ref = O.unet_forward(sd, desc, x, lvl)
    G.assert_close(got, ref, what='two heads, scale-shift eps')
    assert (ref - one).abs().max().item() > 2e-5 * max(1.0, ref.abs().max().item())
    _train_against_autograd(monkeypatch, 'sr3_tiny', n_head=2)


@pytest.mark.parametrize('base', ['sr3_tiny', 'ddpm_tiny'])
def test_exact_size_workspaces_with_the_flag(base):
    """The workspace contract (tests/test_gpu_workspace_contract.py, tests/guarded.py) with the flag set: sr3_unet_forward and
    sr3_train_step_ex in guarded buffers of exactly sr3_workspace_bytes / sr3_train_workspace_bytes, filled with NaN patterns and then
    with zeros -- every band intact, the results finite and bit-equal across the fills."""
    import ctypes as C
    from guarded import Guarded, N, Z, TENSOR_BAND
    from sr3_hip import lib as L
    d = G.dev()
    netG, sd, desc, opt = _net(base, phase='train')
    un = netG.denoise_fn
    plan, lib = un.plan, un.plan.lib
    un.ensure_derived()
    sr3 = desc['variant'] == 'sr3'
    cc = 3 if sr3 else 0
    g = torch.Generator().manual_seed(15)
    hr, cond, z, x = (torch.rand(B, 3, 16, 16, generator=g).to(d) * 2 - 1 for _ in range(4))
    lvl = torch.tensor([0.35, 0.85], device=d)
    tstep = torch.tensor([4, 1], dtype=torch.long, device=d)
    ca, cb = lvl.clone(), (1 - lvl ** 2).sqrt()
    params, freq = un.arena.data, un.freq
    need, tneed = plan.workspace_bytes(B), int(lib.sr3_train_workspace_bytes(plan.handle, B, cc))
    assert tneed > 0, lib.sr3_last_error()
    results = []
    for fill in (N, Z):
        ws, tws = Guarded(need, fill, d), Guarded(tneed, fill, d)
        eps = torch.full((B, 3, 16, 16), float('nan'), device=d)
        L.check(lib.sr3_unet_forward(plan.handle, L.ptr(x), L.ptr(cond) if sr3 else None, cc, L.ptr(lvl) if sr3 else None,
                                     None if sr3 else L.ptr(tstep), L.ptr(freq), None, None, L.ptr(params), ws.ptr, need, L.ptr(eps), B, G.stream()))
        gg = Guarded(plan.param_floats * 4, fill, d, TENSOR_BAND)
        loss = torch.full((1,), float('nan'), device=d)
        L.check(lib.sr3_train_step_ex(plan.handle, L.ptr(hr), L.ptr(cond) if sr3 else None, cc, L.ptr(z), L.ptr(ca), L.ptr(cb), L.ptr(lvl) if sr3 else None,
                                      None if sr3 else L.ptr(tstep), L.ptr(freq), L.ptr(params), gg.ptr, tws.ptr, tneed, L.ptr(loss),
                                      C.c_float(1.0 / (B * 3 * 16 * 16)), C.c_float(0.1), C.c_uint(4242), 0, None, None, B, None, None, None, -1,
                                      C.c_float(0.0), G.stream()))
        torch.cuda.synchronize()
        assert ws.intact() and tws.intact() and gg.intact(), 'a call wrote outside its exact-size buffer'
        grads = gg.view(torch.float32).clone()
        is_param = torch.zeros(plan.param_floats, dtype=torch.bool, device=d)
        for e in plan.table:
            is_param[e['offset']:e['offset'] + e['numel']] = True
        assert bool(torch.isfinite(eps).all()) and bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grads[is_param]).all())
        results.append((eps, loss, grads[is_param]))
    for a, b in zip(*results):
        assert torch.equal(a, b), 'the result depends on what the workspace held'
