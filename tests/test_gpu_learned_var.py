"""Learned reverse-process variance on the GPU: the output conv at 6 and 8 rows, a learned-variance checkpoint under the fused step,
the hybrid loss kernel, the whole training step against float64 autograd, the tail kernel, and a ten-step ancestral chain.

Tolerances.  The project's where an existing test pins one for the same code: the output conv 2e-5 * max(1, |ref|)
(test_gpu_ops.py), the training step's loss rel 1e-5 and gradients normwise rel 1e-4 (test_gpu_train.py), a chain 1e-4
(test_gpu_sampler.py).  The loss kernel's variance lanes and sums and the tail's sigma z are new arithmetic (exp / tanh / log in fp32,
a difference of two CDFs): their bounds are 4 x the worst error of the same formulas evaluated in fp32 NumPy against float64 on these
very inputs, on the CPU (learned_var_ref.vlb_f32 / sigma_f32) -- the device's exp / tanh / log differ from NumPy's by
a few ulp, and the cancellation in the CDF difference amplifies that:

    d vlb / d v     measured 1.636e-06 (scaled by max(1, |ref|))      -> TOL_DV   = 6.6e-06
    loss, vlb sums  measured 1.114e-07 (relative)                     -> TOL_SUM  = 4.5e-07
    one tail step   measured 1.190e-07 (scaled by max(1, |ref|_inf))  -> TOL_STEP = 4.8e-07"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import DESCS, SCHEDS, CONDITIONAL, opt_for      # noqa: E402
import gpu_util as G                                          # noqa: E402
import learned_var_ref as R                                   # noqa: E402
from test_learned_var_cpu import loss_inputs, _ac             # noqa: E402

from sr3_hip import lib as L                                  # noqa: E402

TOL_DV, TOL_SUM, TOL_STEP = 6.6e-6, 4.5e-7, 4.8e-7
KW, KB = 'denoise_fn.final_conv.block.3.weight', 'denoise_fn.final_conv.block.3.bias'
CHAIN_SCHED = dict(schedule='linear', n_timestep=20, linear_start=1e-6, linear_end=1e-2)


def build6(name, phase='val', lam=0.001, sched=None, sampler=None, seed=1234):
    """The tiny net `name` with out_channel 6 under the key, weights random and seeded; -> (model, its state dict on the CPU)."""
    import model as Model
    opt = opt_for(name, phase=phase, gpu=True)
    opt['model']['unet']['out_channel'] = 6
    opt['model']['diffusion']['learned_variance'] = {'lambda': lam}
    if sched is not None:
        opt['model']['beta_schedule'] = {'train': dict(sched), 'val': dict(sched)}
    if sampler is not None:
        opt['model']['beta_schedule']['val']['sampler'] = sampler
    torch.manual_seed(seed)
    m = Model.create_model(opt)
    gen = torch.Generator().manual_seed(seed + 1)
    sd = {k: v.cpu() for k, v in m.netG.state_dict().items()}
    for k, v in sd.items():          # (the train phase's orthogonal init zeroes every bias, the default init leaves FiLM small: seeded values)
        if k.startswith('denoise_fn.') and v.dim() == 1 and '.block.0.' not in k and '.norm.' not in k and v.is_floating_point() and 'inv_freq' not in k:
            sd[k] = torch.randn(v.shape, generator=gen) * 0.1
    m.netG.load_state_dict(sd, strict=True)
    m.netG.show_progress = False
    if phase == 'val':                 # (the constructor applies the train schedule; the phase's own carries the sampler block)
        m.set_new_noise_schedule(opt['model']['beta_schedule']['val'], schedule_phase='val')
    return m, sd


def build3(name, sd6, phase='val', sched=None, sampler=None):
    """The 3-row network made of the first three filter rows of `sd6`."""
    import model as Model
    opt = opt_for(name, phase=phase, gpu=True)
    if sched is not None:
        opt['model']['beta_schedule'] = {'train': dict(sched), 'val': dict(sched)}
    if sampler is not None:
        opt['model']['beta_schedule']['val']['sampler'] = sampler
    m = Model.create_model(opt)
    sd3 = dict(sd6)
    sd3[KW], sd3[KB] = sd6[KW][:3].contiguous(), sd6[KB][:3].contiguous()
    m.netG.load_state_dict(sd3, strict=True)
    m.netG.show_progress = False
    if phase == 'val':
        m.set_new_noise_schedule(opt['model']['beta_schedule']['val'], schedule_phase='val')
    return m, sd3


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- 1. output conv -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('Cc', [8, 32])                      # 8: the not-FULL instantiation, 32: FULL
@pytest.mark.parametrize('H,W', [(16, 16), (16, 48)])        # 48: a ragged 32-wide tile column plus a second tile
@pytest.mark.parametrize('Cout', [6, 8])
def test_conv_out_six_and_eight_rows(Cout, H, W, Cc):
    lib, d, B = L.load(), G.dev(), 3
    x = _rand(B, Cc, H, W, seed=1)
    ss = torch.stack([_rand(B, Cc, seed=2) * 0.3 + 1.0, _rand(B, Cc, seed=3) * 0.3], dim=2).contiguous()
    w = _rand(Cout, Cc, 3, 3, seed=4) * 0.1
    bias = _rand(Cout, seed=5)
    out = torch.full((B, Cout, H, W), float('nan'), device=d)
    xd, ssd, wd, biasd = G.nhwc(x).to(d), ss.to(d), G.ohwi(w).to(d), bias.to(d)
    L.check(lib.sr3_conv_out_f32(L.ptr(xd), L.ptr(ssd), B, H, W, Cc, L.ptr(wd), L.ptr(biasd), Cout, L.ptr(out), G.stream()))
    torch.cuda.synchronize()
    G.assert_close(out.cpu(), G.conv_ref(x, None, w, bias=bias, ss=ss, act=2), what='conv_out Cout %d' % Cout)
    # the first three rows of the same filters are the 3-row conv, bit for bit (what every existing sampler launches)
    out3 = torch.full((B, 3, H, W), float('nan'), device=d)
    L.check(lib.sr3_conv_out_f32(L.ptr(xd), L.ptr(ssd), B, H, W, Cc, L.ptr(wd), L.ptr(biasd), 3, L.ptr(out3), G.stream()))
    torch.cuda.synchronize()
    assert torch.equal(out3, out[:, :3])


@pytest.mark.parametrize('Cout', [5, 7, 9])
def test_conv_out_other_row_counts_stay_refused(Cout):
    lib, d = L.load(), G.dev()
    t = torch.zeros(4096, device=d)
    rc = lib.sr3_conv_out_f32(L.ptr(t), L.ptr(t), 1, 8, 8, 8, L.ptr(t), L.ptr(t), Cout, L.ptr(t), G.stream())
    assert rc == -2 and ('conv_out: Cout %d > 4 unsupported' % Cout) in lib.sr3_last_error().decode()


@pytest.mark.parametrize('name', ['sr3_tiny', 'sr3_seam', 'ddpm_tiny'])
def test_fused_step_on_a_learned_variance_checkpoint_is_the_three_row_step(name):
    m6, sd6 = build6(name, sampler={'type': 'ddim', 'steps': 4, 'eta': 0.5})
    m3, _ = build3(name, sd6, sampler={'type': 'ddim', 'steps': 4, 'eta': 0.5})
    d = G.dev()
    B, H = 2, 16
    x, z = _rand(B, 3, H, H, seed=6).to(d), _rand(B, 3, H, H, seed=7).to(d)
    cond = _rand(B, 3, H, H, seed=8).to(d) if CONDITIONAL[name] else None
    outs = []
    for m in (m6, m3):
        netG, un = m.netG, m.netG.denoise_fn
        tables, level, t_map, c3, noisy = netG._step_rule()
        step2 = torch.tensor([-7, 2], dtype=torch.int32, device=d)
        xs, eps = x.clone(), torch.full_like(x, float('nan'))
        un.reverse_step(xs, z, tables, step2, cond=cond, level_table=level, eps_out=eps, t_map=t_map)
        torch.cuda.synchronize()
        assert step2.tolist() == [2, 1] and bool(torch.isfinite(xs).all())
        outs.append((xs, eps))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # the forward: the prediction rows alone by default, all six on request -- the same first three
    time = torch.full((B,), 0.7, device=d) if DESCS[name]['variant'] == 'sr3' else torch.tensor([1, 3], device=d)
    e3 = m3.netG.denoise_fn(x, time, cond=cond)
    e6 = m6.netG.denoise_fn(x, time, cond=cond)
    full = m6.netG.denoise_fn(x, time, cond=cond, full=True)
    assert tuple(e6.shape) == (B, 3, H, H) and tuple(full.shape) == (B, 6, H, H)
    assert torch.equal(e6, e3) and torch.equal(full[:, :3], e3) and float(full[:, 3:].abs().max()) > 0.0
    from oracle import sr3_oracle as O
    inp = x.cpu() if cond is None else torch.cat([cond.cpu(), x.cpu()], 1)
    tt = time.cpu().view(-1, 1) if DESCS[name]['variant'] == 'sr3' else time.cpu()
    with torch.no_grad():
        ref = O.unet_forward(sd6, dict(DESCS[name], out_channel=6), inp, tt)
    G.assert_close(full.cpu(), ref, what='%s six-row forward' % name)


# ---- 2. the loss kernel ---------------------------------------------------------------------------------------------------------------

def _hybrid_call(d, lam, scale, kind, delta, tgt):
    lib, dev = L.load(), G.dev()
    B, C2, H, W = d['out'].shape
    C_, HW = C2 // 2, H * W
    g8 = torch.full((B, HW, 8), float('nan'), device=dev)
    loss, vlb = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    scratch = torch.empty(int(lib.sr3_hybrid_loss_grad_scratch_bytes()), dtype=torch.uint8, device=dev)
    t = {k: d[k].to(dev).contiguous() for k in ('z', 'out', 'hr', 'xt', 'scal32')}
    L.check(lib.sr3_hybrid_loss_grad_f32(L.ptr(t['z']), L.ptr(t['out']), L.ptr(t['hr']), L.ptr(t['xt']), *[L.ptr(v) for v in tgt],
                                         L.ptr(t['scal32']), C.c_float(lam), B, C_, HW, kind, C.c_float(delta), C.c_float(scale),
                                         L.ptr(g8), L.ptr(loss), L.ptr(vlb), L.ptr(scratch), G.stream()))
    torch.cuda.synchronize()
    return g8, loss, vlb


@pytest.mark.parametrize('kind,tables', [(0, False), (1, True), (2, True)])
def test_hybrid_loss_kernel(kind, tables):
    lib, dev = L.load(), G.dev()
    d = loss_inputs()
    B, C_, HW = 4, 3, 256
    assert d['scal'][:, 6].tolist() == [1.0, 1.0, 0.0, 0.0] and bool((d['hr'].abs() > 0.999).any())
    assert float(d['out'][:, 3:].min()) < -1.4 and float(d['out'][:, 3:].max()) > 1.4
    lam, scale, delta = 0.5, 0.125, 0.7                    # (powers of two: the scaling of the lanes is exact)
    tg = None
    tgt = (None, None, None)
    if tables:
        tg = (torch.tensor([0.9, 0.5, 1.0, 0.2]), torch.tensor([-0.3, 0.8, 0.0, 0.9]), torch.tensor([1.0, 0.25, 2.0, 0.5]))
        tgt = tuple(t.to(dev) for t in tg)
    g8, loss, vlb = _hybrid_call(d, lam, scale, kind, delta, tgt)
    # prediction lanes: sr3_loss_grad_f32 on the same inputs, bit for bit
    g4 = torch.full((B, HW, 4), float('nan'), device=dev)
    l4 = torch.zeros(1, device=dev)
    scr = torch.empty(int(lib.sr3_loss_grad_scratch_bytes()), dtype=torch.uint8, device=dev)
    pred, zd, hrd = d['out'][:, :3].contiguous().to(dev), d['z'].to(dev), d['hr'].to(dev)
    L.check(lib.sr3_loss_grad_f32(L.ptr(zd), L.ptr(pred), L.ptr(hrd), *[L.ptr(v) for v in tgt], B, C_, HW, kind,
                                  C.c_float(delta), C.c_float(scale), L.ptr(g4), L.ptr(l4), L.ptr(scr), G.stream()))
    torch.cuda.synchronize()
    assert torch.equal(g8[:, :, :3], g4[:, :, :3]) and not g8[:, :, 6:].any() and bool(torch.isfinite(g8).all())
    # variance lanes and the sums against the float64 reference
    out = d['out'].double().clone().requires_grad_(True)
    tot, vsum = R.hybrid_loss(d['z'], d['hr'], d['xt'], out, d['scal32'].double(), lam, kind=('l1', 'l2', 'huber')[kind], delta=delta,
                              tgt=None if tg is None else tg[:2], weight=None if tg is None else tg[2])
    gref, = torch.autograd.grad(vsum, [out])
    dv_ref = gref[:, 3:].reshape(B, C_, HW).permute(0, 2, 1)                  # d vlb / d v, [B, HW, C]
    dv = g8[:, :, 3:6].cpu().double() / (lam * scale)
    err = ((dv - dv_ref).abs() / dv_ref.abs().clamp(min=1.0)).max().item()
    tot, vsum = float(tot.detach()), float(vsum.detach())
    e_tot = abs(float(loss) - tot) / abs(tot)
    e_vlb = abs(float(vlb) - vsum) / abs(vsum)
    print('kind %d: d vlb / d v err %.3e (max |ref| %.3g), loss rel %.3e, vlb rel %.3e' % (kind, err, float(dv_ref.abs().max()), e_tot, e_vlb))
    assert float(dv_ref.abs().max()) > 1e-2
    assert err <= TOL_DV, err
    assert e_tot <= TOL_SUM and e_vlb <= TOL_SUM, (e_tot, e_vlb)
    # the same bits every run
    g8b, lossb, vlbb = _hybrid_call(d, lam, scale, kind, delta, tgt)
    assert torch.equal(g8, g8b) and torch.equal(loss, lossb) and torch.equal(vlb, vlbb)
    # lambda = 0: the variance lanes are exactly zero and the loss is the pixel loss's
    g0, loss0, _ = _hybrid_call(d, 0.0, scale, kind, delta, tgt)
    assert not g0[:, :, 3:].any() and torch.equal(g0[:, :, :3], g4[:, :, :3])
    assert abs(float(loss0) - float(l4)) <= 1.2e-7 * abs(float(l4))      # (the same terms; the plain L1 / L2 kernel adds them in another order)


def test_hybrid_loss_refusals():
    lib, dev = L.load(), G.dev()
    t = torch.zeros(4096, device=dev)
    args = lambda **kw: [kw.get('z', L.ptr(t)), L.ptr(t), L.ptr(t), kw.get('xt', L.ptr(t)), None, None, None, kw.get('scal', L.ptr(t)),
                         C.c_float(kw.get('lam', 0.1)), 1, kw.get('ch', 3), 16, 0, C.c_float(1.0), C.c_float(1.0), L.ptr(t), L.ptr(t), None,
                         L.ptr(t), G.stream()]
    for kw, code, text in ((dict(scal=None), -1, 'is NULL'), (dict(xt=None), -1, 'is NULL'), (dict(lam=-1.0), -1, 'vlb_lambda'),
                           (dict(lam=float('nan')), -1, 'vlb_lambda'), (dict(ch=5), -1, 'channels 5 is outside 1..4')):
        assert lib.sr3_hybrid_loss_grad_f32(*args(**kw)) == code and text in lib.sr3_last_error().decode(), kw


# ---- 3. the whole training step -------------------------------------------------------------------------------------------------------

def _train_inputs(name, B, H, W):
    hr = (_rand(B, 3, H, W, seed=31) * 0.5).clamp(-1, 1)
    sr = (_rand(B, 3, H, W, seed=32) * 0.5).clamp(-1, 1)
    z = _rand(B, 3, H, W, seed=33)
    return hr, sr, z


def _ref_step(name, sd, hr, sr, z, ca, cb, time, scal, lam):
    """float64 autograd of the oracle's UNet + the reference loss (L1, sum-reduced) -> (loss, vlb sum, {key: d(loss / numel)})."""
    from oracle import sr3_oracle as O
    sdr = {k: (v.double().clone().requires_grad_(k.startswith('denoise_fn.') and 'inv_freq' not in k) if v.is_floating_point() else v)
           for k, v in sd.items()}
    hr, sr, z = hr.double(), sr.double(), z.double()
    xt = ca.double().view(-1, 1, 1, 1) * hr + cb.double().view(-1, 1, 1, 1) * z
    inp = torch.cat([sr, xt], 1) if CONDITIONAL[name] else xt
    out = O.unet_forward(sdr, dict(DESCS[name], out_channel=6), inp, time)
    tot, vlb = R.hybrid_loss(z, hr, xt, out, scal, lam, kind='l1')
    params = {k: v for k, v in sdr.items() if v.is_floating_point() and v.requires_grad}
    grads = torch.autograd.grad(tot / hr.numel(), list(params.values()))
    with torch.no_grad():
        cond = R.nll_conditioning(hr, xt, out[:, :3], out[:, 3:], scal)
    return float(tot.detach()), float(vlb.detach()), {k[len('denoise_fn.'):]: g for k, g in zip(params, grads)}, cond


@pytest.mark.parametrize('name,H,W,t', [('sr3_tiny', 16, 16, 1), ('sr3_tiny', 16, 32, 5), ('ddpm_tiny', 16, 16, (0, 4)), ('ddpm_tiny', 16, 32, (3, 0))])
def test_training_step_matches_float64_autograd(name, H, W, t):
    lam = 0.05                                               # (large enough that the variance rows' gradient is well above rounding)
    m6, sd6 = build6(name, phase='train', lam=lam)
    d = G.dev()
    netG, un = m6.netG, m6.netG.denoise_fn
    B = 2
    hr, sr, z = _train_inputs(name, B, H, W)
    data = {'HR': hr.to(d), 'SR': sr.to(d)}
    sr3 = DESCS[name]['variant'] == 'sr3'
    if sr3:
        loss = netG.p_losses(data, noise=z.to(d), t=t)
        steps = np.full(B, t - 1)
        g32 = torch.FloatTensor(np.full(B, netG.sqrt_alphas_cumprod_prev[t]))        # on the grid: the level the sampler feeds at step t
        ca, cb, time = g32, (1 - g32 ** 2).sqrt(), g32.double().view(-1, 1)
    else:
        tt = torch.tensor(t, dtype=torch.long)
        loss = netG.p_losses(data, noise=z.to(d), t=tt.to(d))
        steps = np.asarray(t)
        ca, cb, time = netG.sqrt_alphas_cumprod.cpu()[tt], netG.sqrt_one_minus_alphas_cumprod.cpu()[tt], tt
    torch.cuda.synchronize()
    s = SCHEDS[name]
    ac = np.cumprod(1.0 - np.linspace(s['linear_start'], s['linear_end'], s['n_timestep'], dtype=np.float64))
    scal = R.step_scalars(R.walk_tables(ac, s['n_timestep']), steps)
    scal32 = netG._hyb_table.cpu()[torch.as_tensor(steps)]
    np.testing.assert_allclose(scal32.numpy(), scal, rtol=2e-7)          # the engine's rows are the walk's, rounded to fp32
    ref_tot, ref_vlb, ref, cond = _ref_step(name, sd6, hr, sr, z, ca, cb, time, scal32.double(), lam)
    got_vlb = float(netG.last_vlb) * hr.numel()
    print('%s %dx%d t=%s: loss %.6f (ref %.6f), vlb %.6f (ref %.6f; fp32 conditioning of the last-step logs %.3g)'
          % (name, H, W, t, float(loss), ref_tot, got_vlb, ref_vlb, cond))
    assert abs(float(loss) - ref_tot) <= 1e-5 * abs(ref_tot)
    # the logged L_vlb: the loss's tolerance, plus what fp32 can know of the last step's logs on an untrained network -- a far tail's bin
    # mass is a difference of two fp32 CDF values next to 1 (learned_var_ref.nll_conditioning; 0 for a KL step)
    assert abs(got_vlb - ref_vlb) <= 1e-5 * abs(ref_vlb) + cond
    bad, worst = [], 0.0
    for key, grad in un.named_gradients():
        r = ref[key]
        num, den = (grad.cpu().double() - r).norm().item(), max(r.norm().item(), 1e-7)
        worst = max(worst, num / den if den > 1e-6 else 0.0)
        if num / den > 1e-4 and den > 1e-6:
            bad.append((num / den, key, den))
    print('worst normwise gradient error %.2e' % worst)
    assert not bad, sorted(bad, reverse=True)[:8]
    gw = dict(un.named_gradients())
    assert float(gw['final_conv.block.3.weight'][3:].abs().max()) > 0.0 and float(gw['final_conv.block.3.bias'][3:].abs().max()) > 0.0
    # the same bits every run
    arena0, loss0 = un.grad_arena.clone(), float(loss)
    again = netG.p_losses(data, noise=z.to(d), t=t if sr3 else tt.to(d))
    torch.cuda.synchronize()
    assert float(again) == loss0 and torch.equal(un.grad_arena, arena0)
    # lambda = 0: the variance rows' gradient is exactly zero, the prediction rows are the 3-row network's step bit for bit
    netG.set_learned_variance(0.0)
    l0 = netG.p_losses(data, noise=z.to(d), t=t if sr3 else tt.to(d))
    torch.cuda.synchronize()
    gw = {k: v.clone() for k, v in un.named_gradients()}
    assert not gw['final_conv.block.3.weight'][3:].any() and not gw['final_conv.block.3.bias'][3:].any()
    m3, _ = build3(name, sd6, phase='train')
    if sr3:
        l3 = m3.netG.p_losses(data, noise=z.to(d), gamma=g32)
    else:
        l3 = m3.netG.p_losses(data, noise=z.to(d), t=tt.to(d))
    torch.cuda.synchronize()
    g3 = dict(m3.netG.denoise_fn.named_gradients())
    assert abs(float(l0) - float(l3)) <= 1.2e-7 * abs(float(l3))         # (the same terms, summed per pixel first)
    assert torch.equal(gw['final_conv.block.3.weight'][:3], g3['final_conv.block.3.weight'])
    assert torch.equal(gw['final_conv.block.3.bias'][:3], g3['final_conv.block.3.bias'])


def test_optimize_parameters_logs_l_vlb():
    m6, _ = build6('sr3_tiny', phase='train', lam=0.001)
    hr, sr, _ = _train_inputs('sr3_tiny', 2, 16, 16)
    np.random.seed(3)
    torch.manual_seed(3)
    m6.feed_data({'HR': hr, 'SR': sr})
    m6.optimize_parameters()
    log = m6.get_current_log()
    assert set(log) >= {'l_pix', 'l_vlb'} and np.isfinite(log['l_vlb']) and log['l_vlb'] > 0.0 and np.isfinite(log['l_pix'])
    un = m6.netG.denoise_fn
    with pytest.raises(L.Sr3Error, match='step_scalars go together'):      # the plain step refuses a plan with variance rows
        un.train_step(hr.to(G.dev()), sr.to(G.dev()), hr.to(G.dev()), torch.ones(2, device=G.dev()), torch.zeros(2, device=G.dev()),
                      torch.ones(2, device=G.dev()), None, grad_scale=1.0)


# ---- 4. the tail ----------------------------------------------------------------------------------------------------------------------

def _tail_tables(dev):
    tabs = R.walk_tables(_ac(), 10)
    sigma = np.sqrt(tabs['beta_tilde'])
    sigma[0] = 0.0
    names = ('a', 'b', 'c1', 'c2')
    dev_tabs = [torch.tensor(tabs[k], dtype=torch.float32).to(dev) for k in names] + [torch.tensor(sigma, dtype=torch.float32).to(dev)]
    lb = torch.tensor(tabs['log_beta'], dtype=torch.float32).to(dev)
    lt = torch.tensor(tabs['log_beta_tilde'], dtype=torch.float32).to(dev)
    return tabs, dev_tabs, lb, lt


def _tail_call(x, out, z, j, dev_tabs, lb, lt, clip=1, c3=None, hist=None):
    step2 = torch.tensor([-9, j], dtype=torch.int32, device=x.device)
    rc = L.load().sr3_learned_var_step(L.ptr(x), L.ptr(out), L.ptr(z), x.shape[0], x.shape[1], x.shape[2], x.shape[3],
                                       *[L.ptr(t) for t in dev_tabs], L.ptr(lb), L.ptr(lt), L.ptr(step2), clip, L.ptr(c3), L.ptr(hist),
                                       G.stream())
    torch.cuda.synchronize()
    return rc, step2


@pytest.mark.parametrize('H,W,aligned', [(8, 12, False), (16, 16, True)])      # the scalar path (a pointer off 16 bytes), the 16-byte path
def test_learned_var_tail(H, W, aligned):
    lib, dev = L.load(), G.dev()
    tabs, dev_tabs, lb, lt = _tail_tables(dev)
    B, C_ = 3, 3
    n = B * C_ * H * W
    x0 = _rand(B, C_, H, W, seed=21)
    out = torch.cat([_rand(B, C_, H, W, seed=22), torch.rand(B, C_, H, W, generator=torch.Generator().manual_seed(23)) * 3 - 1.5], 1).contiguous()
    z = _rand(B, C_, H, W, seed=24)
    outd, zd = out.to(dev), z.to(dev)
    buf = torch.zeros(n + 8, device=dev)

    def fresh():
        off = 0 if aligned else 1
        x = buf[off:off + n].view(B, C_, H, W)
        x.copy_(x0)
        assert (x.data_ptr() % 16 == 0) == aligned
        return x
    for j in (9, 4, 1, 0):
        row = [tabs[k][j] for k in ('a', 'b', 'c1', 'c2', 'log_beta', 'log_beta_tilde')]
        row32 = [float(np.float32(v)) for v in row]
        x = fresh()
        rc, step2 = _tail_call(x, outd, zd, j, dev_tabs, lb, lt)
        assert rc == 0 and step2.tolist() == [j, j - 1]
        x = x.clone()                                        # (fresh() hands out the same storage again)
        ref = R.ancestral_step(x0, out, z, row32, clip=True, last=j == 0)
        err = (x.cpu().double() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
        assert err <= TOL_STEP, (j, err)
        # the mean: k_p_sample_update with sigma = 0 on the prediction rows, bit for bit (no z: the tail adds sigma * 0)
        xm = fresh()
        rc, _ = _tail_call(xm, outd, None, j, dev_tabs, lb, lt)
        mean = x0.to(dev).clone()
        zero_sigma = torch.zeros_like(dev_tabs[4])
        pred = outd[:, :3].contiguous()
        L.check(lib.sr3_p_sample_step_ex(L.ptr(mean), L.ptr(pred), None, *[L.ptr(t) for t in dev_tabs[:4]], L.ptr(zero_sigma),
                                         None, None, j, B, C_ * H * W, 1, G.stream()))
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(xm, mean)
        xm = xm.clone()
        if j == 0:
            assert torch.equal(x, mean)                      # the last row adds no noise
        else:
            assert not torch.equal(x, mean)
            sig = torch.from_numpy(R.sigma_f32(out[:, 3:].numpy(), row32[4], row32[5]))
            d = (x.cpu().double() - mean.cpu().double()) - sig.double() * z.double()      # sigma z, to the rounding of the last sum
            assert d.abs().max().item() <= TOL_STEP * max(1.0, ref.abs().max().item())
    # both paths give the same bits
    xa = torch.empty(B, C_, H, W, device=dev).copy_(x0)
    xb = buf[1:1 + n].view(B, C_, H, W).copy_(x0)
    assert _tail_call(xa, outd, zd, 4, dev_tabs, lb, lt)[0] == 0 and _tail_call(xb, outd, zd, 4, dev_tabs, lb, lt)[0] == 0
    assert torch.equal(xa, xb)
    # no clamp: differs where x0 leaves [-1, 1]
    xc = torch.empty(B, C_, H, W, device=dev).copy_(x0)
    assert _tail_call(xc, outd, zd, 4, dev_tabs, lb, lt, clip=0)[0] == 0 and not torch.equal(xc, xa)


def test_learned_var_tail_host_checks():
    """Each host check once, in the order the entry runs them, with its code and message."""
    lib, dev = L.load(), G.dev()
    _, dev_tabs, lb, lt = _tail_tables(dev)
    x = torch.zeros(1, 3, 4, 4, device=dev)
    out = torch.zeros(1, 6, 4, 4, device=dev)
    step2 = torch.zeros(2, dtype=torch.int32, device=dev)
    before = x.clone()

    def call(x_=x, out_=out, z=None, dims=(1, 3, 4, 4), c3=None, hist=None, step=step2):
        return lib.sr3_learned_var_step(L.ptr(x_), L.ptr(out_), L.ptr(z), *dims, *[L.ptr(t) for t in dev_tabs], L.ptr(lb), L.ptr(lt),
                                        L.ptr(step), 1, L.ptr(c3), L.ptr(hist), G.stream())
    msg = lambda: lib.sr3_last_error().decode()
    assert call(out_=None) == -1 and msg() == 'learned_var_step: out_nchw is NULL'
    assert call(step=None) == -1 and msg() == 'learned_var_step: step2_dev is NULL'
    assert call(dims=(0, 3, 4, 4)) == -1 and 'batch, channels, height and width must be positive (got 0, 3, 4, 4)' in msg()
    assert call(dims=(32768, 1, 32768, 1)) == -2 and msg() == 'learned_var_step: image batch too large (batch * channels * height * width >= 2^31)'
    assert call(c3=dev_tabs[0], hist=torch.zeros_like(x)) == -2 and 'no multistep history' in msg()
    assert call(z=x) == -1 and msg() == 'learned_var_step: x_nchw overlaps z_nchw'
    assert call(x_=out[:, :3]) == -1 and msg() == 'learned_var_step: x_nchw overlaps out_nchw'
    torch.cuda.synchronize()
    assert torch.equal(x, before) and step2.tolist() == [0, 0]           # nothing was launched


# ---- 5. chains ------------------------------------------------------------------------------------------------------------------------

def test_ten_step_ancestral_chain_replayed_graph_against_the_reference():
    from oracle import sr3_oracle as O
    name, S = 'sr3_tiny', 10
    m6, sd6 = build6(name, sched=CHAIN_SCHED, sampler={'type': 'ancestral', 'steps': S})
    d = G.dev()
    netG = m6.netG
    assert netG.sampler == dict(type='ancestral', steps=S, eta=1.0)
    cond = _rand(2, 3, 16, 16, seed=41).clamp(-1, 1).to(d)
    shape = tuple(cond.shape)
    outs = []
    for use_graph in (True, False):
        netG.use_graph = use_graph
        torch.manual_seed(11)
        outs.append(netG.p_sample_loop(cond, continous=True).clone())
    st = next(iter(netG._loop_cache.values()))
    assert st['graph'] is not None and st['step'].tolist() == [0, -1] and st['out2'].shape == (2, 6, 16, 16)
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())      # the replayed graph is the eager chain
    # the chain's draws, replayed: x_T, then one z per step in the order the steps are taken
    torch.manual_seed(11)
    x = torch.randn(shape, device=d).cpu()
    zs = [torch.empty(shape, device=d).normal_().cpu() for _ in range(S)]
    s = CHAIN_SCHED
    ac = np.cumprod(1.0 - np.linspace(s['linear_start'], s['linear_end'], s['n_timestep'], dtype=np.float64))
    tabs = R.walk_tables(ac, S)
    assert netG._sampler_tau.tolist() == tabs['tau'].tolist()
    desc = dict(DESCS[name], out_channel=6)
    for i, j in enumerate(reversed(range(S))):
        level = torch.FloatTensor([np.sqrt(ac[tabs['tau'][j]])]).repeat(2, 1)
        with torch.no_grad():
            out = O.unet_forward(sd6, desc, torch.cat([cond.cpu(), x], 1), level)
        row = [float(np.float32(tabs[k][j])) for k in ('a', 'b', 'c1', 'c2', 'log_beta', 'log_beta_tilde')]
        x = R.ancestral_step(x, out, zs[i], row, clip=True, last=j == 0).float()
    err = float((outs[0][-2:].cpu().double() - x.double()).abs().max())
    print('ten-step ancestral chain: error %.2e' % err)
    assert err <= 1e-4, err
    # noise_seq drives the same loop eagerly: indexed by the step index
    seq = torch.stack(list(reversed(zs))).to(d)
    torch.manual_seed(11)
    x_T = torch.randn(shape, device=d)
    injected = netG.p_sample_loop(cond, continous=True, x_T=x_T, noise_seq=seq)
    assert float((injected[-2:].cpu().double() - x.double()).abs().max()) <= 1e-4


def test_ddim_on_a_learned_variance_checkpoint_is_ddim_on_the_three_row_network():
    name, S = 'sr3_tiny', 10
    sampler = {'type': 'ddim', 'steps': S, 'eta': 0.0}
    m6, sd6 = build6(name, sched=CHAIN_SCHED, sampler=sampler)
    m3, _ = build3(name, sd6, sched=CHAIN_SCHED, sampler=sampler)
    d = G.dev()
    cond = _rand(2, 3, 16, 16, seed=41).clamp(-1, 1).to(d)
    x_T = _rand(2, 3, 16, 16, seed=42).to(d)
    a = m6.netG.p_sample_loop(cond, continous=True, x_T=x_T)
    b = m3.netG.p_sample_loop(cond, continous=True, x_T=x_T)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    # ... and the ancestral DDPM chain of the DDPM variant runs through the timestep map
    m, _ = build6('ddpm_tiny', sampler={'type': 'ancestral', 'steps': 4})
    torch.manual_seed(5)
    out = m.netG.p_sample_loop((2, 3, 16, 16), continous=False)
    assert tuple(out.shape) == (2, 3, 16, 16) and bool(torch.isfinite(out).all())
    assert m.netG._sampler_tau.tolist() == [0, 2, 3, 5]
