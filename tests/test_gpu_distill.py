"""Progressive distillation on the GPU: the two kernels of csrc/distill.hip bit-equal to their NumPy float32 restatements
(tests/test_distill_cpu.py) -- every operation is a separately rounded fp32 operation, so equality is the criterion and no tolerance
applies; `Distiller.step` against CPU autograd of the oracle (both teacher forwards through oracle.sr3_oracle.unet_forward, the target
written out in float64 here, loss and gradients through the oracle's UNet; the project's tolerances for these fixtures,
tests/test_gpu_train.py: loss relative 1e-5, gradients normwise relative 1e-4 for entries with |ref| > 1e-6); its bitwise guarantees;
and a chain on an explicit walk."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import DESCS, SCHEDS, CONDITIONAL, load_golden, opt_for      # noqa: E402
import gpu_util as G                                             # noqa: E402
from oracle import sr3_oracle as O                               # noqa: E402
from test_distill_cpu import alphas_cumprod, np_distill_target, np_teacher_step      # noqa: E402

F = np.float32


# ---- the kernels --------------------------------------------------------------------------------------------------------------------

def _dev(a, offset):
    """the array on the device, 16-byte aligned (offset 0) or one float past it"""
    flat = torch.empty(a.size + 8, device=G.dev())
    t = flat[offset:offset + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 * offset and t.is_contiguous()
    return t


def _out(shape, offset):
    flat = torch.full((int(np.prod(shape)) + 8,), float('nan'), device=G.dev())
    return flat, flat[offset:offset + int(np.prod(shape))].view(shape)


_data = {}


def kernel_data(shape):
    """inputs and per-image coefficients for one shape, once: z_t, two pairs of network outputs, and coefficient rows of a real walk
    (sr3_tiny, N = 4, v-prediction) with k = 1 (w1 = 0) in the first image and k = N in the last"""
    if shape not in _data:
        from sr3_hip.distill import distill_coefs, distill_walks
        g = np.random.default_rng(sum(shape))
        B = shape[0]
        ac = alphas_cumprod('sr3_tiny')
        k = np.array(([1, 4, 2, 3] * B)[:B])
        co = {n: v.astype(F) for n, v in distill_coefs(ac, distill_walks(ac, 4, 'logsnr')[0], k, 'v').items()}
        assert co['w1'][0] == 0.0 and co['w2'][0] == 1.0
        arrs = [(1.5 * g.standard_normal(shape)).astype(F) for _ in range(5)]
        _data[shape] = (arrs, co)
    return _data[shape]


def run_teacher_step(x, oc, ou, scale, co, clip, offset, in_place=False):
    from sr3_hip import lib as L
    B, per = x.shape[0], int(np.prod(x.shape[1:]))
    dx, doc = _dev(x, offset), _dev(oc, offset)
    dou = None if ou is None else _dev(ou, offset)
    rows = torch.from_numpy(np.stack([co[n] for n in ('a1', 'b1', 'c1', 'c2')])).to(G.dev())
    f1, x_next = _out(x.shape, offset)
    f2, x0 = _out(x.shape, offset)
    if in_place:
        x_next = dx
    L.check(L.load().sr3_teacher_step_f32(L.ptr(dx), L.ptr(doc), L.ptr(dou), scale, L.ptr(rows[0]), L.ptr(rows[1]), L.ptr(rows[2]), L.ptr(rows[3]),
                                          B, per, 1 if clip else 0, L.ptr(x_next), L.ptr(x0), G.stream()))
    torch.cuda.synchronize()
    for flat, used in ((f1, not in_place), (f2, True)):      # nothing outside the output is written
        n = per * B if used else 0
        assert bool(torch.isnan(flat[:offset]).all()) and bool(torch.isnan(flat[offset + n:]).all())
    if not in_place:
        assert np.array_equal(dx.cpu().numpy(), x)
    return x_next.cpu().numpy(), x0.cpu().numpy()


def run_distill_target(z_t, x_mid, oc, ou, scale, x0f, co, clip, offset):
    from sr3_hip import lib as L
    B, per = z_t.shape[0], int(np.prod(z_t.shape[1:]))
    dz, dm, doc, df = (_dev(a, offset) for a in (z_t, x_mid, oc, x0f))
    dou = None if ou is None else _dev(ou, offset)
    rows = torch.from_numpy(np.stack([co[n] for n in ('a2', 'b2', 'w1', 'w2', 's1', 's2')])).to(G.dev())
    f1, x_tgt = _out(z_t.shape, offset)
    f2, eps_tgt = _out(z_t.shape, offset)
    L.check(L.load().sr3_distill_target_f32(L.ptr(dz), L.ptr(dm), L.ptr(doc), L.ptr(dou), scale, L.ptr(df), *[L.ptr(r) for r in rows], B, per,
                                            1 if clip else 0, L.ptr(x_tgt), L.ptr(eps_tgt), G.stream()))
    torch.cuda.synchronize()
    for flat in (f1, f2):
        assert bool(torch.isnan(flat[:offset]).all()) and bool(torch.isnan(flat[offset + per * B:]).all())
    return x_tgt.cpu().numpy(), eps_tgt.cpu().numpy()


# (3, 3, 8, 8): the 16-byte form; (2, 3, 5, 7): 105 values per image, the one-value form; offset 1: every image pointer one float past
# a 16-byte boundary, the one-value form on a shape that would take the other; (3, 3, 160, 160): 900 workgroups (225 in the 16-byte form)
SHAPES = [((3, 3, 8, 8), 0), ((2, 3, 5, 7), 0), ((3, 3, 8, 8), 1), ((3, 3, 160, 160), 0), ((2, 3, 5, 7), 1)]


@pytest.mark.parametrize('clip', [True, False])
@pytest.mark.parametrize('guided', [False, True])
@pytest.mark.parametrize('shape,offset', SHAPES)
def test_kernels_are_bit_equal_to_the_restatement(shape, offset, guided, clip):
    (z_t, oc1, ou1, oc2, ou2), co = kernel_data(shape)
    scale = 1.5
    u1, u2 = (ou1, ou2) if guided else (None, None)
    want_mid, want_x0 = np_teacher_step(z_t, oc1, u1, scale, co['a1'], co['b1'], co['c1'], co['c2'], clip)
    raw = np_teacher_step(z_t, oc1, u1, scale, co['a1'], co['b1'], co['c1'], co['c2'], False)[1]
    assert (np.abs(raw) < 1).any() and (np.abs(raw) > 1).any()              # the clamp has both branches to take
    got_mid, got_x0 = run_teacher_step(z_t, oc1, u1, scale, co, clip, offset)
    assert got_x0.tobytes() == want_x0.tobytes() and got_mid.tobytes() == want_mid.tobytes()
    got_ip, got_x0_ip = run_teacher_step(z_t, oc1, u1, scale, co, clip, offset, in_place=True)
    assert got_ip.tobytes() == want_mid.tobytes() and got_x0_ip.tobytes() == want_x0.tobytes()
    want_t, want_e = np_distill_target(z_t, want_mid, oc2, u2, scale, want_x0, co['a2'], co['b2'], co['w1'], co['w2'], co['s1'], co['s2'], clip)
    raw2 = np_teacher_step(want_mid, oc2, u2, scale, co['a2'], co['b2'], co['c1'], co['c2'], False)[1]
    assert (np.abs(raw2) < 1).any() and (np.abs(raw2) > 1).any()
    got_t, got_e = run_distill_target(z_t, want_mid, oc2, u2, scale, want_x0, co, clip, offset)
    assert got_t.tobytes() == want_t.tobytes() and got_e.tobytes() == want_e.tobytes()
    assert np.array_equal(got_t[0], np.clip(raw2[0], F(-1), F(1)) if clip else raw2[0])      # k = 1: the second prediction itself


# ---- Distiller.step against the oracle ------------------------------------------------------------------------------------------------

NAMES = ['sr3_tiny', 'ddpm_tiny', 'sr3_uncond']
_pairs = {}


def pair(name):
    """(train-phase student model, val-phase teacher model, golden record, golden weights): both networks hold the golden weights"""
    import model as Model
    if name not in _pairs:
        g, sd = load_golden(name)
        s = Model.create_model(opt_for(name, phase='train', gpu=True))
        t = Model.create_model(opt_for(name, phase='val', gpu=True))
        for m in (s, t):
            m.netG.load_state_dict(sd, strict=True)
        _pairs[name] = (s, t, g, sd)
    return _pairs[name]


def draws(name, g, N):
    hr, z = torch.from_numpy(g['loop/hr']), torch.from_numpy(g['train/z'])
    assert hr.shape[0] == 2
    return hr, torch.from_numpy(g['loop/sr']), z, torch.tensor([1, N])


def _forward(sd, name, x, cond, co, which, b):
    desc = DESCS[name]
    if desc['variant'] == 'sr3':
        time = torch.from_numpy(co['alpha_' + which].astype(F)).view(b, 1)
    else:
        time = torch.from_numpy(co['t_node' if which == 't' else 't_mid']).long()
    return O.unet_forward(sd, desc, x.float() if cond is None else torch.cat([cond, x.float()], 1), time)


def oracle_distill(name, g, sd, N, teacher_pred, student_pred, scale):
    """(loss, {key: gradient of loss / numel}): the teacher's two steps and the target in float64 on the oracle's forwards, then the L2
    loss of the student's prediction kind and torch autograd through the oracle's UNet"""
    from sr3_hip.distill import distill_coefs, distill_walks
    hr, sr, z, k = draws(name, g, N)
    b = hr.shape[0]
    cond = sr if CONDITIONAL[name] else None
    ac = alphas_cumprod(name)
    co = distill_coefs(ac, distill_walks(ac, N, 'logsnr')[0], k.numpy(), teacher_pred)
    c = {n: torch.from_numpy(np.asarray(v, dtype=np.float64)).view(-1, 1, 1, 1) for n, v in co.items() if not n.startswith('t_')}

    def teacher_out(x, which):
        with torch.no_grad():
            out = _forward(sd, name, x, cond, co, which, b).double()
            if scale is not None:
                ou = _forward(sd, name, x, torch.zeros_like(cond), co, which, b).double()
                out = ou + scale * (out - ou)
        return out
    z_t = c['alpha_t'] * hr.double() + c['sigma_t'] * z.double()
    x1 = (c['a1'] * z_t - c['b1'] * teacher_out(z_t, 't')).clamp(-1.0, 1.0)
    z_m = c['c1'] * x1 + c['c2'] * z_t
    x2 = (c['a2'] * z_m - c['b2'] * teacher_out(z_m, 'm')).clamp(-1.0, 1.0)
    x_t = c['w1'] * x1 + c['w2'] * x2
    eps_t = c['s1'] * z_t - c['s2'] * x_t
    sdr = {n: v.clone().requires_grad_(v.is_floating_point() and n.startswith('denoise_fn.')) for n, v in sd.items()}
    out = _forward(sdr, name, c['alpha_t'] * x_t + c['sigma_t'] * eps_t, cond, co, 't', b).double()
    target = eps_t if student_pred == 'eps' else c['alpha_t'] * eps_t - c['sigma_t'] * x_t
    loss = ((target - out) ** 2).sum()
    params = {n: v for n, v in sdr.items() if v.requires_grad}
    grads = torch.autograd.grad(loss / hr.numel(), list(params.values()))
    return float(loss.detach()), dict(zip(params, grads))


def engine_distill(name, N, student_pred, scale, repeat=1):
    from sr3_hip.distill import Distiller
    s, t, g, sd = pair(name)
    d = G.dev()
    hr, sr, z, k = draws(name, g, N)
    s.netG.set_prediction(student_pred)
    s.netG.set_objective('l2')
    try:
        ds = Distiller(s.netG, t.netG, steps=N, walk='logsnr', guidance_scale=scale)
        outs = []
        for _ in range(repeat):
            loss = ds.step({'HR': hr.to(d), 'SR': sr.to(d)}, k=k, noise=z.to(d), drop_seed=7)
            torch.cuda.synchronize()
            outs.append((float(loss), s.netG.denoise_fn.grad_arena.clone()))
        grads = [(n, v.cpu().clone()) for n, v in s.netG.denoise_fn.named_gradients()]
    finally:
        s.netG.set_prediction('eps')
        s.netG.objective = None
    return ds, outs, grads


CASES = [(n, p, None) for n in NAMES for p in ('eps', 'v')] + [('sr3_tiny', 'v', 1.5)]


@pytest.mark.parametrize('name,student_pred,scale', CASES)
def test_step_matches_oracle_autograd(name, student_pred, scale):
    N = SCHEDS[name]['n_timestep'] // 2
    s, t, g, sd = pair(name)
    ref_loss, ref_grads = oracle_distill(name, g, sd, N, 'eps', student_pred, scale)
    ds, outs, grads = engine_distill(name, N, student_pred, scale)
    loss = outs[0][0]
    assert ds.student_sampler() == dict(type='ddim', steps=N, eta=0.0, walk=[int(v) for v in ds.tau2[1::2]])
    bad, worst = [], 0.0
    for key, grad in grads:
        ref = ref_grads['denoise_fn.' + key]
        num, den = (grad - ref).norm().item(), max(ref.norm().item(), 1e-7)
        if den > 1e-6:
            worst = max(worst, num / den)
            if num / den > 1e-4:
                bad.append((num / den, key))
    print('%s %s scale %s: loss %.9g ref %.9g (rel %.2e), worst gradient rel %.2e' % (name, student_pred, scale, loss, ref_loss, abs(loss - ref_loss) / abs(ref_loss), worst))
    assert ref_loss > 0 and abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (loss, ref_loss)
    assert not bad, sorted(bad, reverse=True)[:8]


def test_v_teacher_matches_oracle_autograd():
    """the teacher's prediction kind picks a, b of both its steps: a v-teacher (the same weights read as v) against the oracle"""
    name, N = 'sr3_tiny', 4
    s, t, g, sd = pair(name)
    t.netG.set_prediction('v')
    try:
        ref_loss, ref_grads = oracle_distill(name, g, sd, N, 'v', 'v', None)
        ds, outs, grads = engine_distill(name, N, 'v', None)
    finally:
        t.netG.set_prediction('eps')
    loss = outs[0][0]
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (loss, ref_loss)
    for key, grad in grads:
        ref = ref_grads['denoise_fn.' + key]
        if ref.norm().item() > 1e-6:
            assert (grad - ref).norm().item() <= 1e-4 * ref.norm().item(), key


@pytest.mark.parametrize('name', ['sr3_tiny', 'ddpm_tiny'])
def test_step_is_bitwise_reproducible(name):
    N = SCHEDS[name]['n_timestep'] // 2
    _, outs, _ = engine_distill(name, N, 'v', 1.5 if name == 'sr3_tiny' else None, repeat=2)
    assert outs[0][0] == outs[1][0] and torch.equal(outs[0][1], outs[1][1]) and np.isfinite(outs[0][0])


@pytest.mark.parametrize('name', ['sr3_tiny', 'ddpm_tiny'])
def test_teacher_is_never_written(name):
    """three optimize_parameters iterations with the Distiller in place of p_losses (draws from torch's RNG): the teacher's arena is
    bitwise what it was, the student's moved, the loss stayed finite"""
    import model as Model
    from sr3_hip.distill import Distiller
    g, sd = load_golden(name)
    m = Model.create_model(opt_for(name, phase='train', gpu=True))
    m.netG.load_state_dict(sd, strict=True)
    _, t, _, _ = pair(name)
    N = SCHEDS[name]['n_timestep'] // 2
    m.distiller = Distiller(m.netG, t.netG, steps=N)
    before_t = t.netG.denoise_fn.arena.data.clone()
    before_s = m.netG.denoise_fn.arena.data.clone()
    assert torch.equal(before_t, before_s)
    torch.manual_seed(11)
    m.feed_data({'HR': torch.from_numpy(g['loop/hr']), 'SR': torch.from_numpy(g['loop/sr'])})
    for _ in range(3):
        m.optimize_parameters()
        assert np.isfinite(m.get_current_log()['l_pix'])
    torch.cuda.synchronize()
    assert torch.equal(t.netG.denoise_fn.arena.data, before_t)
    assert not torch.equal(m.netG.denoise_fn.arena.data, before_s) and bool(torch.isfinite(m.netG.denoise_fn.arena.data).all())


def test_refusals_before_anything_is_launched():
    from sr3_hip.distill import Distiller
    s, t, _, _ = pair('sr3_tiny')
    su, tu, _, _ = pair('sr3_uncond')
    _, td, _, _ = pair('ddpm_tiny')
    with pytest.raises(ValueError, match='unconditional'):
        Distiller(su.netG, tu.netG, steps=4, guidance_scale=1.5)
    with pytest.raises(ValueError, match='more than the schedule'):
        Distiller(s.netG, t.netG, steps=5)
    with pytest.raises(ValueError, match='variant|model'):
        Distiller(s.netG, td.netG, steps=2)
    with pytest.raises(ValueError, match='differ'):
        Distiller(s.netG, tu.netG, steps=4)
    with pytest.raises(ValueError, match='of its own'):
        Distiller(s.netG, s.netG, steps=4)
    with pytest.raises(ValueError, match='has 4 timesteps but steps is 8'):
        Distiller(s.netG, t.netG, steps=4, walk=[1, 3, 5, 7])
    ds = Distiller(s.netG, t.netG, steps=2, walk=[1, 3, 5, 7])                 # the next round: the student walk of N = 4 as teacher walk
    assert ds.tau2.tolist() == [1, 3, 5, 7] and ds.student_sampler()['walk'] == [3, 7] and ds.state() == {'steps': 2, 'walk': [3, 7]}


# ---- a chain on an explicit walk ------------------------------------------------------------------------------------------------------

def test_explicit_walk_chain_follows_the_numpy_tables():
    """set_sampler(4, walk=tau_s) on sr3_tiny: every step of the chain against the float64 update on `sampler_tables` of the same walk
    with the oracle UNet's output at that walk's level (the sampler tests' single-step criterion, 2e-5 * max(1, |ref|_inf)), and
    p_sample_loop is those steps"""
    from sr3_hip.diffusion import sampler_tables
    from sr3_hip.distill import distill_walks
    from test_gpu_sampler import _loop_inputs, _oracle_eps, build
    name = 'sr3_tiny'
    m, g, sd, _ = build(name)
    d = G.dev()
    netG = m.netG
    ac = alphas_cumprod(name)
    tau_s = distill_walks(ac, 4, 'logsnr')[1]
    assert tau_s[0] != 0
    tabs = sampler_tables(ac, 4, 0.0, walk=list(tau_s))
    netG.set_sampler(4, walk=tau_s)
    assert netG._sampler_tau.tolist() == tau_s.tolist()
    cond, x_T, zs, arg = _loop_inputs(name, g, d)
    st = netG._loop_state(tuple(x_T.shape), tuple(x_T.shape), d)
    netG.denoise_fn.ensure_derived()
    st['img'].copy_(x_T)
    st['cond'].copy_(cond)
    st['step'].fill_(3)
    worst = 0.0
    for j in reversed(range(4)):
        x_in = st['img'].cpu()
        netG._one_step(st, draw_noise=False)
        assert st['z_used'] is False
        eps = _oracle_eps(sd, name, ac, tau_s, j, x_in, cond.cpu())
        G.assert_close(st['eps'].cpu(), eps, what='eps at step index %d' % j)
        x0 = (tabs['a'][j] * x_in.double() - tabs['b'][j] * eps.double()).clamp(-1.0, 1.0)
        worst = max(worst, G.assert_close(st['img'].cpu(), tabs['c1'][j] * x0 + tabs['c2'][j] * x_in.double(), what='step index %d' % j))
    stepped = st['img'].clone()
    out = netG.p_sample_loop(arg, continous=True, x_T=x_T)
    assert torch.equal(out[-2:], stepped)
    print('explicit walk %s: worst step error %.2e' % (tau_s.tolist(), worst))


# ---- the config key, two rounds -------------------------------------------------------------------------------------------------------

def test_config_key_chains_two_rounds(tmp_path):
    """train.distill through create_model: the teacher comes from a checkpoint the package wrote (its prediction kind from *_opt.pth), the
    student starts from its weights, optimize_parameters steps the Distiller, *_opt.pth records the student's chain, and the next
    round -- whose teacher is that student -- takes the recorded walk as its teacher walk whatever its own "walk" key says"""
    import model as Model
    name = 'sr3_tiny'
    g, sd = load_golden(name)

    def opt_of(phase, distill=None, resume=None):
        opt = opt_for(name, phase=phase, gpu=True)
        opt['path'].update(checkpoint=str(tmp_path), resume_state=resume)
        opt['model']['diffusion']['prediction'] = 'v'
        if distill is not None:
            opt['train']['distill'] = distill
        return opt
    m0 = Model.create_model(opt_of('train'))
    m0.netG.load_state_dict(sd, strict=True)
    m0.save_network(0, 0)
    data = {'HR': torch.from_numpy(g['loop/hr']), 'SR': torch.from_numpy(g['loop/sr'])}
    # round 1: 8 -> 4
    m1 = Model.create_model(opt_of('train', {'teacher': str(tmp_path / 'I0_E0'), 'steps': 4, 'walk': 'logsnr', 'guidance_scale': None}))
    ds = m1.distiller
    assert ds is not None and ds.steps == 4 and ds.tau2.tolist() == list(range(8)) and ds.teacher.prediction == 'v' and ds.guidance_scale is None
    t_arena = ds.teacher.denoise_fn.arena.data
    assert t_arena.data_ptr() != m1.netG.denoise_fn.arena.data_ptr() and ds.teacher.denoise_fn.plan is not m1.netG.denoise_fn.plan
    assert torch.equal(t_arena, m0.netG.denoise_fn.arena.data) and torch.equal(m1.netG.denoise_fn.arena.data, t_arena)
    before = t_arena.clone()
    torch.manual_seed(3)
    m1.feed_data(dict(data))
    m1.optimize_parameters()
    assert np.isfinite(m1.get_current_log()['l_pix'])
    assert torch.equal(t_arena, before) and not torch.equal(m1.netG.denoise_fn.arena.data, before)
    m1.save_network(1, 5)
    ck = torch.load(str(tmp_path / 'I5_E1_opt.pth'), map_location='cpu')
    assert ck['engine'] == {'prediction': 'v', 'distill': {'steps': 4, 'walk': [1, 3, 5, 7]}}
    m1.set_new_noise_schedule(opt_of('train')['model']['beta_schedule']['val'], schedule_phase='val')      # validation during training
    assert m1.netG.sampler == ds.student_sampler() == dict(type='ddim', steps=4, eta=0.0, walk=[1, 3, 5, 7])
    # round 2: 4 -> 2, the teacher is round 1's student
    m2 = Model.create_model(opt_of('train', {'teacher': str(tmp_path / 'I5_E1'), 'steps': 2, 'walk': 'time'}))
    assert m2.distiller.tau2.tolist() == [1, 3, 5, 7] and m2.distiller.tau_s.tolist() == [3, 7]
    assert torch.equal(m2.distiller.teacher.denoise_fn.arena.data, m1.netG.denoise_fn.arena.data)
    assert torch.equal(m2.netG.denoise_fn.arena.data, m1.netG.denoise_fn.arena.data)
    m2.feed_data(dict(data))
    m2.optimize_parameters()
    assert np.isfinite(m2.get_current_log()['l_pix'])
    m2.save_network(2, 9)
    assert torch.load(str(tmp_path / 'I9_E2_opt.pth'), map_location='cpu')['engine']['distill'] == {'steps': 2, 'walk': [3, 7]}
    # a resumed round keeps the resumed weights, not the teacher's
    m3 = Model.create_model(opt_of('train', {'teacher': str(tmp_path / 'I0_E0'), 'steps': 4}, resume=str(tmp_path / 'I5_E1')))
    assert torch.equal(m3.netG.denoise_fn.arena.data, m1.netG.denoise_fn.arena.data) and m3.begin_step == 5
    assert torch.equal(m3.distiller.teacher.denoise_fn.arena.data, before)
    # the val phase samples round 1's student on its walk
    mv = Model.create_model(opt_of('val', resume=str(tmp_path / 'I5_E1')))
    mv.netG.show_progress = False
    mv.set_new_noise_schedule(opt_of('val')['model']['beta_schedule']['val'], schedule_phase='val')
    assert mv.netG.sampler == dict(type='ddim', steps=4, eta=0.0, walk=[1, 3, 5, 7])
    mv.feed_data(dict(data))
    mv.test(continous=False)
    assert tuple(mv.SR.shape) == (3, 16, 16) and bool(torch.isfinite(mv.SR).all())
    # a teacher walk that does not fit the requested steps is refused by name
    with pytest.raises(ValueError, match='has 4 timesteps but steps is 8'):
        Model.create_model(opt_of('train', {'teacher': str(tmp_path / 'I5_E1'), 'steps': 4}))
