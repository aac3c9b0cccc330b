"""Self-conditioning on the GPU (csrc/selfcond.hip, the 9-channel input conv, the 16-channel pad of the first conv's weight gradient,
EngineDiffusion.set_self_condition): the write-back kernel bit for bit against the NumPy restatement of tests/selfcond_ref.py, the
9-channel input conv against float64, and the model-level paths -- forward, training step, sampling chains -- against the oracle.

Shapes: the kernel at 4 x 4 (one 16-byte access per row) and 3 x 5 (the one-element form), three images so that the middle one can
be dropped; the input conv at the four shapes that take each dispatch; the tiny fixture (inner 8, 16 x 16) widened to in_channel 9
for training and sampling, and the inner-32 fixture at 16 x 32, the smallest model whose input conv runs on the MFMA form."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

import gpu_util as G                                                                      # noqa: E402
import selfcond_ref as R                                                                  # noqa: E402
from oracle import sr3_oracle as O                                                        # noqa: E402
from sr3_hip import lib as L                                                              # noqa: E402
from test_consistency_cpu import project                                                  # noqa: E402

F = np.float32
GUARD = 1024          # floats of sentinel around dst, in the same allocation
SENTINEL = 7.25
# four rows that differ; the step-index form reads row 2
TAB_A = [1.1, 0.7, 0.9, 0.6]
TAB_B = [0.2, 0.75, 0.43, 0.7]
ROW = 2


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------------------

def _guarded(arr, d, mis=0):
    """arr on the device with GUARD sentinels on both sides in one allocation, `mis` floats off a 16-byte boundary: (view, buffer, offset)"""
    t = torch.as_tensor(arr)
    buf = torch.full((t.numel() + 2 * GUARD,), SENTINEL, device=d)
    assert buf.data_ptr() % 16 == 0
    off = GUARD + mis
    buf[off:off + t.numel()].copy_(t.reshape(-1))
    return buf[off:off + t.numel()].view(t.shape), buf, off


def _call(x, out, a, b, step, keep, clip, dst, first, dims=None):
    B, Cc, H, W = x.shape if dims is None else dims
    rc = L.load().sr3_selfcond_x0_f32(L.ptr(x), L.ptr(out), L.ptr(a), L.ptr(b), L.ptr(step), L.ptr(keep), clip, B, Cc, H, W, L.ptr(dst),
                                      0 if dst is None else dst.shape[1], first, G.stream())
    torch.cuda.synchronize()
    return rc


def _inputs(hw):
    rng = np.random.default_rng(100 * hw[0] + hw[1])
    x, out = (rng.standard_normal((3, 3) + hw).astype(F) for _ in range(2))
    return x, 1.5 * out


@pytest.mark.parametrize('clip', [1, 0], ids=['clip', 'noclip'])
@pytest.mark.parametrize('form', ['per_image', 'step_index'])
@pytest.mark.parametrize('hw,mis', [((4, 4), 0), ((3, 5), 0), ((4, 4), 1)], ids=['4x4', '3x5', '4x4-misaligned'])
def test_write_back_is_bit_exact(hw, mis, form, clip):
    d = G.dev()
    x, out = _inputs(hw)
    xd, od = torch.from_numpy(x).to(d), torch.from_numpy(out).to(d)
    if form == 'per_image':
        a, b, step = np.asarray(TAB_A[:3], F), np.asarray(TAB_B[:3], F), None
        ra, rb = a, b
    else:
        a, b, step = np.asarray(TAB_A, F), np.asarray(TAB_B, F), torch.tensor([ROW], dtype=torch.int32, device=d)
        ra, rb = a[ROW], b[ROW]
    ad, bd = torch.from_numpy(a).to(d), torch.from_numpy(b).to(d)
    raw = R.x0_f32(ra, rb, x, out, False)
    assert (np.abs(raw) > 1.0).any() and (np.abs(raw) < 1.0).any()          # the clamp matters and is not everything
    for dst_channels, first in ((6, 3), (3, 0)):
        for keep in ([1, 0, 1], None):
            rng = np.random.default_rng(5)
            dst0 = rng.standard_normal((3, dst_channels) + hw).astype(F)
            dst0[1] = np.nan                                               # a dropped image's old content does not matter either
            dst, buf, off = _guarded(dst0, d, mis)
            kd = None if keep is None else torch.tensor(keep, dtype=torch.int32, device=d)
            assert _call(xd, od, ad, bd, step, kd, clip, dst, first) == 0, L.load().sr3_last_error()
            want = R.write_back(dst0, x, out, ra, rb, keep, clip, first)
            got = dst.cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (dst_channels, first, keep)
            if keep is not None:
                assert not got[1, first:first + 3].any() and not np.signbit(got[1, first:first + 3]).any()      # +0.0
            assert bool((buf[:off] == SENTINEL).all()) and bool((buf[off + dst.numel():] == SENTINEL).all()), 'wrote outside dst'
            if step is not None:
                assert step.tolist() == [ROW]                              # the counter is read, never moved
    assert torch.equal(xd.cpu(), torch.from_numpy(x)) and torch.equal(od.cpu(), torch.from_numpy(out))


def test_dropped_images_are_not_read():
    """x and out of a dropped image may hold anything: its channels are +0.0, not 0 * NaN"""
    d = G.dev()
    x, out = _inputs((4, 4))
    x[1], out[1] = np.nan, np.inf
    dst = torch.full((3, 6, 4, 4), SENTINEL, device=d)
    a, b = (torch.tensor(t[:3], device=d) for t in (TAB_A, TAB_B))
    keep = torch.tensor([1, 0, 1], dtype=torch.int32, device=d)
    assert _call(torch.from_numpy(x).to(d), torch.from_numpy(out).to(d), a, b, None, keep, 1, dst, 3) == 0
    got = dst.cpu().numpy()
    assert not got[1, 3:].any() and np.isfinite(got).all() and (got[:, :3] == SENTINEL).all()


def test_refusals_launch_nothing():
    d = G.dev()
    lib = L.load()
    x, out = (torch.from_numpy(t).to(d) for t in _inputs((4, 4)))
    a, b = (torch.tensor(t[:3], device=d) for t in (TAB_A, TAB_B))
    dst = torch.full((3, 6, 4, 4), SENTINEL, device=d)
    both = torch.full((2 * 3 * 3 * 4 * 4,), SENTINEL, device=d)           # dst and a source inside one buffer: a partial overlap
    xin = both[:144].view(3, 3, 4, 4)
    xin.copy_(x)
    half = both[72:72 + 144].view(3, 3, 4, 4)
    BAD = -1
    cases = [(dict(x=None), 'selfcond_x0: x_nchw is NULL'), (dict(out=None), 'selfcond_x0: out_nchw is NULL'),
             (dict(a=None), 'selfcond_x0: tab_a is NULL'), (dict(b=None), 'selfcond_x0: tab_b is NULL'),
             (dict(dst=None), 'selfcond_x0: dst_nchw is NULL'),
             (dict(dims=(0, 3, 4, 4)), 'selfcond_x0: batch, channels, height and width must be positive (got 0, 3, 4, 4)'),
             (dict(dims=(3, -3, 4, 4)), 'selfcond_x0: batch, channels, height and width must be positive (got 3, -3, 4, 4)'),
             (dict(dims=(3, 3, 0, 4)), 'selfcond_x0: batch, channels, height and width must be positive (got 3, 3, 0, 4)'),
             (dict(dims=(3, 3, 4, 0)), 'selfcond_x0: batch, channels, height and width must be positive (got 3, 3, 4, 0)'),
             (dict(first=4), 'selfcond_x0: dst_first_channel 4 + channels 3 exceeds dst_channels 6'),
             (dict(first=-1), 'selfcond_x0: dst_first_channel must not be negative (got -1)'),
             (dict(x=xin, dst=half, first=0), 'selfcond_x0: dst_nchw overlaps x_nchw'),
             (dict(out=xin, dst=half, first=0), 'selfcond_x0: dst_nchw overlaps out_nchw'),
             (dict(dst=x, first=0), 'selfcond_x0: dst_nchw overlaps x_nchw'),
             (dict(dst=out, first=0), 'selfcond_x0: dst_nchw overlaps out_nchw')]
    for kw, text in cases:
        args = dict(x=x, out=out, a=a, b=b, step=None, keep=None, clip=1, dst=dst, first=3, dims=(3, 3, 4, 4))
        args.update(kw)
        rc = _call(**args)
        assert rc == BAD and lib.sr3_last_error().decode() == text, (kw, rc, lib.sr3_last_error())
    assert bool((dst == SENTINEL).all()) and bool((both[144:] == SENTINEL).all())
    assert torch.equal(xin, x) and torch.equal(x.cpu(), torch.from_numpy(_inputs((4, 4))[0]))


# ---- 2. the 9-channel input conv --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('B,Ca,Cb,H,W,Cout', [(2, 6, 3, 3, 32, 32), (2, 6, 3, 4, 64, 64), (2, 3, 6, 1, 32, 128), (2, 9, 0, 5, 24, 8)],
                         ids=['one-block-per-wave', 'four-per-wave', 'single-row', 'valu'])
def test_conv_in_9_channels(B, Ca, Cb, H, W, Cout):
    """sr3_conv_in_f32 against float64 F.conv2d at the tolerance of tests/test_gpu_ops.py::test_conv_in (2e-5 max(1, |ref|))"""
    d = G.dev()
    gen = torch.Generator().manual_seed(31 * H + W + Cout)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    a, b = rnd(B, Ca, H, W), (rnd(B, Cb, H, W) if Cb else None)
    w, bias = rnd(Cout, Ca + Cb, 3, 3) * 0.2, rnd(Cout)
    out = torch.full((B, H, W, Cout), float('nan'), device=d)
    ad, bd, wd, biasd = a.to(d), (None if b is None else b.to(d)), G.ohwi(w).to(d), bias.to(d)
    L.check(L.load().sr3_conv_in_f32(L.ptr(ad), Ca, L.ptr(bd), Cb, B, H, W, L.ptr(wd), L.ptr(biasd), Cout, L.ptr(out), G.stream()))
    torch.cuda.synchronize()
    x = a if b is None else torch.cat([a, b], 1)
    ref = TF.conv2d(x.double(), w.double(), bias.double(), padding=1)
    err = G.assert_close(G.nchw(out).cpu(), ref, what='conv_in 9')
    print('conv_in %s: max abs err %.3e' % ((B, Ca, Cb, H, W, Cout), err))


# ---- the models -------------------------------------------------------------------------------------------------------------------------

_models = {}


def _model(name, phase):
    """one self-conditioned model per (fixture, phase), the widened golden weights loaded: (netG, golden record, state dict)"""
    import model as Model
    if (name, phase) not in _models:
        m = Model.create_model(R.opt9(name, phase=phase))
        g, sd = R.widened(name)
        m.netG.load_state_dict(sd, strict=True)
        m.netG.show_progress = False
        _models[(name, phase)] = (m, g, sd)
    m, g, sd = _models[(name, phase)]
    netG = m.netG
    # every test starts from the same settings
    netG.set_prediction('eps')
    netG.set_sampler(None)
    netG.set_consistency(None)
    netG.set_backprojection(None)
    netG.set_self_condition(0.5)
    netG.use_graph = True
    return netG, g, sd


# ---- 3. the forward of a model whose input conv takes the MFMA form --------------------------------------------------------------------

def test_unet_forward_16x32_inner32():
    d = G.dev()
    netG, g, sd = _model('sr3_seam', 'val')
    gen = torch.Generator().manual_seed(3)
    x, cond = torch.randn(2, 3, 16, 32, generator=gen), torch.rand(2, 6, 16, 32, generator=gen) * 2 - 1
    level = torch.tensor([0.93, 0.41])
    eps = netG.denoise_fn(x.to(d), level.to(d), cond=cond.to(d)).cpu()
    with torch.no_grad():
        ref = O.unet_forward(sd, R.desc9('sr3_seam'), torch.cat([cond, x], 1), level.view(2, 1))
    err = (eps - ref).abs().max().item()
    tol = 2e-5 * max(1.0, ref.abs().max().item())
    print('unet forward 16 x 32: max abs err %.3e (tolerance %.3e)' % (err, tol))
    assert err <= tol
    ops = netG.denoise_fn.plan.op_list(2)
    ci = [i for i, o in enumerate(ops) if o['kind'] == 20]
    assert len(ci) == 1 and ops[ci[0]]['cin'] == 9 and (ops[ci[0]]['h_out'], ops[ci[0]]['w_out']) == (16, 32)
    print('input conv fused its statistics: %d; next op kind %d' % (ops[ci[0]]['fused_output_stats'], ops[ci[0] + 1]['kind']))
    if ops[ci[0]]['fused_output_stats']:
        assert ops[ci[0] + 1]['kind'] != 30, 'a stand-alone statistics pass follows an input conv that fused its statistics'


# ---- 4. the training step ---------------------------------------------------------------------------------------------------------------

FLAGS = [1, 0, 1, 1]


def _train_batch():
    gen = torch.Generator().manual_seed(41)
    hr, sr = (torch.rand(4, 3, 16, 16, generator=gen) * 2 - 1 for _ in range(2))
    z = torch.randn(4, 3, 16, 16, generator=gen)
    gamma = torch.tensor([0.97, 0.85, 0.6, 0.35])
    return hr, sr, z, gamma


_two_pass = {}


def _oracle(sd, prediction):
    if prediction not in _two_pass:
        hr, sr, z, gamma = _train_batch()
        _two_pass[prediction] = R.p_losses_two_pass(sd, R.desc9('sr3_tiny'), hr, sr, gamma, z, FLAGS, prediction)
    return _two_pass[prediction]


def _engine_step(netG, **kw):
    d = G.dev()
    hr, sr, z, gamma = _train_batch()
    loss = netG.p_losses({'HR': hr.to(d), 'SR': kw.pop('sr', sr).to(d)}, noise=z.to(d), gamma=gamma, **kw)
    torch.cuda.synchronize()
    return float(loss), netG.denoise_fn.grad_arena.clone()


@pytest.mark.parametrize('prediction', ['eps', 'v'])
def test_training_step_matches_the_two_pass_oracle(prediction):
    """tolerances of tests/test_gpu_train.py for this model size: loss relative 1e-5, gradients normwise relative 1e-4 where |ref| > 1e-6"""
    netG, g, sd = _model('sr3_tiny', 'train')
    netG.set_prediction(prediction)
    ref_loss, ref_grads, ref_sc = _oracle(sd, prediction)
    loss, _ = _engine_step(netG, self_cond=FLAGS)
    print('%s: loss %.6f, oracle %.6f' % (prediction, loss, ref_loss))
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (loss, ref_loss)
    # what the first pass left in the self-conditioning channels: the flagged images' clamped x0, zeros for the other
    sc = netG._self_cond_buf[:, 3:].cpu()
    assert not sc[1].any() and float((sc.double() - ref_sc).abs().max()) <= 2e-5
    assert torch.equal(netG._self_cond_buf[:, :3].cpu(), _train_batch()[1])
    worst = []
    for key, grad in netG.denoise_fn.named_gradients():
        ref = ref_grads[key]
        num, den = (grad.cpu().double() - ref).norm().item(), max(ref.norm().item(), 1e-7)
        worst.append((num / den, key, den))
    worst.sort(reverse=True)
    print('%s: worst gradients (rel err, key, |ref|): %s' % (prediction, worst[:3]))
    bad = [w for w in worst if w[0] > 1e-4 and w[2] > 1e-6]
    assert not bad, bad[:8]
    # the three new input channels of the first conv get a gradient of their own (an 8-channel pad would have dropped channel 8)
    gw = dict(netG.denoise_fn.named_gradients())['downs.0.weight']
    assert tuple(gw.shape) == (8, 9, 3, 3) and all(float(gw[:, c].abs().max()) > 0 for c in range(9))


def test_training_step_flags_off_and_reproducible():
    netG, g, sd = _model('sr3_tiny', 'train')
    hr, sr, z, gamma = _train_batch()
    # all flags 0: bitwise the plain step on a conditioning tensor whose extra channels are zero (no first pass runs)
    calls = []
    real = netG.denoise_fn.forward
    netG.denoise_fn.forward = lambda *a, **kw: (calls.append(1), real(*a, **kw))[1]
    try:
        l0, g0 = _engine_step(netG, self_cond=[0, 0, 0, 0])
        assert calls == []
        l1, g1 = _engine_step(netG, self_cond=FLAGS)
        assert calls == [1]
    finally:
        del netG.denoise_fn.forward
    netG.set_self_condition(None)
    lp, gp = _engine_step(netG, sr=torch.cat([sr, torch.zeros_like(sr)], 1))
    assert l0 == lp and torch.equal(g0, gp)
    assert l1 != l0 and not torch.equal(g1, g0)                              # the estimate is an input like any other
    netG.set_self_condition(0.5)
    # two runs of the same step: bitwise equal
    l2, g2 = _engine_step(netG, self_cond=FLAGS)
    assert l2 == l1 and torch.equal(g2, g1)
    # drawn flags: prob 1 flags every image, prob 0 none -- and the draws in front of them stay where they were
    netG.set_self_condition(1.0)
    l3, g3 = _engine_step(netG)
    la, ga = _engine_step(netG, self_cond=[1, 1, 1, 1])
    assert l3 == la and torch.equal(g3, ga)
    netG.set_self_condition(0.0)
    l4, g4 = _engine_step(netG)
    assert l4 == l0 and torch.equal(g4, g0)
    # cond_drop zeroes the LR channels only
    netG.set_self_condition(0.5)
    _engine_step(netG, self_cond=FLAGS, cond_keep=[1, 0, 1, 1])
    buf = netG._self_cond_buf.cpu()
    assert not buf[1, :3].any() and torch.equal(buf[0, :3], sr[0]) and bool(buf[0, 3:].any()) and not buf[1, 3:].any()
    netG.set_cond_drop(0.0)


# ---- 5. sampling --------------------------------------------------------------------------------------------------------------------------

def _tables(netG):
    tables, level, t_map, c3, noisy = netG._step_rule()
    tabs = {k: t.cpu().numpy() for k, t in zip(R.KEYS, tables)}
    if c3 is not None:
        tabs['c3'] = c3.cpu().numpy()
    return tabs, level.cpu().numpy(), noisy


def _close(got, want, what):
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    tol = 2e-5 * max(1.0, float(np.abs(want).max()))
    assert err <= tol, '%s: max abs err %.3e > %.3e' % (what, err, tol)
    return err


def _chain(netG, g, sd, seed=17, x0_rule=None):
    """The replayed chain of p_sample_loop, then the same graph replayed by hand from the same start, every step checked against the
    oracle's step from the ENGINE's state before it (image, self-conditioning channels, history, the z the graph drew): the per-step
    tolerance applies to every step.  -> (p_sample_loop's snapshots, the state)"""
    d = G.dev()
    cond, x_T = (torch.from_numpy(g['loop/' + n]).to(d) for n in ('sr', 'x_T'))
    B = cond.shape[0]
    netG.use_graph = True
    netG.p_sample_loop(cond, continous=True, x_T=x_T)                       # (captures)
    torch.manual_seed(seed)
    out = netG.p_sample_loop(cond, continous=True, x_T=x_T).clone()
    st = next(reversed(netG._loop_cache.values()))
    assert st['graph'] is not None and st['self_condition'] is True and tuple(st['cond'].shape) == (B, 6, 16, 16)
    tabs, level, noisy = _tables(netG)
    T = len(tabs['a'])
    assert out.shape[0] == B * (T + 1) and torch.equal(out[:B], cond) and st['step'].tolist()[1] == -1
    st['img'].copy_(x_T)
    st['cond'][:, 3:].zero_()
    if st.get('hist') is not None:
        st['hist'].zero_()
    st['step'].fill_(T - 1)
    torch.manual_seed(seed)
    desc = R.desc9('sr3_tiny')
    worst = 0.0
    for k, j in enumerate(reversed(range(T))):
        x, sc = st['img'].cpu(), st['cond'][:, 3:].cpu()
        hist = st['hist'].cpu().numpy() if st.get('hist') is not None else None
        st['graph'].replay()
        torch.cuda.synchronize()
        assert torch.equal(st['img'], out[(k + 1) * B:(k + 2) * B]), 'the hand-replayed chain is not p_sample_loop\'s at step index %d' % j
        z = st['z'].cpu().numpy() if noisy else None
        rule = None if x0_rule is None else (lambda x0: x0_rule(x0, st))
        new, x0, h1, _ = R.sample_step(sd, desc, cond.cpu(), sc, x, level[j + 1], tabs, j, z, hist, rule)
        e1 = _close(st['img'].cpu().numpy(), new, 'x after step index %d' % j)
        e2 = _close(st['cond'][:, 3:].cpu().numpy(), x0, 'x0 fed back after step index %d' % j)
        print('step index %d: max abs err x %.3e, fed-back x0 %.3e' % (j, e1, e2))
        worst = max(worst, e1, e2)
        assert torch.equal(st['cond'][:, :3], cond)                         # the LR channels are written once
        if hist is not None and x0_rule is None:
            assert torch.equal(st['cond'][:, 3:], st['hist']), 'the x0 fed back is not the tail\'s x0 at step index %d' % j
    assert st['step'].tolist()[1] == -1
    return out, st


@pytest.mark.parametrize('rule', ['ancestral', 'ddim', 'dpmpp_2m'])
def test_replayed_chain_against_the_oracle(rule):
    d = G.dev()
    netG, g, sd = _model('sr3_tiny', 'val')
    if rule != 'ancestral':
        netG.set_sampler(8 if rule == 'ddim' else 5, kind=rule)
    out, st = _chain(netG, g, sd)
    assert bool(torch.isfinite(out).all()) and ('hist' in st) == (rule == 'dpmpp_2m')
    # replayed and eager chains are bitwise equal (the ancestral rule draws its noise: the same seed on both sides)
    cond, x_T = (torch.from_numpy(g['loop/' + n]).to(d) for n in ('sr', 'x_T'))
    netG.use_graph = False
    torch.manual_seed(17)
    eager = netG.p_sample_loop(cond, continous=True, x_T=x_T)
    assert torch.equal(eager, out)
    netG.use_graph = True


def test_every_prediction_runs():
    netG, g, sd = _model('sr3_tiny', 'val')
    for p in ('v', 'x0'):
        netG.set_prediction(p)
        out, _ = _chain(netG, g, sd)
        assert bool(torch.isfinite(out).all())


def test_consistency_rule_on_a_self_conditioned_chain():
    """with "consistency": {"block": 4} the chain runs, the result's block means meet that rule's bound (1e-6 at strength 1,
    tests/test_gpu_consistency.py), and what is fed back is still the network's raw clamped x0, not the projected one"""
    from sr3_hip.diffusion import block_means
    d = G.dev()
    netG, g, sd = _model('sr3_tiny', 'val')
    netG.set_consistency(4)
    cond = torch.from_numpy(g['loop/sr']).to(d)
    y = block_means(cond, 4)
    out, st = _chain(netG, g, sd, x0_rule=lambda x0, st: project(x0, st['ymean'].cpu().numpy(), 4, 1.0))
    assert torch.equal(st['ymean'], y)
    err = float((block_means(out[-2:].contiguous(), 4) - y).abs().max())
    print('consistency error of the self-conditioned result: %.3e' % err)
    assert err <= 1e-6
    # back-projection runs too
    netG.set_consistency(None)
    netG.set_backprojection(4)
    res = netG.p_sample_loop(cond)
    assert bool(torch.isfinite(res).all())
    netG.set_backprojection(None)


def test_item_seeds_make_an_image_independent_of_its_batch():
    """the same noise streams; the engine's rounding between batch sizes is the bound of tests/test_gpu_dist.py (1e-4)"""
    d = G.dev()
    netG, g, sd = _model('sr3_tiny', 'val')
    cond = torch.from_numpy(g['loop/sr']).to(d)
    both = netG.p_sample_loop(cond, continous=True, item_seeds=[101, 202]).clone()
    again = netG.p_sample_loop(cond, continous=True, item_seeds=[101, 202])
    assert torch.equal(both, again)                                         # a second chain starts from zero self-conditioning channels again
    for i, seed in enumerate((101, 202)):
        alone = netG.p_sample_loop(cond[i:i + 1].contiguous(), continous=True, item_seeds=[seed])
        diff = float((both[i::2] - alone).abs().max())
        print('image %d alone against in a batch of 2: max abs diff %.3e' % (i, diff))
        assert diff <= 1e-4
    assert float((both[-2] - both[-1]).abs().max()) > 1e-3


def test_other_models_and_weights():
    """the DDPM variant's ancestral chain, an unconditional SR3 model and EMA weights: each runs, replayed = eager"""
    import model as Model
    d = G.dev()
    for name, shape in (('ddpm_tiny', (2, 3, 16, 16)), ('sr3_uncond', (2, 3, 16, 16))):
        opt = R.opt9(name, prob=0.5)
        opt['model']['unet']['in_channel'] = 6
        m = Model.create_model(opt)
        netG = m.netG
        netG.show_progress = False
        x_T = torch.randn(shape, generator=torch.Generator().manual_seed(2)).to(d)
        outs = []
        for use_graph in (False, True):
            netG.use_graph = use_graph
            torch.manual_seed(23)
            outs.append(netG.p_sample_loop(shape, continous=True, x_T=x_T).clone())
        st = next(reversed(netG._loop_cache.values()))
        assert tuple(st['cond'].shape) == shape and st['self_condition'] and bool(st['cond'].abs().max() > 0)
        assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[1]).all())
    netG, g, sd = _model('sr3_tiny', 'val')
    un = netG.denoise_fn
    un.ema_from_weights()
    cond, x_T = (torch.from_numpy(g['loop/' + n]).to(d) for n in ('sr', 'x_T'))
    torch.manual_seed(29)
    live = netG.p_sample_loop(cond, x_T=x_T).clone()
    with un.use_weights('ema'):
        torch.manual_seed(29)
        ema = netG.p_sample_loop(cond, x_T=x_T).clone()
    assert torch.equal(live, ema)                                           # the EMA is a copy of the weights here: the same chain on the other arena
