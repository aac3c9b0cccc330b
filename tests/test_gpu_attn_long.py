"""Key-blocked attention (csrc/attention_long.hip; mode bit 1 of sr3_attention_ex_f32, plan option attn_long) on the GPU:

  * the kernel per op against float64, at token counts the score-strip kernels cannot hold, ragged N, small / odd C, and forced where
    the strip fits; NaN-filled outputs and NaN guard regions behind qkv and out;
  * its error against float64 next to the strip kernels' on the same data (the project's gate for a second form of one op);
  * whole UNets at 80 x 64 ... 384 x 384 against the reference fixture / the CPU oracle, the captured reverse step, the drop-in
    surface, plan switching.

No refusal is turned into a skip here: every listed shape must run."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_util as G                                # noqa: E402
from helpers import SCHEDS, load_golden, opt_for      # noqa: E402
from sr3_hip import lib as L                        # noqa: E402
from test_gpu_bench_configs import _build           # noqa: E402

GUARD = 4096      # floats of NaN behind every tensor, in the same allocation


def _guarded(t, dev, fill=None):
    """`t` (or a `fill`-filled tensor of its shape) on the device with GUARD NaNs behind it in ONE allocation: (view, whole buffer)."""
    n = t.numel()
    buf = torch.full((n + GUARD,), float('nan'), device=dev, dtype=t.dtype)
    if fill is None:
        buf[:n].copy_(t.reshape(-1))
    else:
        buf[:n].fill_(fill)
    return buf[:n].view(t.shape), buf


def _guard_intact(buf, n):
    return bool(torch.isnan(buf[n:]).all())


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _qkv(B, N, C, kind, seed=11):
    qkv = _rand(B, N, 3 * C, seed=seed)
    if kind == 'heavy':           # log-normal magnitudes: large logits, peaked softmax, a running maximum that moves between chunks
        qkv = qkv.sign() * torch.exp(1.5 * qkv.abs()) * 0.3
    return qkv


def _ref64(qkv, C):
    q, k, v = qkv.double().split(C, dim=2)
    return torch.softmax(q @ k.transpose(1, 2) / math.sqrt(C), -1) @ v


def _attn(qkv, C, mode):
    """sr3_attention_ex_f32 with NaN guards behind qkv and out, out NaN-filled: the output on the CPU."""
    lib, d = L.load(), G.dev()
    B, N, _ = qkv.shape
    qd, _qbuf = _guarded(qkv, d)
    out, obuf = _guarded(torch.empty(B, N, C), d, fill=float('nan'))
    L.check(lib.sr3_attention_ex_f32(L.ptr(qd), B, N, C, L.ptr(out), mode, G.stream()))
    torch.cuda.synchronize()
    assert _guard_intact(obuf, out.numel()), 'the kernel wrote behind the output'
    got = out.cpu()
    assert not torch.isnan(got).any(), 'a NaN inside the output: an unwritten element, or a guard region read into a result'
    return got


LONG_SHAPES = [(1, 2304, 512), (2, 4096, 512), (1, 1900, 512), (1, 9216, 128), (2, 1088, 128), (1, 1280, 16), (2, 100, 48),
               (16, 256, 512), (1, 1337, 256), (3, 40, 128)]


@pytest.mark.parametrize('kind', ['normal', 'heavy'])
@pytest.mark.parametrize('mode', [2, 3])
@pytest.mark.parametrize('B,N,C', LONG_SHAPES, ids=['b%d_n%d_c%d' % s for s in LONG_SHAPES])
def test_key_blocked_attention_against_float64_with_guards(B, N, C, mode, kind):
    qkv = _qkv(B, N, C, kind)
    ref = _ref64(qkv, C)
    got = _attn(qkv, C, mode)
    err = G.assert_close(got, ref, what='key-blocked attention B%d N%d C%d mode %d %s' % (B, N, C, mode, kind))
    print('B%d N%d C%d mode %d %s: max abs err %.2e, |ref|max %.2f' % (B, N, C, mode, kind, err, ref.abs().max().item()))


def test_strip_kernels_keep_their_refusal_at_long_token_counts():
    lib, d = L.load(), G.dev()
    qd = torch.zeros(1, 2304, 3 * 128, device=d)
    out = torch.zeros(1, 2304, 128, device=d)
    for mode in (0, 1):
        with pytest.raises(L.Sr3Error, match='does not fit the LDS score strip'):
            L.check(lib.sr3_attention_ex_f32(L.ptr(qd), 1, 2304, 128, L.ptr(out), mode, G.stream()))
    with pytest.raises(L.Sr3Error, match='does not fit the LDS score strip'):
        L.check(lib.sr3_attention_f32(L.ptr(qd), 1, 2304, 128, L.ptr(out), G.stream()))
    for mode in (2, 3):
        with pytest.raises(L.Sr3Error, match='exceeds 2\\^31 elements'):
            L.check(lib.sr3_attention_ex_f32(L.ptr(qd), 1024, 2304, 512, L.ptr(out), mode, G.stream()))


BOTH_SHAPES = [(16, 256, 512), (4, 64, 512), (2, 1024, 128), (2, 1088, 128)]


@pytest.mark.parametrize('B,N,C', BOTH_SHAPES, ids=['b%d_n%d_c%d' % s for s in BOTH_SHAPES])
def test_key_blocked_error_not_above_the_strip_kernels(B, N, C):
    """Where both forms run: the key-blocked kernel's error against float64 must not exceed the strip kernel's on the same data (rms
    within 5 %, max within 25 % -- 4x on heavy-tailed data, where the max is a noisy statistic: the margins of
    test_attention_split_error_not_above_fp32_mfma), mode 3 against mode 1 and mode 2 against mode 0.  The online form adds one
    rounding per accumulator per 512-key chunk against N roundings in the accumulation itself.  (2, 1088, 128) spans three chunks; at
    1088 tokens the strip side is the staged fp32 kernel in both comparisons, as it is in a plan.  The four figures per case
    are printed before the assertions."""
    for kind in ('normal', 'heavy'):
        qkv = _qkv(B, N, C, kind)
        ref = _ref64(qkv, C)
        for long_mode, strip_mode in ((3, 1), (2, 0)):
            a, a2, s = _attn(qkv, C, long_mode), _attn(qkv, C, long_mode), _attn(qkv, C, strip_mode)
            e_l = G.assert_close(a, ref, what='attention (key-blocked, mode %d, %s)' % (long_mode, kind))
            e_s = G.assert_close(s, ref, what='attention (strip, mode %d, %s)' % (strip_mode, kind))
            rms_l = (a.double() - ref).pow(2).mean().sqrt().item()
            rms_s = (s.double() - ref).pow(2).mean().sqrt().item()
            print('attention B%d N%d C%d %s: max/rms err key-blocked (mode %d) %.2e/%.2e  strip (mode %d) %.2e/%.2e  |ref|max %.2f'
                  % (B, N, C, kind, long_mode, e_l, rms_l, strip_mode, e_s, rms_s, ref.abs().max().item()))
            assert torch.equal(a, a2), 'two runs of the key-blocked kernel differ'
            assert not torch.equal(a, s)                      # (the key-blocked kernel really ran)
            assert rms_l <= 1.05 * rms_s, (rms_l, rms_s)
            assert e_l <= (1.25 if kind == 'normal' else 4.0) * e_s + 1e-8 * ref.abs().max().item(), (e_l, e_s)


# ---- whole UNet ------------------------------------------------------------------------------------------------------------

def _build_long(name):
    netG, sd, desc, opt, c = _build(name)
    netG.denoise_fn.plan.set_option('attn_long', 1)
    return netG, sd, desc, opt, c


@pytest.mark.parametrize('S,B', [(128, 16), (256, 1)])
def test_attn_long_changes_nothing_where_the_strip_fits(S, B):
    netG, sd, desc, opt, c = _build('sr3_16_128')
    d = G.dev()
    x = torch.randn(B, 6, S, S, generator=torch.Generator().manual_seed(3)).to(d)
    lvl = torch.linspace(0.05, 0.999, B).view(B, 1).to(d)
    un = netG.denoise_fn
    base = un(x, lvl).clone()
    ops = un.plan.op_list(B)
    un.plan.set_option('attn_long', 1)
    assert un.plan.op_list(B) == ops and all(o['tile_cfg'] != 24 for o in ops)
    assert torch.equal(un(x, lvl), base)


def _tiny(long_attention=True):
    import model as Model
    opt = opt_for('sr3_tiny', phase='val', gpu=True)
    if long_attention is not None:
        opt['model']['unet']['long_attention'] = long_attention
    m = Model.create_model(opt)
    _, sd = load_golden('sr3_tiny')
    m.netG.load_state_dict(sd, strict=True)
    m.netG.show_progress = False
    return m, sd


@pytest.mark.parametrize('hw', ['80x64', '96x96'])
def test_sr3_tiny_long_against_the_reference_fixture(hw):
    d = G.dev()
    m, sd = _tiny()
    g, _ = load_golden('sr3_long')
    k = hw + '/'
    x, t = torch.from_numpy(g[k + 'unet/x']), torch.from_numpy(g[k + 'unet/time'])
    un = m.netG.denoise_fn
    eps = un(x.to(d), t.to(d)).cpu()
    assert any(o['kind'] == 60 and o['tile_cfg'] == 24 for o in un.plan.op_list(x.shape[0]))
    err = G.assert_close(eps, torch.from_numpy(g[k + 'unet/eps']), what='sr3_tiny %s eps' % hw)
    print('sr3_tiny %s: eps max abs err against the reference %.2e' % (hw, err))
    # the fixture's p_sample step: forward on cat([cond, x]) at the step's noise level, then the engine's step update
    # (to keep the fixture small its inputs are the halves of unet/x: condition = channels 0-2, x_t = channels 3-5)
    from oracle import sr3_oracle as O
    sr, xs, z = x[:, :3].contiguous().to(d), x[:, 3:].contiguous().to(d), torch.from_numpy(g[k + 'step/z']).to(d)
    ts = int(g[k + 'step/t'])
    tab = O.schedule_tables(SCHEDS['sr3_tiny'])
    lvl = torch.full((xs.shape[0], 1), float(tab['sqrt_alphas_cumprod_prev'][ts + 1]), dtype=torch.float32, device=d)
    e = un(xs, lvl, cond=sr)
    xo = xs.clone()
    m.netG._step_update(xo, e, z, step_host=ts)
    G.assert_close(xo.cpu(), torch.from_numpy(g[k + 'step/out']), what='sr3_tiny %s p_sample' % hw)


@pytest.mark.parametrize('name,H,W,B', [('sr3_16_128', 384, 384, 1), ('sr3_16_128', 256, 384, 2), ('ddpm_128', 384, 384, 1)])
def test_fullsize_eps_vs_oracle_beyond_the_score_strip(name, H, W, B):
    from oracle import sr3_oracle as O
    netG, sd, desc, opt, c = _build_long(name)
    d = G.dev()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, desc['in_channel'], H, W, generator=g)
    if name == 'ddpm_128':
        lvl = torch.tensor([1500, 20][:B], dtype=torch.long)
    else:
        lvl = torch.linspace(0.05, 0.999, B).view(B, 1)
    got = netG.denoise_fn(x.to(d), lvl.to(d)).cpu()
    ops = netG.denoise_fn.plan.op_list(B)
    assert any(o['kind'] == 60 and o['tile_cfg'] == 24 for o in ops)
    with torch.no_grad():
        ref = O.unet_forward(sd, desc, x, lvl)
    assert got.shape == ref.shape == (B, 3, H, W)
    err = G.assert_close(got, ref, what='%s weights at %dx%d batch %d' % (name, H, W, B))
    print('%s %dx%d batch %d: eps max abs err %.2e (|ref|max %.2f); attention ops %s' % (
        name, H, W, B, err, ref.abs().max().item(), [(o['h_out'], o['tile_cfg']) for o in ops if o['kind'] == 60]))


def test_reverse_step_captured_at_384x384():
    """sr3_reverse_step captured and replayed at 384 x 384 (attention at 2304 tokens on the key-blocked kernel): bit-identical to the
    three-call form on the same inputs, and a short chain within the 1e-4 drift bound of the CPU oracle over its tail (the bound
    and construction of test_reverse_step_captured_at_128x192)."""
    from oracle import sr3_oracle as O
    netG, sd, desc, opt, c = _build_long('sr3_16_128')
    d = G.dev()
    B, H, W = 1, 384, 384
    shape = (B, 3, H, W)
    tab = O.schedule_tables(opt['model']['beta_schedule']['val'])
    g = torch.Generator().manual_seed(8)
    x0 = torch.randn(shape, generator=g)
    cond = torch.rand(shape, generator=g) * 2 - 1
    netG.denoise_fn.plan.set_geometry(H, W)
    st = netG._loop_state(shape, shape, d)
    netG.denoise_fn.ensure_derived()
    netG._capture(st)
    t = 700
    st['img'].copy_(x0); st['cond'].copy_(cond); st['step'].fill_(t)
    st['graph'].replay()
    torch.cuda.synchronize()
    z = st['z'].clone()
    got = st['img'].clone()
    assert int(st['step'][1].item()) == t - 1
    x = x0.to(d)
    lvl = torch.full((B,), float(tab['sqrt_alphas_cumprod_prev'][t + 1]), dtype=torch.float32, device=d)
    eps = netG.denoise_fn(x, lvl, cond=cond.to(d))
    assert torch.equal(eps, st['eps'])
    netG._step_update(x, eps, z, step_host=t)
    assert torch.equal(x, got), 'captured reverse step != forward + p_sample update'
    STEPS, TAIL = 6, 3
    st['img'].copy_(x0); st['step'].fill_(STEPS - 1)
    zs, keep = {}, None
    for i in reversed(range(STEPS)):
        if i + 1 == TAIL:
            keep = st['img'][:1].clone()
        st['graph'].replay()
        zs[i] = st['z'][:1].cpu()
    torch.cuda.synchronize()
    xc = keep.cpu()
    with torch.no_grad():
        for i in reversed(range(TAIL)):
            xc = O.p_sample(sd, desc, tab, xc, i, zs[i], condition_x=cond[:1])
    err = (st['img'][:1].cpu() - xc).abs().max().item()
    print('384x384 chain: CPU oracle over the last %d of %d steps: max |engine - oracle| = %.1e' % (TAIL, STEPS, err))
    assert err <= 1e-4, err


def test_dropin_with_and_without_the_config_key():
    d = G.dev()
    g, _ = load_golden('sr3_long')
    sr = torch.from_numpy(g['96x96/unet/x'][:, :3]).clamp(-1, 1).contiguous()
    m, sd = _tiny(long_attention=True)
    assert m.netG.denoise_fn.plan.options.get('attn_long') == 1
    torch.manual_seed(5)
    m.feed_data({'HR': sr.clone(), 'SR': sr})
    m.test(continous=False)
    assert tuple(m.SR.shape) == (3, 96, 96) and bool(torch.isfinite(m.SR).all())
    torch.manual_seed(5)
    again = m.netG.p_sample_loop(sr.to(d), continous=False)
    assert torch.equal(m.SR.to(d).reshape(again.shape), again)
    m0, _ = _tiny(long_attention=None)
    m0.feed_data({'HR': sr.clone(), 'SR': sr})
    with pytest.raises(L.Sr3Error) as ei:
        m0.test(continous=False)
    assert '2304 tokens' in str(ei.value) and 'long_attention' in str(ei.value)


def test_switching_across_the_long_kernel_is_bit_stable():
    netG, sd, desc, opt, c = _build_long('sr3_16_128')
    d = G.dev()
    g = torch.Generator().manual_seed(6)
    xa = torch.randn(1, 6, 128, 128, generator=g).to(d)
    xb = torch.randn(1, 6, 384, 384, generator=g).to(d)
    lvl = torch.tensor([0.4], device=d).view(1, 1)
    un = netG.denoise_fn
    first = un(xa, lvl).clone()
    mid = un(xb, lvl).clone()
    assert mid.shape == (1, 3, 384, 384) and bool(torch.isfinite(mid).all())
    assert any(o['tile_cfg'] == 24 for o in un.plan.op_list(1))
    third = un(xa, lvl).clone()
    assert torch.equal(first, third)
    assert all(o['tile_cfg'] != 24 for o in un.plan.op_list(1))
    fresh, _, _, _, _ = _build('sr3_16_128')
    assert torch.equal(fresh.denoise_fn(xa, lvl), first)
