"""Image sizes other than the config's image_size (sr3_plan_set_geometry) on the GPU, everything through the C ABI / the drop-in
package, references on the CPU:

  * the ragged instantiation of the two-workgroup Winograd kernel (tile 23) per op against float64, with NaN-filled outputs and
    NaN-filled guard regions behind every tensor (nothing outside B*H*W*Cout may be written, nothing outside an input may be read
    into a result), fused statistics against float64 sums, split-K, and the project's accuracy gate for the split arithmetic;
  * the whole UNet at rectangular / non-native sizes against the CPU oracle, the captured reverse step, plan switching;
  * the drop-in surface (feed_data / test / a validation loader with mixed sizes).

No refusal is turned into a skip here: every listed geometry must run."""
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


def conv_call_guarded(src0, src1, w, bias=None, ss=None, act=0, film=None, res0=None, res1=None, ups=0, tile_cfg=23, ksplit=1,
                      want_stats=False):
    """gpu_util.conv_call for 3x3 stride-1 problems with every activation-sized tensor followed by a NaN guard: returns
    (out NCHW cpu, stats [B,Cout,2] cpu or None); asserts that nothing was written behind the output or the statistics."""
    lib, d = L.load(), G.dev()
    B, C0, Hs, Ws = src0.shape
    C1 = 0 if src1 is None else src1.shape[1]
    Cout, Cin = w.shape[0], w.shape[1]
    Ho, Wo = Hs << ups, Ws << ups
    s0, _ = _guarded(G.nhwc(src0), d)
    s1 = None if src1 is None else _guarded(G.nhwc(src1), d)[0]
    r0 = None if res0 is None else _guarded(G.nhwc(res0), d)[0]
    r1 = None if res1 is None else _guarded(G.nhwc(res1), d)[0]
    g = lambda t: None if t is None else t.contiguous().to(d)
    wd, bd, ssd, fd = g(G.ohwi(w)), g(bias), g(ss), g(film)
    out, obuf = _guarded(torch.empty(B, Ho, Wo, Cout), d, fill=float('nan'))
    stats = sbuf = None
    if want_stats:
        # 0: no fused statistics for this problem (a split-K reduce whose row blocks do not divide the map: a plan then runs the
        # stand-alone pass); the direct epilogue always has them
        T = int(lib.sr3_conv_stats_slices(B, Hs, Ws, ups, Cin, Cout, tile_cfg, ksplit))
        assert T > 0 or ksplit != 1
        if T > 0:
            stats, sbuf = _guarded(torch.empty(B, T, Cout, 2, dtype=torch.float64), d, fill=float('nan'))
    nb = int(lib.sr3_conv_scratch_bytes(B, Ho, Wo, Cin, Cout, 3, tile_cfg, ksplit))
    scratch = torch.empty(max(nb, 16), dtype=torch.uint8, device=d)
    L.check(lib.sr3_conv_f32(L.ptr(s0), C0, L.ptr(s1), C1, B, Hs, Ws, ups, 1, 3, Cout, L.ptr(wd), L.ptr(bd), L.ptr(ssd), act, L.ptr(fd),
                             0 if film is None else film.shape[1], L.ptr(r0), 0 if res0 is None else res0.shape[1], L.ptr(r1),
                             0 if res1 is None else res1.shape[1], L.ptr(out), L.ptr(stats), tile_cfg, ksplit, L.ptr(scratch), nb,
                             G.stream()))
    torch.cuda.synchronize()
    assert _guard_intact(obuf, out.numel()), 'the kernel wrote behind the output'
    if sbuf is not None:
        assert _guard_intact(sbuf, stats.numel()), 'the kernel wrote behind the statistics'
    return G.nchw(out).cpu(), (None if stats is None else stats.cpu().sum(1))


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _problem(B, C0, C1, H, W, Cout, ups, act, film, res, seed, Hp=None, Wp=None):
    """A fused conv problem on H x W SOURCE maps and -- same seeds, so the same values wherever both exist -- the problem on
    Hp x Wp >= H x W maps it is the top-left crop of.  Returns (small problem, padded problem) as (src0, src1, w, kwargs)."""
    Hp, Wp = Hp or H, Wp or W
    Cin = C0 + C1
    big0 = _rand(B, C0, Hp, Wp, seed=seed)
    big1 = _rand(B, C1, Hp, Wp, seed=seed + 1) if C1 else None
    w = _rand(Cout, Cin, 3, 3, seed=seed + 2, scale=1.0 / math.sqrt(Cin * 9))
    kw = dict(ups=ups, act=act, bias=_rand(Cout, seed=seed + 3))
    if act:
        kw['ss'] = torch.stack([_rand(B, Cin, seed=seed + 4) * 0.3 + 1.0, _rand(B, Cin, seed=seed + 5) * 0.3], dim=2).contiguous()
    if film:
        kw['film'] = _rand(B, Cout, seed=seed + 6)
    bigres = None
    if res == 'concat':           # identity residual: the (two-source) input itself
        assert Cout == Cin and ups == 0
    elif res:
        bigres = _rand(B, Cout, Hp << ups, Wp << ups, seed=seed + 7)

    def cut(t, h, w_):
        return None if t is None else t[:, :, :h, :w_].contiguous()
    out = []
    for h, w_ in ((H, W), (Hp, Wp)):
        k = dict(kw)
        a0, a1 = cut(big0, h, w_), cut(big1, h, w_)
        if res == 'concat':
            k['res0'], k['res1'] = a0, a1
        elif res:
            k['res0'] = cut(bigres, h << ups, w_ << ups)
        out.append((a0, a1, w, k))
    return out


# name, B, C0, C1, H, W (source), Cout, ups, act, film, res  -- output maps (8,24) (12,24) (11,22) (24,40) (44,88)
RAGGED_CASES = [
    ('r8x24_two_src_idres', 3, 32, 32, 8, 24, 64, 0, 2, True, 'concat'),
    ('r12x24_concat_film', 2, 48, 16, 12, 24, 72, 0, 2, True, False),
    ('r11x22_odd_res', 3, 64, 0, 11, 22, 40, 0, 1, False, True),
    ('r11x22_plain', 2, 24, 8, 11, 22, 96, 0, 0, False, False),
    ('r24x40_up_from_12x20', 2, 64, 0, 12, 20, 64, 1, 0, False, False),
    ('r24x40_deep', 1, 256, 128, 24, 40, 128, 0, 2, True, True),
    ('r44x88_up_from_22x44', 1, 32, 0, 22, 44, 40, 1, 2, True, True),
    ('r44x88_concat', 2, 64, 32, 44, 88, 64, 0, 2, True, 'res'),
]


@pytest.mark.parametrize('ksplit', [1, 2, 0])
@pytest.mark.parametrize('case', RAGGED_CASES, ids=[c[0] for c in RAGGED_CASES])
def test_ragged_tile_against_float64_with_guards(case, ksplit):
    name, B, C0, C1, H, W, Cout, ups, act, film, res = case
    (s0, s1, w, kw), _ = _problem(B, C0, C1, H, W, Cout, ups, act, film, res, seed=21)
    ref = G.conv_ref(s0, s1, w, **kw)
    got, st = conv_call_guarded(s0, s1, w, tile_cfg=23, ksplit=ksplit, want_stats=True, **kw)
    assert got.shape == ref.shape
    assert not torch.isnan(got).any(), 'a NaN inside the output: an unwritten pixel, or a guard region read into a result'
    err = G.assert_close(got, ref, what='%s ks%d (tile 23)' % (name, ksplit))
    print('%s ks%d: max abs err %.2e, |ref|max %.2f' % (name, ksplit, err, ref.abs().max().item()))
    assert st is not None or ksplit != 1
    if st is not None:
        assert torch.allclose(st[:, :, 0], got.double().sum(dim=(2, 3)), rtol=1e-9, atol=1e-9)
        assert torch.allclose(st[:, :, 1], (got.double() ** 2).sum(dim=(2, 3)), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize('ksplit', [1, 2])
@pytest.mark.parametrize('case', RAGGED_CASES, ids=[c[0] for c in RAGGED_CASES])
def test_ragged_tile_error_not_above_fp32_winograd(case, ksplit):
    """The project's gate for the 3 x bf16 split arithmetic (test_winograd_split_error_not_above_fp32_winograd: rms within 5 %, max
    within 25 % of the exact-fp32 Winograd kernel's error against float64), for tile 23.  The fp32 kernel (tile 11) does not take a
    ragged map, so it runs the PADDED problem: the same tensors continued (same seeds) to the next multiple of 16 of the output map.
    Both errors are taken over the pixels of the ragged map, each against the float64 result of the problem its kernel ran: every
    pixel but the last row / column has the same inputs in both, the last row / column sees data instead of zero padding."""
    name, B, C0, C1, H, W, Cout, ups, act, film, res = case
    up = lambda v: (-(-(v << ups) // 16) * 16) >> ups
    small, big = _problem(B, C0, C1, H, W, Cout, ups, act, film, res, seed=21, Hp=up(H), Wp=up(W))
    Ho, Wo = H << ups, W << ups
    ref_s = G.conv_ref(small[0], small[1], small[2], **small[3])
    ref_b = G.conv_ref(big[0], big[1], big[2], **big[3])[:, :, :Ho, :Wo]
    got, _ = conv_call_guarded(small[0], small[1], small[2], tile_cfg=23, ksplit=ksplit, **small[3])
    base, _ = G.conv_call(big[0], big[1], big[2], tile_cfg=11, ksplit=ksplit, stride=1, **big[3])
    base = base[:, :, :Ho, :Wo]
    e_s = G.assert_close(got, ref_s, what=name + ' (tile 23)')
    e_w = G.assert_close(base, ref_b, what=name + ' (tile 11, padded problem)')
    rms_s = (got.double() - ref_s).pow(2).mean().sqrt().item()
    rms_w = (base.double() - ref_b).pow(2).mean().sqrt().item()
    print('%s ks%d: max/rms err ragged split %.2e/%.2e  fp32 Winograd (padded) %.2e/%.2e  |ref|max %.2f'
          % (name, ksplit, e_s, rms_s, e_w, rms_w, ref_s.abs().max().item()))
    assert rms_s <= 1.05 * rms_w, (rms_s, rms_w)
    assert e_s <= 1.25 * e_w + 1e-8 * ref_s.abs().max().item(), (e_s, e_w)


@pytest.mark.parametrize('ksplit', [1, 2])
def test_ragged_tile_on_a_whole_multiple_gives_the_bits_of_tile_13(ksplit):
    (s0, s1, w, kw), _ = _problem(2, 48, 16, 24, 32, 72, 0, 2, True, True, seed=5)
    a, sa = G.conv_call(s0, s1, w, tile_cfg=13, ksplit=ksplit, want_stats=True, **kw)
    b, sb = conv_call_guarded(s0, s1, w, tile_cfg=23, ksplit=ksplit, want_stats=True, **kw)
    assert torch.equal(a, b) and torch.equal(sa, sb)


def test_tile_13_keeps_its_refusal_on_ragged_maps():
    (s0, s1, w, kw), _ = _problem(2, 32, 0, 12, 24, 64, 0, 0, False, False, seed=5)
    with pytest.raises(L.Sr3Error, match='does not fit'):
        G.conv_call(s0, s1, w, tile_cfg=13, ksplit=1, **kw)


# ---- whole UNet ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('H,W,B', [(128, 192, 4), (176, 128, 2), (64, 64, 16), (256, 256, 1)])
def test_fullsize_sr3_eps_vs_oracle(H, W, B):
    from oracle import sr3_oracle as O
    netG, sd, desc, opt, c = _build('sr3_16_128')
    d = G.dev()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 6, H, W, generator=g)
    lvl = torch.linspace(0.05, 0.999, B).view(B, 1)
    got = netG.denoise_fn(x.to(d), lvl.to(d)).cpu()
    tiles = sorted(set(o['tile_cfg'] for o in netG.denoise_fn.plan.op_list(B) if o['kind'] == 50))
    with torch.no_grad():
        ref = O.unet_forward(sd, desc, x, lvl)
    assert got.shape == ref.shape == (B, 3, H, W)
    err = G.assert_close(got, ref, what='SR3 16->128 weights at %dx%d batch %d' % (H, W, B))
    print('%dx%d batch %d: eps max abs err %.2e (|ref|max %.2f); conv tiles %s' % (H, W, B, err, ref.abs().max().item(), tiles))
    if (H, W) in ((128, 192), (176, 128)):
        assert 23 in tiles


def test_ddpm_128_eps_vs_oracle_at_128x160():
    from oracle import sr3_oracle as O
    netG, sd, desc, opt, c = _build('ddpm_128')
    d = G.dev()
    B, H, W = 2, 128, 160          # mults [1,1,2,2,4,4]: multiples of 32; levels down to 4 x 5
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, 3, H, W, generator=g)
    t = torch.tensor([1500, 20], dtype=torch.long)
    got = netG.denoise_fn(x.to(d), t.to(d)).cpu()
    with torch.no_grad():
        ref = O.unet_forward(sd, desc, x, t)
    err = G.assert_close(got, ref, what='DDPM-128 at 128x160')
    print('DDPM-128 at 128x160: eps max abs err %.2e' % err)


def _tiny(dev):
    import model as Model
    m = Model.create_model(opt_for('sr3_tiny', phase='val', gpu=True))
    _, sd = load_golden('sr3_tiny')
    m.netG.load_state_dict(sd, strict=True)
    m.netG.show_progress = False
    return m, sd


@pytest.mark.parametrize('hw', ['16x24', '24x16'])
def test_sr3_tiny_rect_against_the_reference_fixture(hw):
    d = G.dev()
    m, sd = _tiny(d)
    g, _ = load_golden('sr3_rect')
    k = hw + '/'
    x, t = torch.from_numpy(g[k + 'unet/x']), torch.from_numpy(g[k + 'unet/time'])
    eps = m.netG.denoise_fn(x.to(d), t.to(d)).cpu()
    G.assert_close(eps, torch.from_numpy(g[k + 'unet/eps']), what='sr3_tiny %s eps' % hw)
    sr, x_T, zs = (torch.from_numpy(g[k + n]) for n in ('loop/sr', 'loop/x_T', 'loop/zs'))
    out = m.netG.p_sample_loop(sr.to(d), continous=True, x_T=x_T.to(d), noise_seq=zs.to(d)).cpu()
    ref = torch.from_numpy(g[k + 'loop/ret_continous'])
    assert out.shape == ref.shape
    assert (out - ref).abs().max().item() <= 1e-4


def test_reverse_step_captured_at_128x192():
    """sr3_reverse_step captured and replayed at 128 x 192: bit-identical to the three-call form (forward, p_sample update, counter
    decrement) on the same inputs, and a short chain within the 1e-4 drift bound of the CPU oracle over its tail."""
    from oracle import sr3_oracle as O
    netG, sd, desc, opt, c = _build('sr3_16_128')
    d = G.dev()
    B, H, W = 2, 128, 192
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
    # three-call form
    x = x0.to(d)
    lvl = torch.full((B,), float(tab['sqrt_alphas_cumprod_prev'][t + 1]), dtype=torch.float32, device=d)
    eps = netG.denoise_fn(x, lvl, cond=cond.to(d))
    assert torch.equal(eps, st['eps'])
    netG._step_update(x, eps, z, step_host=t)
    assert torch.equal(x, got), 'captured reverse step != forward + p_sample update'
    # short chain: the last TAIL steps of the schedule, CPU oracle on the first image from the engine's own state
    STEPS, TAIL = 12, 5
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
    print('128x192 chain: CPU oracle over the last %d of %d steps: max |engine - oracle| = %.1e' % (TAIL, STEPS, err))
    assert err <= 1e-4, err


def test_switching_geometries_on_one_plan_is_bit_stable():
    netG, sd, desc, opt, c = _build('sr3_16_128')
    d = G.dev()
    B = 2
    g = torch.Generator().manual_seed(6)
    xa = torch.randn(B, 6, 128, 128, generator=g).to(d)
    xb = torch.randn(B, 6, 128, 192, generator=g).to(d)
    lvl = torch.tensor([0.3, 0.9], device=d).view(B, 1)
    un = netG.denoise_fn
    first = un(xa, lvl).clone()
    assert un.plan.geometry == (128, 128)
    mid = un(xb, lvl).clone()
    assert un.plan.geometry == (128, 192) and mid.shape == (B, 3, 128, 192) and bool(torch.isfinite(mid).all())
    third = un(xa, lvl).clone()
    assert torch.equal(first, third)
    fresh, _, _, _, _ = _build('sr3_16_128')
    assert torch.equal(fresh.denoise_fn(xa, lvl), first)
    # the graph cache: one state per (shape, launch list); going back does not recapture, and never replays another size's graph
    sa, sb = (B, 3, 128, 128), (B, 3, 128, 192)
    un.plan.set_geometry(128, 128)
    s1 = netG._loop_state(sa, sa, d)
    un.plan.set_geometry(128, 192)
    s2 = netG._loop_state(sb, sb, d)
    un.plan.set_geometry(128, 128)
    assert netG._loop_state(sa, sa, d) is s1 and s1 is not s2 and s2['img'].shape == sb
    # errors that stay errors
    with pytest.raises(L.Sr3Error, match='multiples of 16'):
        un(torch.randn(B, 6, 130, 128, device=d), lvl)
    with pytest.raises(L.Sr3Error, match='does not match the plan'):
        un(torch.randn(B, 5, 128, 128, device=d), lvl)
    assert torch.equal(un(xa, lvl), first)


# ---- drop-in ---------------------------------------------------------------------------------------------------------------

def test_dropin_test_continous_on_a_16x24_item():
    d = G.dev()
    m, sd = _tiny(d)
    g, _ = load_golden('sr3_rect')
    sr = torch.from_numpy(g['16x24/loop/sr'])
    m.feed_data({'HR': sr.clone(), 'SR': sr})
    m.test(continous=True)
    T = SCHEDS['sr3_tiny']['n_timestep']
    n_snap = sum(1 for i in range(T) if i % (1 | (T // 10)) == 0)
    assert tuple(m.SR.shape) == (sr.shape[0] * (1 + n_snap), 3, 16, 24) == tuple(g['16x24/loop/ret_continous'].shape)
    assert bool(torch.isfinite(m.SR).all())
    vis = m.get_current_visuals()
    assert tuple(vis['SR'].shape) == tuple(m.SR.shape) and tuple(vis['INF'].shape) == (sr.shape[0], 3, 16, 24)
    m.test(continous=False)
    assert tuple(m.SR.shape) == (3, 16, 24)


def test_validation_wave_of_mixed_sizes_equals_the_items_alone():
    """Items of sizes A, A, B, A in one wave: only equal sizes share a chain, and with the per-item noise streams every item's image is
    the one it gets alone (same kernels: the ragged / small maps of sr3_tiny do not change tile with the batch; allow rounding)."""
    from sr3_hip.dist import ValWave
    d = G.dev()
    m, sd = _tiny(d)
    g = torch.Generator().manual_seed(12)
    sizes = [(16, 24), (16, 24), (24, 16), (16, 24)]
    conds = [(torch.rand(1, 3, h, w, generator=g) * 2 - 1).to(d) for h, w in sizes]
    wave = ValWave(conds, first_item=0, streams=True)
    m.netG.eval()
    got = [wave.result(m.netG, i, False) for i in range(4)]
    for i, (h, w) in enumerate(sizes):
        assert tuple(got[i].shape) == (3, h, w)
        alone = ValWave([conds[i]], first_item=i, streams=True).result(m.netG, 0, False)
        assert (got[i] - alone).abs().max().item() <= 1e-4, i
    assert not torch.equal(got[0], got[1])
