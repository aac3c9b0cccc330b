"""Per-op parity of the HIP kernels (through the C ABI) against float64 CPU references.
Tolerance: 2e-5 * max(1, |ref|_inf)  (~10x the reference's own fp32 reorder noise)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sr3_hip import lib as L                      # noqa: E402
import gpu_util as G                              # noqa: E402


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


DROP_CASES = [
    # name, B, C0, H, W, Cout, X0, X1 (fused res_conv sources, 0 = none), residual, tile_cfg, ksplit
    ('cfg5_16x16', 2, 64, 16, 16, 128, 0, 0, True, 5, 1),
    ('cfg5_x2', 2, 128, 16, 16, 128, 96, 32, False, 5, 1),
    ('cfg5_splitk', 3, 128, 8, 8, 128, 0, 0, True, 5, 2),
    ('cfg6_8wave_64x32', 2, 64, 32, 16, 64, 0, 0, True, 6, 1),
    ('cfg6_8wave_x2', 1, 64, 32, 32, 64, 64, 32, False, 6, 1),
    ('im2col_small', 3, 32, 4, 4, 32, 0, 0, True, 3, 1),
    ('auto', 2, 64, 16, 16, 64, 0, 0, True, 0, 0),
    # the geometries of the B = 64 training plan bench.py times (C3): 128^2 layers on the 8-wave 64x32 form of the
    # 256x64 tile, 64^2 layers on the 128x128 tile (the plan swaps the 8-wave 256x128 tile out for dropout convs)
    ('c3_128sq_64to64_x2_192', 1, 64, 128, 128, 64, 128, 64, False, 6, 1),
    ('c3_64sq_128to128_x2_256', 1, 128, 64, 64, 128, 128, 128, False, 5, 1),
    # round 3: the Winograd kernel's dropout instantiation (what the training plan's block2 convs run on maps >= 16x16)
    ('wino_16x16', 2, 64, 16, 16, 128, 0, 0, True, 11, 1),
    ('wino_splitk', 2, 128, 16, 16, 64, 0, 0, True, 11, 2),
    ('wino_c3_64sq_128to128', 1, 128, 64, 64, 128, 0, 0, True, 11, 1),
    ('wino_c3_128sq_64to64', 1, 64, 128, 128, 64, 0, 0, False, 11, 1),
    # round 4: the dropout form of the 3 x bf16 split instantiation (tile 12: what the training plan's block2 convs run)
    ('wino_split_16x16', 2, 64, 16, 16, 128, 0, 0, True, 12, 1),
    ('wino_split_splitk', 2, 128, 16, 16, 64, 0, 0, True, 12, 2),
    ('wino_split_c3_64sq_128to128', 1, 128, 64, 64, 128, 0, 0, True, 12, 1),
    # round 4: the four-image tile of the 8x8 maps (split-K only)
    ('wino_8x8_b4', 4, 128, 8, 8, 128, 0, 0, True, 11, 2),
    ('wino_8x8_b8_512', 8, 512, 8, 8, 64, 0, 0, False, 11, 0),
]


@pytest.mark.parametrize('case', DROP_CASES, ids=[c[0] for c in DROP_CASES])
def test_conv_dropout(case):
    """Train-mode Block: conv3x3(dropout(silu(gn(x)))) (+ fused res_conv) through sr3_conv_dropout_f32 vs a float64
    reference that applies the same counter-based mask (oracle.sr3_oracle.hash32 restates the engine's hash)."""
    import numpy as np
    import torch.nn.functional as F
    from oracle import sr3_oracle as O
    name, B, C0, H, W, Cout, X0, X1, use_res, tile_cfg, ksplit = case
    lib = L.load()
    d = G.dev()
    p_drop, seed = 0.2, 0x1234ABCD
    cc = ('drop', B, C0, 0, H, W, Cout, 3, 1, 0, 2, True, use_res, True)
    src0, _, w, kw = _make_case(cc, seed=31)
    # float64 reference with the engine's mask (NHWC linear index of the activated input)
    x = src0.double() * kw['ss'][:, :, 0].double()[:, :, None, None] + kw['ss'][:, :, 1].double()[:, :, None, None]
    x = x * torch.sigmoid(x)
    idx = ((np.arange(B)[:, None, None, None] * H + np.arange(H)[None, None, :, None]) * W
           + np.arange(W)[None, None, None, :]) * C0 + np.arange(C0)[None, :, None, None]
    with np.errstate(over='ignore'):
        hv = O.hash32(idx.astype(np.uint32) * np.uint32(0x9E3779B9) + np.uint32(seed))
    keep = torch.from_numpy((hv >= np.uint32(int(p_drop * 4294967296.0))).astype(np.float64))
    assert 0.75 < keep.mean().item() < 0.85
    x = x * keep * float(np.float32(1.0 / (1.0 - p_drop)))
    ref = F.conv2d(x, w.double(), kw['bias'].double(), padding=1) + kw['film'].double()[:, :, None, None]
    if use_res:
        ref = ref + kw['res0'].double()
    g = lambda t: None if t is None else t.to(d)
    x2a = x2b = w2 = b2 = None
    if X0:
        x2a = _rand(B, X0, H, W, seed=41)
        x2b = _rand(B, X1, H, W, seed=42) if X1 else None
        w2 = _rand(Cout, X0 + X1, 1, 1, seed=43) * 0.1
        b2 = _rand(Cout, seed=44)
        ref = ref + F.conv2d((x2a if x2b is None else torch.cat([x2a, x2b], 1)).double(), w2.double(), b2.double())
    dv = dict(s0=g(G.nhwc(src0)), w=g(G.ohwi(w)), bias=g(kw['bias']), ss=g(kw['ss']), film=g(kw['film']),
              res=g(G.nhwc(kw['res0'])) if use_res else None,
              x2a=None if x2a is None else g(G.nhwc(x2a)), x2b=None if x2b is None else g(G.nhwc(x2b)),
              w2=None if w2 is None else g(w2.reshape(Cout, -1).contiguous()), b2=g(b2))
    out = torch.full((B, H, W, Cout), float('nan'), device=d)
    nb = int(lib.sr3_conv_scratch_bytes(B, H, W, C0, Cout, 3, tile_cfg, ksplit))
    scratch = torch.empty(max(nb, 16), dtype=torch.uint8, device=d)
    L.check(lib.sr3_conv_dropout_f32(L.ptr(dv['s0']), C0, B, H, W, Cout, L.ptr(dv['w']), L.ptr(dv['bias']), L.ptr(dv['ss']),
                                     2, L.ptr(dv['film']), Cout, L.ptr(dv['res']), Cout, L.ptr(dv['x2a']), X0,
                                     L.ptr(dv['x2b']), X1, L.ptr(dv['w2']), L.ptr(dv['b2']), L.ptr(out), None, tile_cfg,
                                     ksplit, L.ptr(scratch), nb, seed, p_drop, G.stream()))
    torch.cuda.synchronize()
    G.assert_close(G.nchw(out).cpu(), ref, what='dropout conv ' + name)


CONV_CASES = [
    # name, B, C0, C1, H, W, Cout, k, stride, ups, act, film, res, bias
    ('plain3x3', 2, 64, 0, 16, 16, 64, 3, 1, 0, 0, False, False, True),
    ('gn_silu_film', 2, 64, 0, 16, 16, 128, 3, 1, 0, 2, True, False, True),
    ('gn_silu_res', 2, 128, 0, 8, 8, 128, 3, 1, 0, 2, False, True, True),
    ('concat', 2, 64, 32, 16, 16, 64, 3, 1, 0, 2, True, False, True),
    ('concat_idres', 1, 32, 32, 8, 8, 64, 3, 1, 0, 2, False, 'concat', True),
    ('stride2', 2, 64, 0, 16, 16, 64, 3, 2, 0, 0, False, False, True),
    ('upsample', 2, 64, 0, 8, 8, 64, 3, 1, 1, 0, False, False, True),
    ('k1_affine_nobias', 2, 64, 0, 8, 8, 192, 1, 1, 0, 1, False, False, False),
    ('k1_res', 2, 96, 0, 8, 8, 64, 1, 1, 0, 0, False, True, True),
    ('ragged', 3, 24, 0, 10, 10, 40, 3, 1, 0, 2, True, True, True),
    ('ragged_concat_k1', 3, 8, 12, 6, 10, 24, 1, 1, 0, 0, False, False, True),
    ('tiny_img', 5, 32, 0, 4, 4, 32, 3, 1, 0, 2, True, True, True),
    ('deepK', 1, 512, 512, 8, 8, 64, 3, 1, 0, 2, False, False, True),
    ('halo_oddB', 3, 32, 0, 8, 8, 64, 3, 1, 0, 2, True, True, True),
    ('halo_32x32_up', 1, 64, 0, 16, 16, 128, 3, 1, 1, 2, True, True, True),
    ('halo_concat_seam', 2, 48, 16, 16, 32, 96, 3, 1, 0, 2, False, 'res', True),
]


def _make_case(case, seed=1):
    name, B, C0, C1, H, W, Cout, k, stride, ups, act, film, res, bias = case
    Cin = C0 + C1
    src0 = _rand(B, C0, H, W, seed=seed)
    src1 = _rand(B, C1, H, W, seed=seed + 1) if C1 else None
    w = _rand(Cout, Cin, k, k, seed=seed + 2, scale=1.0 / math.sqrt(Cin * k * k))
    kw = dict(ups=ups, stride=stride, act=act)
    if bias:
        kw['bias'] = _rand(Cout, seed=seed + 3)
    if act:
        ss = torch.stack([_rand(B, Cin, seed=seed + 4) * 0.3 + 1.0, _rand(B, Cin, seed=seed + 5) * 0.3], dim=2)
        kw['ss'] = ss.contiguous()
    if film:
        kw['film'] = _rand(B, Cout, seed=seed + 6)
    pad = k // 2
    Ho = ((H << ups) + 2 * pad - k) // stride + 1
    Wo = ((W << ups) + 2 * pad - k) // stride + 1
    if res == 'concat':
        kw['res0'], kw['res1'] = src0, src1
    elif res:
        kw['res0'] = _rand(B, Cout, Ho, Wo, seed=seed + 7)
    return src0, src1, w, kw


@pytest.mark.parametrize('case', CONV_CASES, ids=[c[0] for c in CONV_CASES])
@pytest.mark.parametrize('tile_cfg,ksplit', [(0, 0), (1, 1), (2, 1), (3, 1), (4, 1), (1, 3), (3, 2), (5, 1), (6, 1), (5, 2),
                                             (6, 2), (7, 1), (8, 1), (7, 2), (9, 1), (10, 1), (9, 2), (10, 3),
                                             (11, 1), (11, 2), (11, 0),
                                             (14, 1), (15, 1), (16, 1), (17, 1), (14, 3), (16, 2)])
def test_conv(case, tile_cfg, ksplit):
    src0, src1, w, kw = _make_case(case)
    # a refusal is asserted, never skipped on: the halo and Winograd tiles by their restated rules (gpu_util); the im2col tiles refuse
    # nothing -- with more splits than k-steps (conv_igemm_forward launches them all) the splits past the last k-step write zero slabs
    # and the reduce still gives the conv
    why = G.conv_expected_refusal(src0.shape[0], w.shape[1], w.shape[0], src0.shape[2], src0.shape[3], kw['ups'], tile_cfg, ksplit,
                                  k=w.shape[2], stride=kw['stride'])
    if why:
        with pytest.raises(L.Sr3Error, match=why):
            G.conv_call(src0, src1, w, tile_cfg=tile_cfg, ksplit=ksplit, **kw)
        return
    got, _ = G.conv_call(src0, src1, w, tile_cfg=tile_cfg, ksplit=ksplit, **kw)
    ref = G.conv_ref(src0, src1, w, **kw)
    assert not torch.isnan(got).any()
    G.assert_close(got, ref, what=case[0])


@pytest.mark.parametrize('ksplit', [1, 2])
@pytest.mark.parametrize('tile_cfg', [0, 3, 5, 6, 9, 10, 11, 12, 13])
@pytest.mark.parametrize('case', [('stats8', 3, 64, 0, 8, 8, 96, 3, 1, 0, 2, True, True, True),
                                  ('stats32', 2, 32, 32, 32, 32, 160, 3, 1, 0, 2, True, True, True),
                                  ('stats_up', 2, 32, 0, 16, 16, 64, 3, 1, 1, 0, False, False, True)],
                         ids=['8x8', '32x32', 'up32'])
def test_conv_fused_output_stats(ksplit, tile_cfg, case):
    src0, src1, w, kw = _make_case(case)
    lib = L.load()
    fits = lib.sr3_conv_stats_slices(src0.shape[0], src0.shape[2], src0.shape[3], kw['ups'], w.shape[1], w.shape[0],
                                     tile_cfg, ksplit) > 0
    if not fits:      # the halo kernel (direct) and the split-K reduce kernel fuse the statistics
        with pytest.raises(L.Sr3Error):
            G.conv_call(src0, src1, w, ksplit=ksplit, tile_cfg=tile_cfg, want_stats=True, **kw)
        return
    # every tile: a refusal is asserted, never skipped on (the halo tiles are geometry-restricted, and an explicit split-K that the
    # problem's K cannot fill is refused on them and on the Winograd tiles; tile 0 takes the halo tile conv_pick chooses)
    why = G.conv_expected_refusal(src0.shape[0], w.shape[1], w.shape[0], src0.shape[2], src0.shape[3], kw['ups'], tile_cfg, ksplit)
    if why:
        with pytest.raises(L.Sr3Error, match=why):
            G.conv_call(src0, src1, w, ksplit=ksplit, tile_cfg=tile_cfg, want_stats=True, **kw)
        return
    got, st = G.conv_call(src0, src1, w, ksplit=ksplit, tile_cfg=tile_cfg, want_stats=True, **kw)
    ref = G.conv_ref(src0, src1, w, **kw)
    G.assert_close(got, ref)
    s1 = got.double().sum(dim=(2, 3))
    s2 = (got.double() ** 2).sum(dim=(2, 3))
    assert torch.allclose(st[:, :, 0], s1, rtol=1e-9, atol=1e-9)
    assert torch.allclose(st[:, :, 1], s2, rtol=1e-9, atol=1e-9)


WINO_CASES = [
    # name, B, C0, C1, H, W, Cout, k, stride, ups, act, film, res, bias  -- the layer shapes of the BASELINE.json networks
    ('w128_64to64', 2, 64, 0, 128, 128, 64, 3, 1, 0, 2, True, True, True),
    ('w128_concat192to64', 1, 128, 64, 128, 128, 64, 3, 1, 0, 2, True, False, True),
    ('w64_up_128to128', 2, 128, 0, 32, 32, 128, 3, 1, 1, 0, False, False, True),
    ('w32_concat768to256', 1, 512, 256, 32, 32, 256, 3, 1, 0, 2, True, 'res', True),
    ('w16_512to512', 3, 512, 0, 16, 16, 512, 3, 1, 0, 2, True, True, True),
    ('w16_1024to512_oddB', 3, 512, 512, 16, 16, 512, 3, 1, 0, 2, True, False, True),
    ('w16x48_ragged_cout', 2, 24, 8, 16, 48, 40, 3, 1, 0, 2, True, True, True),
    # round 4: 8x8 maps, four images per workgroup tile (batch % 4 == 0), split-K only
    ('w8_512to512_b4', 4, 512, 0, 8, 8, 512, 3, 1, 0, 2, True, True, True),
    ('w8_concat1024to512_b8', 8, 512, 512, 8, 8, 512, 3, 1, 0, 2, True, False, True),
    ('w8_ragged_cout_b4', 4, 24, 8, 8, 8, 40, 3, 1, 0, 2, True, True, True),
    ('w8_plain_b12', 12, 64, 0, 8, 8, 64, 3, 1, 0, 0, False, 'res', True),
]


STRESS_CASES = [
    # name, B, C0, C1, H, W, Cout, act, scale of the GroupNorm (scale, shift) pairs
    ('stress_128_64to64', 2, 64, 0, 128, 128, 64, 2, 30.0),
    ('stress_32_concat768to256', 1, 512, 256, 32, 32, 256, 2, 30.0),
    ('stress_16_512to512_affine_only', 2, 512, 0, 16, 16, 512, 1, 300.0),
]


@pytest.mark.parametrize('tile', [11, 12, 13], ids=['fp32', 'split', 'split2wg'])
@pytest.mark.parametrize('ksplit', [0, 1])
@pytest.mark.parametrize('case', STRESS_CASES, ids=[c[0] for c in STRESS_CASES])
def test_winograd_conv_stress_absolute_bound(case, ksplit, tile):
    """The Winograd kernel on data built to hurt it -- activations up to ~1e3 after the GroupNorm affine (heavy-tailed, with
    sign flips between neighbouring pixels, so the input transform's differences cancel), filters with a few output and
    input channels 30x larger than the rest -- against an ABSOLUTE float64 criterion, not the direct kernel's error:
    every output element must lie within 4 * gamma_K * conv(|a|, |w|) of the float64 result, K = 9 Cin multiply-adds,
    gamma_K = K u / (1 - K u), u = 2^-24: four times the classic worst-case bound of a K-term fp32 dot product.  (The
    F(2x2,3x3) transforms add O(1) roundings per term with coefficients 0, +-1, +-1/2; measured ratios are ~1e-2 of it.)"""
    import torch.nn.functional as F
    name, B, C0, C1, H, W, Cout, act, amp = case
    Cin = C0 + C1
    g = torch.Generator().manual_seed(99)
    x = torch.randn(B, Cin, H, W, generator=g)
    x = x * torch.exp(1.5 * torch.randn(B, Cin, H, W, generator=g))           # log-normal magnitudes: heavy tails
    checker = ((torch.arange(H)[:, None] + torch.arange(W)[None, :]) % 2 * 2 - 1).float()
    x[:, ::7] = x[:, ::7].abs() * checker                                     # pixel-to-pixel sign flips on some channels
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    w[::5] *= 30.0                                                            # a few loud output channels
    w[:, ::11] *= 30.0                                                        # ... and loud input channels
    ss = torch.stack([torch.randn(B, Cin, generator=g) * amp, torch.randn(B, Cin, generator=g) * amp], dim=2).contiguous()
    bias = torch.randn(Cout, generator=g)
    src0, src1 = (x[:, :C0].contiguous(), x[:, C0:].contiguous()) if C1 else (x, None)
    kw = dict(ups=0, stride=1, act=act, ss=ss, bias=bias)
    got, _ = G.conv_call(src0, src1, w, tile_cfg=tile, ksplit=ksplit, **kw)
    ref = G.conv_ref(src0, src1, w, **kw)
    a = x.double() * ss[:, :, 0].double()[:, :, None, None] + ss[:, :, 1].double()[:, :, None, None]
    if act == 2:
        a = a * torch.sigmoid(a)
    mag = F.conv2d(a.abs(), w.double().abs(), None, padding=1) + bias.double().abs()[None, :, None, None]
    K = 9 * Cin
    u = 2.0 ** -24
    gamma = K * u / (1 - K * u)
    err = (got.double() - ref).abs()
    ratio = (err / (4 * gamma * mag + 1e-300)).max().item()
    print('%s ks%d tile %d: |a|max %.3g, |ref|max %.3g, max err %.3g, rms err %.3g, max err / (4 gamma_K conv(|a|,|w|)) = %.3g'
          % (name, ksplit, tile, a.abs().max().item(), ref.abs().max().item(), err.max().item(), err.pow(2).mean().sqrt().item(), ratio))
    assert torch.isfinite(got).all()
    assert a.abs().max().item() > 500.0                                      # the case really is a stress case
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize('ksplit', [0, 1, 3])
@pytest.mark.parametrize('case', WINO_CASES, ids=[c[0] for c in WINO_CASES])
def test_winograd_conv_error_is_fp32_class(case, ksplit):
    """The Winograd F(2x2,3x3) kernel (tile 11, what the inference plan runs) against a float64 reference next to the
    direct fp32 MFMA kernels on the same data: same stated tolerance, and its error must stay within a small factor of
    the direct kernel's (F(2x2,3x3) transforms only use 0, +-1, +-1/2: fp32-class, not a reduced-precision mode)."""
    src0, src1, w, kw = _make_case(case, seed=7)
    why = G.wino_expected_refusal(case[1], case[2] + case[3], case[4], case[5], case[9], 11, ksplit)
    if why:                            # asserted, not skipped: an unexpected refusal of a production tile fails
        with pytest.raises(L.Sr3Error, match=why):
            G.conv_call(src0, src1, w, tile_cfg=11, ksplit=ksplit, **kw)
        return
    ref = G.conv_ref(src0, src1, w, **kw)
    got, _ = G.conv_call(src0, src1, w, tile_cfg=11, ksplit=ksplit, **kw)
    direct, _ = G.conv_call(src0, src1, w, tile_cfg=0 if case[4] >= 16 else 5, ksplit=0, **kw)
    assert not torch.isnan(got).any()
    e_w = G.assert_close(got, ref, what=case[0] + ' (Winograd)')
    e_d = G.assert_close(direct, ref, what=case[0] + ' (direct)')
    rms_w = (got.double() - ref).pow(2).mean().sqrt().item()
    rms_d = (direct.double() - ref).pow(2).mean().sqrt().item()
    print('%s ks%d: max/rms err Winograd %.2e/%.2e  direct %.2e/%.2e  |ref|max %.2f'
          % (case[0], ksplit, e_w, rms_w, e_d, rms_d, ref.abs().max().item()))
    assert e_w <= 4.0 * e_d + 1e-7 * ref.abs().max().item(), (e_w, e_d)
    assert rms_w <= 3.0 * rms_d + 1e-8 * ref.abs().max().item(), (rms_w, rms_d)


def test_winograd_two_workgroup_tile_on_maps_8_mod_16_high():
    """conv3x3_wino2.hip's 8 x 16 tile takes maps whose height is a multiple of 8 but not of 16 (the 8-wave kernel does not): against
    float64 at the stated tolerance, direct epilogue with statistics and split-K."""
    case = ('w24x32', 2, 48, 16, 24, 32, 72, 3, 1, 0, 2, True, 'res', True)
    src0, src1, w, kw = _make_case(case, seed=11)
    ref = G.conv_ref(src0, src1, w, **kw)
    with pytest.raises(L.Sr3Error, match='does not fit'):
        G.conv_call(src0, src1, w, tile_cfg=12, ksplit=1, **kw)
    for ks in (1, 2):
        got, st = G.conv_call(src0, src1, w, tile_cfg=13, ksplit=ks, want_stats=True, **kw)
        G.assert_close(got, ref, what='24x32 tile 13 ks%d' % ks)
        assert torch.allclose(st[:, :, 0], got.double().sum(dim=(2, 3)), rtol=1e-9, atol=1e-9)
        assert torch.allclose(st[:, :, 1], (got.double() ** 2).sum(dim=(2, 3)), rtol=1e-9, atol=1e-9)


SPLIT_GATE_CASES = list(WINO_CASES)          # (round 5: the four-image 8x8 tile has its split instantiation too -- tile 12 only)


@pytest.mark.parametrize('tile', [12, 13], ids=['8wave', '2wg'])
@pytest.mark.parametrize('ksplit', [0, 1, 2])
@pytest.mark.parametrize('case', SPLIT_GATE_CASES, ids=[c[0] for c in SPLIT_GATE_CASES])
def test_winograd_split_error_not_above_fp32_winograd(case, ksplit, tile):
    """Gate of the `wino_split` plan option (tile 12: the Winograd kernel's 3 x bf16 split instantiation -- every fp32 operand
    as h + m + l, six bf16 MFMA products per term, fp32 accumulation): on every layer shape of the BASELINE networks its error
    against float64 must not exceed the exact-fp32 Winograd kernel's (tile 11) on the same data -- rms within 5 %, max within
    25 % (the max of ~1e6 samples is a noisy statistic) -- and it must meet the same stated tolerance."""
    if case[4] < 16 and tile == 13:
        with pytest.raises(L.Sr3Error, match='does not fit'):       # conv3x3_wino2.hip covers maps >= 16 wide
            G.conv_call(*_make_case(case, seed=7)[:3], tile_cfg=13, ksplit=ksplit, **_make_case(case, seed=7)[3])
        return
    src0, src1, w, kw = _make_case(case, seed=7)
    why = G.wino_expected_refusal(case[1], case[2] + case[3], case[4], case[5], case[9], tile, ksplit)
    if why:                            # asserted, not skipped: an unexpected refusal of a production tile fails
        with pytest.raises(L.Sr3Error, match=why):
            G.conv_call(src0, src1, w, tile_cfg=tile, ksplit=ksplit, **kw)
        return
    ref = G.conv_ref(src0, src1, w, **kw)
    got, _ = G.conv_call(src0, src1, w, tile_cfg=tile, ksplit=ksplit, **kw)
    base, _ = G.conv_call(src0, src1, w, tile_cfg=11, ksplit=0 if G.wino_expected_refusal(case[1], case[2] + case[3], case[4], case[5], case[9], 11, ksplit) else ksplit, **kw)
    assert not torch.isnan(got).any()
    e_s = G.assert_close(got, ref, what=case[0] + ' (Winograd, 3 x bf16 split)')
    e_w = G.assert_close(base, ref, what=case[0] + ' (Winograd, fp32 MFMA)')
    rms_s = (got.double() - ref).pow(2).mean().sqrt().item()
    rms_w = (base.double() - ref).pow(2).mean().sqrt().item()
    print('%s ks%d tile %d: max/rms err split %.2e/%.2e  fp32 Winograd %.2e/%.2e  |ref|max %.2f'
          % (case[0], ksplit, tile, e_s, rms_s, e_w, rms_w, ref.abs().max().item()))
    assert rms_s <= 1.05 * rms_w, (rms_s, rms_w)
    assert e_s <= 1.25 * e_w + 1e-8 * ref.abs().max().item(), (e_s, e_w)


# every kind of 1x1 / stride-2 conv of the BASELINE networks (name, B, C0, C1, H, W, Cout, k, stride, ups, act, film, res, bias)
GEMM_SPLIT_CASES = [
    ('qkv_16', 2, 512, 0, 16, 16, 1536, 1, 1, 0, 1, False, False, False),
    ('attn_out_16', 2, 512, 0, 16, 16, 512, 1, 1, 0, 0, False, True, True),
    ('res_conv_1024_16', 2, 512, 512, 16, 16, 512, 1, 1, 0, 0, False, False, True),
    ('res_conv_192_128', 1, 128, 64, 128, 128, 64, 1, 1, 0, 0, False, False, True),
    ('res_conv_64_64', 2, 64, 0, 64, 64, 128, 1, 1, 0, 0, False, False, True),
    ('qkv_64x64_c1024', 1, 1024, 0, 32, 32, 3072, 1, 1, 0, 1, False, False, False),
    ('down_128', 1, 64, 0, 128, 128, 64, 3, 2, 0, 0, False, False, True),
    ('down_16', 2, 512, 0, 16, 16, 512, 3, 2, 0, 0, False, False, True),
    ('down_rect_32x64', 2, 128, 0, 32, 64, 256, 3, 2, 0, 0, False, False, True),
    ('n64_affine_320', 2, 96, 32, 16, 32, 320, 1, 1, 0, 1, True, True, True),        # Cout % 128 != 0: the 64 x 64 tile, with every epilogue term
    ('down_64to64', 1, 64, 0, 64, 64, 64, 3, 2, 0, 0, False, False, True),
]


def _gemm1x1_fits(k, stride, Cout, C1=0, act=0):
    """What gemm1x1.hip takes (tile 22): 1x1 stride 1, or Downsample's bare 3x3 stride 2 (one source, no activation); Cout % 64 == 0
    (Cout % 128 != 0: its 64 x 64 tile, waves 2 x 2)."""
    return Cout % 64 == 0 and ((k == 1 and stride == 1) or (k == 3 and stride == 2 and C1 == 0 and act == 0))


@pytest.mark.parametrize('tile,ksplit', [(14, 1), (16, 1), (15, 2), (18, 1), (19, 1), (20, 1), (21, 1), (19, 2), (20, 3), (22, 1), (22, 2), (22, 0), (0, 0)])
@pytest.mark.parametrize('case', GEMM_SPLIT_CASES, ids=[c[0] for c in GEMM_SPLIT_CASES])
def test_gemm_split_error_not_above_fp32_mfma(case, tile, ksplit):
    """Gate of the `gemm_split` plan option (tiles 14-17: the im2col kernel's 3 x bf16 split instantiations -- operands split
    into h + m + l while they are staged, six bf16 MFMA products per term, fp32 accumulation; tiles 18-21: the same with the
    weights pre-split into bf16 planes, which is what a plan runs): on the 1x1 / stride-2 layer
    shapes of the BASELINE networks the error against float64 is not above the exact-fp32 instantiation's (tile 3) on the
    same data, and the stated tolerance holds.  (0, 0) is the ABI's auto pick, which stays on the fp32 MFMA."""
    # (no plan uses a 128-wide tile for Cout <= 64, but the kernel takes it: half of each tile's columns hang over Cout and are masked)
    src0, src1, w, kw = _make_case(case, seed=11)
    if tile == 22 and not _gemm1x1_fits(case[7], case[8], case[6], case[3], case[10]):
        # tile 22 = the plain GEMM kernel of gemm1x1.hip (plan option gemm2): 1x1 stride 1 or 3x3 stride 2, Cout % 128 == 0 only -- asserted, not skipped
        with pytest.raises(L.Sr3Error, match='does not fit'):
            G.conv_call(src0, src1, w, tile_cfg=22, ksplit=ksplit, **kw)
        return
    ref = G.conv_ref(src0, src1, w, **kw)
    got, _ = G.conv_call(src0, src1, w, tile_cfg=tile, ksplit=ksplit, **kw)
    base, _ = G.conv_call(src0, src1, w, tile_cfg=3, ksplit=ksplit, **kw)
    assert not torch.isnan(got).any()
    e_s = G.assert_close(got, ref, what=case[0] + ' (im2col, 3 x bf16 split)')
    e_f = G.assert_close(base, ref, what=case[0] + ' (im2col, fp32 MFMA)')
    rms_s = (got.double() - ref).pow(2).mean().sqrt().item()
    rms_f = (base.double() - ref).pow(2).mean().sqrt().item()
    scale = ref.abs().max().item()
    print('%s tile %d ks%d: max/rms err split %.2e/%.2e  fp32 MFMA %.2e/%.2e  |ref|max %.2f' % (case[0], tile, ksplit, e_s, rms_s, e_f, rms_f, scale))
    if tile == 0:
        assert torch.equal(got, base) or e_s <= 2.0 * e_f
        return
    if tile == 22 and ksplit == 0:
        # the plain GEMM's own split-K pick differs from the im2col kernel's (32-row tiles fill the chip without a split where the im2col
        # tile splits), and a split-K sum is the more accurate one (shorter fp32 chains): compare with the fp32 MFMA on the LONGER chain too
        base1, _ = G.conv_call(src0, src1, w, tile_cfg=3, ksplit=1, **kw)
        rms_f = max(rms_f, (base1.double() - ref).pow(2).mean().sqrt().item())
        e_f = max(e_f, (base1.double() - ref).abs().max().item())
    assert rms_s <= 1.1 * rms_f + 1e-9 * scale, (rms_s, rms_f)
    assert e_s <= 1.5 * e_f + 1e-8 * scale, (e_s, e_f)
    if 18 <= tile <= 21:      # pre-split weights are the same three bf16 terms the kernel would have built itself: identical results
        same, _ = G.conv_call(src0, src1, w, tile_cfg=tile - 4, ksplit=ksplit, **kw)
        assert torch.equal(got, same), 'pre-split weights changed the result'


GEMM_STRESS_CASES = [
    # name, B, C0, C1, H, W, Cout, ksize, stride, act, scale of the GroupNorm (scale, shift) pairs
    ('stress_qkv_512to1536', 2, 512, 0, 16, 16, 1536, 1, 1, 1, 300.0),      # attention qkv: post-GroupNorm affine, no SiLU
    ('stress_s2_512to512', 2, 512, 0, 16, 16, 512, 3, 2, 0, 1.0),           # Downsample: raw feature maps, K = 4608
    ('stress_res_conv_768to256', 1, 512, 256, 32, 32, 256, 1, 1, 0, 1.0),   # res_conv over the skip concat
]


@pytest.mark.parametrize('tile', [3, 16, 18, 19, 20, 21, 22], ids=['fp32', 'split_64x64', 'pre_128x128', 'pre_128x64', 'pre_64x64', 'pre_64x128', 'gemm1x1'])
@pytest.mark.parametrize('ksplit', [1, 2])
@pytest.mark.parametrize('case', GEMM_STRESS_CASES, ids=[c[0] for c in GEMM_STRESS_CASES])
def test_gemm_split_stress_absolute_bound(case, ksplit, tile):
    """The im2col SPLIT tiles on data built to hurt them (the companion of test_winograd_conv_stress_absolute_bound): log-normal
    heavy-tailed inputs up to ~1e3 with pixel-to-pixel sign flips, a few output / input channels of the filters 30x louder than
    the rest, against an ABSOLUTE float64 criterion: every output within 4 gamma_K conv(|a|, |w|) of the float64 result,
    K = ksize^2 Cin, gamma_K = K u / (1 - K u), u = 2^-24 -- the fp32-class claim of the headline dtype on every input, not
    only on N(0, 1)-like data.  The fp32 MFMA tile runs the same case for the record."""
    import torch.nn.functional as F
    name, B, C0, C1, H, W, Cout, k, stride, act, amp = case
    Cin = C0 + C1
    g = torch.Generator().manual_seed(199)
    x = torch.randn(B, Cin, H, W, generator=g)
    x = x * torch.exp(1.5 * torch.randn(B, Cin, H, W, generator=g))
    checker = ((torch.arange(H)[:, None] + torch.arange(W)[None, :]) % 2 * 2 - 1).float()
    x[:, ::7] = x[:, ::7].abs() * checker
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(k * k * Cin)
    w[::5] *= 30.0
    w[:, ::11] *= 30.0
    bias = torch.randn(Cout, generator=g)
    kw = dict(ups=0, stride=stride, bias=bias)
    a = x.double()
    if act:
        ss = torch.stack([torch.randn(B, Cin, generator=g) * amp, torch.randn(B, Cin, generator=g) * amp], dim=2).contiguous()
        kw.update(act=act, ss=ss)
        a = a * ss[:, :, 0].double()[:, :, None, None] + ss[:, :, 1].double()[:, :, None, None]
        if act == 2:
            a = a * torch.sigmoid(a)
    src0, src1 = (x[:, :C0].contiguous(), x[:, C0:].contiguous()) if C1 else (x, None)
    if tile == 22 and not _gemm1x1_fits(k, stride, Cout, C1, act):
        with pytest.raises(L.Sr3Error, match='does not fit'):        # the plain GEMM kernel: 1x1 stride 1 / bare 3x3 stride 2 only
            G.conv_call(src0, src1, w, tile_cfg=22, ksplit=ksplit, **kw)
        return
    got, _ = G.conv_call(src0, src1, w, tile_cfg=tile, ksplit=ksplit, **kw)
    ref = G.conv_ref(src0, src1, w, **kw)
    mag = F.conv2d(a.abs(), w.double().abs(), None, stride=stride, padding=k // 2) + bias.double().abs()[None, :, None, None]
    K = k * k * Cin
    u = 2.0 ** -24
    gamma = K * u / (1 - K * u)
    err = (got.double() - ref).abs()
    ratio = (err / (4 * gamma * mag + 1e-300)).max().item()
    print('%s ks%d tile %d: |a|max %.3g, |ref|max %.3g, max err %.3g, rms err %.3g, max err / (4 gamma_K conv(|a|,|w|)) = %.3g'
          % (name, ksplit, tile, a.abs().max().item(), ref.abs().max().item(), err.max().item(), err.pow(2).mean().sqrt().item(), ratio))
    assert torch.isfinite(got).all()
    assert a.abs().max().item() > 500.0                                      # the case really is a stress case
    assert ratio <= 1.0, ratio


@pytest.mark.experiments
@pytest.mark.parametrize('K', [(64, 0), (512, 0), (512, 512)], ids=['K576', 'K4608', 'K9216'])
def test_split_bf16_error_is_fp32_class(K):
    """The opt-in split-bf16 instantiations (tile 7 / 10) against a float64 reference: their error must be of the
    same size as the exact-fp32 MFMA instantiations' (tile 5 / 9) on the same data -- i.e. no precision is given up."""
    C0, C1 = K
    B, H, Cout = 2, 32, 128
    src0 = _rand(B, C0, H, H, seed=41) * 3.0
    src1 = _rand(B, C1, H, H, seed=42) * 3.0 if C1 else None
    w = _rand(Cout, C0 + C1, 3, 3, seed=43) * (1.0 / math.sqrt(9 * (C0 + C1)))
    ss = torch.stack([1.0 + 0.3 * _rand(B, C0 + C1, seed=44), 0.2 * _rand(B, C0 + C1, seed=45)], 2)
    kw = dict(bias=_rand(Cout, seed=46), ss=ss, act=2)
    ref = G.conv_ref(src0, src1, w, **kw)
    errs = {}
    for cfg in (5, 7, 9, 10):
        got, _ = G.conv_call(src0, src1, w, tile_cfg=cfg, ksplit=1, **kw)
        d = (got.double() - ref)
        errs[cfg] = (d.abs().max().item(), d.pow(2).mean().sqrt().item())
    scale = ref.abs().max().item()
    print('K=%d |ref|max %.2f  max/rms err: fp32 128x128 %.2e/%.2e  split %.2e/%.2e | fp32 256x128 %.2e/%.2e  split %.2e/%.2e'
          % (9 * (C0 + C1), scale, *errs[5], *errs[7], *errs[9], *errs[10]))
    for exact, split in ((5, 7), (9, 10)):
        assert errs[split][0] <= 2.0 * errs[exact][0] + 1e-7 * scale, (errs[exact], errs[split])
        assert errs[split][1] <= 2.0 * errs[exact][1] + 1e-8 * scale, (errs[exact], errs[split])


@pytest.mark.parametrize('tile_cfg,ksplit', [(0, 0), (5, 1), (6, 1), (5, 2), (6, 3), (7, 1), (8, 1), (9, 1), (10, 1), (9, 2)])
@pytest.mark.parametrize('shape', [(2, 64, 0, 16, 16, 128, 96, 32), (3, 32, 0, 8, 8, 64, 24, 8), (1, 128, 0, 32, 32, 64, 192, 0)],
                         ids=['16x16', '8x8_oddB', '32x32'])
def test_block_conv_with_fused_res_conv(shape, tile_cfg, ksplit):
    """block2 conv3x3 + res_conv 1x1 of the (concat) block input in one launch."""
    import torch.nn.functional as F
    B, C0, C1, H, W, Cout, X0, X1 = shape
    lib = L.load()
    d = G.dev()
    case = ('blk', B, C0, C1, H, W, Cout, 3, 1, 0, 2, True, False, True)
    src0, src1, w, kw = _make_case(case)
    x2a = _rand(B, X0, H, W, seed=21)
    x2b = _rand(B, X1, H, W, seed=22) if X1 else None
    w2 = _rand(Cout, X0 + X1, 1, 1, seed=23) * 0.1
    b2 = _rand(Cout, seed=24)
    ref = G.conv_ref(src0, src1, w, **kw) + F.conv2d((x2a if x2b is None else torch.cat([x2a, x2b], 1)).double(),
                                                     w2.double(), b2.double())
    g = lambda t: None if t is None else t.to(d)
    dv = dict(s0=g(G.nhwc(src0)), w=g(G.ohwi(w)), bias=g(kw['bias']), ss=g(kw['ss']), film=g(kw['film']),
              x2a=g(G.nhwc(x2a)), x2b=None if x2b is None else g(G.nhwc(x2b)), w2=g(w2.reshape(Cout, -1).contiguous()),
              b2=g(b2))
    out = torch.full((B, H, W, Cout), float('nan'), device=d)
    nb = int(lib.sr3_conv_scratch_bytes(B, H, W, C0, Cout, 3, tile_cfg, ksplit))
    scratch = torch.empty(max(nb, 16), dtype=torch.uint8, device=d)
    rc = lib.sr3_block_conv_f32(L.ptr(dv['s0']), C0, None, 0, B, H, W, Cout, L.ptr(dv['w']), L.ptr(dv['bias']),
                                L.ptr(dv['ss']), 2, L.ptr(dv['film']), Cout, L.ptr(dv['x2a']), X0, L.ptr(dv['x2b']), X1,
                                L.ptr(dv['w2']), L.ptr(dv['b2']), L.ptr(out), None, tile_cfg, ksplit, L.ptr(scratch),
                                nb, G.stream())
    torch.cuda.synchronize()
    why = G.conv_expected_refusal(B, C0 + C1, Cout, H, W, 0, tile_cfg, ksplit)      # the halo tiles are geometry-restricted: asserted
    if why:
        with pytest.raises(L.Sr3Error, match=why):
            L.check(rc)
        return
    L.check(rc)
    G.assert_close(G.nchw(out).cpu(), ref, what='block conv + res_conv')


@pytest.mark.parametrize('B,HW,C', [(2, 256, 64), (3, 100, 24), (2, 16384, 64), (4, 64, 512), (1, 16, 1024)])
def test_groupnorm_stats_and_fold(B, HW, C):
    lib = L.load()
    d = G.dev()
    x = _rand(B, HW, C, seed=3) * 2 + 0.5
    xd = x.to(d)
    T = int(lib.sr3_groupnorm_stats_slices(B, HW, C))
    st = torch.full((B, T, C, 2), float('nan'), dtype=torch.float64, device=d)     # no zeroing required
    L.check(lib.sr3_groupnorm_stats_f32(L.ptr(xd), B, HW, C, L.ptr(st), G.stream()))
    torch.cuda.synchronize()
    assert torch.allclose(st[..., 0].sum(1).cpu(), x.double().sum(1), rtol=1e-12, atol=1e-9)
    assert torch.allclose(st[..., 1].sum(1).cpu(), (x.double() ** 2).sum(1), rtol=1e-12, atol=1e-9)
    # fold as a concat of two halves with groups straddling the seam where possible
    C0 = C // 2 - 4 if C >= 16 else C
    C1 = C - C0
    groups = 4 if C % 4 == 0 else 1
    gamma, beta = _rand(C, seed=4) * 0.2 + 1, _rand(C, seed=5) * 0.2
    st0 = st[:, :, :C0].contiguous()
    # second source with a different number of partials (as a tensor from another producer would have)
    st1 = None
    T1 = 0
    if C1:
        half = st[:, :, C0:] * 0.5
        st1 = torch.cat([half, half], dim=1).contiguous()
        T1 = 2 * T
    ss = torch.empty(B, C, 2, device=d)
    gd, bd = gamma.to(d), beta.to(d)          # keep device copies alive across the async call
    L.check(lib.sr3_groupnorm_fold_f32(L.ptr(st0), C0, T, L.ptr(st1), C1, T1, B, HW, groups, L.ptr(gd),
                                       L.ptr(bd), 1e-5, L.ptr(ss), G.stream()))
    torch.cuda.synchronize()
    xn = x.permute(0, 2, 1).reshape(B, C, HW, 1)
    ref = F.group_norm(xn.double(), groups, gamma.double(), beta.double(), eps=1e-5)
    got = xn.double() * ss[:, :, 0].cpu().double()[:, :, None, None] + ss[:, :, 1].cpu().double()[:, :, None, None]
    G.assert_close(got, ref, tol=5e-6, what='gn fold')


# the last three are the smallest shapes the host rule sends to k_attention_v2<2,4,.>, <1,4,.> and <1,2,.> (qblocks * B >= 256 keeps the
# channels of a workgroup unsplit): the TN = 4 strip form of the shared P V loop runs in no other per-op test
@pytest.mark.parametrize('B,N,C', [(2, 256, 512), (2, 64, 512), (3, 16, 256), (2, 64, 16), (1, 1024, 128),
                                   (8, 1024, 512), (40, 224, 512), (40, 224, 256)])
def test_attention(B, N, C):
    lib = L.load()
    d = G.dev()
    qkv = _rand(B, N, 3 * C, seed=7)
    qd = qkv.to(d)
    q, k, v = qkv.double().split(C, dim=2)
    p = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(C), -1)
    ref = p @ v
    out = torch.full((B, N, C), float('nan'), device=d)
    L.check(lib.sr3_attention_f32(L.ptr(qd), B, N, C, L.ptr(out), G.stream()))
    torch.cuda.synchronize()
    G.assert_close(out.cpu(), ref, what='attention')
    for mode in (0, 1):       # fp32 MFMA / 3 x bf16 split, both on the strip kernels
        out = torch.full((B, N, C), float('nan'), device=d)
        L.check(lib.sr3_attention_ex_f32(L.ptr(qd), B, N, C, L.ptr(out), mode, G.stream()))
        torch.cuda.synchronize()
        G.assert_close(out.cpu(), ref, what='attention mode %d' % mode)


@pytest.mark.parametrize('B,N,C', [(16, 256, 512), (4, 64, 512), (2, 1024, 128), (8, 256, 256)], ids=['c2_16x16', 'c2_8x8', 'n1024', 'c256'])
def test_attention_split_error_not_above_fp32_mfma(B, N, C):
    """Gate of the `attn_split` plan option (k_attention_v2's 3 x bf16 split instantiation: Q K^T and P V as six bf16 MFMA
    products of 3-way split fp32 operands, fp32 accumulation) on the attention shapes of the BASELINE networks (16 x 16 and 8 x 8
    maps, C = 512) and two more: its error against float64 must not exceed the fp32-MFMA kernel's on the same data (rms within
    5 %, max within 25 %), on N(0, 1) inputs AND on heavy-tailed ones (log-normal magnitudes: large logits, peaked softmax)."""
    lib = L.load()
    d = G.dev()
    for kind in ('normal', 'heavy'):
        qkv = _rand(B, N, 3 * C, seed=11)
        if kind == 'heavy':
            qkv = qkv.sign() * torch.exp(1.5 * qkv.abs()) * 0.3
        qd = qkv.to(d)
        outs = []
        for split in (1, 0):
            out = torch.full((B, N, C), float('nan'), device=d)
            L.check(lib.sr3_attention_ex_f32(L.ptr(qd), B, N, C, L.ptr(out), split, G.stream()))
            torch.cuda.synchronize()
            outs.append(out.cpu())
        q, k, v = qkv.double().split(C, dim=2)
        ref = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(C), -1) @ v
        e_s = G.assert_close(outs[0], ref, what='attention (3 x bf16 split, %s)' % kind)
        e_f = G.assert_close(outs[1], ref, what='attention (fp32 MFMA, %s)' % kind)
        rms_s = (outs[0].double() - ref).pow(2).mean().sqrt().item()
        rms_f = (outs[1].double() - ref).pow(2).mean().sqrt().item()
        print('attention B%d N%d C%d %s: max/rms err split %.2e/%.2e  fp32 MFMA %.2e/%.2e  |ref|max %.2f'
              % (B, N, C, kind, e_s, rms_s, e_f, rms_f, ref.abs().max().item()))
        assert not torch.equal(outs[0], outs[1])          # (the split instantiation really ran)
        assert rms_s <= 1.05 * rms_f, (rms_s, rms_f)
        # (the max over ~1e6 heavy-tailed samples is a noisy statistic -- it falls on either side by up to 3x from case to case;
        #  the rms gate above is the strict one)
        assert e_s <= (1.25 if kind == 'normal' else 4.0) * e_f + 1e-8 * ref.abs().max().item(), (e_s, e_f)


@pytest.mark.parametrize('B,N,C', [(2, 64, 32), (1, 256, 512), (2, 100, 48), (1, 1024, 64), (1, 1024, 1024), (2, 600, 96), (1, 480, 64),
                                   (1, 512, 128)])
def test_attention_backward(B, N, C):
    """dqkv of the attention core vs float64 autograd; N > ~480 takes the key-blocked path (needs the forward output)."""
    lib = L.load()
    d = G.dev()
    qkv = _rand(B, N, 3 * C, seed=11) * (2.0 if C < 256 else 1.0)
    dout = _rand(B, N, C, seed=12)
    qd, gd = qkv.to(d), dout.to(d)
    out = torch.empty(B, N, C, device=d)
    L.check(lib.sr3_attention_f32(L.ptr(qd), B, N, C, L.ptr(out), G.stream()))
    dq = torch.full((B, N, 3 * C), float('nan'), device=d)
    L.check(lib.sr3_attention_bwd_f32(L.ptr(qd), L.ptr(gd), L.ptr(out), B, N, C, L.ptr(dq), G.stream()))
    torch.cuda.synchronize()
    x = qkv.double().requires_grad_(True)
    q, k, v = x.split(C, dim=2)
    o = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(C), -1) @ v
    o.backward(dout.double())
    ref = x.grad
    got = dq.cpu().double()
    for name, sl in (('dq', slice(0, C)), ('dk', slice(C, 2 * C)), ('dv', slice(2 * C, 3 * C))):
        r, g_ = ref[:, :, sl], got[:, :, sl]
        rel = (g_ - r).norm() / r.norm()
        assert rel < 2e-5, (name, float(rel))
        assert (g_ - r).abs().max() <= 1e-4 * max(1.0, float(r.abs().max())), name
    # the slab form (what the training step runs): no atomics -- two runs bit-equal, and within rounding of the atomics form
    nb = int(lib.sr3_attention_bwd_scratch_bytes(B, N, C))
    assert nb == -(-N // 32) * B * N * 2 * C * 4
    scratch = torch.empty(nb, dtype=torch.uint8, device=d)
    runs = []
    for _ in range(2):
        dqs = torch.full((B, N, 3 * C), float('nan'), device=d)          # (no zeroing needed: every element is written)
        scratch.fill_(0xff)
        L.check(lib.sr3_attention_bwd_ex_f32(L.ptr(qd), L.ptr(gd), L.ptr(out), B, N, C, L.ptr(dqs), L.ptr(scratch), nb, G.stream()))
        torch.cuda.synchronize()
        runs.append(dqs)
    assert torch.equal(runs[0], runs[1]), 'slab form is not bitwise reproducible'
    assert torch.equal(runs[0][:, :, :C], dq[:, :, :C])                   # dQ: the same stores
    for name, sl in (('dk', slice(C, 2 * C)), ('dv', slice(2 * C, 3 * C))):
        r, g_ = ref[:, :, sl], runs[0].cpu().double()[:, :, sl]
        assert (g_ - r).norm() / r.norm() < 2e-5, name
    with pytest.raises(L.Sr3Error, match='scratch too small'):
        L.check(lib.sr3_attention_bwd_ex_f32(L.ptr(qd), L.ptr(gd), L.ptr(out), B, N, C, L.ptr(dqs), L.ptr(scratch), nb - 4, G.stream()))
    if N <= 256:            # the single-strip path does not read the forward output
        dq2 = torch.empty_like(dq)
        L.check(lib.sr3_attention_bwd_f32(L.ptr(qd), L.ptr(gd), None, B, N, C, L.ptr(dq2), G.stream()))
        torch.cuda.synchronize()
        assert torch.allclose(dq2, dq, rtol=1e-4, atol=1e-5)
    elif N >= 1024:
        with pytest.raises(L.Sr3Error):
            L.check(lib.sr3_attention_bwd_f32(L.ptr(qd), L.ptr(gd), None, B, N, C, L.ptr(dq), G.stream()))


WGRAD_CASES = [
    # name, B, C0, C1, H, W, Cout, k, stride, ups, act     (what sr3_train_step meets, and the odd shapes it does not)
    ('w3_128to128_16', 4, 128, 0, 16, 16, 128, 3, 1, 0, 0),
    ('w3_concat192to320_act', 2, 128, 64, 16, 16, 320, 3, 1, 0, 2),
    ('w1_concat384to128', 2, 256, 128, 32, 32, 128, 1, 1, 0, 0),
    ('w3_s2_128to128', 2, 128, 0, 32, 32, 128, 3, 2, 0, 0),
    ('w3_up_256to256', 2, 256, 0, 8, 8, 256, 3, 1, 1, 0),
    ('w3_ragged_M100_136to200_act', 1, 136, 0, 10, 10, 200, 3, 1, 0, 1),
    ('w3_64to64_128', 2, 64, 0, 64, 64, 64, 3, 1, 0, 0),
    ('w1_96to64', 2, 96, 0, 16, 16, 64, 1, 1, 0, 2),
]


@pytest.mark.parametrize('split', [0, 1])
@pytest.mark.parametrize('case', WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_conv_weight_gradient_per_op(case, split):
    """Every weight-gradient kernel of wgrad.hip through its per-op entry against float64 autograd of F.conv2d: the 3 x bf16 split
    kernel (layers with more than 64 channels on both sides, `split` = 1) on concat inputs, channel counts that are not multiples of
    128, pixel counts that are not multiples of 32, stride 2, the x2-upsampled input and its fused activation form; the 9-tap and
    generic fp32-MFMA kernels on the rest.  Normwise 2e-6 (fp32 class); split not worse than 1.25 x the fp32 kernel where both run."""
    import torch.nn.functional as F
    name, B, C0, C1, H, W, Cout, k, stride, ups, act = case
    lib = L.load()
    d = G.dev()
    Cin = C0 + C1
    x0 = _rand(B, C0, H, W, seed=31)
    x1 = _rand(B, C1, H, W, seed=32) if C1 else None
    ss = torch.stack([_rand(B, Cin, seed=33) * 0.3 + 1.0, _rand(B, Cin, seed=34) * 0.3], dim=2).contiguous() if act else None
    pad = k // 2
    Ho = ((H << ups) + 2 * pad - k) // stride + 1
    Wo = ((W << ups) + 2 * pad - k) // stride + 1
    dy = _rand(B, Cout, Ho, Wo, seed=35)
    a = (x0 if x1 is None else torch.cat([x0, x1], 1)).double()
    if act:
        a = a * ss[:, :, 0].double()[:, :, None, None] + ss[:, :, 1].double()[:, :, None, None]
        if act == 2:
            a = a * torch.sigmoid(a)
    if ups:
        a = F.interpolate(a, scale_factor=2, mode='nearest')
    w = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, requires_grad=True)
    F.conv2d(a, w, None, stride=stride, padding=pad).backward(dy.double())
    ref = w.grad
    g = lambda t: None if t is None else t.to(d)
    x0d, x1d, ssd, dyd = g(G.nhwc(x0)), (None if x1 is None else g(G.nhwc(x1))), g(ss), g(G.nhwc(dy))      # (kept alive across the calls)

    def run(sp):
        nb = int(lib.sr3_conv_wgrad_scratch_bytes(B, H, W, ups, stride, k, C0, C1, Cout, sp))
        scratch = torch.empty(max(nb, 16), dtype=torch.uint8, device=d)
        dw = torch.full((Cout, k * k, Cin), float('nan'), device=d)
        L.check(lib.sr3_conv_wgrad_f32(L.ptr(x0d), C0, L.ptr(x1d), C1, B, H, W, ups, stride, k, Cout,
                                       L.ptr(ssd), act, L.ptr(dyd), L.ptr(dw), sp, L.ptr(scratch), nb, G.stream()))
        torch.cuda.synchronize()
        got = dw.cpu().view(Cout, k, k, Cin).permute(0, 3, 1, 2).double()
        return (got - ref).norm().item() / ref.norm().item()
    e = run(split)
    assert e < 2e-6, (name, split, e)
    if split and Cout > 64 and Cin > 64:
        e0 = run(0)
        print('%s: weight-gradient rel err vs float64: split %.2e, fp32 MFMA %.2e' % (name, e, e0))
        assert e <= 1.25 * e0 + 1e-8, (e, e0)


@pytest.mark.parametrize('variant', [0, 1])
def test_film_embed(variant):
    lib = L.load()
    d = G.dev()
    B, inner, Fn = 3, 64, 200
    w1, b1 = _rand(4 * inner, inner, seed=1) * 0.1, _rand(4 * inner, seed=2) * 0.1
    w2, b2 = _rand(inner, 4 * inner, seed=3) * 0.1, _rand(inner, seed=4) * 0.1
    wf, bf = _rand(Fn, inner, seed=5) * 0.1, _rand(Fn, seed=6) * 0.1
    if variant == 0:
        level = torch.tensor([0.999, 0.5, 0.013])
        tstep = None
        count = inner // 2
        freq = torch.exp(-math.log(1e4) * (torch.arange(count, dtype=torch.float32) / count))
        arg = level[:, None] * freq[None]
    else:
        level = None
        tstep = torch.tensor([0, 999, 1999], dtype=torch.long)
        freq = torch.exp(torch.arange(0, inner, 2, dtype=torch.float32) * (-math.log(10000) / inner))
        arg = torch.outer(tstep.float(), freq)
    enc = torch.cat([arg.sin(), arg.cos()], -1).double()
    h = enc @ w1.double().t() + b1.double()
    h = h * torch.sigmoid(h)
    t = h @ w2.double().t() + b2.double()
    if variant == 1:
        t = t * torch.sigmoid(t)
    ref = t @ wf.double().t() + bf.double()
    g = lambda x: None if x is None else x.to(d)
    temb = torch.empty(B, inner, device=d)
    film = torch.empty(B, Fn, device=d)
    dv = [g(t_) for t_ in (level, tstep, freq, w1, b1, w2, b2, wf, bf)]    # held until after the sync
    L.check(lib.sr3_film_embed_f32(variant, B, inner, *[L.ptr(t_) for t_ in dv], Fn,
                                   L.ptr(temb), L.ptr(film), G.stream()))
    torch.cuda.synchronize()
    G.assert_close(film.cpu(), ref, tol=1e-5, what='film')


@pytest.mark.parametrize('B,Ca,Cb,H,W,Cout', [(2, 3, 3, 16, 16, 64), (3, 3, 0, 10, 12, 8), (1, 3, 3, 128, 128, 64)])
def test_conv_in(B, Ca, Cb, H, W, Cout):
    lib = L.load()
    d = G.dev()
    a = _rand(B, Ca, H, W, seed=1)
    b = _rand(B, Cb, H, W, seed=2) if Cb else None
    w = _rand(Cout, Ca + Cb, 3, 3, seed=3) * 0.2
    bias = _rand(Cout, seed=4)
    out = torch.full((B, H, W, Cout), float('nan'), device=d)
    ad, bd, wd, biasd = a.to(d), (None if b is None else b.to(d)), G.ohwi(w).to(d), bias.to(d)
    L.check(lib.sr3_conv_in_f32(L.ptr(ad), Ca, L.ptr(bd), Cb, B, H, W, L.ptr(wd), L.ptr(biasd), Cout, L.ptr(out),
                                G.stream()))
    torch.cuda.synchronize()
    x = a if b is None else torch.cat([a, b], 1)
    ref = F.conv2d(x.double(), w.double(), bias.double(), padding=1)
    G.assert_close(G.nchw(out).cpu(), ref, what='conv_in')


@pytest.mark.parametrize('B,H,W,Cc,Cout', [(2, 16, 16, 64, 3), (3, 10, 40, 8, 3), (1, 128, 128, 64, 3)])
def test_conv_out(B, H, W, Cc, Cout):
    lib = L.load()
    d = G.dev()
    x = _rand(B, Cc, H, W, seed=1)
    ss = torch.stack([_rand(B, Cc, seed=2) * 0.3 + 1.0, _rand(B, Cc, seed=3) * 0.3], dim=2).contiguous()
    w = _rand(Cout, Cc, 3, 3, seed=4) * 0.1
    bias = _rand(Cout, seed=5)
    out = torch.full((B, Cout, H, W), float('nan'), device=d)
    xd, ssd, wd, biasd = G.nhwc(x).to(d), ss.to(d), G.ohwi(w).to(d), bias.to(d)
    L.check(lib.sr3_conv_out_f32(L.ptr(xd), L.ptr(ssd), B, H, W, Cc, L.ptr(wd), L.ptr(biasd), Cout, L.ptr(out),
                                 G.stream()))
    torch.cuda.synchronize()
    ref = G.conv_ref(x, None, w, bias=bias, ss=ss, act=2)
    G.assert_close(out.cpu(), ref, what='conv_out')


def test_p_sample_step_bit_exact():
    """The fused update must equal the reference's elementwise torch ops bit for bit."""
    from oracle import sr3_oracle as O
    lib = L.load()
    d = G.dev()
    tab = O.schedule_tables(dict(schedule='linear', n_timestep=50, linear_start=1e-6, linear_end=1e-2))
    T = tab['num_timesteps']
    sig = (0.5 * torch.from_numpy(tab['posterior_log_variance_clipped'])).exp()
    sig[0] = 0
    tabs = [torch.from_numpy(tab[k]).to(d) for k in ('sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod',
                                                     'posterior_mean_coef1', 'posterior_mean_coef2')] + [sig.to(d)]
    B = 3
    x, eps, z = _rand(B, 3, 16, 16, seed=1), _rand(B, 3, 16, 16, seed=2), _rand(B, 3, 16, 16, seed=3)
    ed, zd = eps.to(d), z.to(d)
    for t in (T - 1, 17, 0):
        xd = x.to(d).clone()
        L.check(lib.sr3_p_sample_step(L.ptr(xd), L.ptr(ed), L.ptr(zd), *[L.ptr(t_) for t_ in tabs], None,
                                      None, t, B, 3 * 16 * 16, G.stream()))
        torch.cuda.synchronize()
        ref = O.p_sample_update(tab, x, eps, t, z)
        assert torch.equal(xd.cpu(), ref), t
        xd = (3.0 * x).to(d).clone()                      # clip_denoised = 0 (sr3_p_sample_step_ex), |x0| > 1 on most elements
        L.check(lib.sr3_p_sample_step_ex(L.ptr(xd), L.ptr(ed), L.ptr(zd), *[L.ptr(t_) for t_ in tabs], None,
                                         None, t, B, 3 * 16 * 16, 0, G.stream()))
        torch.cuda.synchronize()
        assert torch.equal(xd.cpu(), O.p_sample_update(tab, 3.0 * x, eps, t, z, clip_denoised=False)), t
        assert not torch.equal(xd.cpu(), O.p_sample_update(tab, 3.0 * x, eps, t, z))
    # per-sample t (DDPM API) and device step counter
    tps = torch.tensor([0, 5, 49], dtype=torch.long)
    xd = x.to(d).clone()
    tpd = tps.to(d)
    L.check(lib.sr3_p_sample_step(L.ptr(xd), L.ptr(ed), L.ptr(zd), *[L.ptr(t_) for t_ in tabs], None,
                                  L.ptr(tpd), 0, B, 3 * 16 * 16, G.stream()))
    torch.cuda.synchronize()
    for b in range(B):
        ref = O.p_sample_update(tab, x[b:b + 1], eps[b:b + 1], int(tps[b]), z[b:b + 1])
        assert torch.equal(xd[b:b + 1].cpu(), ref)
    step = torch.tensor([17], dtype=torch.int32, device=d)
    xd = x.to(d).clone()
    L.check(lib.sr3_p_sample_step(L.ptr(xd), L.ptr(ed), L.ptr(zd), *[L.ptr(t_) for t_ in tabs],
                                  L.ptr(step), None, 0, B, 3 * 16 * 16, G.stream()))
    L.check(lib.sr3_step_decrement(L.ptr(step), G.stream()))
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), O.p_sample_update(tab, x, eps, 17, z)) and int(step.item()) == 16


def test_q_sample_bit_exact():
    lib = L.load()
    d = G.dev()
    B = 4
    x0, z = _rand(B, 3, 8, 8, seed=1), _rand(B, 3, 8, 8, seed=2)
    g = torch.rand(B)
    ca, cb = g, (1 - g ** 2).sqrt()
    out = torch.empty(B, 3, 8, 8, device=d)
    dv = [x0.to(d), z.to(d), ca.to(d), cb.to(d)]
    L.check(lib.sr3_q_sample(*[L.ptr(t_) for t_ in dv], B, 3 * 64, L.ptr(out), G.stream()))
    torch.cuda.synchronize()
    ref = ca.view(-1, 1, 1, 1) * x0 + cb.view(-1, 1, 1, 1) * z
    assert torch.equal(out.cpu(), ref)


def test_split3_selftest():
    """The device self-test of split3_pair (the shipped form depends on register-resident selector constants and on
    v_dot2c_f32_bf16's exact result): 2^21 fp32 patterns, every one must equal h + m + l bit for bit."""
    import ctypes as C
    scratch = torch.zeros(1, dtype=torch.int32, device=G.dev())
    bad = C.c_int(-1)
    L.check(L.load().sr3_selftest_split3(L.ptr(scratch), C.byref(bad), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert bad.value == 0


def test_error_convention():
    lib = L.load()
    d = G.dev()
    x = torch.zeros(1, 4, 4, 6, device=d)      # C0 = 6 is not a multiple of 4
    w = torch.zeros(8, 9, 6, device=d)
    out = torch.zeros(1, 4, 4, 8, device=d)
    rc = lib.sr3_conv_f32(L.ptr(x), 6, None, 0, 1, 4, 4, 0, 1, 3, 8, L.ptr(w), None, None, 0, None, 0, None, 0, None, 0,
                          L.ptr(out), None, 0, 0, None, 0, G.stream())
    assert rc == -2 and b'multiples of 4' in lib.sr3_last_error()
    with pytest.raises(L.Sr3Error):
        L.check(rc)
