"""Per-op parity of the training backward's own kernels (through the C ABI) against float64 CPU autograd of the plain torch operation:
GroupNorm(+SiLU, +dropout) backward, the data gradient of a conv on every kernel the backward can choose, gradient routing, the bias /
FiLM column sums and the embedding backward.  The entries run the functions sr3_train_step's backward walk runs."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sr3_hip import lib as L                      # noqa: E402
import gpu_util as G                              # noqa: E402

NAN = float('nan')


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=G.dev())


def _bytes(n):
    return torch.empty(max(int(n), 256), dtype=torch.uint8, device=G.dev())


def _relerr(got, ref):
    ref = ref.double()
    return ((got.double() - ref).norm() / ref.norm()).item()


# ---- GroupNorm(+SiLU, +dropout) backward ------------------------------------------------------------------------------------------

GN_EPS = 1e-5
GN_CASES = [
    # B, C0, C1, H, W, groups, act, dropout p, ss / mr from the library's own stats + fold entries
    (2, 8, 16, 5, 7, 4, 2, 0.0, False),          # cpg 6: a group straddles the two sources; odd pixel count
    (2, 8, 16, 5, 7, 4, 2, 0.0, True),           # ... with the tables the step itself would read
    (3, 24, 0, 10, 10, 4, 2, 0.0, False),
    (1, 320, 0, 8, 8, 32, 2, 0.0, False),        # two channel blocks of the reduce, the second ragged (80 quads over 64 lanes)
    (2, 64, 0, 32, 32, 32, 1, 0.0, False),       # several pixel slices per image
    (1, 192, 128, 16, 16, 32, 2, 0.0, False),
    (2, 8, 0, 16, 24, 4, 2, 0.2, False),         # dropout between the activation and the conv
]
DROP_SEED, DROP_KEY = 0x1234ABCD, 5


def _gn_function(x, gamma, beta, groups, act, mask, dA):
    """the plain torch operation in x's dtype -> (the normalised input u, the activated and dropped input, its contraction with dA)"""
    u = F.group_norm(x, groups, gamma, beta, eps=GN_EPS)
    u.retain_grad()
    y = u * torch.sigmoid(u) if act == 2 else u
    if mask is not None:
        y = y * mask.to(x.dtype)
    return u, y, (y * dA.to(x.dtype)).sum()


def _gn_autograd(dtype, x, gamma, beta, groups, act, mask, dA):
    xs, gs, bs = (t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
    u, a, loss = _gn_function(xs, gs, bs, groups, act, mask, dA)
    loss.backward()
    return dict(dx=xs.grad, dgamma=gs.grad, dbeta=bs.grad, aout=a.detach(), du=u.grad)


def _gn_tables(x, gamma, beta, groups):
    """(scale, shift) per (image, channel) and (mean, rstd) per (image, group), evaluated in float64 and rounded once to fp32"""
    B, Cc = x.shape[:2]
    xg = x.double().reshape(B, groups, -1)
    mean = xg.mean(2)
    rstd = 1.0 / torch.sqrt(xg.var(2, unbiased=False) + GN_EPS)
    cpg = Cc // groups
    scale = rstd.repeat_interleave(cpg, 1) * gamma.double()[None]
    shift = beta.double()[None] - mean.repeat_interleave(cpg, 1) * scale
    return torch.stack([scale, shift], 2).float().contiguous(), torch.stack([mean, rstd], 2).float().contiguous()


def _gn_library_tables(lib, x0d, x1d, B, HW, C0, C1, groups, gd, bd):
    """ss / mr as the step makes them: the statistics pass per source, then the fold that keeps (mean, rstd)"""
    stats = []
    for xd, Cs in ((x0d, C0), (x1d, C1)):
        if xd is None:
            stats.append((None, 0, 0))
            continue
        T = int(lib.sr3_groupnorm_stats_slices(B, HW, Cs))
        st = _nan(B, T, Cs, 2, dtype=torch.float64)
        L.check(lib.sr3_groupnorm_stats_f32(L.ptr(xd), B, HW, Cs, L.ptr(st), G.stream()))
        stats.append((st, Cs, T))
    ss, mr = _nan(B, C0 + C1, 2), _nan(B, groups, 2)
    (s0, _, T0), (s1, _, T1) = stats
    L.check(lib.sr3_groupnorm_fold_mr_f32(L.ptr(s0), C0, T0, L.ptr(s1), C1, T1, B, HW, groups, L.ptr(gd), L.ptr(bd), GN_EPS, L.ptr(ss), L.ptr(mr),
                                          G.stream()))
    torch.cuda.synchronize()
    assert not torch.isnan(ss).any() and not torch.isnan(mr).any()
    return ss, mr


@pytest.mark.parametrize('case', GN_CASES, ids=['B%d_%d+%d_%dx%d_g%d_act%d_p%g%s' % (c[:8] + ('_libstats' if c[8] else '',)) for c in GN_CASES])
def test_groupnorm_act_backward(case):
    """dx0 / dx1 / dgamma / dbeta, the activated input and du (what dA is rewritten with) against float64 autograd of F.group_norm
    (-> SiLU -> the oracle's dropout mask) contracted with dA.  The bound is not a constant: torch's own fp32 CPU autograd of the same
    function on the same inputs is evaluated next to the kernel, and the kernel's normwise error may be at most twice that comparator's
    for each quantity (the margin covers the 1-ulp expf + 1-ulp v_rcp sigmoid and a different order of the roundings)."""
    from oracle import sr3_oracle as O
    B, C0, C1, H, W, groups, act, p, libstats = case
    lib, d = L.load(), G.dev()
    Cc, HW = C0 + C1, H * W
    x = _rand(B, Cc, H, W, seed=11) * 1.5 + 0.3
    gamma, beta = _rand(Cc, seed=12) * 0.3 + 1.0, _rand(Cc, seed=13) * 0.3
    dA = _rand(B, Cc, H, W, seed=14)
    mask = O.dropout_mask((B, Cc, H, W), p, DROP_SEED, DROP_KEY) if p else None
    lseed = (DROP_SEED + (DROP_KEY + 1) * 0x632BE5AB) & 0xFFFFFFFF
    ref = _gn_autograd(torch.float64, x, gamma, beta, groups, act, mask, dA)
    cmp32 = _gn_autograd(torch.float32, x, gamma, beta, groups, act, mask, dA)

    x0d = G.nhwc(x[:, :C0]).to(d)
    x1d = G.nhwc(x[:, C0:]).to(d) if C1 else None
    gd, bd = gamma.to(d), beta.to(d)
    if libstats:
        ss, mr = _gn_library_tables(lib, x0d, x1d, B, HW, C0, C1, groups, gd, bd)
    else:
        ss, mr = (t.to(d) for t in _gn_tables(x, gamma, beta, groups))
    nb = int(lib.sr3_groupnorm_act_bwd_scratch_bytes(B, HW, Cc, groups))
    assert nb > 0
    old0, old1 = _rand(B, H, W, C0, seed=15).to(d), (_rand(B, H, W, C1, seed=16).to(d) if C1 else None)

    def run(acc0, acc1):
        dAd = G.nhwc(dA).to(d)
        out = dict(dgamma=_nan(Cc), dbeta=_nan(Cc), aout=_nan(B, H, W, Cc), dx0=old0.clone() if acc0 else _nan(B, H, W, C0),
                   dx1=None if not C1 else (old1.clone() if acc1 else _nan(B, H, W, C1)))
        scratch = _bytes(nb)
        L.check(lib.sr3_groupnorm_act_bwd_f32(L.ptr(dAd), L.ptr(x0d), C0, L.ptr(x1d), C1, B, HW, L.ptr(ss), L.ptr(mr), groups, act, L.ptr(gd),
                                              lseed, p, L.ptr(out['dgamma']), L.ptr(out['dbeta']), L.ptr(out['dx0']), acc0, L.ptr(out['dx1']),
                                              acc1, L.ptr(out['aout']), L.ptr(scratch), nb, G.stream()))
        torch.cuda.synchronize()
        out['du'] = dAd
        return out

    first, again, other = run(1, 0), run(1, 0), run(0, 1)
    for k, v in first.items():              # two runs: the same bits; the flags move nothing but their own destination
        if v is not None:
            assert torch.equal(v, again[k]), k
            if k not in ('dx0', 'dx1'):
                assert torch.equal(v, other[k]), k
    plain0, plain1 = other['dx0'], first['dx1']                 # flag off: a plain store over the NaN pre-fill
    assert not torch.isnan(plain0).any() and (plain1 is None or not torch.isnan(plain1).any())
    assert torch.equal(first['dx0'], old0 + plain0)             # flag on: old + dx, one fp32 add
    if C1:
        assert torch.equal(other['dx1'], old1 + plain1)
    got = dict(dx0=G.nchw(plain0).cpu(), dgamma=first['dgamma'].cpu(), dbeta=first['dbeta'].cpu(), aout=G.nchw(first['aout']).cpu(),
               du=G.nchw(first['du']).cpu())
    want = dict(dx0=(ref['dx'][:, :C0], cmp32['dx'][:, :C0]), dgamma=(ref['dgamma'], cmp32['dgamma']), dbeta=(ref['dbeta'], cmp32['dbeta']),
                aout=(ref['aout'], cmp32['aout']), du=(ref['du'], cmp32['du']))
    if C1:
        got['dx1'] = G.nchw(plain1).cpu()
        want['dx1'] = (ref['dx'][:, C0:], cmp32['dx'][:, C0:])
    bad = []
    for k in sorted(got):
        assert not torch.isnan(got[k]).any(), k
        e_k, e_c = _relerr(got[k], want[k][0]), _relerr(want[k][1], want[k][0])
        print('groupnorm backward %s %s: kernel %.3e, torch fp32 CPU autograd %.3e (normwise vs float64)' % (case, k, e_k, e_c))
        if not e_k <= 2.0 * e_c:
            bad.append((k, e_k, e_c))
    assert not bad, 'normwise error above twice the fp32 comparator\'s (quantity, kernel, comparator): %s' % bad


# ---- gradient routing --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('Hs,Ws', [(5, 7), (16, 24)])
@pytest.mark.parametrize('ups', [0, 1])
@pytest.mark.parametrize('C0,C1', [(8, 0), (8, 16), (128, 64)])
def test_grad_route(C0, C1, ups, Hs, Ws, B):
    """The routing kernel copies or adds: bit equality with fp32 torch doing the same adds in the kernel's order -- ((a + b) + c) + d for
    the 2 x 2 children of the nearest x2 upsample, then + the destination's old value where the flag is on."""
    lib, d = L.load(), G.dev()
    Cc = C0 + C1
    g = _rand(B, Hs << ups, Ws << ups, Cc, seed=21)
    s = g
    if ups:
        s = ((g[:, 0::2, 0::2] + g[:, 0::2, 1::2]) + g[:, 1::2, 0::2]) + g[:, 1::2, 1::2]
    old0, old1 = _rand(B, Hs, Ws, C0, seed=22), (_rand(B, Hs, Ws, C1, seed=23) if C1 else None)
    gd = g.to(d)
    for acc0 in (0, 1):
        for acc1 in ((0, 1) if C1 else (0,)):
            d0 = old0.to(d) if acc0 else _nan(B, Hs, Ws, C0)
            d1 = None if not C1 else (old1.to(d) if acc1 else _nan(B, Hs, Ws, C1))
            L.check(lib.sr3_grad_route_f32(L.ptr(gd), C0, C1, B, Hs, Ws, ups, L.ptr(d0), acc0, L.ptr(d1), acc1, G.stream()))
            torch.cuda.synchronize()
            r0 = s[..., :C0] + old0 if acc0 else s[..., :C0]
            assert torch.equal(d0.cpu(), r0.contiguous()), (acc0, acc1)
            if C1:
                r1 = s[..., C0:] + old1 if acc1 else s[..., C0:]
                assert torch.equal(d1.cpu(), r1.contiguous()), (acc0, acc1)


# ---- bias / FiLM column sums -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode', ['bias', 'film', 'both'])
@pytest.mark.parametrize('B,HW,Cc', [(3, 35, 8), (2, 1024, 64), (1, 64, 320), (4, 256, 4), (4, 256, 8)])
def test_colsums(B, HW, Cc, mode):
    """Bias gradient (sum over images and pixels) and FiLM gradient rows (sum over pixels) against the float64 sum: a double accumulation
    rounded once to fp32, |got - ref| <= 2^-24 |ref| + 1e-12 sum |g| per element.  The FiLM rows land in a wider table at an offset:
    nothing else of the table may change."""
    lib, d = L.load(), G.dev()
    g = _rand(B, HW, Cc, seed=31) + 0.25
    gd = g.to(d)
    stride, row = 2 * Cc + 12, 8
    table0 = _rand(B, stride, seed=32)
    table = table0.to(d)
    table[:, row:row + Cc] = NAN
    dbias = _nan(Cc) if mode != 'film' else None
    nb = int(lib.sr3_colsums_scratch_bytes(B, HW, Cc))
    scratch = _bytes(nb)
    film_ptr = C.c_void_p(table.data_ptr() + 4 * row) if mode != 'bias' else None
    L.check(lib.sr3_colsums_f32(L.ptr(gd), B, HW, Cc, L.ptr(dbias), film_ptr, stride, L.ptr(scratch), nb, G.stream()))
    torch.cuda.synchronize()
    gg = g.double()

    def check(got, ref, mag, what):
        err = (got.double() - ref).abs()
        bound = 2.0 ** -24 * ref.abs() + 1e-12 * mag
        assert not torch.isnan(got).any() and bool((err <= bound).all()), '%s: worst err / bound %.3g' % (what, (err / bound).max().item())
    if mode != 'film':
        check(dbias.cpu(), gg.sum((0, 1)), gg.abs().sum((0, 1)), 'bias gradient')
    out = table.cpu()
    keep = torch.ones(stride, dtype=torch.bool)
    keep[row:row + Cc] = False
    assert torch.equal(out[:, keep], table0[:, keep])
    if mode != 'bias':
        check(out[:, row:row + Cc], gg.sum(1), gg.abs().sum(1), 'FiLM rows')
    else:
        assert bool(torch.isnan(out[:, row:row + Cc]).all())


# ---- data gradient of a conv -------------------------------------------------------------------------------------------------------

WINOGRAD_TILES = {11, 12, 13, 23}
GENERIC_TILES = set(range(1, 11)) | set(range(14, 18))        # im2col / halo kernels: what the backward lands on without derived filters


def _tiny_plan(**options):
    from sr3_hip import engine as E
    p = E.Plan('sr3', 6, 3, 8, 4, [1, 2], [8], 1, 16)
    geometry = options.pop('geometry', None)
    for k, v in options.items():
        p.set_option(k, v)
    if geometry:
        p.set_geometry(*geometry)
    return p


def _dgrad_call(plan, dy, w, B, Hs, Ws, ups, stride, with_derived=True, slab_room=None):
    """dy NCHW [B, CoutP, Ho, Wo], w OIHW [Cout_w, Cin, k, k] (CPU) -> (dA NCHW cpu, tile, ksplit, derived kind).  with_derived False:
    no room for derived filters; slab_room: bytes of split-K room behind the filters instead of what the query asks for."""
    lib, d = L.load(), G.dev()
    Cout_w, Cin, k, _ = w.shape
    CoutP = dy.shape[1]
    nd, base = C.c_size_t(0), C.c_size_t(0)
    nb = int(lib.sr3_conv_dgrad_scratch_bytes(plan.handle, B, Hs, Ws, ups, stride, k, Cin, CoutP, C.byref(nd), C.byref(base)))
    assert nb >= base.value > 0
    if slab_room is not None:
        nb = base.value + slab_room
    scratch = _bytes(nb)
    derived = _bytes(nd.value) if with_derived and nd.value else None
    dyd, wd = G.nhwc(dy).to(d), G.ohwi(w).to(d)
    dA = _nan(B, Hs << ups, Ws << ups, Cin)
    tile, ks, kind = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    L.check(lib.sr3_conv_dgrad_f32(plan.handle, L.ptr(dyd), L.ptr(wd), Cout_w, CoutP, B, Hs, Ws, ups, stride, k, Cin, L.ptr(dA), L.ptr(scratch), nb,
                                   L.ptr(derived), nd.value if derived is not None else 0, C.byref(tile), C.byref(ks), C.byref(kind), G.stream()))
    torch.cuda.synchronize()
    return G.nchw(dA).cpu(), tile.value, ks.value, kind.value


def _dgrad_ref(dy, w, B, Hs, Ws, ups, stride):
    """float64 autograd of F.conv2d: the gradient w.r.t. the conv's input behind the nearest x2 upsample (the entry's dA: before routing)"""
    Cout_w, Cin, k, _ = w.shape
    x = torch.zeros(B, Cin, Hs, Ws, dtype=torch.float64, requires_grad=True)
    xi = F.interpolate(x, scale_factor=2, mode='nearest') if ups else x
    xi.retain_grad()
    y = F.conv2d(xi, w.double(), None, stride=stride, padding=k // 2)
    y.backward(dy[:, :Cout_w].double())
    return xi.grad


DGRAD_CASES = [
    # name, plan options, B, Hs, Ws, Cin, Cout_w, CoutP, ksize, stride, ups, expected tile, expected derived kind, split-K expected (None: either)
    ('wino_2wg', {}, 1, 16, 16, 32, 32, 32, 3, 1, 0, 13, 2, None),
    ('wino_8wave', {'wino2': 0}, 1, 16, 16, 32, 32, 32, 3, 1, 0, 12, 2, None),
    ('wino_fp32', {'wino_split': 0}, 1, 16, 16, 32, 32, 32, 3, 1, 0, 11, 1, None),
    ('wino_four_image', {}, 4, 8, 8, 64, 32, 32, 3, 1, 0, 11, 1, True),
    ('geom_8x16_multiple', {'train_geom': 1, 'geometry': (24, 40)}, 2, 24, 16, 32, 32, 32, 3, 1, 0, 13, 2, None),
    ('geom_ragged', {'train_geom': 1, 'geometry': (24, 40)}, 2, 24, 40, 24, 40, 40, 3, 1, 0, 23, 2, None),
    ('gemm_128_from_64', {}, 1, 8, 8, 128, 64, 64, 1, 1, 0, 22, 3, None),
    ('gemm_128_from_256_slabs', {}, 1, 8, 8, 128, 256, 256, 1, 1, 0, 22, 3, True),
    ('gemm_n64', {}, 1, 8, 8, 64, 64, 64, 1, 1, 0, 22, 3, None),
    ('gemm_n64_off', {'gemm_n64': 0}, 1, 8, 8, 64, 64, 64, 1, 1, 0, 16, 0, None),
    ('generic_3x3', {}, 3, 10, 12, 24, 8, 8, 3, 1, 0, 3, 0, None),
    ('generic_1x1', {}, 2, 5, 7, 24, 40, 40, 1, 1, 0, 16, 0, None),
    ('stride2_generic', {}, 2, 16, 24, 16, 16, 16, 3, 2, 0, 3, 0, None),
    ('stride2_wino', {}, 4, 16, 16, 128, 128, 128, 3, 2, 0, 13, 2, None),
    ('upsample', {}, 2, 8, 8, 32, 32, 32, 3, 1, 1, 13, 2, None),
    ('out_block_3_of_4', {}, 1, 16, 16, 32, 3, 4, 3, 1, 0, 13, 2, None),
    ('out_block_6_of_8', {}, 1, 16, 16, 32, 6, 8, 3, 1, 0, 13, 2, None),
]


def _dgrad_inputs(case):
    name, opts, B, Hs, Ws, Cin, Cout_w, CoutP, k, stride, ups, tile, kind, split = case
    Ho, Wo = ((Hs << ups) + 2 * (k // 2) - k) // stride + 1, ((Ws << ups) + 2 * (k // 2) - k) // stride + 1
    # the lanes of dy beyond Cout_w: in the step the loss kernel writes them 0; here they hold finite garbage, which the zero rows of the
    # flipped-transposed filters must keep out of dA
    dy = _rand(B, CoutP, Ho, Wo, seed=41)
    dy[:, Cout_w:] = _rand(B, CoutP - Cout_w, Ho, Wo, seed=42) * 7.0 + 3.0
    w = _rand(Cout_w, Cin, k, k, seed=43, scale=1.0 / math.sqrt(Cout_w * k * k))
    return dy, w


@pytest.mark.parametrize('case', DGRAD_CASES, ids=[c[0] for c in DGRAD_CASES])
def test_conv_dgrad(case):
    """dy -> dA through zero insertion (stride 2), the flipped-transposed (and zero-padded) filters, their derived forms and the kernel
    choose_dgrad picks, against the float64 x.grad of F.conv2d.  Each case asserts the kernel it ran; the bound is the forward suite's for
    that kernel: G.assert_close's default for the direct, im2col and GEMM tiles, and for the Winograd tiles (11, 12, 13, 23) on top of it
    the fp32-class bound of test_gpu_ops.py's test_winograd_conv_error_is_fp32_class against the direct kernel on the same data -- max
    error within 4 x and rms error within 3 x the direct kernel's (+ 1e-7 / 1e-8 of max |ref|).  The same problem on the general kernels
    (winograd 0, gemm2 0) is that direct result: it must meet its own bound, and the two agree within the sum of their bounds."""
    name, opts, B, Hs, Ws, Cin, Cout_w, CoutP, k, stride, ups, tile, kind, split = case
    dy, w = _dgrad_inputs(case)
    ref = _dgrad_ref(dy, w, B, Hs, Ws, ups, stride)
    got, t, ks, kd = _dgrad_call(_tiny_plan(**dict(opts)), dy, w, B, Hs, Ws, ups, stride)
    assert (t, kd) == (tile, kind), 'ran tile %d (ksplit %d, derived kind %d), expected tile %d / kind %d' % (t, ks, kd, tile, kind)
    assert ks >= 1 and (split is None or (ks > 1) == split), ks
    assert not torch.isnan(got).any()
    e = G.assert_close(got, ref, what='dgrad ' + name)
    general, tg, ksg, kdg = _dgrad_call(_tiny_plan(**dict(opts, winograd=0, gemm2=0)), dy, w, B, Hs, Ws, ups, stride)
    assert tg in GENERIC_TILES and kdg == 0, (tg, kdg)
    eg = G.assert_close(general, ref, what='dgrad ' + name + ' (general kernels)')
    scale = max(1.0, ref.abs().max().item())
    assert (got - general).abs().max().item() <= 2 * 2e-5 * scale
    rms, rmsg = (got.double() - ref).pow(2).mean().sqrt().item(), (general.double() - ref).pow(2).mean().sqrt().item()
    print('dgrad %s: tile %d ksplit %d max / rms err %.2e / %.2e; general kernels tile %d ksplit %d max / rms err %.2e / %.2e; |ref|max %.2f'
          % (name, t, ks, e, rms, tg, ksg, eg, rmsg, ref.abs().max().item()))
    if t in WINOGRAD_TILES:
        assert e <= 4.0 * eg + 1e-7 * ref.abs().max().item(), (e, eg)
        assert rms <= 3.0 * rmsg + 1e-8 * ref.abs().max().item(), (rms, rmsg)


@pytest.mark.parametrize('name', ['wino_2wg', 'gemm_128_from_64', 'gemm_128_from_256_slabs'])
def test_conv_dgrad_falls_back_without_room(name):
    """The step takes a kernel that reads derived filters only where they fit, and the GEMM kernel only where its split-K slabs fit too:
    with no room for either, the entry lands on the general kernels -- same result to the bound -- instead of refusing."""
    case = [c for c in DGRAD_CASES if c[0] == name][0]
    _, opts, B, Hs, Ws, Cin, Cout_w, CoutP, k, stride, ups, tile, kind, split = case
    dy, w = _dgrad_inputs(case)
    ref = _dgrad_ref(dy, w, B, Hs, Ws, ups, stride)
    got, t, ks, kd = _dgrad_call(_tiny_plan(**dict(opts)), dy, w, B, Hs, Ws, ups, stride, with_derived=False)
    assert t in GENERIC_TILES and kd == 0, (t, kd)
    G.assert_close(got, ref, what='dgrad fallback ' + name)
    if split:        # derived filters fit, the GEMM kernel's slabs do not: the general kernel, which splits less (here: not at all)
        got, t, ks, kd = _dgrad_call(_tiny_plan(**dict(opts)), dy, w, B, Hs, Ws, ups, stride, slab_room=0)
        assert t in GENERIC_TILES and kd == 0 and ks == 1, (t, ks, kd)
        G.assert_close(got, ref, what='dgrad slab fallback ' + name)


# ---- embedding / FiLM backward -----------------------------------------------------------------------------------------------------

EMBED_CASES = [(0, 1, 8, 40), (1, 3, 8, 40), (0, 3, 64, 1000), (1, 2, 128, 136), (0, 2, 256, 24), (0, 2, 4, 5)]


@pytest.mark.parametrize('variant,B,inner,Fn', EMBED_CASES)
def test_embed_backward(variant, B, inner, Fn):
    """The six gradients of encoding -> Linear -> Swish -> Linear (-> Swish, ddpm) -> FiLM Linear contracted with dfilm, against float64
    autograd on the encoding of the same fp32 level * freq argument (test_film_embed's forward reference): normwise 2e-6, the fp32-class
    bound of the weight gradients.  inner 64 / 128 / 256 walk the 4 / 2 / 1 row partitions of the FiLM input gradient, F < 16 leaves
    row chunks empty."""
    lib, d = L.load(), G.dev()
    w1, b1 = _rand(4 * inner, inner, seed=1) * 0.1, _rand(4 * inner, seed=2) * 0.1
    w2, b2 = _rand(inner, 4 * inner, seed=3) * 0.1, _rand(inner, seed=4) * 0.1
    wf, bf = _rand(Fn, inner, seed=5) * 0.1, _rand(Fn, seed=6) * 0.1
    dfilm = _rand(B, Fn, seed=7)
    if variant == 0:
        level, tstep = torch.tensor([0.999, 0.5, 0.013])[:B].contiguous(), None
        count = inner // 2
        freq = torch.exp(-math.log(1e4) * (torch.arange(count, dtype=torch.float32) / count))
        arg = level[:, None] * freq[None]
    else:
        level, tstep = None, torch.tensor([0, 999, 1999], dtype=torch.long)[:B].contiguous()
        freq = torch.exp(torch.arange(0, inner, 2, dtype=torch.float32) * (-math.log(10000) / inner))
        arg = torch.outer(tstep.float(), freq)
    enc = torch.cat([arg.sin(), arg.cos()], -1).double()
    P = [t.double().clone().requires_grad_(True) for t in (w1, b1, w2, b2, wf, bf)]
    h = enc @ P[0].t() + P[1]
    h = h * torch.sigmoid(h)
    t = h @ P[2].t() + P[3]
    if variant == 1:
        t = t * torch.sigmoid(t)
    ((t @ P[4].t() + P[5]) * dfilm.double()).sum().backward()
    g = lambda v: None if v is None else v.to(d)
    dv = [g(v) for v in (level, tstep, freq, w1, b1, w2, b2, wf, dfilm)]
    nb = int(lib.sr3_embed_bwd_scratch_bytes(B, inner))

    def run():
        outs = [_nan(*v.shape) for v in (w1, b1, w2, b2, wf, bf)]
        scratch = _bytes(nb)
        L.check(lib.sr3_embed_bwd_f32(variant, B, inner, Fn, *[L.ptr(v) for v in dv], *[L.ptr(o) for o in outs], L.ptr(scratch), nb, G.stream()))
        torch.cuda.synchronize()
        return outs
    first, again = run(), run()
    bad = []
    for name, got, got2, p in zip(('dw1', 'db1', 'dw2', 'db2', 'dwf', 'dbf'), first, again, P):
        assert torch.equal(got, got2), name
        assert not torch.isnan(got).any(), name
        e = _relerr(got.cpu(), p.grad)
        print('embed backward variant %d B %d inner %d F %d %s: normwise %.3e' % (variant, B, inner, Fn, name, e))
        if not e <= 2e-6:
            bad.append((name, e))
    assert not bad, bad
