"""Per-op parity of the scale-shift modulation's two entries (through the C ABI): sr3_groupnorm_fold_mod_f32 against float64, and
sr3_groupnorm_act_bwd_mod_f32 against float64 autograd of tests/adagn_ref.py's normalisation under the bound tests/test_gpu_backward_ops.py
applies to the plain entry (at most twice the error of torch's own fp32 CPU autograd of the same function); their bits against the plain
entries' where the rows are zero; their refusals.  All shapes are tiny: B <= 3, 16 pixels.

(The pairs a FUSED fold writes have no per-op door: their bit equality with this entry's is checked through a plan, fold_fuse 0
against 1, in tests/test_gpu_scale_shift_unet.py.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from sr3_hip import lib as L                      # noqa: E402
import gpu_util as G                              # noqa: E402
import adagn_ref                                  # noqa: E402
import test_gpu_backward_ops as BO                # noqa: E402  (its helpers and its bound: _rand, _nan, _bytes, _relerr, _gn_tables)

EPS = BO.GN_EPS
SHAPES = [(32, 32), (64, 16), (192, 2)]           # (C, groups): 1, 4 and 96 channels per group -- the last exceeds the 64 lanes of the write loop
HW, H, W = 16, 4, 4
PAD = 8                                           # floats between the images' rows of mod / dmod: mod_stride = 2 C + PAD


def _mod(B, C, seed):
    """[B][2 C + PAD]: scales in [-1.5, 1.5] with one (b, c) at exactly -1 (1 + s = 0), shifts, and a NaN pad nobody may read"""
    g = torch.Generator().manual_seed(seed)
    m = torch.full((B, 2 * C + PAD), float('nan'))
    m[:, :C] = torch.rand(B, C, generator=g) * 3 - 1.5
    m[:, C:2 * C] = torch.randn(B, C, generator=g) * 0.5
    m[B - 1, C // 2 + 1] = -1.0
    return m


def _stats(lib, xd, B, Cs):
    T = int(lib.sr3_groupnorm_stats_slices(B, HW, Cs))
    st = BO._nan(B, T, Cs, 2, dtype=torch.float64)
    L.check(lib.sr3_groupnorm_stats_f32(L.ptr(xd), B, HW, Cs, L.ptr(st), G.stream()))
    return st, T


def _fold(lib, entry, srcs, B, groups, gd, bd, mod=None, mr=True):
    """ss [B][C][2], mr [B][groups][2] of the virtual concat of `srcs` (NHWC device tensors) through `entry`"""
    C = sum(s.shape[-1] for s in srcs)
    st = [_stats(lib, s, B, s.shape[-1]) for s in srcs] + [(None, 0)]
    ss, mrt = BO._nan(B, C, 2), (BO._nan(B, groups, 2) if mr else None)
    args = [L.ptr(st[0][0]), srcs[0].shape[-1], st[0][1], L.ptr(st[1][0]), C - srcs[0].shape[-1], st[1][1], B, HW, groups, L.ptr(gd), L.ptr(bd), EPS,
            L.ptr(ss)]
    if entry == 'mod':
        rc = lib.sr3_groupnorm_fold_mod_f32(*args, L.ptr(mrt), L.ptr(mod), mod.shape[1], G.stream())
    else:
        rc = lib.sr3_groupnorm_fold_mr_f32(*args, L.ptr(mrt), G.stream())
    torch.cuda.synchronize()
    return rc, ss, mrt


FOLD_CASES = [(C, g, 0) for C, g in SHAPES] + [(64, 16, 24)]         # the last: two concat sources of 24 + 40 channels, a group across the seam


@pytest.mark.parametrize('C,groups,C0', FOLD_CASES, ids=['C%d_g%d%s' % (c, g, '_concat%d' % c0 if c0 else '') for c, g, c0 in FOLD_CASES])
def test_fold_mod_against_float64_and_the_plain_fold(C, groups, C0):
    lib, d, B = L.load(), G.dev(), 3
    x = BO._rand(B, C, H, W, seed=31) * 1.5 + 0.3
    gamma, beta = BO._rand(C, seed=32) * 0.3 + 1.0, BO._rand(C, seed=33) * 0.3
    mod = _mod(B, C, 34)
    xd = G.nhwc(x).to(d)
    srcs = [xd] if not C0 else [xd[..., :C0].contiguous(), xd[..., C0:].contiguous()]
    gd, bd, modd = gamma.to(d), beta.to(d), mod.to(d)
    rc, ss, mr = _fold(lib, 'mod', srcs, B, groups, gd, bd, modd)
    L.check(rc)
    assert not torch.isnan(ss).any() and not torch.isnan(mr).any()
    ref = adagn_ref.modulated_norm(x.double(), groups, gamma.double(), beta.double(), mod[:, :C].double(), mod[:, C:2 * C].double())
    ssc = ss.cpu().double()
    got = x.double() * ssc[:, :, 0, None, None] + ssc[:, :, 1, None, None]
    err = G.assert_close(got, ref, what='modulated fold')
    print('fold_mod C %d groups %d C0 %d: max abs err of x sc + sh against float64 %.2e (|ref| max %.2f)' % (C, groups, C0, err, ref.abs().max().item()))
    # 1 + s = 0: the pair is (0, t) exactly -- the shift alone survives
    b, c = B - 1, C // 2 + 1
    assert ss[b, c, 0].item() == 0.0 and ss[b, c, 1].item() == mod[b, C + c].item()
    # without mr: the same pairs
    rc, ss2, _ = _fold(lib, 'mod', srcs, B, groups, gd, bd, modd, mr=False)
    L.check(rc)
    assert torch.equal(ss, ss2)
    # rows of zeros: the bits of the plain fold, pairs and (mean, rstd)
    zero = torch.zeros_like(modd)
    rc, ssz, mrz = _fold(lib, 'mod', srcs, B, groups, gd, bd, zero)
    L.check(rc)
    rc, ssp, mrp = _fold(lib, 'plain', srcs, B, groups, gd, bd)
    L.check(rc)
    assert torch.equal(ssz, ssp) and torch.equal(mrz, mrp) and torch.equal(mr, mrp)


# ---- backward ------------------------------------------------------------------------------------------------------------------------

DROP_SEED, DROP_KEY = 0x1234ABCD, 5


def _autograd(dtype, x, gamma, beta, groups, mod, C, mask, dA):
    xs, gs, bs, sc, sh = (t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta, mod[:, :C], mod[:, C:2 * C]))
    u = adagn_ref.modulated_norm(xs, groups, gs, bs, sc, sh)
    u.retain_grad()
    y = u * torch.sigmoid(u)
    if mask is not None:
        y = y * mask.to(dtype)
    (y * dA.to(dtype)).sum().backward()
    return dict(dx=xs.grad, dgamma=gs.grad, dbeta=bs.grad, dscale=sc.grad, dshift=sh.grad, du=u.grad, aout=y.detach())


def _tables(x, gamma, beta, groups, mod, C):
    """the modulated (scale, shift) pairs and (mean, rstd), evaluated in float64 and rounded once to fp32"""
    ss, mr = BO._gn_tables(x, gamma, beta, groups)
    B = x.shape[0]
    xg = x.double().reshape(B, groups, -1)
    mean, rstd = xg.mean(2), 1.0 / torch.sqrt(xg.var(2, unbiased=False) + EPS)
    cpg = C // groups
    sc = rstd.repeat_interleave(cpg, 1) * gamma.double()[None]
    sh = beta.double()[None] - mean.repeat_interleave(cpg, 1) * sc
    m = 1 + mod[:, :C].double()
    return torch.stack([sc * m, sh * m + mod[:, C:2 * C].double()], 2).float().contiguous(), ss, mr


def _bwd(lib, entry, dA, xd, B, C, groups, ss, mr, gd, p, lseed, bd=None, modd=None):
    d = G.dev()
    dAd = G.nhwc(dA).to(d)
    out = dict(dgamma=BO._nan(C), dbeta=BO._nan(C), aout=BO._nan(B, H, W, C), dx=BO._nan(B, H, W, C))
    nb = int(lib.sr3_groupnorm_act_bwd_scratch_bytes(B, HW, C, groups))
    scratch = BO._bytes(nb)
    args = [L.ptr(dAd), L.ptr(xd), C, None, 0, B, HW, L.ptr(ss), L.ptr(mr), groups, 2, L.ptr(gd), lseed, p, L.ptr(out['dgamma']), L.ptr(out['dbeta']),
            L.ptr(out['dx']), 0, None, 0, L.ptr(out['aout']), L.ptr(scratch), nb]
    if entry == 'mod':
        out['dmod'] = BO._nan(*modd.shape)
        rc = lib.sr3_groupnorm_act_bwd_mod_f32(*args, L.ptr(bd), L.ptr(modd), modd.shape[1], L.ptr(out['dmod']), G.stream())
    else:
        rc = lib.sr3_groupnorm_act_bwd_f32(*args, G.stream())
    torch.cuda.synchronize()
    out['du'] = dAd
    return rc, out


@pytest.mark.parametrize('p', [0.0, 0.2], ids=['nodrop', 'drop0.2'])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('C,groups', SHAPES, ids=['C%d_g%d' % s for s in SHAPES])
def test_act_bwd_mod_against_float64_autograd(C, groups, B, p):
    """du, dx, dgamma, dbeta, the activated input and the rows' gradients against float64 autograd of GN(x) (1 + s) + t -> SiLU -> the
    oracle's dropout mask, contracted with dA, under test_groupnorm_act_backward's bound: the kernel's normwise error may be at most
    twice that of torch's fp32 CPU autograd of the same function on the same inputs, per quantity."""
    from oracle import sr3_oracle as O
    lib, d = L.load(), G.dev()
    x = BO._rand(B, C, H, W, seed=41) * 1.5 + 0.3
    gamma, beta = BO._rand(C, seed=42) * 0.3 + 1.0, BO._rand(C, seed=43) * 0.3
    dA = BO._rand(B, C, H, W, seed=44)
    mod = _mod(B, C, 45)
    mask = O.dropout_mask((B, C, H, W), p, DROP_SEED, DROP_KEY) if p else None
    lseed = (DROP_SEED + (DROP_KEY + 1) * 0x632BE5AB) & 0xFFFFFFFF
    ref = _autograd(torch.float64, x, gamma, beta, groups, mod, C, mask, dA)
    cmp32 = _autograd(torch.float32, x, gamma, beta, groups, mod, C, mask, dA)
    ssm, ss0, mr = (t.to(d) for t in _tables(x, gamma, beta, groups, mod, C))
    xd, gd, bd, modd = G.nhwc(x).to(d), gamma.to(d), beta.to(d), mod.to(d)

    rc, first = _bwd(lib, 'mod', dA, xd, B, C, groups, ssm, mr, gd, p, lseed, bd, modd)
    L.check(rc)
    rc, again = _bwd(lib, 'mod', dA, xd, B, C, groups, ssm, mr, gd, p, lseed, bd, modd)
    L.check(rc)
    for k in first:                          # two runs: the same bits (NaN pads included)
        assert torch.equal(first[k].view(torch.int32), again[k].view(torch.int32)), k
    dmod = first['dmod'].cpu()
    assert torch.isnan(dmod[:, 2 * C:]).all(), 'the entry wrote beyond the 2 C entries of an image'
    got = dict(dx=G.nchw(first['dx']).cpu(), dgamma=first['dgamma'].cpu(), dbeta=first['dbeta'].cpu(), aout=G.nchw(first['aout']).cpu(),
               du=G.nchw(first['du']).cpu(), dscale=dmod[:, :C], dshift=dmod[:, C:2 * C])
    bad = []
    for k in sorted(got):
        assert not torch.isnan(got[k]).any(), k
        e_k, e_c = BO._relerr(got[k], ref[k]), BO._relerr(cmp32[k], ref[k])
        print('modulated groupnorm backward C %d groups %d B %d p %g %s: kernel %.3e, torch fp32 CPU autograd %.3e (normwise vs float64)'
              % (C, groups, B, p, k, e_k, e_c))
        if not e_k <= 2.0 * e_c:
            bad.append((k, e_k, e_c))
    assert not bad, 'normwise error above twice the fp32 comparator\'s (quantity, kernel, comparator): %s' % bad

    # rows of zeros: the plain entry's dx, dgamma, dbeta (and du, aout) bits, on the same unmodulated tables
    zero = torch.zeros_like(modd)
    rc, z = _bwd(lib, 'mod', dA, xd, B, C, groups, ss0.to(d), mr, gd, p, lseed, bd, zero)
    L.check(rc)
    rc, plain = _bwd(lib, 'plain', dA, xd, B, C, groups, ss0.to(d), mr, gd, p, lseed)
    L.check(rc)
    for k in plain:
        assert torch.equal(z[k], plain[k]), k


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    """NULL mod, mod_stride < 2 C, C % groups, C % 4 (and, backward, NULL beta / dmod): the code, the entry's name in the message, and
    every output as it was."""
    lib, d = L.load(), G.dev()
    B, C, groups = 2, 32, 8
    x = BO._rand(B, C, H, W, seed=51)
    xd = G.nhwc(x).to(d)
    gd, bd = torch.ones(C, device=d), torch.zeros(C, device=d)
    modd = torch.zeros(B, 2 * C, device=d)
    st, T = _stats(lib, xd, B, C)
    torch.cuda.synchronize()
    BAD, UNS = -1, -2

    def fold(C_=C, groups_=groups, mod_=modd, stride_=2 * C):
        ss, mr = BO._nan(B, C, 2), BO._nan(B, groups, 2)
        rc = lib.sr3_groupnorm_fold_mod_f32(L.ptr(st), C_, T, None, 0, 0, B, HW, groups_, L.ptr(gd), L.ptr(bd), EPS, L.ptr(ss), L.ptr(mr),
                                            L.ptr(mod_), stride_, G.stream())
        torch.cuda.synchronize()
        assert torch.isnan(ss).all() and torch.isnan(mr).all(), 'a refused fold wrote its outputs'
        return rc, (lib.sr3_last_error() or b'').decode()

    for kw, code in ((dict(mod_=None), BAD), (dict(stride_=2 * C - 1), BAD), (dict(groups_=5), UNS), (dict(C_=30, groups_=5, stride_=64), UNS)):
        rc, msg = fold(**kw)
        assert rc == code and msg.startswith('sr3_groupnorm_fold_mod_f32'), (kw, rc, msg)

    ss, mr = (t.to(d) for t in BO._gn_tables(x, gd.cpu(), bd.cpu(), groups))
    nb = int(lib.sr3_groupnorm_act_bwd_scratch_bytes(B, HW, C, groups))
    scratch = BO._bytes(nb)
    dA0 = BO._rand(B, H, W, C, seed=52).to(d)

    def bwd(C_=C, groups_=groups, mod_=modd, stride_=2 * C, beta_=bd, dmod_=True):
        dA = dA0.clone()
        outs = [BO._nan(C), BO._nan(C), BO._nan(B, H, W, C), BO._nan(B, H, W, C), BO._nan(B, 2 * C)]
        rc = lib.sr3_groupnorm_act_bwd_mod_f32(L.ptr(dA), L.ptr(xd), C_, None, 0, B, HW, L.ptr(ss), L.ptr(mr), groups_, 2, L.ptr(gd), 0, 0.0,
                                               L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(outs[2]), 0, None, 0, L.ptr(outs[3]), L.ptr(scratch), nb,
                                               L.ptr(beta_), L.ptr(mod_), stride_, L.ptr(outs[4]) if dmod_ else None, G.stream())
        torch.cuda.synchronize()
        assert torch.equal(dA, dA0) and all(torch.isnan(o).all() for o in outs), 'a refused backward wrote its outputs'
        return rc, (lib.sr3_last_error() or b'').decode()

    for kw, code in ((dict(mod_=None), BAD), (dict(beta_=None), BAD), (dict(dmod_=False), BAD), (dict(stride_=2 * C - 1), BAD),
                     (dict(groups_=5), UNS), (dict(C_=30, groups_=5, stride_=64), UNS)):
        rc, msg = bwd(**kw)
        assert rc == code and msg.startswith('sr3_groupnorm_act_bwd_mod_f32'), (kw, rc, msg)
