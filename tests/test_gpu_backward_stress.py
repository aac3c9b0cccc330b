"""The training backward's own kernels (through the C ABI) on data built to hurt them -- tests/backward_stress.py holds the generators, the
float64 references and the conditions, which tests/test_backward_stress_cpu.py asserts without a device:

  * k_attention_bwd (all three instantiations, one head and several) on peaked softmax rows;
  * the weight-gradient kernels of wgrad.hip on heavy-tailed operands against an absolute float64 bound;
  * k_act_bwd_reduce / k_gn_bwd_apply on groups with a DC offset and on a nearly constant group.

Every case prints the kernel's error next to torch's fp32 CPU autograd's on the same data (profiles/backward_stress.txt is one run)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import backward_stress as S                       # noqa: E402
import gpu_util as G                              # noqa: E402
import test_gpu_backward_ops as T                 # noqa: E402  (the harness of test_groupnorm_act_backward)
from sr3_hip import lib as L                      # noqa: E402

NAN = float('nan')


def _nan(*shape):
    return torch.full(shape, NAN, device=G.dev())


# ---- attention backward on peaked softmax -------------------------------------------------------------------------------------------

def _attn_forward(qd, B, N, C, heads):
    """the forward output the library writes, as the existing backward tests make it"""
    lib = L.load()
    out = _nan(B, N, C)
    if heads == 1:
        L.check(lib.sr3_attention_f32(L.ptr(qd), B, N, C, L.ptr(out), G.stream()))
    else:
        L.check(lib.sr3_attention_heads_f32(L.ptr(qd), B, N, C, heads, L.ptr(out), 0, G.stream()))
    torch.cuda.synchronize()
    assert not torch.isnan(out).any()
    return out


def _attn_run(entry, qd, gd, od, B, N, C, heads, scratch):
    lib = L.load()
    dq = _nan(B, N, 3 * C)
    if scratch is not None:
        scratch.fill_(0xff)
    if entry == 'atomics':
        L.check(lib.sr3_attention_bwd_f32(L.ptr(qd), L.ptr(gd), L.ptr(od), B, N, C, L.ptr(dq), G.stream()))
    elif entry == 'slabs':
        L.check(lib.sr3_attention_bwd_ex_f32(L.ptr(qd), L.ptr(gd), L.ptr(od), B, N, C, L.ptr(dq), L.ptr(scratch), scratch.numel(), G.stream()))
    else:
        L.check(lib.sr3_attention_bwd_heads_f32(L.ptr(qd), L.ptr(gd), L.ptr(od), B, N, C, heads, L.ptr(dq), L.ptr(scratch), scratch.numel(),
                                                G.stream()))
    torch.cuda.synchronize()
    return dq


@pytest.mark.parametrize('case', S.ATTN_CASES, ids=[S.attn_id(c) for c in S.ATTN_CASES])
def test_attention_backward_on_peaked_softmax(case):
    """dq / dk / dv on the suite's 'heavy' qkv -- log-normal magnitudes, most softmax rows one-hot, so that dS = P o (dP - rowsum(dP o P))
    cancels and the key-blocked kernel's running maximum moves between key blocks -- against float64 autograd, under the constants of
    test_gpu_attn_heads.py: normwise below 2e-5, max error at most 1e-4 max(1, |ref|max), no NaN over a NaN pre-fill.  One head runs the
    atomics entry, the slab entry and the heads entry; the slab entries must give the same bits twice over a 0xff-filled scratch.  The
    key-blocked shapes take rowsum(dP o P) from the forward output they are handed: once the one the library wrote, once the float64
    forward rounded once to fp32, and both must pass.  The data's conditions (at least half of the rows peaked above 0.9; torch's fp32
    CPU autograd within half of each gate) are asserted here and, without a device, in test_backward_stress_cpu.py."""
    B, N, C, heads = case
    lib, d = L.load(), G.dev()
    r = S.attn_reference(*case)
    assert r['peaked'] >= S.ATTN_PEAKED_SHARE, r['peaked']
    cmp_err = S.attn_errors(r['cmp32'], r['ref'], C, heads)
    for name, rel, mx in cmp_err:
        assert rel <= 0.5 * S.ATTN_REL and mx <= 0.5 * S.ATTN_MAX, (name, rel, mx)
    qd, gd = r['qkv'].to(d), r['dout'].to(d)
    blocked = S.attn_key_blocked(N)
    sources = [('library forward', _attn_forward(qd, B, N, C, heads))]
    if blocked:
        sources.append(('float64 forward', r['out32'].to(d)))
    nb = int(lib.sr3_attention_bwd_scratch_bytes(B, N, C))
    scratch = torch.empty(nb, dtype=torch.uint8, device=d)
    entries = ('atomics', 'slabs', 'heads') if heads == 1 else ('heads',)
    bad = []
    for what, od in sources:
        for entry in entries:
            got = _attn_run(entry, qd, gd, od, B, N, C, heads, None if entry == 'atomics' else scratch)
            assert not torch.isnan(got).any(), '%s, %s: an unwritten gradient element' % (entry, what)
            if entry != 'atomics':
                assert torch.equal(got, _attn_run(entry, qd, gd, od, B, N, C, heads, scratch)), '%s, %s: two runs differ' % (entry, what)
            for (name, rel, mx), (_, crel, cmx) in zip(S.attn_errors(got.cpu(), r['ref'], C, heads), cmp_err):
                print('attention backward %s peaked %.2f %s (%s) %s: kernel normwise %.2e max/scale %.2e; torch fp32 CPU autograd %.2e %.2e; '
                      'ratio %.2f %.2f' % (S.attn_id(case), r['peaked'], entry, what, name, rel, mx, crel, cmx, rel / crel, mx / cmx))
                if not (rel < S.ATTN_REL and mx <= S.ATTN_MAX):
                    bad.append((entry, what, name, rel, mx))
    assert not bad, '(entry, forward operand, gradient, normwise, max / scale) outside 2e-5 / 1e-4: %s' % bad


# ---- weight gradient on heavy-tailed operands ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', S.WGRAD_CASES, ids=[c[0] for c in S.WGRAD_CASES])
def test_conv_weight_gradient_stress_absolute_bound(case):
    """sr3_conv_wgrad_f32 under `split` 0 and 1 on the operands of test_winograd_conv_stress_absolute_bound -- log-normal magnitudes,
    sign flips between neighbouring pixels, a GroupNorm affine of size 30 / 300 in the kernel's prologue (activations in the thousands),
    an output gradient with loud channels -- against that test's ABSOLUTE criterion transposed to the pixel contraction: every element of
    dw within 4 gamma_K mag of float64, mag the float64 weight gradient of the same conv on |a| and |dy|, K = B Ho Wo,
    gamma_K = K u / (1 - K u), u = 2^-24.  Where both kernels run, the 3 x bf16 split kernel's normwise error stays within
    1.25 x the fp32 kernel's + 1e-8 (the relation of test_conv_weight_gradient_per_op).  Which kernel a case lands on: the comments
    of backward_stress.WGRAD_CASES."""
    name, B, C0, C1, H, W, Cout, k, stride, ups, act, amp = case
    lib, d = L.load(), G.dev()
    Cin = C0 + C1
    r = S.wgrad_reference(case)
    assert r['amax'] > S.WGRAD_AMAX, r['amax']                       # the case really is a stress case
    cmp_ratio = S.wgrad_ratio(r['cmp32'], r)
    assert cmp_ratio < S.WGRAD_CMP_RATIO, cmp_ratio                  # ... and plain fp32 arithmetic is far inside the bound
    g = lambda t: None if t is None else t.to(d)
    x = r['x']
    x0d, x1d = g(G.nhwc(x[:, :C0])), (g(G.nhwc(x[:, C0:])) if C1 else None)
    ssd, dyd = g(r['ss']), g(G.nhwc(r['dy']))
    rel, bad = {}, []
    for split in (0, 1):
        nb = int(lib.sr3_conv_wgrad_scratch_bytes(B, H, W, ups, stride, k, C0, C1, Cout, split))
        scratch = torch.empty(max(nb, 16), dtype=torch.uint8, device=d)
        dw = _nan(Cout, k * k, Cin)
        L.check(lib.sr3_conv_wgrad_f32(L.ptr(x0d), C0, L.ptr(x1d), C1, B, H, W, ups, stride, k, Cout, L.ptr(ssd), act, L.ptr(dyd), L.ptr(dw),
                                       split, L.ptr(scratch), nb, G.stream()))
        torch.cuda.synchronize()
        got = dw.cpu().view(Cout, k, k, Cin).permute(0, 3, 1, 2)
        assert torch.isfinite(got).all(), 'split %d: a non-finite or unwritten element' % split
        ratio, rel[split] = S.wgrad_ratio(got, r), S.wgrad_relerr(got, r)
        print('wgrad stress %s split %d (%s kernel): K %d, |a|max %.3g, |ref|max %.3g, max err / (4 gamma_K mag) %.3g, normwise %.2e; '
              'torch fp32 CPU autograd %.3g, %.2e; ratio %.2f'
              % (name, split, '3 x bf16 split' if S.wgrad_runs_split(case, split) else 'fp32', r['K'], r['amax'], r['ref'].abs().max().item(),
                 ratio, rel[split], cmp_ratio, S.wgrad_relerr(r['cmp32'], r), ratio / cmp_ratio))
        if not ratio <= 1.0:
            bad.append((split, ratio))
    assert not bad, '(split, max err / bound) above 1: %s' % bad
    if S.wgrad_runs_split(case, 1):
        assert rel[1] != rel[0]                                      # (the split kernel really ran)
        assert rel[1] <= 1.25 * rel[0] + 1e-8, rel


# ---- GroupNorm(+SiLU) backward on offset and near-constant groups -------------------------------------------------------------------

@pytest.mark.parametrize('case', S.GN_CASES, ids=[S.gn_id(c) for c in S.GN_CASES])
def test_groupnorm_act_backward_on_offset_groups(case):
    """sr3_groupnorm_act_bwd_f32 where its terms cancel: every channel rides on a DC offset (|mean| / std above 2 for most groups) and the
    first group is nearly constant (|mean| / std ~ 600, variance 2.5e-5 next to eps, rstd ~ 170), under a heavy-tailed dA.  The fp32
    tables ss / mr are operands of the entry (float64 rounded once: _gn_tables), so the truth is the float64 evaluation FROM those tables
    (backward_stress.gn_truth_from_tables) -- their rounding is the fold's.  The gate is test_groupnorm_act_backward's: per quantity the
    kernel's normwise error is at most twice that of torch's fp32 CPU autograd against plain float64; so are its two-run and flag
    identities."""
    B, C0, C1, H, W, groups, act = case
    lib, d = L.load(), G.dev()
    Cc, HW = C0 + C1, H * W
    r = S.gn_reference(case)
    off = r['offset']
    assert off.max().item() > 100.0 and (off > 2.0).double().mean().item() >= 0.5
    x, dA = r['x'], r['dA']
    x0d = G.nhwc(x[:, :C0]).to(d)
    x1d = G.nhwc(x[:, C0:]).to(d) if C1 else None
    gd, bd, ss, mr = r['gamma'].to(d), r['beta'].to(d), r['ss'].to(d), r['mr'].to(d)
    nb = int(lib.sr3_groupnorm_act_bwd_scratch_bytes(B, HW, Cc, groups))
    assert nb > 0
    old0, old1 = T._rand(B, H, W, C0, seed=15).to(d), (T._rand(B, H, W, C1, seed=16).to(d) if C1 else None)

    def run(acc0, acc1):
        dAd = G.nhwc(dA).to(d)
        out = dict(dgamma=_nan(Cc), dbeta=_nan(Cc), aout=_nan(B, H, W, Cc), dx0=old0.clone() if acc0 else _nan(B, H, W, C0),
                   dx1=None if not C1 else (old1.clone() if acc1 else _nan(B, H, W, C1)))
        scratch = T._bytes(nb)
        L.check(lib.sr3_groupnorm_act_bwd_f32(L.ptr(dAd), L.ptr(x0d), C0, L.ptr(x1d), C1, B, HW, L.ptr(ss), L.ptr(mr), groups, act, L.ptr(gd),
                                              0, 0.0, L.ptr(out['dgamma']), L.ptr(out['dbeta']), L.ptr(out['dx0']), acc0, L.ptr(out['dx1']),
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
    dx = G.nchw(plain0 if not C1 else torch.cat([plain0, plain1], 3)).cpu()
    got = dict(dx=dx, dgamma=first['dgamma'].cpu(), dbeta=first['dbeta'].cpu(), aout=G.nchw(first['aout']).cpu(), du=G.nchw(first['du']).cpu())
    bad = []
    for k in S.GN_QUANTITIES:
        assert not torch.isnan(got[k]).any(), k
        e_k, e_c = T._relerr(got[k], r['truth'][k]), r['cmp_err'][k]
        print('groupnorm backward stress %s |mean|/std max %.0f %s: kernel %.3e (normwise vs float64 from the fp32 tables), torch fp32 CPU '
              'autograd %.3e (vs float64); ratio %.2f' % (S.gn_id(case), off.max().item(), k, e_k, e_c, e_k / e_c if e_c else 0.0))
        if not e_k <= 2.0 * e_c:
            bad.append((k, e_k, e_c))
    assert not bad, 'normwise error above twice the fp32 comparator\'s (quantity, kernel, comparator): %s' % bad

    # Not gated: how far the library's own tables (the statistics pass and the fold the step runs) put x scale + shift from float64
    # F.group_norm on this data.  test_groupnorm_stats_and_fold's 5e-6 was never claimed under offsets; DESIGN.md records the figure.
    lss, lmr = T._gn_library_tables(lib, x0d, x1d, B, HW, C0, C1, groups, gd, bd)
    lss = lss.cpu().double()
    u_lib = x.double() * lss[:, :, 0, None, None] + lss[:, :, 1, None, None]
    u_ref = F.group_norm(x.double(), groups, r['gamma'].double(), r['beta'].double(), eps=T.GN_EPS)
    u_tab = x.double() * r['ss'].double()[:, :, 0, None, None] + r['ss'].double()[:, :, 1, None, None]
    cpg = Cc // groups
    for what, sl in (('the near-constant group', slice(0, cpg)), ('the other groups', slice(cpg, Cc))):
        print('groupnorm fold under offsets %s, %s: max |x scale + shift - F.group_norm| library tables %.3e, float64 tables rounded once %.3e '
              '(|u|max %.2f)' % (S.gn_id(case), what, (u_lib - u_ref)[:, sl].abs().max().item(), (u_tab - u_ref)[:, sl].abs().max().item(),
                                 u_ref[:, sl].abs().max().item()))
