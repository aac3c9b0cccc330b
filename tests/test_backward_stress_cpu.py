"""The conditions on the data of tests/test_gpu_backward_stress.py, asserted from the float64 references alone (tests/backward_stress.py;
no device): the data is as hostile as the GPU test's docstrings say -- peaked softmax rows, activations in the thousands, groups with a
DC offset or next to no variance -- and torch's own fp32 CPU autograd of the same function on the same data stays well inside every
gate, so a kernel that misses one is worse than plain fp32 arithmetic, not unlucky."""
import pytest
import torch

import backward_stress as S


@pytest.mark.parametrize('case', S.ATTN_CASES, ids=[S.attn_id(c) for c in S.ATTN_CASES])
def test_attention_data_is_peaked_and_fp32_autograd_is_inside_half_the_gate(case):
    B, N, C, heads = case
    r = S.attn_reference(*case)
    assert torch.isfinite(r['ref']).all() and torch.isfinite(r['cmp32']).all()
    print('attention backward %s: peaked rows %.2f' % (S.attn_id(case), r['peaked']))
    assert r['peaked'] >= S.ATTN_PEAKED_SHARE, r['peaked']
    for name, rel, mx in S.attn_errors(r['cmp32'], r['ref'], C, heads):
        print('attention backward %s %s: torch fp32 CPU autograd normwise %.2e, max / scale %.2e' % (S.attn_id(case), name, rel, mx))
        assert rel <= 0.5 * S.ATTN_REL, (name, rel)
        assert mx <= 0.5 * S.ATTN_MAX, (name, mx)
    # the float64 forward rounded once is a legitimate `out_fwd` operand: within an fp32 ulp of the float64 output
    assert (r['out32'].double() - r['out64']).abs().max().item() <= 2.0 ** -24 * r['out64'].abs().max().item()


def test_attention_cases_reach_the_three_instantiations():
    """the host rule of attention_backward restated: Npad <= 448 two stages, <= 480 one, key-blocked beyond"""
    kinds = {}
    for B, N, C, heads in S.ATTN_CASES:
        Npad = (N + 31) & ~31
        kinds.setdefault(('blocked' if S.attn_key_blocked(N) else 'one stage' if Npad > 448 else 'two stages', heads > 1), []).append(N)
    assert set(kinds) == {(k, mh) for k in ('two stages', 'one stage', 'blocked') for mh in (False, True)}, kinds
    assert not S.attn_key_blocked(480) and S.attn_key_blocked(481)


@pytest.mark.parametrize('case', S.WGRAD_CASES, ids=[c[0] for c in S.WGRAD_CASES])
def test_wgrad_data_is_heavy_and_fp32_autograd_is_inside_a_quarter_of_the_bound(case):
    r = S.wgrad_reference(case)
    ratio = S.wgrad_ratio(r['cmp32'], r)
    print('wgrad %s: K %d, |a|max %.3g, |ref|max %.3g, torch fp32 CPU autograd max err / bound %.3g, normwise %.2e'
          % (case[0], r['K'], r['amax'], r['ref'].abs().max().item(), ratio, S.wgrad_relerr(r['cmp32'], r)))
    assert torch.isfinite(r['ref']).all() and torch.isfinite(r['cmp32']).all()
    assert r['amax'] > S.WGRAD_AMAX, r['amax']
    assert ratio < S.WGRAD_CMP_RATIO, ratio
    assert bool((r['bound'] > 0).all())


def test_wgrad_cases_cover_the_kernels():
    """wgrad_pick's split condition restated: the split kernel runs on four of the cases under `split` = 1 and on none under `split` = 0"""
    assert [c[0] for c in S.WGRAD_CASES if S.wgrad_runs_split(c, 1)] == ['w3_128to128_silu', 'w3_ragged_M100_136to200_affine', 'w3_s2_128to128_raw',
                                                                         'w3_up_128to128_raw']
    assert not any(S.wgrad_runs_split(c, 0) for c in S.WGRAD_CASES)


@pytest.mark.parametrize('case', S.GN_CASES, ids=[S.gn_id(c) for c in S.GN_CASES])
def test_groupnorm_data_has_offset_and_near_constant_groups(case):
    B, C0, C1, H, W, groups, act = case
    r = S.gn_reference(case)
    off = r['offset']
    print('groupnorm backward %s: |mean| / std max %.3g, median %.3g; rstd max %.4g; comparator %s'
          % (S.gn_id(case), off.max().item(), off.median().item(), r['mr'][:, :, 1].max().item(),
             ', '.join('%s %.2e' % (k, r['cmp_err'][k]) for k in S.GN_QUANTITIES)))
    assert off.max().item() > 100.0
    assert (off > 2.0).double().mean().item() >= 0.5
    var0 = r['x'].double().reshape(B, groups, -1).var(2, unbiased=False)[:, 0]
    assert bool((var0 > 1e-5).all()) and bool((var0 < 1e-4).all()), var0             # the order of eps = 1e-5
    assert all(r['cmp_err'][k] < 1e-3 for k in S.GN_QUANTITIES), r['cmp_err']        # the comparator is a usable yardstick (du under act 1: exact)


@pytest.mark.parametrize('case', S.GN_CASES, ids=[S.gn_id(c) for c in S.GN_CASES])
def test_groupnorm_truth_from_tables_is_the_autograd_function(case):
    """gn_truth_from_tables on float64 tables is float64 autograd of F.group_norm -> act to rounding: the formula the GPU test holds the
    kernel to is the operation, and the only thing the fp32 tables add is their own rounding."""
    B, C0, C1, H, W, groups, act = case
    r = S.gn_reference(case)
    x, gamma, beta = r['x'], r['gamma'], r['beta']
    Cc, cpg = C0 + C1, (C0 + C1) // groups
    xg = x.double().reshape(B, groups, -1)
    mean, rstd = xg.mean(2), 1.0 / torch.sqrt(xg.var(2, unbiased=False) + 1e-5)
    scale = rstd.repeat_interleave(cpg, 1) * gamma.double()[None]
    shift = beta.double()[None] - mean.repeat_interleave(cpg, 1) * scale
    exact = S.gn_truth_from_tables(x, gamma, r['dA'], torch.stack([scale, shift], 2), torch.stack([mean, rstd], 2), groups, act)
    for k in S.GN_QUANTITIES:
        e = ((exact[k] - r['ref64'][k]).norm() / r['ref64'][k].norm()).item()
        assert e <= 1e-9, (k, e)          # (float64 with cancellation of ~1e3 in u: far below any fp32 figure)
        # and the fp32 tables move the truth by the tables' rounding only: rstd ~ 170 on a mean of 3 -> ~1e-4 at the worst
        t = ((r['truth'][k] - r['ref64'][k]).norm() / r['ref64'][k].norm()).item()
        print('groupnorm backward %s %s: truth from fp32 tables vs float64 autograd %.2e' % (S.gn_id(case), k, t))
        assert t <= 1e-3, (k, t)
