"""Hostile data for the backward per-op tests, with the float64 references and the conditions that make the data hostile.  Plain torch on
the CPU: tests/test_backward_stress_cpu.py asserts the conditions from the references alone, tests/test_gpu_backward_stress.py runs the
kernels on exactly these inputs.

  * attention backward: the suite's 'heavy' qkv (log-normal magnitudes: logits in the hundreds, one-hot softmax rows), where
    dS = P o (dP - rowsum(dP o P)) cancels and the key-blocked kernel's running max moves from block to block;
  * weight gradient: the operands of test_winograd_conv_stress_absolute_bound (heavy tails, loud channels, neighbouring sign flips) on
    both sides of the pixel contraction, under the same absolute float64 bound;
  * GroupNorm(+SiLU) backward: per-channel DC offsets and one nearly constant group (variance of the order of eps), evaluated from the
    fp32 (scale, shift) / (mean, rstd) tables the entry is handed.

Every reference is computed once per case and shared (functools.lru_cache): callers must leave the tensors unchanged."""
import functools
import math

import torch
import torch.nn.functional as F

import mha_ref

U = 2.0 ** -24          # fp32 unit roundoff


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- attention backward on peaked softmax -------------------------------------------------------------------------------------------

# The smallest shapes that reach each instantiation of k_attention_bwd through the host rule of attention_backward (Npad = N rounded up
# to 32): two staging buffers while Npad <= 448, one up to Npad = 480, key blocks of KB = 384 beyond.
ATTN_CASES = [
    # B, N, C, heads
    (2, 100, 48, 1),        # <2, false>: ragged N, C % 32 != 0
    (1, 470, 64, 1),        # <1, false>: single stage, ragged
    (1, 481, 32, 1),        # <2, true>: the first key-blocked N; the last block holds 97 keys, one past a 32-key group
    (2, 100, 96, 2),        # multi-head strip
    (1, 481, 64, 2),        # multi-head, key-blocked
    (1, 470, 128, 4),       # multi-head, one stage
]
ATTN_REL, ATTN_MAX = 2e-5, 1e-4          # the gates of test_gpu_attn_heads.py: normwise, and max error over max(1, |ref|max)
ATTN_PEAK, ATTN_PEAKED_SHARE = 0.9, 0.5  # a row is peaked above 0.9; at least half of all (image, head, row) rows must be


def attn_id(case):
    return 'b%d_n%d_c%d_h%d' % case


def attn_key_blocked(N):
    return ((N + 31) & ~31) > 480


def attn_inputs(B, N, C):
    """(qkv [B][N][3C] of the 'heavy' kind of test_gpu_attn_heads.py / test_attention_split_error_not_above_fp32_mfma, dout [B][N][C])"""
    q = _rand(B, N, 3 * C, seed=11)
    return q.sign() * torch.exp(1.5 * q.abs()) * 0.3, _rand(B, N, C, seed=12)


def _attn_core(x, C, heads):
    if heads > 1:
        return mha_ref.core(x, C, heads)
    q, k, v = x.split(C, dim=2)         # (the formula of test_attention_backward)
    return torch.softmax(q @ k.transpose(1, 2) / math.sqrt(C), -1) @ v


def _attn_autograd(dtype, qkv, dout, C, heads):
    x = qkv.to(dtype).requires_grad_(True)
    o = _attn_core(x, C, heads)
    o.backward(dout.to(dtype))
    return x.grad, o.detach()


@functools.lru_cache(maxsize=None)
def attn_reference(B, N, C, heads):
    """dict: qkv, dout (fp32 inputs); ref (float64 dqkv), out64 (float64 forward), out32 (that rounded once to fp32), cmp32 (torch's
    fp32 CPU autograd of the same function), peaked (share of softmax rows whose maximum exceeds ATTN_PEAK)"""
    qkv, dout = attn_inputs(B, N, C)
    ref, out64 = _attn_autograd(torch.float64, qkv, dout, C, heads)
    cmp32, _ = _attn_autograd(torch.float32, qkv, dout, C, heads)
    d = C // heads
    q, k, _ = qkv.double().view(B, N, heads, 3 * d).chunk(3, dim=3)
    p = torch.softmax(torch.einsum('bmhc,bnhc->bhmn', q, k) / math.sqrt(C), -1)
    peaked = (p.max(-1).values > ATTN_PEAK).double().mean().item()
    return dict(qkv=qkv, dout=dout, ref=ref, out64=out64, out32=out64.float(), cmp32=cmp32, peaked=peaked)


def attn_parts(t, C, heads):
    """dqkv [B][N][3C] -> (dq, dk, dv), each [B][N][heads][d]: q | k | v of every head"""
    B, N, _ = t.shape
    d = C // heads
    v = t.view(B, N, heads, 3 * d)
    return [v[..., i * d:(i + 1) * d] for i in range(3)]


def attn_errors(got, ref, C, heads):
    """[(name, normwise error, max error / max(1, |ref|max))] for dq, dk, dv against the float64 gradient"""
    out = []
    for name, g_, r in zip(('dq', 'dk', 'dv'), attn_parts(got.double(), C, heads), attn_parts(ref, C, heads)):
        out.append((name, ((g_ - r).norm() / r.norm()).item(), (g_ - r).abs().max().item() / max(1.0, r.abs().max().item())))
    return out


# ---- weight gradient on heavy-tailed operands ---------------------------------------------------------------------------------------

# The kernel each case lands on, by wgrad_pick of csrc/wgrad.hip: the split kernel where split is asked for and Cout > 64 and Cin > 64;
# else the 9-tap kernel (3 x 3, stride 1, no upsample, one source, NO fused activation, a map 8 | W wide); else k_conv_wgrad<TN, TC>, the
# generic one-tap-per-workgroup fp32-MFMA kernel (128 x 128 where both channel counts exceed 64, else 64 x 64).  k_conv_wgrad_split<ACT>
# is the 3 x bf16 one (128 x 128, with or without the fused prologue).
WGRAD_CASES = [
    # name, B, C0, C1, H, W, Cout, k, stride, ups, act, amp of the (scale, shift) pairs
    # the fused activation keeps it off the 9-tap kernel: k_conv_wgrad<64, 64> under either `split`
    ('w3_64to64_silu', 2, 64, 0, 16, 16, 64, 3, 1, 0, 2, 30.0),
    # split 0: k_conv_wgrad<128, 128>; split 1: k_conv_wgrad_split<true>
    ('w3_128to128_silu', 2, 128, 0, 16, 16, 128, 3, 1, 0, 2, 30.0),
    # 100 pixels (ragged last 32-pixel chunk), 136 and 200 channels (ragged tiles): k_conv_wgrad<128, 128> / k_conv_wgrad_split
    ('w3_ragged_M100_136to200_affine', 1, 136, 0, 10, 10, 200, 3, 1, 0, 1, 300.0),
    # Cout = 64: k_conv_wgrad<64, 64> under either `split`; the concat seam at channel 96 and the in-kernel affine prologue
    ('w1_concat96+32to64_affine', 2, 96, 32, 16, 16, 64, 1, 1, 0, 1, 300.0),
    # stride 2 on the raw features: k_conv_wgrad<128, 128> / k_conv_wgrad_split<false>
    ('w3_s2_128to128_raw', 2, 128, 0, 16, 16, 128, 3, 2, 0, 0, None),
    # the x2-upsampled address: k_conv_wgrad<128, 128> / k_conv_wgrad_split<false>
    ('w3_up_128to128_raw', 2, 128, 0, 8, 8, 128, 3, 1, 1, 0, None),
    # no activation, one source, stride 1, 32 | W: the one shape here the 9-tap rule accepts -- k_conv_wgrad9 under either `split`
    ('w3_64to64_raw_9tap', 2, 64, 0, 32, 32, 64, 3, 1, 0, 0, None),
]
# The log-normal magnitudes are exp(1.5 N(0, 1)) as in the forward stress tests, except on the upsample case: its 16 384 raw samples, with
# no GroupNorm affine to amplify them, peak near 300 at 1.5 -- below the stress condition -- so its tail is drawn heavier.
WGRAD_SIGMA = {'w3_up_128to128_raw': 2.0}
WGRAD_AMAX = 500.0          # the case is a stress case: |a|max above this
WGRAD_CMP_RATIO = 0.25      # torch's fp32 autograd on the same data must stay below this share of the bound


def wgrad_runs_split(case, split):
    """where wgrad_pick (csrc/wgrad.hip) takes the split kernel"""
    _, B, C0, C1, H, W, Cout, k, stride, ups, act, amp = case
    return bool(split) and Cout > 64 and C0 + C1 > 64


def wgrad_out_hw(case):
    _, B, C0, C1, H, W, Cout, k, stride, ups, act, amp = case
    pad = k // 2
    return ((H << ups) + 2 * pad - k) // stride + 1, ((W << ups) + 2 * pad - k) // stride + 1


def _checker(H, W):
    return ((torch.arange(H)[:, None] + torch.arange(W)[None, :]) % 2 * 2 - 1).float()


def wgrad_inputs(case):
    """(x NCHW over the concat, ss [B][Cin][2] or None, dy NCHW): the recipe of test_winograd_conv_stress_absolute_bound, generator seed
    99 -- log-normal magnitudes, every 7th channel |x| times a pixel checkerboard, (scale, shift) of size amp -- and an output gradient
    with every 5th channel 30 x louder and channels 1, 10, 19, ... |dy| times the checkerboard"""
    _, B, C0, C1, H, W, Cout, k, stride, ups, act, amp = case
    Cin = C0 + C1
    Ho, Wo = wgrad_out_hw(case)
    g = torch.Generator().manual_seed(99)
    x = torch.randn(B, Cin, H, W, generator=g)
    x = x * torch.exp(WGRAD_SIGMA.get(case[0], 1.5) * torch.randn(B, Cin, H, W, generator=g))
    x[:, ::7] = x[:, ::7].abs() * _checker(H, W)
    ss = None
    if act:
        ss = torch.stack([torch.randn(B, Cin, generator=g) * amp, torch.randn(B, Cin, generator=g) * amp], dim=2).contiguous()
    dy = torch.randn(B, Cout, Ho, Wo, generator=g)
    dy[:, ::5] *= 30.0
    dy[:, 1::9] = dy[:, 1::9].abs() * _checker(Ho, Wo)
    return x, ss, dy


def _wgrad_activated(x, ss, act, ups):
    a = x
    if act:
        a = a * ss[:, :, 0].to(x.dtype)[:, :, None, None] + ss[:, :, 1].to(x.dtype)[:, :, None, None]
        if act == 2:
            a = a * torch.sigmoid(a)
    if ups:
        a = F.interpolate(a, scale_factor=2, mode='nearest')
    return a


def _wgrad_of(a, dy, Cout, k, stride):
    w = torch.zeros(Cout, a.shape[1], k, k, dtype=a.dtype, requires_grad=True)
    F.conv2d(a, w, None, stride=stride, padding=k // 2).backward(dy)
    return w.grad


@functools.lru_cache(maxsize=None)
def wgrad_reference(case):
    """dict: x, ss, dy (fp32 inputs); ref (float64 dw OIHW), bound (4 gamma_K mag, elementwise: mag the float64 weight gradient of the
    same conv on |a| and |dy|, K = B Ho Wo the length of the pixel contraction, gamma_K = K u / (1 - K u)), amax (|a|max), cmp32
    (torch's fp32 CPU autograd on the same data)"""
    _, B, C0, C1, H, W, Cout, k, stride, ups, act, amp = case
    x, ss, dy = wgrad_inputs(case)
    a = _wgrad_activated(x.double(), ss, act, ups)
    ref = _wgrad_of(a, dy.double(), Cout, k, stride)
    mag = _wgrad_of(a.abs(), dy.double().abs(), Cout, k, stride)
    Ho, Wo = wgrad_out_hw(case)
    K = B * Ho * Wo
    gamma = K * U / (1 - K * U)
    cmp32 = _wgrad_of(_wgrad_activated(x, ss, act, ups), dy, Cout, k, stride)
    return dict(x=x, ss=ss, dy=dy, ref=ref, bound=4 * gamma * mag, amax=a.abs().max().item(), cmp32=cmp32, K=K)


def wgrad_ratio(got, r):
    """max over the elements of |got - ref| / bound"""
    return ((got.double() - r['ref']).abs() / (r['bound'] + 1e-300)).max().item()


def wgrad_relerr(got, r):
    return ((got.double() - r['ref']).norm() / r['ref'].norm()).item()


# ---- GroupNorm(+SiLU) backward on offset and near-constant groups -------------------------------------------------------------------

GN_CASES = [
    # B, C0, C1, H, W, groups, act
    (2, 8, 16, 5, 7, 4, 2),             # cpg 6: a group straddles the two sources; odd pixel count
    (1, 320, 0, 8, 8, 32, 2),           # two channel blocks of the reduce, the second ragged
    (2, 64, 0, 32, 32, 32, 1),          # several pixel slices per image
]
GN_QUANTITIES = ('dx', 'dgamma', 'dbeta', 'aout', 'du')


def gn_id(case):
    return 'B%d_%d+%d_%dx%d_g%d_act%d' % case


def _gn_ops():
    import test_gpu_backward_ops as T          # the harness of test_groupnorm_act_backward (plain torch at import: no device needed)
    return T


def gn_inputs(case):
    """x: N(0, 0.2^2) around per-channel DC offsets N(6, 2^2); the first group N(3, (5e-3)^2) -- a variance of 2.5e-5 next to
    eps = 1e-5, rstd about 170.  dA: log-normal magnitudes times N(0, 1).  gamma, beta as in test_groupnorm_act_backward."""
    B, C0, C1, H, W, groups, act = case
    Cc = C0 + C1
    cpg = Cc // groups
    x = _rand(B, Cc, H, W, seed=11) * 0.2 + (_rand(1, Cc, 1, 1, seed=15) * 2.0 + 6.0)
    x[:, :cpg] = _rand(B, cpg, H, W, seed=16) * 5e-3 + 3.0
    gamma, beta = _rand(Cc, seed=12) * 0.3 + 1.0, _rand(Cc, seed=13) * 0.3
    dA = _rand(B, Cc, H, W, seed=14) * torch.exp(1.5 * _rand(B, Cc, H, W, seed=17))
    return x, gamma, beta, dA


def gn_truth_from_tables(x, gamma, dA, ss, mr, groups, act):
    """The float64 evaluation of what the entry computes FROM ITS fp32 TABLES ss [B][C][2] (scale, shift) and mr [B][G][2] (mean, rstd):
    u = x scale + shift, a = act(u), du = dA act'(u), xhat = (x - mean) rstd, dbeta = sum du, dgamma = sum du xhat and
    dx = rstd (gamma du - (S1 + xhat S2) / n) with S1 = sum gamma du, S2 = sum gamma du xhat over an (image, group).  The tables'
    own rounding (the fold's) is an operand here, not an error."""
    B, Cc, H, W = x.shape
    cpg = Cc // groups
    xd, ssd, mrd, gm = x.double(), ss.double(), mr.double(), gamma.double()
    u = xd * ssd[:, :, 0, None, None] + ssd[:, :, 1, None, None]
    du, a = dA.double(), u
    if act == 2:
        sg = torch.sigmoid(u)
        du, a = du * sg * (1.0 + u * (1.0 - sg)), u * sg
    mean = mrd[:, :, 0].repeat_interleave(cpg, 1)[:, :, None, None]
    rstd = mrd[:, :, 1].repeat_interleave(cpg, 1)[:, :, None, None]
    xh = (xd - mean) * rstd
    gdu = gm[None, :, None, None] * du
    S1 = gdu.reshape(B, groups, -1).sum(2).repeat_interleave(cpg, 1)[:, :, None, None]
    S2 = (gdu * xh).reshape(B, groups, -1).sum(2).repeat_interleave(cpg, 1)[:, :, None, None]
    dx = rstd * (gdu - (S1 + xh * S2) / (cpg * H * W))
    return dict(dx=dx, dgamma=(du * xh).sum((0, 2, 3)), dbeta=du.sum((0, 2, 3)), aout=a, du=du)


@functools.lru_cache(maxsize=None)
def gn_reference(case):
    """dict: x, gamma, beta, dA (fp32 inputs); ss, mr (the float64 tables rounded once to fp32: _gn_tables of the existing test); truth
    (gn_truth_from_tables of them); ref64 / cmp32 (float64 / fp32 CPU autograd of F.group_norm -> act, contracted with dA); cmp_err
    (per quantity the comparator's normwise error against ref64: half the gate); offset (|mean| / std per (image, group))"""
    B, C0, C1, H, W, groups, act = case
    T = _gn_ops()
    x, gamma, beta, dA = gn_inputs(case)
    ss, mr = T._gn_tables(x, gamma, beta, groups)
    ref64 = T._gn_autograd(torch.float64, x, gamma, beta, groups, act, None, dA)
    cmp32 = T._gn_autograd(torch.float32, x, gamma, beta, groups, act, None, dA)
    cmp_err = {k: T._relerr(cmp32[k], ref64[k]) for k in GN_QUANTITIES}
    xg = x.double().reshape(B, groups, -1)
    offset = xg.mean(2).abs() / xg.std(2, unbiased=False)
    return dict(x=x, gamma=gamma, beta=beta, dA=dA, ss=ss, mr=mr, truth=gn_truth_from_tables(x, gamma, dA, ss, mr, groups, act),
                ref64=ref64, cmp32=cmp32, cmp_err=cmp_err, offset=offset)
