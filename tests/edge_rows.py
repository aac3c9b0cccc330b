"""The per-op operand contract table: one row per (entry, kernel, edge shape) -- the smallest shapes at which each kernel has a ragged
edge: a pixel count, a channel tail or an output width that is no multiple of the tile, a concat seam inside a chunk, an absent image, an
overhanging tile (a plain helper module, shared by tests/test_gpu_edge_operands.py -- every operand between bands under two fills on the
GPU -- and tests/test_edge_rows_cpu.py -- the rows' refusal rules, scratch sizes and checks, without a device).

The contract: an entry reads and writes its operands at their exact extents.  Nothing from outside an operand may reach a result, and
nothing may be written outside one.

Rows have the format of tests/scratch_rows.py (`Row`, lazily built `spec()` with ins / outs / query / call / check / expect), and on top
  exact    () -> {name: CPU tensor}        every output's float64 reference rounded once to the output's type: `check` must pass on it
  tol      {name: float | None}            per compared output, the tolerance of `check` as the displacement of one element it still
                                           accepts (None: the comparison is bit-exact); ten times that must fail
  refusal  lib -> message | None           conv rows: the restated refusal rule of the row's tile (gpu_util); every row's must be None
  same     {name: (a, b) -> bool}          only where atomics accumulate an output: what must be equal between two runs in its place
A row's `query` may return 0 (the entry has no scratch, or this launch needs none).

`check` is the float64 comparison of the op's own test at that test's tolerance; each builder names the test.

What the table does not see: an out-of-range load whose value is discarded by a select before any arithmetic (several kernels load
unconditionally and mask afterwards; their out-of-range lanes read element 0 of the same buffer, so such a load is in range by
construction, and one that is not leaves no trace in a result).  The bands keep it inside memory the test owns.

Entries without a row, because their own tests already run their edge shapes with bands in front of and behind every operand:
  sr3_conv_out_f32                     tests/test_gpu_conv_out_lines.py
  the key-blocked attention (modes 2, 3; tile 24)   tests/test_gpu_attn_long.py
  every entry that takes a scratch, at whole shapes   tests/scratch_rows.py through tests/test_gpu_scratch_contract.py
sr3_adam_ema_step has a row: tests/test_gpu_optim.py and tests/test_gpu_ema.py band none of its operands.  Its length is 1004, not a
length that is no multiple of 4: the entry takes whole 16-byte vectors only and refuses any other n.  So does sr3_q_sample per image:
its ragged row has 108 elements per image (27 vectors, a fraction of a block), where sr3_p_sample_step_ex runs 105 with a scalar tail."""
import ctypes as C
import math

import torch
import torch.nn.functional as F

import gpu_util as G
from gpu_util import nchw, nhwc, ohwi
from scratch_rows import Row, rand, relerr

CLOSE = 2e-5          # gpu_util.assert_close's default: |got - ref| <= 2e-5 * max(1, |ref|_inf)


def cached(fn):
    box = []

    def get():
        if not box:
            box.append(fn())
        return box[0]
    return get


def close_tol(ref, tol=CLOSE):
    return tol * max(1.0, float(ref.abs().max()))


def stats_of(out_nhwc, T):
    """[B][T][Cout][2] partials whose sums are the statistics of this output (all in slice 0)."""
    o = out_nhwc.double()
    st = torch.zeros(o.shape[0], T, o.shape[3], 2, dtype=torch.float64)
    st[:, 0, :, 0], st[:, 0, :, 1] = o.sum(dim=(1, 2)), (o * o).sum(dim=(1, 2))
    return st


def check_stats(got):
    """tests/test_gpu_ops.py::test_conv_fused_output_stats: the partials sum to the statistics of the output as written"""
    st, o = got['stats'].sum(1), got['out'].double()
    assert torch.allclose(st[:, :, 0], o.sum(dim=(1, 2)), rtol=1e-9, atol=1e-9)
    assert torch.allclose(st[:, :, 1], (o * o).sum(dim=(1, 2)), rtol=1e-9, atol=1e-9)


def stats_tol(out_nhwc):
    o = out_nhwc.double()
    return 1e-9 * (1.0 + float((o * o).sum(dim=(1, 2)).max()))


def conv_spec(ins, outs, call, query, ref_nhwc, T, what, refusal, expect=None):
    """The common tail of the conv rows: `out` against the float64 reference under gpu_util.assert_close (tests/test_gpu_ops.py::test_conv
    and its neighbours), the fused statistics against the output."""
    def check(got):
        G.assert_close(got['out'], ref_nhwc(), what=what)
        if T > 0:
            check_stats(got)

    def exact():
        e = {'out': ref_nhwc().float()}
        if T > 0:
            e['stats'] = stats_of(e['out'], T)
        return e
    tol = {'out': close_tol(ref_nhwc())}
    if T > 0:
        tol['stats'] = stats_tol(ref_nhwc().float())
    return dict(ins=ins, outs=outs, call=call, check=check, query=query, exact=exact, tol=tol, refusal=refusal, expect=expect)


# ---- sr3_conv_f32 (tests/test_gpu_ops.py::test_conv, ::test_conv_fused_output_stats; the Winograd tiles: ::test_winograd_conv_error_is_fp32_class
# and ::test_winograd_split_error_not_above_fp32_winograd, the GEMM tile: tests/test_gpu_gemm_epilogue.py -- all under assert_close) --------------

def conv_refusal(tile, ks, B, Hs, Ws, C0, C1, Cout, k, stride, ups):
    Cin = C0 + C1

    def rule(lib):
        if tile in (5, 6, 9):
            return G.halo_expected_refusal(B, Cin, Hs, Ws, ups, tile, ks, k, stride)
        if tile in (11, 12, 13, 25):
            return G.wino_expected_refusal(B, Cin, Hs, Ws, ups, 13 if tile == 25 else tile, ks, k, stride)
        if tile == 23:          # the ragged Winograd tile: any map; the split rule of the other Winograd tiles
            return G.wino_expected_refusal(B, Cin, 16, 16, 0, 13, ks, k, stride)
        if tile == 22:          # the plain GEMM: the library's own host query
            pad = k // 2
            Ho, Wo = ((Hs << ups) + 2 * pad - k) // stride + 1, ((Ws << ups) + 2 * pad - k) // stride + 1
            return None if lib.sr3_gemm_tile(B, Ho, Wo, Cin, Cout, k, None, None) == 1 else 'does not fit'
        assert tile in (1, 2, 3, 4, 14, 15, 16, 17), tile          # the im2col tiles take every shape
        return None
    return rule


def conv_edge(tile, ks, B, Hs, Ws, C0, C1, Cout, k=3, stride=1, ups=0, act=2, film=True, res='plain', RC0=0, tag=''):
    Cin = C0 + C1

    def build():
        from sr3_hip import lib as L
        lib = L.load()
        pad = k // 2
        Ho, Wo = ((Hs << ups) + 2 * pad - k) // stride + 1, ((Ws << ups) + 2 * pad - k) // stride + 1
        x0, x1 = rand(B, C0, Hs, Ws, seed=1), (rand(B, C1, Hs, Ws, seed=2) if C1 else None)
        w = rand(Cout, Cin, k, k, seed=3, scale=1.0 / math.sqrt(Cin * k * k))
        kw = dict(ups=ups, stride=stride, act=act, bias=rand(Cout, seed=4))
        ins = {'src0': nhwc(x0), 'w': ohwi(w), 'bias': kw['bias']}
        if C1:
            ins['src1'] = nhwc(x1)
        if act:
            kw['ss'] = torch.stack([rand(B, Cin, seed=5) * 0.3 + 1.0, rand(B, Cin, seed=6) * 0.3], dim=2).contiguous()
            ins['ss'] = kw['ss']
        if film:
            kw['film'] = ins['film'] = rand(B, Cout, seed=7)
        rc0 = rc1 = 0
        if res == 'plain':
            kw['res0'], rc0 = rand(B, Cout, Ho, Wo, seed=8), Cout
            ins['res0'] = nhwc(kw['res0'])
        elif res == 'concat':
            rc0, rc1 = RC0, Cout - RC0
            kw['res0'], kw['res1'] = rand(B, rc0, Ho, Wo, seed=8), rand(B, rc1, Ho, Wo, seed=9)
            ins['res0'], ins['res1'] = nhwc(kw['res0']), nhwc(kw['res1'])
        # (the slices query speaks of a stride-1 conv: a stride-2 conv's statistics are those of its output map)
        T = int(lib.sr3_conv_stats_slices(B, Ho, Wo, 0, Cin, Cout, tile, ks) if stride == 2 else lib.sr3_conv_stats_slices(B, Hs, Ws, ups, Cin, Cout, tile, ks))
        if k == 1:
            T = 0
        outs = {'out': ((B, Ho, Wo, Cout), torch.float32)}
        if T > 0:
            outs['stats'] = ((B, T, Cout, 2), torch.float64)

        def call(lib, P, scratch, nbytes, stream):
            return lib.sr3_conv_f32(P['src0'], C0, P.get('src1'), C1, B, Hs, Ws, ups, stride, k, Cout, P['w'], P['bias'], P.get('ss'), act,
                                    P.get('film'), Cout if film else 0, P.get('res0'), rc0, P.get('res1'), rc1, P['out'], P.get('stats'),
                                    tile, ks, scratch, nbytes, stream)
        expect = None
        if tile <= 9:          # no derived filters: the slabs alone
            expect = 0 if ks == 1 else ks * B * Ho * Wo * Cout * 4
        return conv_spec(ins, outs, call, lambda lib: int(lib.sr3_conv_scratch_bytes(B, Ho, Wo, Cin, Cout, k, tile, ks)),
                         cached(lambda: nhwc(G.conv_ref(x0, x1, w, **kw))), T, 'conv tile %d ksplit %d' % (tile, ks),
                         conv_refusal(tile, ks, B, Hs, Ws, C0, C1, Cout, k, stride, ups), expect)
    rid = 'conv_t%d_k%d_%dx%dx%d_%d+%dto%d_%dx%d%s%s%s' % (tile, ks, B, Hs, Ws, C0, C1, Cout, k, k, '_s2' if stride == 2 else '', '_up' if ups else '', tag)
    return Row(rid, 'sr3_conv_scratch_bytes', 'sr3_conv_f32', build)


# ---- sr3_conv_dropout_f32 (tests/test_gpu_ops.py::test_conv_dropout) and sr3_block_conv_f32 (::test_block_conv_with_fused_res_conv) -----------

DROP_SEED, DROP_P = 0x1234ABCD, 0.2


def dropout_keep(B, H, W, Cin):
    """the engine's counter-based mask on the NHWC linear index of the activated input, as an NCHW float64 tensor with 1 / (1 - p) folded in"""
    import numpy as np
    from oracle import sr3_oracle as O
    idx = ((np.arange(B)[:, None, None, None] * H + np.arange(H)[None, None, :, None]) * W
           + np.arange(W)[None, None, None, :]) * Cin + np.arange(Cin)[None, :, None, None]
    with np.errstate(over='ignore'):
        hv = O.hash32(idx.astype(np.uint32) * np.uint32(0x9E3779B9) + np.uint32(DROP_SEED))
    keep = torch.from_numpy((hv >= np.uint32(int(DROP_P * 4294967296.0))).astype(np.float64))
    return keep * float(np.float32(1.0 / (1.0 - DROP_P)))


def block_edge(entry, tile, B, H, W, Cin, Cout, X0, X1, residual=False):
    """entry 'dropout': conv3x3(dropout(silu(gn(x)))) + FiLM (+ residual) (+ the fused res_conv of x2); 'block': the same without the
    mask through sr3_block_conv_f32.  ksplit 1: the big kernel's own epilogue writes the caller's output."""
    drop = entry == 'dropout'

    def build():
        from sr3_hip import lib as L
        x = rand(B, Cin, H, W, seed=1)
        w = rand(Cout, Cin, 3, 3, seed=2, scale=1.0 / math.sqrt(Cin * 9))
        bias, film = rand(Cout, seed=3), rand(B, Cout, seed=9)
        ss = torch.stack([1.0 + rand(B, Cin, seed=7, scale=0.3), rand(B, Cin, seed=8, scale=0.3)], 2).contiguous()
        ins = {'src': nhwc(x), 'w': ohwi(w), 'bias': bias, 'ss': ss, 'film': film}
        res = rand(B, Cout, H, W, seed=10) if residual else None
        if residual:
            ins['res'] = nhwc(res)
        x2a = x2b = w2 = b2 = None
        if X0:
            x2a, x2b = rand(B, X0, H, W, seed=21), (rand(B, X1, H, W, seed=22) if X1 else None)
            w2, b2 = rand(Cout, X0 + X1, 1, 1, seed=23) * 0.1, rand(Cout, seed=24)
            ins.update(x2a=nhwc(x2a), w2=w2.reshape(Cout, -1).contiguous(), b2=b2)
            if X1:
                ins['x2b'] = nhwc(x2b)
        T = int(L.load().sr3_conv_stats_slices(B, H, W, 0, Cin, Cout, tile, 1))
        outs = {'out': ((B, H, W, Cout), torch.float32)}
        if T > 0:
            outs['stats'] = ((B, T, Cout, 2), torch.float64)

        def call(lib, P, scratch, nbytes, stream):
            if drop:
                return lib.sr3_conv_dropout_f32(P['src'], Cin, B, H, W, Cout, P['w'], P['bias'], P['ss'], 2, P['film'], Cout, P.get('res'),
                                                Cout if residual else 0, P.get('x2a'), X0, P.get('x2b'), X1, P.get('w2'), P.get('b2'), P['out'],
                                                P.get('stats'), tile, 1, scratch, nbytes, DROP_SEED, DROP_P, stream)
            return lib.sr3_block_conv_f32(P['src'], Cin, None, 0, B, H, W, Cout, P['w'], P['bias'], P['ss'], 2, P['film'], Cout, P['x2a'], X0,
                                          P.get('x2b'), X1, P['w2'], P['b2'], P['out'], P.get('stats'), tile, 1, scratch, nbytes, stream)

        def ref():
            a = x.double() * ss[:, :, 0].double()[:, :, None, None] + ss[:, :, 1].double()[:, :, None, None]
            a = a * torch.sigmoid(a)
            if drop:
                a = a * dropout_keep(B, H, W, Cin)
            r = F.conv2d(a, w.double(), bias.double(), padding=1) + film.double()[:, :, None, None]
            if residual:
                r = r + res.double()
            if X0:
                r = r + F.conv2d((x2a if x2b is None else torch.cat([x2a, x2b], 1)).double(), w2.double(), b2.double())
            return nhwc(r)
        return conv_spec(ins, outs, call, lambda lib: int(lib.sr3_conv_scratch_bytes(B, H, W, Cin, Cout, 3, tile, 1)), cached(ref), T,
                         '%s conv tile %d' % (entry, tile), conv_refusal(tile, 1, B, H, W, Cin, 0, Cout, 3, 1, 0), 0 if tile <= 9 else None)
    rid = '%s_t%d_k1_%dx%dx%d_%dto%d_x2_%d+%d%s' % ('conv_dropout' if drop else 'block_conv', tile, B, H, W, Cin, Cout, X0, X1, '_res' if residual else '')
    return Row(rid, 'sr3_conv_scratch_bytes', 'sr3_conv_dropout_f32' if drop else 'sr3_block_conv_f32', build)


# ---- sr3_conv_in_f32 (tests/test_gpu_ops.py::test_conv_in) ---------------------------------------------------------------------------------------

def plain_spec(ins, outs, call, ref, cmp, extra=None, same=None):
    """Rows without scratch.  ref: cached () -> {name: reference}; cmp: {name: ('close', tol) | ('norm', tol) | ('bits',)}; an output
    without an entry in cmp is written but not compared by the op's test (it must still be finite)."""
    def check(got):
        r = ref()
        for k, c in cmp.items():
            if c[0] == 'close':
                G.assert_close(got[k], r[k], tol=c[1], what=k)
            elif c[0] == 'norm':
                e = relerr(got[k], r[k])
                assert e <= c[1], (k, e)
            else:
                assert G_same(got[k], r[k]), '%s: %d elements differ from the oracle' % (k, int((got[k] != r[k]).sum()))
        if extra:
            extra(got, r)

    def exact():
        r = ref()
        return {k: r[k].to(o.dtype if torch.is_tensor(o) else o[1]) for k, o in outs.items()}

    def tol():
        r, t = ref(), {}
        for k, c in cmp.items():
            t[k] = close_tol(r[k], c[1]) if c[0] == 'close' else c[1] * float(r[k].double().norm()) if c[0] == 'norm' else None
        return t
    return dict(ins=ins, outs=outs, call=call, check=check, query=lambda lib: 0, exact=exact, tol=tol(), same=same or {})


def G_same(a, b):
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def conv_in_row(B, Ca, Cb, H, W, Cout):
    def build():
        a, b = rand(B, Ca, H, W, seed=1), (rand(B, Cb, H, W, seed=2) if Cb else None)
        w, bias = rand(Cout, Ca + Cb, 3, 3, seed=3) * 0.2, rand(Cout, seed=4)
        ins = {'a': a, 'w': ohwi(w), 'bias': bias}
        if Cb:
            ins['b'] = b

        def call(lib, P, scratch, nbytes, stream):
            return lib.sr3_conv_in_f32(P['a'], Ca, P.get('b'), Cb, B, H, W, P['w'], P['bias'], Cout, P['out'], stream)
        ref = cached(lambda: {'out': nhwc(F.conv2d((a if b is None else torch.cat([a, b], 1)).double(), w.double(), bias.double(), padding=1))})
        return plain_spec(ins, {'out': ((B, H, W, Cout), torch.float32)}, call, ref, {'out': ('close', CLOSE)})
    return Row('conv_in_%dx%d+%dx%dx%d_to%d' % (B, Ca, Cb, H, W, Cout), None, 'sr3_conv_in_f32', build)


# ---- attention: sr3_attention_ex_f32 (tests/test_gpu_ops.py::test_attention), sr3_attention_heads_f32 (tests/test_gpu_attn_heads.py::
# test_forward_against_float64), sr3_attention_bwd_f32 (tests/test_gpu_ops.py::test_attention_backward) ------------------------------------------

def attention_row(B, N, Cc, mode, heads=0):
    def build():
        import mha_ref
        qkv = rand(B, N, 3 * Cc, seed=7 if not heads else 11)

        def call(lib, P, scratch, nbytes, stream):
            if heads:
                return lib.sr3_attention_heads_f32(P['qkv'], B, N, Cc, heads, P['out'], mode, stream)
            return lib.sr3_attention_ex_f32(P['qkv'], B, N, Cc, P['out'], mode, stream)

        def ref():
            if heads:
                return {'out': mha_ref.core(qkv.double(), Cc, heads)}
            q, k, v = qkv.double().split(Cc, dim=2)
            return {'out': torch.softmax(q @ k.transpose(1, 2) / math.sqrt(Cc), -1) @ v}
        return plain_spec({'qkv': qkv}, {'out': ((B, N, Cc), torch.float32)}, call, cached(ref), {'out': ('close', CLOSE)})
    return Row('attention%s_%dx%dx%d_mode%d' % ('_heads%d' % heads if heads else '', B, N, Cc, mode), None,
               'sr3_attention_heads_f32' if heads else 'sr3_attention_ex_f32', build)


def attention_bwd_row(B, N, Cc, with_out):
    """The form without scratch: dK and dV are accumulated with atomics, so between two runs only dQ is the same stores."""
    def build():
        qkv = rand(B, N, 3 * Cc, seed=11) * (2.0 if Cc < 256 else 1.0)
        dout = rand(B, N, Cc, seed=12)

        def grads():
            x = qkv.double().requires_grad_(True)
            q, k, v = x.split(Cc, dim=2)
            o = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(Cc), -1) @ v
            o.backward(dout.double())
            return x.grad, o.detach()
        both = cached(grads)
        ins = {'qkv': qkv, 'dout': dout}
        if with_out:
            ins['fwd'] = both()[1].float()

        def call(lib, P, scratch, nbytes, stream):
            return lib.sr3_attention_bwd_f32(P['qkv'], P['dout'], P.get('fwd'), B, N, Cc, P['dqkv'], stream)
        parts = (('dq', slice(0, Cc)), ('dk', slice(Cc, 2 * Cc)), ('dv', slice(2 * Cc, 3 * Cc)))

        def check(got):
            ref = both()[0]
            for name, sl in parts:
                r, g_ = ref[:, :, sl], got['dqkv'].double()[:, :, sl]
                assert (g_ - r).norm() / r.norm() < 2e-5, name
                assert (g_ - r).abs().max() <= 1e-4 * max(1.0, float(r.abs().max())), name
        ref = both()[0]
        at = int(ref.abs().argmax())          # the tolerance of the part (dq, dk or dv) this element lies in
        r = ref[:, :, parts[(at % (3 * Cc)) // Cc][1]]
        tol = min(2e-5 * float(r.norm()), 1e-4 * max(1.0, float(r.abs().max())))
        return dict(ins=ins, outs={'dqkv': ((B, N, 3 * Cc), torch.float32)}, call=call, check=check, query=lambda lib: 0,
                    exact=lambda: {'dqkv': both()[0].float()}, tol={'dqkv': tol},
                    same={'dqkv': lambda a, b: G_same(a[:, :, :Cc], b[:, :, :Cc])})
    return Row('attention_bwd_%dx%dx%d%s' % (B, N, Cc, '_fwd' if with_out else ''), None, 'sr3_attention_bwd_f32', build)


# ---- sr3_conv_wgrad_f32 (tests/test_gpu_ops.py::test_conv_weight_gradient_per_op: float64 autograd of F.conv2d, normwise 2e-6) --------------

def wgrad_edge(kernel, B, Hs, Ws, C0, C1, Cout, act, split, msplit, ups=0):
    """One row per compute kernel of csrc/wgrad.hip, 3x3 stride 1, at the smallest shape where that kernel has every ragged edge.
    `msplit`: the pixel split wgrad_pick gives the shape (asserted through the query, as scratch_rows.wgrad_row does: the slabs of both
    `split` values have this size at these shapes); the scratch is 16-byte aligned by contract."""
    Cin = C0 + C1

    def build():
        Ho, Wo = Hs << ups, Ws << ups
        x0, x1 = rand(B, C0, Hs, Ws, seed=31), (rand(B, C1, Hs, Ws, seed=32) if C1 else None)
        dy = rand(B, Cout, Ho, Wo, seed=35)
        ins = {'src0': nhwc(x0), 'dy': nhwc(dy)}
        if C1:
            ins['src1'] = nhwc(x1)
        ss = None
        if act:
            ss = ins['ss'] = torch.stack([rand(B, Cin, seed=33) * 0.3 + 1.0, rand(B, Cin, seed=34) * 0.3], dim=2).contiguous()

        def call(lib, P, scratch, nbytes, stream):
            return lib.sr3_conv_wgrad_f32(P['src0'], C0, P.get('src1'), C1, B, Hs, Ws, ups, 1, 3, Cout, P.get('ss'), act, P['dy'], P['dw'], split,
                                          scratch, nbytes, stream)

        def grad():
            a = (x0 if x1 is None else torch.cat([x0, x1], 1)).double()
            if act:
                a = a * ss[:, :, 0].double()[:, :, None, None] + ss[:, :, 1].double()[:, :, None, None]
                if act == 2:
                    a = a * torch.sigmoid(a)
            if ups:
                a = F.interpolate(a, scale_factor=2, mode='nearest')
            w = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
            F.conv2d(a, w, None, stride=1, padding=1).backward(dy.double())
            return w.grad.permute(0, 2, 3, 1).reshape(Cout, 9, Cin).contiguous()
        ref = cached(grad)

        def check(got):
            e = relerr(got['dw'], ref())
            assert e < 2e-6, (kernel, e)
        return dict(ins=ins, outs={'dw': ((Cout, 9, Cin), torch.float32)}, call=call, check=check, expect=msplit * Cout * 9 * Cin * 4,
                    query=lambda lib: int(lib.sr3_conv_wgrad_scratch_bytes(B, Hs, Ws, ups, 1, 3, C0, C1, Cout, split)),
                    exact=lambda: {'dw': ref().float()}, tol={'dw': 2e-6 * float(ref().norm())})
    rid = 'wgrad_%s_%dx%dx%d_%d+%dto%d%s_act%d_split%d' % (kernel, B, Hs, Ws, C0, C1, Cout, '_up' if ups else '', act, split)
    return Row(rid, 'sr3_conv_wgrad_scratch_bytes', 'sr3_conv_wgrad_f32', build, align=16)


# ---- the small entries -----------------------------------------------------------------------------------------------------------------------------

def gn_stats_row(B, HW, Cc):
    """tests/test_gpu_ops.py::test_groupnorm_stats_and_fold, first half: the partials sum to the float64 sums (rtol 1e-12, atol 1e-9)"""
    def build():
        from sr3_hip import lib as L
        x = rand(B, HW, Cc, seed=3) * 2 + 0.5
        T = int(L.load().sr3_groupnorm_stats_slices(B, HW, Cc))

        def call(lib, P, scratch, nbytes, stream):
            return lib.sr3_groupnorm_stats_f32(P['x'], B, HW, Cc, P['st'], stream)

        def check(got):
            st = got['st']
            assert torch.allclose(st[..., 0].sum(1), x.double().sum(1), rtol=1e-12, atol=1e-9)
            assert torch.allclose(st[..., 1].sum(1), (x.double() ** 2).sum(1), rtol=1e-12, atol=1e-9)

        def exact():
            st = torch.zeros(B, T, Cc, 2, dtype=torch.float64)
            st[:, 0, :, 0], st[:, 0, :, 1] = x.double().sum(1), (x.double() ** 2).sum(1)
            return {'st': st}
        return dict(ins={'x': x}, outs={'st': ((B, T, Cc, 2), torch.float64)}, call=call, check=check, query=lambda lib: 0, exact=exact,
                    tol={'st': 1e-9 + 1e-12 * float((x.double() ** 2).sum(1).max())})
    return Row('groupnorm_stats_%dx%dx%d' % (B, HW, Cc), None, 'sr3_groupnorm_stats_f32', build)


def gn_fold_row(B, HW, Cc):
    """... second half: the fold of two concat sources with different slice counts, groups straddling the seam; x * scale + shift against
    float64 F.group_norm under assert_close at 5e-6."""
    def build():
        x = rand(B, HW, Cc, seed=3) * 2 + 0.5
        C0 = Cc // 2 - 4
        C1, groups, T0 = Cc - C0, 4, 3
        gamma, beta = rand(Cc, seed=4) * 0.2 + 1, rand(Cc, seed=5) * 0.2
        xd = x.double()
        bounds = [0] + [HW * (i + 1) // T0 for i in range(T0)]          # T0 pixel slices, ragged
        st = torch.stack([torch.stack([xd[:, a:b].sum(1), (xd[:, a:b] ** 2).sum(1)], -1) for a, b in zip(bounds, bounds[1:])], 1)   # [B][T0][C][2]
        st0 = st[:, :, :C0].contiguous()
        half = st[:, :, C0:] * 0.5
        st1 = torch.cat([half, half], dim=1).contiguous()          # the second source with twice the partials

        def call(lib, P, scratch, nbytes, stream):
            return lib.sr3_groupnorm_fold_f32(P['st0'], C0, T0, P['st1'], C1, 2 * T0, B, HW, groups, P['gamma'], P['beta'], 1e-5, P['ss'], stream)
        xn = x.permute(0, 2, 1).reshape(B, Cc, HW, 1).double()
        gn = cached(lambda: F.group_norm(xn, groups, gamma.double(), beta.double(), eps=1e-5))

        def check(got):
            ss = got['ss'].double()
            G.assert_close(xn * ss[:, :, 0][:, :, None, None] + ss[:, :, 1][:, :, None, None], gn(), tol=5e-6, what='gn fold')

        def exact():
            xg = xn.reshape(B, groups, -1)
            mean, rstd = xg.mean(2), 1.0 / torch.sqrt(xg.var(2, unbiased=False) + 1e-5)
            scale = rstd.repeat_interleave(Cc // groups, 1) * gamma.double()[None]
            shift = beta.double()[None] - mean.repeat_interleave(Cc // groups, 1) * scale
            return {'ss': torch.stack([scale, shift], 2).float()}
        return dict(ins={'st0': st0, 'st1': st1, 'gamma': gamma, 'beta': beta}, outs={'ss': ((B, Cc, 2), torch.float32)}, call=call, check=check,
                    query=lambda lib: 0, exact=exact, tol={'ss': close_tol(gn(), 5e-6)})
    return Row('groupnorm_fold_%dx%dx%d' % (B, HW, Cc), None, 'sr3_groupnorm_fold_f32', build)


def film_embed_row(variant):
    """tests/test_gpu_ops.py::test_film_embed: the FiLM table under assert_close at 1e-5 (the embedding itself is written, not compared)"""
    B, inner, Fn = 3, 64, 200

    def build():
        w1, b1 = rand(4 * inner, inner, seed=1) * 0.1, rand(4 * inner, seed=2) * 0.1
        w2, b2 = rand(inner, 4 * inner, seed=3) * 0.1, rand(inner, seed=4) * 0.1
        wf, bf = rand(Fn, inner, seed=5) * 0.1, rand(Fn, seed=6) * 0.1
        ins = dict(w1=w1, b1=b1, w2=w2, b2=b2, wf=wf, bf=bf)
        if variant == 0:
            ins['level'] = level = torch.tensor([0.999, 0.5, 0.013])
            count = inner // 2
            freq = torch.exp(-math.log(1e4) * (torch.arange(count, dtype=torch.float32) / count))
            arg = level[:, None] * freq[None]
        else:
            ins['tstep'] = tstep = torch.tensor([0, 999, 1999], dtype=torch.long)
            freq = torch.exp(torch.arange(0, inner, 2, dtype=torch.float32) * (-math.log(10000) / inner))
            arg = torch.outer(tstep.float(), freq)
        ins['freq'] = freq

        def call(lib, P, scratch, nbytes, stream):
            return lib.sr3_film_embed_f32(variant, B, inner, P.get('level'), P.get('tstep'), P['freq'], P['w1'], P['b1'], P['w2'], P['b2'], P['wf'],
                                          P['bf'], Fn, P['temb'], P['film'], stream)

        def ref():
            enc = torch.cat([arg.sin(), arg.cos()], -1).double()
            h = enc @ w1.double().t() + b1.double()
            h = h * torch.sigmoid(h)
            t = h @ w2.double().t() + b2.double()
            if variant == 1:
                t = t * torch.sigmoid(t)
            return {'temb': t, 'film': t @ wf.double().t() + bf.double()}
        return plain_spec(ins, {'temb': ((B, inner), torch.float32), 'film': ((B, Fn), torch.float32)}, call, cached(ref), {'film': ('close', 1e-5)})
    return Row('film_embed_v%d' % variant, None, 'sr3_film_embed_f32', build)


def grad_route_row(C0, C1, ups, Hs, Ws, B, acc0, acc1):
    """tests/test_gpu_backward_ops.py::test_grad_route: bit equality with fp32 torch doing the same adds in the kernel's order"""
    def build():
        g = rand(B, Hs << ups, Ws << ups, C0 + C1, seed=21)
        s = ((g[:, 0::2, 0::2] + g[:, 0::2, 1::2]) + g[:, 1::2, 0::2]) + g[:, 1::2, 1::2] if ups else g
        old0, old1 = rand(B, Hs, Ws, C0, seed=22), rand(B, Hs, Ws, C1, seed=23)

        def call(lib, P, scratch, nbytes, stream):
            return lib.sr3_grad_route_f32(P['g'], C0, C1, B, Hs, Ws, ups, P['d0'], acc0, P['d1'], acc1, stream)
        ref = cached(lambda: {'d0': (s[..., :C0] + old0 if acc0 else s[..., :C0]).contiguous(),
                              'd1': (s[..., C0:] + old1 if acc1 else s[..., C0:]).contiguous()})
        outs = {'d0': old0 if acc0 else ((B, Hs, Ws, C0), torch.float32), 'd1': old1 if acc1 else ((B, Hs, Ws, C1), torch.float32)}
        return plain_spec({'g': g}, outs, call, ref, {'d0': ('bits',), 'd1': ('bits',)})
    return Row('grad_route_%d+%d_%dx%dx%d_up%d_acc%d%d' % (C0, C1, B, Hs, Ws, ups, acc0, acc1), None, 'sr3_grad_route_f32', build)


def p_sample_row(B, Cc, H, W, t=17):
    """tests/test_gpu_ops.py::test_p_sample_step_bit_exact: the fused update equals the oracle's elementwise torch ops bit for bit"""
    def build():
        from oracle import sr3_oracle as O
        tab = O.schedule_tables(dict(schedule='linear', n_timestep=50, linear_start=1e-6, linear_end=1e-2))
        sig = (0.5 * torch.from_numpy(tab['posterior_log_variance_clipped'])).exp()
        sig[0] = 0
        keys = ('sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod', 'posterior_mean_coef1', 'posterior_mean_coef2')
        ins = {'tab%d' % i: torch.from_numpy(tab[k]).float().contiguous() for i, k in enumerate(keys)}
        ins['tab4'] = sig.float().contiguous()
        x, eps, z = rand(B, Cc, H, W, seed=1), rand(B, Cc, H, W, seed=2), rand(B, Cc, H, W, seed=3)
        ins.update(eps=eps, z=z)

        def call(lib, P, scratch, nbytes, stream):
            return lib.sr3_p_sample_step_ex(P['x'], P['eps'], P['z'], *[P['tab%d' % i] for i in range(5)], None, None, t, B, Cc * H * W, 1, stream)
        return plain_spec(ins, {'x': x}, call, cached(lambda: {'x': O.p_sample_update(tab, x, eps, t, z)}), {'x': ('bits',)})
    return Row('p_sample_step_%dx%d' % (B, Cc * H * W), None, 'sr3_p_sample_step_ex', build)


def q_sample_row(B, Cc, H, W):
    """tests/test_gpu_ops.py::test_q_sample_bit_exact"""
    def build():
        x0, z = rand(B, Cc, H, W, seed=1), rand(B, Cc, H, W, seed=2)
        g = torch.rand(B, generator=torch.Generator().manual_seed(3))
        ca, cb = g, (1 - g ** 2).sqrt()

        def call(lib, P, scratch, nbytes, stream):
            return lib.sr3_q_sample(P['x0'], P['z'], P['ca'], P['cb'], B, Cc * H * W, P['out'], stream)
        ref = cached(lambda: {'out': ca.view(-1, 1, 1, 1) * x0 + cb.view(-1, 1, 1, 1) * z})
        return plain_spec({'x0': x0, 'z': z, 'ca': ca, 'cb': cb}, {'out': ((B, Cc, H, W), torch.float32)}, call, ref, {'out': ('bits',)})
    return Row('q_sample_%dx%d' % (B, Cc * H * W), None, 'sr3_q_sample', build)


def adam_ema_row(n):
    """sr3_adam_ema_step, ema_mode 2.  The weights: the update p' - p against float64 Adam within 2e-6 (tests/test_gpu_train.py::
    test_optimize_parameters_one_adam_step); the moments under assert_close; the EMA against the float64 lerp of the weights as written
    within 2^-23 max(|ema|, |p'|) per element (tests/test_gpu_ema.py::test_fused_step_matches_adam_and_float64_lerp)."""
    lr, b1, b2, eps, step, decay = 1e-3, 0.9, 0.999, 1e-8, 7, 0.9

    def build():
        import numpy as np
        p, g, m = rand(n, seed=1), rand(n, seed=2) * 0.1, rand(n, seed=3) * 0.1
        v = torch.rand(n, generator=torch.Generator().manual_seed(4)) * 0.01
        ema = rand(n, seed=5)
        f32 = lambda a: float(np.float32(a))
        wl = f32(1.0 - decay)

        def call(lib, P, scratch, nbytes, stream):
            c = C.c_float
            return lib.sr3_adam_ema_step(P['p'], P['g'], P['m'], P['v'], P['ema'], n, c(lr), c(b1), c(b2), c(eps), step, c(decay), 2, stream)

        def ref():
            m1 = f32(b1) * m.double() + (1.0 - f32(b1)) * g.double()
            v1 = f32(b2) * v.double() + (1.0 - f32(b2)) * g.double() ** 2
            den = (v1 / (1.0 - f32(b2) ** step)).sqrt() + f32(eps)
            p1 = p.double() - f32(lr) / (1.0 - f32(b1) ** step) * m1 / den
            return {'p': p1, 'm': m1, 'v': v1, 'ema': ema.double() + (p1.float().double() - ema.double()) * wl}

        def extra(got, r):
            assert float(((got['p'].double() - p.double()) - (r['p'] - p.double())).abs().max()) <= 2e-6
            want = ema.double() + (got['p'].double() - ema.double()) * wl
            bound = 2.0 ** -23 * torch.maximum(ema.double().abs(), got['p'].double().abs())
            assert int((~((got['ema'].double() - want).abs() <= bound)).sum()) == 0
        spec = plain_spec({'g': g}, {'p': p, 'm': m, 'v': v, 'ema': ema}, call, cached(ref), {'m': ('close', CLOSE), 'v': ('close', CLOSE)}, extra)
        i = int(spec['exact']()['ema'].abs().argmax())          # (the element the tolerance is taken at: the largest of the output)
        spec['tol'].update(p=2e-6, ema=2.0 ** -23 * max(abs(float(ema[i])), abs(float(spec['exact']()['p'][i]))))
        return spec
    return Row('adam_ema_step_%d' % n, None, 'sr3_adam_ema_step', build)


# ---- the table -----------------------------------------------------------------------------------------------------------------------------------------

def _conv_rows():
    rows = []
    for t in (1, 2, 3, 4, 14, 15, 16, 17):          # im2col: M = 300, a channel tail and a ragged Cout; a seam inside a chunk; stride 2; x2 upsampling
        rows += [conv_edge(t, 1, 3, 10, 10, 24, 0, 40), conv_edge(t, 2, 3, 10, 10, 24, 0, 40),
                 conv_edge(t, 1, 3, 6, 10, 8, 12, 24, k=1), conv_edge(t, 1, 2, 10, 10, 24, 0, 40, stride=2), conv_edge(t, 1, 2, 8, 8, 64, 0, 64, ups=1)]
    # halo: a channel tail and a ragged Cout; a seam inside a chunk, Cout ragged against 64 and 128; the Upsample conv.  The halo kernel
    # splits K over 32-channel chunks and refuses a split that leaves one empty, so the split rows carry a second chunk: 56 channels (the
    # same 24-channel tail, now in the last chunk of the second split) and 64 channels on the two-image tile
    for t in (5, 6, 9):
        rows += [conv_edge(t, 1, 2, 16, 16, 24, 0, 40), conv_edge(t, 2, 2, 16, 16, 56, 0, 40),
                 conv_edge(t, 1, 2, 16, 32, 48, 16, 96, res='concat', RC0=64), conv_edge(t, 1, 1, 16, 16, 64, 0, 128, ups=1, act=0, film=False)]
    rows += [conv_edge(5, 1, 3, 8, 8, 32, 0, 64), conv_edge(5, 2, 3, 8, 8, 64, 0, 64)]          # two images per tile, the last one absent
    for t in (11, 12, 13):
        rows += [conv_edge(t, 1, 2, 16, 16, 24, 0, 40), conv_edge(t, 2, 2, 16, 16, 24, 0, 40), conv_edge(t, 1, 2, 16, 48, 24, 8, 40)]
        if t == 13:
            rows.append(conv_edge(t, 1, 2, 24, 32, 48, 16, 72))          # a map 8 mod 16 high
        rows.append(conv_edge(t, 1, 2, 8, 8, 64, 0, 64, ups=1))
    rows.append(conv_edge(25, 1, 2, 8, 8, 64, 0, 64, ups=1))
    rows += [conv_edge(23, 1, 3, 11, 22, 64, 0, 40), conv_edge(23, 2, 3, 11, 22, 64, 0, 40)]          # tiles hang over the map both ways
    rows += [conv_edge(22, 1, 2, 16, 32, 96, 32, 320, k=1, act=1), conv_edge(22, 1, 2, 16, 16, 64, 0, 64, stride=2, act=0)]
    rows += [block_edge('dropout', 5, 3, 8, 8, 32, 64, 24, 8, residual=True), block_edge('dropout', 5, 2, 16, 16, 128, 128, 96, 32),
             block_edge('dropout', 6, 1, 32, 32, 64, 64, 64, 32), block_edge('dropout', 11, 2, 16, 16, 64, 128, 0, 0, residual=True),
             block_edge('dropout', 12, 2, 16, 16, 64, 128, 0, 0, residual=True),
             block_edge('block', 5, 3, 8, 8, 32, 64, 24, 8), block_edge('block', 6, 2, 16, 16, 64, 128, 96, 32),
             block_edge('block', 9, 2, 16, 16, 64, 128, 96, 32)]
    return rows


CONV_ROWS = _conv_rows()

OTHER_ROWS = [conv_in_row(3, 3, 0, 10, 12, 8), conv_in_row(2, 3, 3, 16, 16, 64)]
# generic kernel with a ragged N; N < 32; a ragged last query block with the channel split; the staging-free kernel without / with key pairs
OTHER_ROWS += [attention_row(B, N, Cc, mode) for (B, N, Cc) in ((2, 100, 48), (3, 16, 256), (1, 72, 512), (2, 64, 512), (1, 256, 256)) for mode in (0, 1)]
OTHER_ROWS += [attention_row(B, N, Cc, mode, heads=2) for (B, N, Cc, modes) in ((3, 16, 64, (0, 1)), (2, 100, 96, (0, 1)), (2, 100, 128, (0, 1, 4, 5)))
               for mode in modes]
OTHER_ROWS += [attention_bwd_row(2, 100, 48, False), attention_bwd_row(2, 64, 32, False), attention_bwd_row(1, 512, 128, True)]
# the weight gradient, one row per compute instantiation.  15 x 15: 225 pixels, 8 chunks whose last holds one pixel, the division decode;
# 36 + 12 -> 40: the seam inside the only 64-channel tile, both tile tails, the in-kernel affine prologue; 40 + 32 -> 68: ragged 128
# tiles on both sides, on the fp32 and on the split kernel with its prologue; 8 x 9 upsampled: 288 pixels, 9 chunks (5 + 4), the
# upsampled address off the power-of-two maps; 2 x 4 x 24: chunks of 4 rows x 8 columns, three side by side, a ragged 64 x 64 tile
WGRAD_ROWS = [wgrad_edge('fp32_64', 1, 15, 15, 36, 12, 40, 1, 0, 2), wgrad_edge('fp32_128', 1, 15, 15, 40, 32, 68, 2, 0, 2),
              wgrad_edge('split_act', 1, 15, 15, 40, 32, 68, 2, 1, 2), wgrad_edge('split_raw', 1, 8, 9, 40, 32, 68, 0, 1, 2, ups=1),
              wgrad_edge('nine_tap', 2, 4, 24, 20, 0, 12, 0, 1, 3)]
OTHER_ROWS += WGRAD_ROWS
OTHER_ROWS += [gn_stats_row(3, 100, 24), gn_stats_row(1, 16, 1024), gn_fold_row(3, 100, 24), gn_fold_row(1, 16, 1024)]
OTHER_ROWS += [film_embed_row(0), film_embed_row(1)]
# the two smallest cases of test_grad_route's list with a concat seam, one accumulate flag each way
OTHER_ROWS += [grad_route_row(8, 16, 0, 5, 7, 1, 1, 0), grad_route_row(8, 16, 1, 5, 7, 1, 0, 1)]
OTHER_ROWS += [p_sample_row(3, 3, 5, 7), p_sample_row(3, 3, 16, 16), q_sample_row(3, 3, 4, 9), q_sample_row(3, 3, 16, 16)]
OTHER_ROWS += [adam_ema_row(1004)]

ROWS = CONV_ROWS + OTHER_ROWS
