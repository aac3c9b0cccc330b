"""The per-op scratch contract table: one row per launch that consumes a `*_scratch_bytes` query of sr3_hip/lib.py (a plain helper
module, shared by tests/test_gpu_scratch_contract.py -- guarded buffers under three fills on the GPU -- and
tests/test_scratch_contract_cpu.py -- undersized and misaligned scratch refused on the host, with made-up pointers).

A row is built lazily (`Row.spec()`) into
  ins    {name: CPU tensor}                       the call's inputs, in the layout the entry reads
  outs   {name: (shape, dtype) | CPU tensor}      outputs (NaN-filled before the call) or in/out tensors (their start value)
  query  lib -> bytes                             the row's `*_scratch_bytes` query
  call   (lib, P, scratch, nbytes, stream) -> rc  the launch; P maps every name of ins / outs (and 'derived') to a pointer
  check  {name: CPU tensor} -> None               the float64 comparison the op's own test makes, at that test's tolerance (GPU only)
and optionally `derived` (bytes of a second caller-owned buffer that is scratch in the same sense), `expect` (the byte count the
query must return, where the shapes were chosen for it) and `min_bytes` (the smallest scratch the entry accepts, where that is
documented to be less than the query).

`align`: the scratch alignment the header states for the entry (0: any).  `small`: the code a too-small scratch is refused with --
SR3_E_NOMEM unless the header documents SR3_E_BADARG for the entry (the optimizer entries, the guided step's select, the
back-projection step and the JPEG round trip, whose tests pin that code); None for an entry without a byte count argument (its scratch
has a constant size)."""
import ctypes as C
import math

import torch
import torch.nn.functional as F

from gpu_util import assert_close, nchw, nhwc, ohwi

NOMEM, ALIGN, UNSUP, BADARG = -4, -3, -2, -1


def rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def relerr(got, ref):
    ref = ref.double()
    return ((got.double() - ref).norm() / ref.norm()).item()


class Row(object):
    def __init__(self, rid, query, entry, build, align=256, small=NOMEM):
        self.id, self.query, self.entry, self.build, self.align, self.small = rid, query, entry, build, align, small
        self._spec = None

    def spec(self):
        if self._spec is None:
            self._spec = self.build()
        return self._spec


# ---- sr3_conv_scratch_bytes: sr3_conv_f32, sr3_block_conv_f32, sr3_conv_dropout_f32 -------------------------------------------------

def conv_row(tile, ks, B, Hs, Ws, Cin, Cout, k, stride=1, ups=0, expect=None, tag=''):
    def build():
        from sr3_hip import lib as L
        lib = L.load()
        pad = k // 2
        Ho, Wo = ((Hs << ups) + 2 * pad - k) // stride + 1, ((Ws << ups) + 2 * pad - k) // stride + 1
        x = rand(B, Cin, Hs, Ws, seed=1)
        w = rand(Cout, Cin, k, k, seed=2, scale=1.0 / math.sqrt(Cin * k * k))
        bias = rand(Cout, seed=3, scale=0.1)
        outs = {'out': ((B, Ho, Wo, Cout), torch.float32)}
        # (the slices query speaks of a stride-1 conv: a stride-2 conv's statistics are those of its output map)
        T = int(lib.sr3_conv_stats_slices(B, Ho, Wo, 0, Cin, Cout, tile, ks) if stride == 2 else lib.sr3_conv_stats_slices(B, Hs, Ws, ups, Cin, Cout, tile, ks))
        if T > 0:
            outs['stats'] = ((B, T, Cout, 2), torch.float64)

        def call(lib, P, scratch, nbytes, stream):
            return lib.sr3_conv_f32(P['src'], Cin, None, 0, B, Hs, Ws, ups, stride, k, Cout, P['w'], P['bias'], None, 0, None, 0, None, 0,
                                    None, 0, P['out'], P.get('stats'), tile, ks, scratch, nbytes, stream)

        def check(got):
            xi = F.interpolate(x.double(), scale_factor=2, mode='nearest') if ups else x.double()
            ref = F.conv2d(xi, w.double(), bias.double(), stride=stride, padding=pad)
            out = nchw(got['out'])
            assert_close(out, ref, what='conv tile %d ksplit %d' % (tile, ks))
            if 'stats' in got:
                st = got['stats'].sum(1)
                assert torch.allclose(st[:, :, 0], out.double().sum(dim=(2, 3)), rtol=1e-9, atol=1e-9)
                assert torch.allclose(st[:, :, 1], (out.double() ** 2).sum(dim=(2, 3)), rtol=1e-9, atol=1e-9)
        return dict(ins={'src': nhwc(x), 'w': ohwi(w), 'bias': bias}, outs=outs, call=call, check=check, expect=expect,
                    query=lambda lib: int(lib.sr3_conv_scratch_bytes(B, Ho, Wo, Cin, Cout, k, tile, ks)))
    return Row('conv_t%d_k%d_%dx%dx%d_%dto%d_%dx%d%s' % (tile, ks, B, Hs, Ws, Cin, Cout, k, k, tag), 'sr3_conv_scratch_bytes', 'sr3_conv_f32',
               build)


def block_conv_row(tile, ks, B, H, W, Cin, Cout, X0, X1):
    """block2's conv3x3 with the 1x1 res_conv of the (concat) block input as a second K segment of the same halo tile, under split-K: the
    slabs of both segments live in scratch (tests/test_gpu_ops.py::test_block_conv_with_fused_res_conv's reference and bound)."""
    def build():
        from sr3_hip import lib as L
        x = rand(B, Cin, H, W, seed=1)
        w = rand(Cout, Cin, 3, 3, seed=2, scale=1.0 / math.sqrt(Cin * 9))
        bias, film = rand(Cout, seed=3, scale=0.1), rand(B, Cout, seed=9)
        ss = torch.stack([1.0 + rand(B, Cin, seed=7, scale=0.1), rand(B, Cin, seed=8, scale=0.1)], 2).contiguous()
        x2a, x2b = rand(B, X0, H, W, seed=21), (rand(B, X1, H, W, seed=22) if X1 else None)
        w2, b2 = rand(Cout, X0 + X1, 1, 1, seed=23) * 0.1, rand(Cout, seed=24)
        ins = {'src': nhwc(x), 'w': ohwi(w), 'bias': bias, 'ss': ss, 'film': film, 'x2a': nhwc(x2a), 'w2': w2.reshape(Cout, -1).contiguous(), 'b2': b2}
        if X1:
            ins['x2b'] = nhwc(x2b)
        outs = {'out': ((B, H, W, Cout), torch.float32)}
        T = int(L.load().sr3_conv_stats_slices(B, H, W, 0, Cin, Cout, tile, ks))
        if T > 0:
            outs['stats'] = ((B, T, Cout, 2), torch.float64)

        def call(lib, P, scratch, nbytes, stream):
            return lib.sr3_block_conv_f32(P['src'], Cin, None, 0, B, H, W, Cout, P['w'], P['bias'], P['ss'], 2, P['film'], Cout, P['x2a'], X0,
                                          P.get('x2b'), X1, P['w2'], P['b2'], P['out'], P.get('stats'), tile, ks, scratch, nbytes, stream)

        def check(got):
            a = x.double() * ss[:, :, 0].double()[:, :, None, None] + ss[:, :, 1].double()[:, :, None, None]
            ref = F.conv2d(a * torch.sigmoid(a), w.double(), bias.double(), padding=1) + film.double()[:, :, None, None]
            ref = ref + F.conv2d((x2a if x2b is None else torch.cat([x2a, x2b], 1)).double(), w2.double(), b2.double())
            out = nchw(got['out'])
            assert_close(out, ref, what='block conv tile %d ksplit %d' % (tile, ks))
            if 'stats' in got:
                st = got['stats'].sum(1)
                assert torch.allclose(st[:, :, 0], out.double().sum(dim=(2, 3)), rtol=1e-9, atol=1e-9)
                assert torch.allclose(st[:, :, 1], (out.double() ** 2).sum(dim=(2, 3)), rtol=1e-9, atol=1e-9)
        return dict(ins=ins, outs=outs, call=call, check=check, query=lambda lib: int(lib.sr3_conv_scratch_bytes(B, H, W, Cin, Cout, 3, tile, ks)))
    return Row('block_conv_t%d_k%d_%dx%dx%d_%dto%d_x2_%d+%d' % (tile, ks, B, H, W, Cin, Cout, X0, X1), 'sr3_conv_scratch_bytes',
               'sr3_block_conv_f32', build)


DROP_SEED, DROP_P = 0x1234ABCD, 0.2


def conv_dropout_row(tile, ks, B, H, W, Cin, Cout):
    def build():
        import numpy as np
        x = rand(B, Cin, H, W, seed=4)
        w = rand(Cout, Cin, 3, 3, seed=5, scale=1.0 / math.sqrt(Cin * 9))
        bias = rand(Cout, seed=6, scale=0.1)
        ss = torch.stack([1.0 + rand(B, Cin, seed=7, scale=0.1), rand(B, Cin, seed=8, scale=0.1)], 2).contiguous()

        def call(lib, P, scratch, nbytes, stream):
            return lib.sr3_conv_dropout_f32(P['src'], Cin, B, H, W, Cout, P['w'], P['bias'], P['ss'], 2, None, 0, None, 0, None, 0, None, 0, None,
                                            None, P['out'], None, tile, ks, scratch, nbytes, DROP_SEED, DROP_P, stream)

        def check(got):
            from oracle import sr3_oracle as O
            a = x.double() * ss[:, :, 0].double()[:, :, None, None] + ss[:, :, 1].double()[:, :, None, None]
            a = a * torch.sigmoid(a)
            idx = ((np.arange(B)[:, None, None, None] * H + np.arange(H)[None, None, :, None]) * W
                   + np.arange(W)[None, None, None, :]) * Cin + np.arange(Cin)[None, :, None, None]
            with np.errstate(over='ignore'):
                hv = O.hash32(idx.astype(np.uint32) * np.uint32(0x9E3779B9) + np.uint32(DROP_SEED))
            keep = torch.from_numpy((hv >= np.uint32(int(DROP_P * 4294967296.0))).astype(np.float64))
            a = a * keep * float(np.float32(1.0 / (1.0 - DROP_P)))
            assert_close(nchw(got['out']), F.conv2d(a, w.double(), bias.double(), padding=1), what='dropout conv tile %d' % tile)
        return dict(ins={'src': nhwc(x), 'w': ohwi(w), 'bias': bias, 'ss': ss}, outs={'out': ((B, H, W, Cout), torch.float32)}, call=call,
                    check=check, query=lambda lib: int(lib.sr3_conv_scratch_bytes(B, H, W, Cin, Cout, 3, tile, ks)))
    return Row('conv_dropout_t%d_k%d_%dx%dx%d_%dto%d' % (tile, ks, B, H, W, Cin, Cout), 'sr3_conv_scratch_bytes', 'sr3_conv_dropout_f32', build)


# ---- sr3_conv_wgrad_scratch_bytes ---------------------------------------------------------------------------------------------------

def wgrad_row(name, B, Hs, Ws, k, Cin, Cout, split, msplit):
    """`msplit`: the pixel split csrc/wgrad.hip's wgrad_pick gives this shape (> 1: the slabs are really used) -- the query must
    return exactly that many slabs."""
    def build():
        x, dy = rand(B, Cin, Hs, Ws, seed=31), rand(B, Cout, Hs, Ws, seed=35)

        def call(lib, P, scratch, nbytes, stream):
            return lib.sr3_conv_wgrad_f32(P['src'], Cin, None, 0, B, Hs, Ws, 0, 1, k, Cout, None, 0, P['dy'], P['dw'], split, scratch, nbytes, stream)

        def check(got):
            w = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, requires_grad=True)
            F.conv2d(x.double(), w, None, stride=1, padding=k // 2).backward(dy.double())
            e = relerr(got['dw'].view(Cout, k, k, Cin).permute(0, 3, 1, 2), w.grad)
            assert e < 2e-6, (name, e)
        return dict(ins={'src': nhwc(x), 'dy': nhwc(dy)}, outs={'dw': ((Cout, k * k, Cin), torch.float32)}, call=call, check=check,
                    expect=msplit * Cout * k * k * Cin * 4,
                    query=lambda lib: int(lib.sr3_conv_wgrad_scratch_bytes(B, Hs, Ws, 0, 1, k, Cin, 0, Cout, split)))
    return Row('wgrad_' + name, 'sr3_conv_wgrad_scratch_bytes', 'sr3_conv_wgrad_f32', build, align=16)


# ---- sr3_conv_dgrad_scratch_bytes (through a plan handle, as tests/test_gpu_backward_ops.py) ----------------------------------------

def dgrad_row(name, opts, B, Hs, Ws, Cin, Cout, k, stride, tile, kind, split):
    def build():
        from sr3_hip import engine as E
        plan = E.Plan('sr3', 6, 3, 8, 4, [1, 2], [8], 1, 16)
        for key, v in opts.items():
            plan.set_option(key, v)
        Ho, Wo = (Hs + 2 * (k // 2) - k) // stride + 1, (Ws + 2 * (k // 2) - k) // stride + 1
        dy = rand(B, Cout, Ho, Wo, seed=41)
        w = rand(Cout, Cin, k, k, seed=43, scale=1.0 / math.sqrt(Cout * k * k))
        nd = C.c_size_t(0)
        nb = int(plan.lib.sr3_conv_dgrad_scratch_bytes(plan.handle, B, Hs, Ws, 0, stride, k, Cin, Cout, C.byref(nd), None))
        # the entry does what the step does: with less room than the chosen kernel's slabs need it falls back to the general kernels
        # (tests/test_gpu_backward_ops.py::test_conv_dgrad_falls_back_without_room), so what it refuses is a scratch below THEIR query
        general = E.Plan('sr3', 6, 3, 8, 4, [1, 2], [8], 1, 16)
        general.set_option('winograd', 0)
        general.set_option('gemm2', 0)
        min_bytes = int(plan.lib.sr3_conv_dgrad_scratch_bytes(general.handle, B, Hs, Ws, 0, stride, k, Cin, Cout, None, None))
        assert 0 < min_bytes <= nb
        ran = {}

        def call(lib, P, scratch, nbytes, stream):
            t, ks, kd = C.c_int(-1), C.c_int(-1), C.c_int(-1)
            rc = lib.sr3_conv_dgrad_f32(plan.handle, P['dy'], P['w'], Cout, Cout, B, Hs, Ws, 0, stride, k, Cin, P['dA'], scratch, nbytes,
                                        P.get('derived'), nd.value if P.get('derived') is not None else 0, C.byref(t), C.byref(ks), C.byref(kd),
                                        stream)
            ran.update(tile=t.value, ksplit=ks.value, kind=kd.value)
            return rc

        def check(got):
            assert (ran['tile'], ran['kind']) == (tile, kind) and (split is None or (ran['ksplit'] > 1) == split), ran
            xx = torch.zeros(B, Cin, Hs, Ws, dtype=torch.float64, requires_grad=True)
            F.conv2d(xx, w.double(), None, stride=stride, padding=k // 2).backward(dy.double())
            assert_close(nchw(got['dA']), xx.grad, what='dgrad ' + name)
        return dict(plan=plan, ins={'dy': nhwc(dy), 'w': ohwi(w)}, outs={'dA': ((B, Hs, Ws, Cin), torch.float32)}, call=call, check=check,
                    derived=nd.value, min_bytes=min_bytes, query=lambda lib: nb)
    return Row('dgrad_' + name, 'sr3_conv_dgrad_scratch_bytes', 'sr3_conv_dgrad_f32', build)


# ---- sr3_groupnorm_act_bwd_scratch_bytes --------------------------------------------------------------------------------------------

def gn_row():
    B, C0, C1, H, W, groups, act = 2, 8, 16, 5, 7, 4, 2          # a group straddles the two sources; odd pixel count
    Cc, HW = C0 + C1, H * W

    def build():
        x = rand(B, Cc, H, W, seed=11) * 1.5 + 0.3
        gamma, beta = rand(Cc, seed=12) * 0.3 + 1.0, rand(Cc, seed=13) * 0.3
        dA = rand(B, Cc, H, W, seed=14)
        xg = x.double().reshape(B, groups, -1)
        mean, rstd = xg.mean(2), 1.0 / torch.sqrt(xg.var(2, unbiased=False) + 1e-5)
        cpg = Cc // groups
        scale = rstd.repeat_interleave(cpg, 1) * gamma.double()[None]
        shift = beta.double()[None] - mean.repeat_interleave(cpg, 1) * scale
        ss, mr = torch.stack([scale, shift], 2).float().contiguous(), torch.stack([mean, rstd], 2).float().contiguous()

        def call(lib, P, scratch, nbytes, stream):
            return lib.sr3_groupnorm_act_bwd_f32(P['dA'], P['x0'], C0, P['x1'], C1, B, HW, P['ss'], P['mr'], groups, act, P['gamma'], 0, 0.0,
                                                 P['dgamma'], P['dbeta'], P['dx0'], 0, P['dx1'], 0, P['aout'], scratch, nbytes, stream)

        def autograd(dtype):
            xs, gs, bs = (t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
            u = F.group_norm(xs, groups, gs, bs, eps=1e-5)
            u.retain_grad()
            a = u * torch.sigmoid(u)
            (a * dA.to(dtype)).sum().backward()
            return dict(dx0=xs.grad[:, :C0], dx1=xs.grad[:, C0:], dgamma=gs.grad, dbeta=bs.grad, aout=a.detach(), dA=u.grad)

        def check(got):
            # the bound of test_groupnorm_act_backward: at most twice the normwise error of torch's own fp32 CPU autograd
            ref, cmp32 = autograd(torch.float64), autograd(torch.float32)
            for key in ref:
                g_ = got[key] if got[key].dim() == 1 else nchw(got[key])
                e_k, e_c = relerr(g_, ref[key]), relerr(cmp32[key], ref[key])
                assert e_k <= 2.0 * e_c, (key, e_k, e_c)
        outs = {'dA': nhwc(dA), 'dgamma': ((Cc,), torch.float32), 'dbeta': ((Cc,), torch.float32), 'dx0': ((B, H, W, C0), torch.float32),
                'dx1': ((B, H, W, C1), torch.float32), 'aout': ((B, H, W, Cc), torch.float32)}
        return dict(ins={'x0': nhwc(x[:, :C0]), 'x1': nhwc(x[:, C0:]), 'ss': ss, 'mr': mr, 'gamma': gamma}, outs=outs, call=call, check=check,
                    query=lambda lib: int(lib.sr3_groupnorm_act_bwd_scratch_bytes(B, HW, Cc, groups)))
    return Row('groupnorm_act_bwd', 'sr3_groupnorm_act_bwd_scratch_bytes', 'sr3_groupnorm_act_bwd_f32', build, align=8)


# ---- sr3_attention_bwd_scratch_bytes: the slab form (the atomics form, sr3_attention_bwd_f32, takes no scratch and is not
# bit-reproducible) ----------------------------------------------------------------------------------------------------------------

def attn_bwd_row():
    B, N, Cc = 2, 100, 48          # four query blocks, the last ragged

    def build():
        qkv, dout = rand(B, N, 3 * Cc, seed=11) * 2.0, rand(B, N, Cc, seed=12)

        def call(lib, P, scratch, nbytes, stream):
            return lib.sr3_attention_bwd_ex_f32(P['qkv'], P['dout'], None, B, N, Cc, P['dqkv'], scratch, nbytes, stream)

        def check(got):
            x = qkv.double().requires_grad_(True)
            q, k, v = x.split(Cc, dim=2)
            (torch.softmax(q @ k.transpose(1, 2) / math.sqrt(Cc), -1) @ v).backward(dout.double())
            for name, sl in (('dq', slice(0, Cc)), ('dk', slice(Cc, 2 * Cc)), ('dv', slice(2 * Cc, 3 * Cc))):
                r, g_ = x.grad[:, :, sl], got['dqkv'].double()[:, :, sl]
                assert (g_ - r).norm() / r.norm() < 2e-5, name
                assert (g_ - r).abs().max() <= 1e-4 * max(1.0, float(r.abs().max())), name
        return dict(ins={'qkv': qkv, 'dout': dout}, outs={'dqkv': ((B, N, 3 * Cc), torch.float32)}, call=call, check=check,
                    expect=-(-N // 32) * B * N * 2 * Cc * 4, query=lambda lib: int(lib.sr3_attention_bwd_scratch_bytes(B, N, Cc)))
    return Row('attention_bwd_ex', 'sr3_attention_bwd_scratch_bytes', 'sr3_attention_bwd_ex_f32', build, align=16)


# ---- sr3_colsums_scratch_bytes ------------------------------------------------------------------------------------------------------

def colsums_row():
    B, HW, Cc = 2, 1024, 64          # several pixel slices per image

    def build():
        g = rand(B, HW, Cc, seed=31) + 0.25

        def call(lib, P, scratch, nbytes, stream):
            return lib.sr3_colsums_f32(P['g'], B, HW, Cc, P['dbias'], P['dfilm'], Cc, scratch, nbytes, stream)

        def check(got):
            gg = g.double()
            for key, ref, mag in (('dbias', gg.sum((0, 1)), gg.abs().sum((0, 1))), ('dfilm', gg.sum(1), gg.abs().sum(1))):
                err = (got[key].double() - ref).abs()
                assert bool((err <= 2.0 ** -24 * ref.abs() + 1e-12 * mag).all()), key
        return dict(ins={'g': g}, outs={'dbias': ((Cc,), torch.float32), 'dfilm': ((B, Cc), torch.float32)}, call=call, check=check,
                    query=lambda lib: int(lib.sr3_colsums_scratch_bytes(B, HW, Cc)))
    return Row('colsums', 'sr3_colsums_scratch_bytes', 'sr3_colsums_f32', build, align=8)


# ---- sr3_embed_bwd_scratch_bytes ----------------------------------------------------------------------------------------------------

def embed_bwd_row():
    B, inner, Fn = 3, 64, 1000

    def build():
        w1, b1 = rand(4 * inner, inner, seed=1) * 0.1, rand(4 * inner, seed=2) * 0.1
        w2, b2 = rand(inner, 4 * inner, seed=3) * 0.1, rand(inner, seed=4) * 0.1
        wf = rand(Fn, inner, seed=5) * 0.1
        dfilm = rand(B, Fn, seed=7)
        level = torch.tensor([0.999, 0.5, 0.013])
        count = inner // 2
        freq = torch.exp(-math.log(1e4) * (torch.arange(count, dtype=torch.float32) / count))
        names = ('dw1', 'db1', 'dw2', 'db2', 'dwf', 'dbf')

        def call(lib, P, scratch, nbytes, stream):
            return lib.sr3_embed_bwd_f32(0, B, inner, Fn, P['level'], None, P['freq'], P['w1'], P['b1'], P['w2'], P['b2'], P['wf'], P['dfilm'],
                                         *[P[n] for n in names], scratch, nbytes, stream)

        def check(got):
            arg = level[:, None] * freq[None]
            enc = torch.cat([arg.sin(), arg.cos()], -1).double()
            Pm = [t.double().clone().requires_grad_(True) for t in (w1, b1, w2, b2, wf, torch.zeros(Fn))]
            h = enc @ Pm[0].t() + Pm[1]
            h = h * torch.sigmoid(h)
            ((((h @ Pm[2].t() + Pm[3]) @ Pm[4].t()) + Pm[5]) * dfilm.double()).sum().backward()
            for n, p in zip(names, Pm):
                assert relerr(got[n], p.grad) <= 2e-6, n
        outs = {n: (tuple(t.shape), torch.float32) for n, t in zip(names, (w1, b1, w2, b2, wf, torch.zeros(Fn)))}
        return dict(ins=dict(level=level, freq=freq, w1=w1, b1=b1, w2=w2, b2=b2, wf=wf, dfilm=dfilm), outs=outs, call=call, check=check,
                    expect=B * 29 * inner * 4, query=lambda lib: int(lib.sr3_embed_bwd_scratch_bytes(B, inner)))
    return Row('embed_bwd', 'sr3_embed_bwd_scratch_bytes', 'sr3_embed_bwd_f32', build, align=4)


# ---- sr3_loss_grad_scratch_bytes / sr3_hybrid_loss_grad_scratch_bytes: constant-size scratch, no byte count argument ----------------

def loss_grad_row():
    B, Cc, H, W, scale = 3, 3, 160, 160, 2.0 ** -10          # 76 800 pixels over 65 536 threads: a second, ragged trip; a pad lane

    def build():
        gen = torch.Generator().manual_seed(1160)
        z, hr = torch.randn(B, Cc, H, W, generator=gen), torch.rand(B, Cc, H, W, generator=gen) * 2 - 1
        e = torch.randn(B, Cc, H, W, generator=gen) * 0.8
        ta, tb, w = torch.tensor([0.9, 0.5, 0.2]), torch.tensor([-0.4, -0.85, 0.97]), torch.tensor([0.75, 1.5, 0.375])

        def call(lib, P, scratch, nbytes, stream):
            return lib.sr3_loss_grad_f32(P['z'], P['e'], P['hr'], P['ta'], P['tb'], P['w'], B, Cc, H * W, 1, 0.0, scale, P['g'], P['loss'], scratch,
                                         stream)

        def check(got):
            # the L2 bound of tests/test_gpu_objective_ops.py: 4 * 2^-23 S w scale c with c = 2, the loss relative 1e-6
            bc = lambda t: t.double().view(B, 1, 1, 1)
            d = bc(ta) * z.double() + bc(tb) * hr.double() - e.double()
            S = (bc(ta) * z.double()).abs() + (bc(tb) * hr.double()).abs() + e.double().abs()
            g = got['g']
            assert bool((g[:, :, Cc:] == 0).all()), 'pad lanes must be written 0'
            gg = g[:, :, :Cc].reshape(B, H, W, Cc).permute(0, 3, 1, 2).double()
            assert bool(((gg + bc(w) * 2 * d * scale).abs() <= 4 * 2.0 ** -23 * S * bc(w) * scale * 2.0).all())
            ref = (bc(w) * d * d).sum().item()
            assert abs(float(got['loss']) - ref) <= 1e-6 * abs(ref)
        return dict(ins=dict(z=z, e=e, hr=hr, ta=ta, tb=tb, w=w), outs={'g': ((B, H * W, 4), torch.float32), 'loss': ((1,), torch.float32)},
                    call=call, check=check, query=lambda lib: int(lib.sr3_loss_grad_scratch_bytes()))
    return Row('loss_grad', 'sr3_loss_grad_scratch_bytes', 'sr3_loss_grad_f32', build, align=8, small=None)


def hybrid_loss_row():
    lam, scale = 0.5, 0.125

    def build():
        from test_learned_var_cpu import loss_inputs
        d = loss_inputs()
        B, C2, H, W = d['out'].shape
        Cc, HW = C2 // 2, H * W

        def call(lib, P, scratch, nbytes, stream):
            return lib.sr3_hybrid_loss_grad_f32(P['z'], P['out'], P['hr'], P['xt'], None, None, None, P['scal32'], lam, B, Cc, HW, 1, 0.0, scale,
                                                P['g8'], P['loss'], P['vlb'], scratch, stream)

        def check(got):
            # tests/test_gpu_learned_var.py::test_hybrid_loss_kernel's float64 reference and tolerances (TOL_DV 6.6e-6, TOL_SUM 4.5e-7)
            import learned_var_ref as R
            out = d['out'].double().clone().requires_grad_(True)
            tot, vsum = R.hybrid_loss(d['z'], d['hr'], d['xt'], out, d['scal32'].double(), lam, kind='l2', delta=0.0, tgt=None, weight=None)
            gref, = torch.autograd.grad(vsum, [out])
            dv_ref = gref[:, Cc:].reshape(B, Cc, HW).permute(0, 2, 1)
            dv = got['g8'][:, :, Cc:2 * Cc].double() / (lam * scale)
            assert not got['g8'][:, :, 2 * Cc:].any()
            assert ((dv - dv_ref).abs() / dv_ref.abs().clamp(min=1.0)).max().item() <= 6.6e-6
            tot, vsum = float(tot.detach()), float(vsum.detach())
            assert abs(float(got['loss']) - tot) <= 4.5e-7 * abs(tot) and abs(float(got['vlb']) - vsum) <= 4.5e-7 * abs(vsum)
        return dict(ins={k: d[k].contiguous() for k in ('z', 'out', 'hr', 'xt', 'scal32')},
                    outs={'g8': ((B, HW, 8), torch.float32), 'loss': ((1,), torch.float32), 'vlb': ((1,), torch.float32)}, call=call, check=check,
                    query=lambda lib: int(lib.sr3_hybrid_loss_grad_scratch_bytes()))
    return Row('hybrid_loss_grad', 'sr3_hybrid_loss_grad_scratch_bytes', 'sr3_hybrid_loss_grad_f32', build, align=8, small=None)


# ---- sr3_abs_quantile_scratch_bytes (the select of the guided step's dynamic thresholding) ------------------------------------------

def abs_quantile_row():
    B, n = 2, 65537          # more than one block per image, an odd length

    def build():
        import numpy as np
        from sr3_hip.diffusion import quantile_rank
        g = np.random.default_rng(31 * B + n)
        v = (g.standard_normal((B, n)) * np.exp(3.0 * g.standard_normal((B, n)))).astype(np.float32)          # heavy-tailed
        rank_lo, frac = quantile_rank(n, 0.995)

        def call(lib, P, scratch, nbytes, stream):
            return lib.sr3_abs_quantile_f32(P['v'], B, n, rank_lo, frac, P['out'], scratch, nbytes, stream)

        def check(got):          # tests/test_gpu_guidance.py: the same bits as the oracle
            from test_guidance_cpu import oracle_quantile
            assert got['out'].numpy().tobytes() == oracle_quantile(v, rank_lo, frac).tobytes()
        return dict(ins={'v': torch.from_numpy(v)}, outs={'out': ((B,), torch.float32)}, call=call, check=check,
                    query=lambda lib: int(lib.sr3_abs_quantile_scratch_bytes(B, n)))
    return Row('abs_quantile', 'sr3_abs_quantile_scratch_bytes', 'sr3_abs_quantile_f32', build, align=4, small=BADARG)


# ---- sr3_backproject_scratch_bytes --------------------------------------------------------------------------------------------------

def backproject_row():
    shape, s, iters, lam, j = (2, 3, 24, 40), 8, 3, 0.5, 2          # 33 taps with clipped borders, an LR width that is no multiple of 4

    def build():
        import numpy as np
        from test_backprojection_cpu import KEYS, oracle_backproject_step, tables_2d
        B, Cc, H, W = shape
        g = np.random.default_rng(1000 * s + sum(shape))
        x, eps, z, h = (torch.from_numpy(g.standard_normal(shape).astype(np.float32)) for _ in range(4))
        y = torch.from_numpy(g.uniform(-1.0, 1.0, (B, Cc, H // s, W // s)).astype(np.float32))
        down, up = tables_2d((H, W), (H // s, W // s), 'bicubic'), tables_2d((H // s, W // s), (H, W), 'bicubic')
        tabs = dict(a=[1.1, 0.7, 0.9, 0.6], b=[0.2, 0.75, 0.43, 0.7], c1=[1.0, 0.45, 0.55, 0.4], c2=[0.0, 0.5, 0.45, -0.2],
                    sigma=[0.0, 0.4, 0.5, 0.25], c3=[0.0, -0.35, 0.5, -0.45])
        tabs = {k: np.asarray(v, dtype=np.float32) for k, v in tabs.items()}
        ins = dict(eps=eps, z=z, y=y, c3=torch.from_numpy(tabs['c3']))
        for k in KEYS:
            ins['tab_' + k] = torch.from_numpy(tabs[k])
        axes = []
        for side, tb in (('d', down), ('u', up)):
            for i, t in enumerate(tb):
                ins['%s%d' % (side, i)] = torch.from_numpy(np.ascontiguousarray(t))
            axes.append((side, tb[1].shape[1], tb[3].shape[1]))

        def call(lib, P, scratch, nbytes, stream):
            ax = []
            for side, kh, kv in axes:
                ax += [P[side + '0'], P[side + '1'], kh, P[side + '2'], P[side + '3'], kv]
            return lib.sr3_backproject_step(P['x'], P['eps'], P['z'], P['y'], B, Cc, H, W, s, iters, lam, *ax, *[P['tab_' + k] for k in KEYS],
                                            P['step2'], 1, P['c3'], P['hist'], scratch, nbytes, stream)

        def check(got):
            # tests/test_gpu_backprojection.py's gate: |got - oracle| <= 4 * 2^-23 * max(1, |oracle|) per element
            wx, wx0 = oracle_backproject_step(x.numpy(), eps.numpy(), z.numpy(), y.numpy(), down, up, lam, iters, tabs, j, 1, h.numpy())
            for key, want in (('x', wx), ('hist', wx0)):
                diff = np.abs(got[key].numpy().astype(np.float64) - want.astype(np.float64))
                assert np.all(diff <= 4.0 * 2.0 ** -23 * np.maximum(1.0, np.abs(want.astype(np.float64)))), key
            assert got['step2'].tolist() == [j, j - 1]
        return dict(ins=ins, outs={'x': x, 'hist': h, 'step2': torch.tensor([-7, j], dtype=torch.int32)}, call=call, check=check,
                    query=lambda lib: int(lib.sr3_backproject_scratch_bytes(B, Cc, H, W, s)))
    return Row('backproject_step', 'sr3_backproject_scratch_bytes', 'sr3_backproject_step', build, align=4, small=BADARG)


# ---- the uint8 image entries: sr3_resize_scratch_bytes, sr3_jpeg_scratch_bytes, sr3_ssim_scratch_bytes, sr3_eval_scratch_bytes -------

def _images(n, H, W, Cc, seed):
    import numpy as np
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, size=(n, H, W, Cc)).astype(np.uint8)
    b = np.clip(a.astype(np.int32) + rng.randint(-30, 31, size=a.shape), 0, 255).astype(np.uint8)
    return a, b


def resize_row():
    n, H, W, Cc, OH, OW = 2, 37, 50, 3, 9, 12

    def build():
        a, _ = _images(n, H, W, Cc, 7)

        def call(lib, P, scratch, nbytes, stream):
            return lib.sr3_resize_u8(P['in'], n, H, W, Cc, OH, OW, 3, scratch, nbytes, P['out'], stream)

        def check(got):          # bit-exact with the restatement of Pillow's ImagingResample (oracle/io_metrics_oracle.py)
            from oracle import io_metrics_oracle as IO
            for i in range(n):
                assert (got['out'][i].numpy() == IO.pil_resize(a[i], (OH, OW), cubic=True)).all(), i
        return dict(ins={'in': torch.from_numpy(a)}, outs={'out': ((n, OH, OW, Cc), torch.uint8)}, call=call, check=check,
                    query=lambda lib: int(lib.sr3_resize_scratch_bytes(n, H, W, Cc, OH, OW)))
    return Row('resize_u8', 'sr3_resize_scratch_bytes', 'sr3_resize_u8', build, align=256)


def jpeg_row():
    n, H, W, Cc, sub = 2, 21, 35, 3, 2          # 4:2:0 on a map that is no multiple of 16: every padding rule

    def build():
        a, _ = _images(n, H, W, Cc, 11)
        a = (a // 3 + a[:, :1, :1] // 2).astype(a.dtype)          # (some smooth structure survives the quantiser)
        q = [35, 90]

        def call(lib, P, scratch, nbytes, stream):
            return lib.sr3_jpeg_u8(P['in'], n, H, W, Cc, P['q'], sub, P['out'], scratch, nbytes, stream)

        def check(got):          # bit-exact with the NumPy restatement of libjpeg's round trip (tests/test_jpeg_cpu.py)
            from test_jpeg_cpu import jpeg_oracle
            for i in range(n):
                assert (got['out'][i].numpy() == jpeg_oracle(a[i], q[i], sub)).all(), i
        return dict(ins={'in': torch.from_numpy(a), 'q': torch.tensor(q, dtype=torch.int32)}, outs={'out': ((n, H, W, Cc), torch.uint8)}, call=call,
                    check=check, query=lambda lib: int(lib.sr3_jpeg_scratch_bytes(n, H, W, Cc, sub)))
    return Row('jpeg_u8', 'sr3_jpeg_scratch_bytes', 'sr3_jpeg_u8', build, align=0, small=BADARG)


def ssim_row(fused):
    n, H, W, Cc = 2, 37, 50, 3

    def build():
        from oracle import io_metrics_oracle as IO
        a, b = _images(n, H, W, Cc, 13)
        if fused:          # the validation chain on fp32 NCHW in [-1, 1] (leaving it: the clamp of tensor2img)
            gen = torch.Generator().manual_seed(9)
            hr = torch.rand(n, Cc, H, W, generator=gen) * 2 - 1
            sr = hr + 0.08 * torch.randn(n, Cc, H, W, generator=gen)
            ins = {'sr': sr, 'hr': hr}
            pairs = lambda: [(IO.tensor2img(sr[i].numpy()), IO.tensor2img(hr[i].numpy())) for i in range(n)]
            outs = {'sse': ((n,), torch.int64), 'ssim': ((n,), torch.float64)}
            query = lambda lib: int(lib.sr3_eval_scratch_bytes(n, Cc, H, W))
        else:
            ins = {'a': torch.from_numpy(a), 'b': torch.from_numpy(b)}
            pairs = lambda: [(a[i], b[i]) for i in range(n)]
            outs = {'ssim': ((n,), torch.float64)}
            query = lambda lib: int(lib.sr3_ssim_scratch_bytes(n, H, W, Cc))

        def call(lib, P, scratch, nbytes, stream):
            if fused:
                return lib.sr3_eval_psnr_ssim_f32(P['sr'], P['hr'], n, Cc, H, W, -1.0, 1.0, scratch, nbytes, P['sse'], P['ssim'], stream)
            return lib.sr3_ssim_u8(P['a'], P['b'], n, H, W, Cc, scratch, nbytes, P['ssim'], stream)

        def check(got):          # tests/test_gpu_io.py: SSIM rel 1e-10 against the oracle, the squared error exact
            import numpy as np
            for i, (u, v) in enumerate(pairs()):
                ref = IO.calculate_ssim(u, v)
                assert abs(float(got['ssim'][i]) - ref) <= 1e-10 * abs(ref), i
                if fused:
                    assert int(got['sse'][i]) == int(((u.astype(np.int64) - v.astype(np.int64)) ** 2).sum()), i
        return dict(ins=ins, outs=outs, call=call, check=check, query=query)
    return Row('eval_psnr_ssim' if fused else 'ssim_u8', 'sr3_eval_scratch_bytes' if fused else 'sr3_ssim_scratch_bytes',
               'sr3_eval_psnr_ssim_f32' if fused else 'sr3_ssim_u8', build, align=8)


# ---- sr3_grad_norm_scratch_bytes: sr3_grad_norm, sr3_grad_accumulate ----------------------------------------------------------------

def grad_norm_row(accumulate):
    n, max_norm = 2 ** 20 + 4, 1.0

    def build():
        gen = torch.Generator().manual_seed(5)
        g = torch.randn(n, generator=gen) * 10.0 ** (torch.rand(n, generator=gen) * 8 - 6)          # eight decades of magnitudes
        a = torch.randn(n, generator=gen)

        def call(lib, P, scratch, nbytes, stream):
            if accumulate:
                return lib.sr3_grad_accumulate(P['acc'], P['g'], n, 0, max_norm, scratch, nbytes, P['out4'], stream)
            return lib.sr3_grad_norm(P['g'], n, max_norm, scratch, nbytes, P['out4'], stream)

        def check(got):
            v = (a + g) if accumulate else g
            if accumulate:
                assert torch.equal(got['acc'], v)
            ref = float(v.double().norm())
            o = got['out4']
            assert abs(float(o[0]) - ref) <= 2.0 ** -22 * ref and float(o[2]) == 1.0 and float(o[3]) == 0.0
            assert abs(float(o[1]) - min(1.0, max_norm / (ref + 1e-6))) <= 2.0 ** -22
        outs = {'out4': ((4,), torch.float32)}
        if accumulate:
            outs['acc'] = a
        return dict(ins={'g': g}, outs=outs, call=call, check=check, query=lambda lib: int(lib.sr3_grad_norm_scratch_bytes(n)))
    return Row('grad_accumulate' if accumulate else 'grad_norm', 'sr3_grad_norm_scratch_bytes', 'sr3_grad_accumulate' if accumulate else 'sr3_grad_norm',
               build, align=8, small=BADARG)


ROWS = [
    # tile_cfg, ksplit | B, H, W, Cin -> Cout, k: the smallest shapes at which each conv kernel family has something in scratch
    conv_row(11, 1, 1, 16, 16, 64, 64, 3, expect=262144), conv_row(11, 2, 1, 16, 16, 64, 64, 3, expect=393216),
    conv_row(12, 2, 1, 16, 16, 64, 64, 3, expect=524288), conv_row(12, 2, 4, 8, 8, 64, 64, 3, expect=524288),          # (the four-image tile)
    conv_row(13, 1, 1, 8, 16, 64, 64, 3, expect=393216), conv_row(13, 2, 1, 8, 16, 64, 64, 3, expect=458752),
    conv_row(13, 2, 1, 4, 8, 64, 64, 3, ups=1, tag='_up'), conv_row(25, 2, 1, 4, 8, 64, 64, 3, ups=1, tag='_up'),
    conv_row(23, 2, 1, 10, 24, 64, 64, 3, expect=516096),
    conv_row(22, 1, 1, 8, 8, 64, 128, 1, expect=49152), conv_row(22, 2, 1, 8, 8, 64, 128, 1, expect=114688),
    conv_row(22, 2, 1, 16, 16, 64, 128, 3, stride=2, expect=507904),
    conv_row(16, 2, 1, 8, 8, 64, 64, 1, expect=32768), conv_row(18, 1, 1, 8, 8, 64, 64, 1, expect=24576), conv_row(20, 2, 1, 8, 8, 64, 64, 1, expect=57344),
    conv_row(3, 2, 1, 8, 8, 32, 64, 3, expect=32768), conv_row(5, 2, 1, 8, 8, 64, 64, 3, expect=32768),
    # the fused res_conv segment under split-K: one x2 source on an 8 x 8 map, a concat x2 source over several tiles
    block_conv_row(5, 2, 1, 8, 8, 64, 64, 64, 0), block_conv_row(5, 2, 2, 16, 16, 64, 128, 96, 32),
    conv_dropout_row(11, 2, 1, 16, 16, 64, 64), conv_dropout_row(12, 2, 1, 16, 16, 64, 64),
    # one shape per kernel of wgrad.hip at which msplit > 1 (wgrad_pick)
    wgrad_row('fp32_64x64_tile', 2, 16, 16, 1, 64, 64, 0, 4), wgrad_row('fp32_128x128_tile', 2, 16, 16, 1, 128, 128, 0, 4),
    wgrad_row('split_kernel', 2, 16, 16, 1, 128, 128, 1, 4), wgrad_row('nine_tap_kernel', 2, 8, 24, 3, 64, 64, 1, 6),
    dgrad_row('winograd', {}, 1, 16, 16, 32, 32, 3, 1, 13, 2, None), dgrad_row('gemm_tile22_slabs', {}, 1, 8, 8, 128, 256, 1, 1, 22, 3, True),
    dgrad_row('stride2_zero_insert', {}, 2, 16, 24, 16, 16, 3, 2, 3, 0, None),
    gn_row(), attn_bwd_row(), colsums_row(), embed_bwd_row(), loss_grad_row(), hybrid_loss_row(), grad_norm_row(False), grad_norm_row(True),
    abs_quantile_row(), backproject_row(), resize_row(), jpeg_row(), ssim_row(False), ssim_row(True),
]
