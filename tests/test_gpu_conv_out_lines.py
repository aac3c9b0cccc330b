"""k_conv_out_nchw (csrc/small_kernels.hip) stages its input per chunk of channels -- 16, half a 128-byte line of a pixel's row, or with
-DSR3_CONV_OUT_LINES 32, a whole line; either way it accumulates per 16-channel sub-chunk in ascending order.  sr3_conv_out_f32 against
float64 at channel counts on every side of both chunk sizes (16: one 16-chunk, a partial 32-chunk; 24: a partial sub-chunk; 48: one and a
half 32-chunks; 64: two; 96: three), at 3, 4 and 6 output rows, on one tile, on a map that overhangs the 8 x 32 tile to the right and below,
and on four tiles.  The default build runs the 16-channel chunk; the 32-channel one is checked by running this file against the variant
library (the recipe is in tools/build_variant.sh).  Input and output sit in guarded tensors: a read past the input is a NaN in the result, a write past the output breaks a band."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_util as G                                # noqa: E402
from guarded import tensor_in, tensor_out           # noqa: E402
from sr3_hip import lib as L                        # noqa: E402

B = 2
MAPS = [(8, 32), (10, 36), (16, 64)]


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize('H,W', MAPS, ids=['%dx%d' % m for m in MAPS])
@pytest.mark.parametrize('Cout', [3, 4, 6])
@pytest.mark.parametrize('Cc', [16, 24, 48, 64, 96])
def test_conv_out_chunk_boundaries(Cc, Cout, H, W):
    lib = L.load()
    d = G.dev()
    x = _rand(B, Cc, H, W, seed=1)
    ss = torch.stack([_rand(B, Cc, seed=2) * 0.3 + 1.0, _rand(B, Cc, seed=3) * 0.3], dim=2).contiguous()
    w = _rand(Cout, Cc, 3, 3, seed=4) * 0.1
    bias = _rand(Cout, seed=5)
    gx, xd = tensor_in(G.nhwc(x), d)
    gw, wd = tensor_in(G.ohwi(w), d)
    go, out = tensor_out((B, Cout, H, W), d)
    ssd, biasd = ss.to(d), bias.to(d)
    L.check(lib.sr3_conv_out_f32(L.ptr(xd), L.ptr(ssd), B, H, W, Cc, L.ptr(wd), L.ptr(biasd), Cout, L.ptr(out), G.stream()))
    torch.cuda.synchronize()
    assert gx.intact() and gw.intact() and go.intact(), 'conv_out wrote outside its output'
    got = out.cpu()
    assert bool(torch.isfinite(got).all())
    ref = G.conv_ref(x, None, w, bias=bias, ss=ss, act=2)
    err = G.assert_close(got, ref, what='conv_out C %d Cout %d %dx%d' % (Cc, Cout, H, W))
    print('conv_out C %d Cout %d %dx%d: max abs err %.3e' % (Cc, Cout, H, W, err))
