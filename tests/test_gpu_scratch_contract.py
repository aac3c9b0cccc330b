"""The scratch contract of the per-op entries: every row of tests/scratch_rows.py -- one per launch that consumes a `*_scratch_bytes`
query -- runs in a guarded scratch (tests/guarded.py) of exactly the queried size under three fills (zeros, NaN patterns, a large
finite pattern), its inputs in guarded buffers with NaN bands and its outputs NaN-filled and guarded.  Per row: rc 0, outputs finite and
BIT-equal across the fills, every band intact, and once the float64 / oracle comparison the op's own test makes, at that test's
tolerance.  A scratch smaller than the query is never passed here (tests/test_scratch_contract_cpu.py checks those refusals without a
device)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_util as G                                             # noqa: E402
import guarded as GD                                             # noqa: E402
from guarded import same_bits                                    # noqa: E402
from scratch_rows import ROWS                                    # noqa: E402
from sr3_hip import lib as L                                     # noqa: E402


@pytest.mark.parametrize('row', ROWS, ids=[r.id for r in ROWS])
def test_per_op_scratch_contract(row):
    GD.run_row(row, L.load(), G.dev(), G.stream(), fills=GD.FILLS, operands=False)          # (shared with tests/test_gpu_edge_operands.py)


@pytest.mark.parametrize('tile_cfg,ksplit', [(13, 2), (12, 2), (22, 2)])
def test_fused_conv_epilogue_in_a_guarded_scratch(tile_cfg, ksplit):
    """gpu_util.conv_call (the helper behind the conv tests) with guard=: two sources, GroupNorm + SiLU prologue (affine alone on the
    GEMM tile), FiLM, bias, a concat residual and fused statistics, in a scratch of exactly the queried size between 1 MiB bands."""
    gen = lambda *shape, seed: torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    B, C0, C1, H, W, Cout = 2, 32, 32, 16, 16, 64
    k = 1 if tile_cfg == 22 else 3
    kw = dict(bias=gen(Cout, seed=3) * 0.1, ss=torch.stack([1 + 0.1 * gen(B, C0 + C1, seed=4), 0.1 * gen(B, C0 + C1, seed=5)], 2),
              act=1 if tile_cfg == 22 else 2, film=gen(B, Cout, seed=6), res0=gen(B, 32, H, W, seed=7), res1=gen(B, 32, H, W, seed=8))
    src0, src1 = gen(B, C0, H, W, seed=1), gen(B, C1, H, W, seed=2)
    w = gen(Cout, C0 + C1, k, k, seed=9) / (3.0 * (C0 + C1) ** 0.5)
    ref = G.conv_ref(src0, src1, w, **kw)
    outs = [G.conv_call(src0, src1, w, tile_cfg=tile_cfg, ksplit=ksplit, want_stats=True, guard=byte, **kw) for _, byte in GD.FILLS]
    G.assert_close(outs[0][0], ref, what='conv tile %d' % tile_cfg)
    for (name, _), (out, st) in zip(GD.FILLS[1:], outs[1:]):
        assert same_bits(out, outs[0][0]) and same_bits(st, outs[0][1]), 'scratch fill %s changes the result' % name
