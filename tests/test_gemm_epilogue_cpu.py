"""Plan option gemm_epi on the host (no GPU): the epilogue form of the plain GEMM kernel (csrc/gemm1x1.hip) is a launch-time switch with
the range 0 .. 2 -- the launch list, the workspace and the derived buffer do not depend on it, the ops keep reporting tile 22 -- and it
did not widen store_wt."""
import ctypes as C

import pytest


def _plan():
    from sr3_hip import engine as E
    return E.Plan('sr3', 6, 3, 64, 32, [1, 2, 4, 8, 8], [16], 2, 128)


def test_gemm_epi_range_and_previous_value():
    from sr3_hip import lib as L
    p = _plan()
    first = p.set_option('gemm_epi', 0)
    assert first in (0, 1, 2)                            # the default: whatever form measured best
    assert p.set_option('gemm_epi', 1) == 0 and p.set_option('gemm_epi', 2) == 1 and p.set_option('gemm_epi', 0) == 2
    for bad in (-1, 3):
        with pytest.raises(L.Sr3Error, match='gemm_epi'):
            p.set_option('gemm_epi', bad)
        assert p.set_option('gemm_epi', 0) == 0          # a refused value changed nothing
    p.set_option('gemm_epi', 2)
    with pytest.raises(L.Sr3Error, match='gemm_epi'):
        p.set_option('gemm_epi', 3)
    assert p.set_option('gemm_epi', first) == 2


def test_gemm_epi_leaves_the_plan_alone_and_ops_report_tile_22():
    p = _plan()
    derived = lambda: int(p.lib.sr3_plan_derived_bytes(p.handle))
    seen = []
    for form in (0, 1, 2):
        p.set_option('gemm_epi', form)
        seen.append((p.op_list(16), p.workspace_bytes(16), derived()))
    assert seen[0] == seen[1] == seen[2]
    convs = [o for o in seen[0][0] if o['kind'] == 50]
    gemm = [o for o in convs if o['tile_cfg'] == 22]
    assert len(gemm) == 34                               # every 1x1 and stride-2 conv of the flagship network
    assert any(o['ksize'] == 1 for o in gemm) and any(o['ksize'] == 3 and o['stride'] == 2 for o in gemm)
    assert not any(o['tile_cfg'] in (27, 28, 29) for o in convs)     # the explicit forms are names of the per-op ABI only


def test_store_wt_still_refuses_8():
    from sr3_hip import lib as L
    p = _plan()
    prev = p.set_option('store_wt', 7)
    with pytest.raises(L.Sr3Error, match='store_wt'):
        p.set_option('store_wt', 8)
    assert p.set_option('store_wt', prev) == 7


def test_gemm_tile_query():
    """sr3_gemm_tile: the (rows, cols) of the workgroup tile per shape -- what tests/test_gpu_gemm_epilogue.py pins its cases with."""
    from sr3_hip import lib as L
    lib = L.load()

    def tile(B, Ho, Wo, Cin, Cout, k):
        r, c = C.c_int(-1), C.c_int(-1)
        ok = lib.sr3_gemm_tile(B, Ho, Wo, Cin, Cout, k, C.byref(r), C.byref(c))
        return (r.value, c.value) if ok else None

    assert tile(1, 4, 8, 32, 128, 1) == (32, 128) and tile(2, 4, 8, 64, 256, 1) == (32, 128)
    assert tile(2, 32, 32, 544, 128, 1) == (64, 128)
    assert tile(1, 8, 8, 32, 64, 1) == (64, 64) and tile(1, 8, 8, 32, 192, 1) == (64, 64)
    assert tile(2, 4, 8, 32, 128, 3) == (32, 128) and tile(2, 4, 8, 32, 64, 3) == (64, 64) and tile(6, 32, 32, 32, 512, 3) == (64, 128)
    assert tile(1, 4, 8, 32, 96, 1) is None and tile(1, 4, 8, 24, 128, 1) is None and tile(1, 4, 4, 32, 128, 1) is None
    assert tile(1, 4, 8, 32, 128, 5) is None
    assert lib.sr3_gemm_tile(1, 4, 8, 32, 128, 1, None, None) == 1
