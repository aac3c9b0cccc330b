"""Plan option store_wt on the host (no GPU): the 4 GiB guard of the write-through buffer stores (32-bit offsets), the option's range,
and that it is a launch-time switch -- the launch list, the workspace and the derived buffer do not depend on it."""
import pytest


def test_write_through_guard_is_4_gib():
    from sr3_hip import lib as L
    lib = L.load()
    assert lib.sr3_store_wt_fits(0) == 1 and lib.sr3_store_wt_fits(16) == 1
    assert lib.sr3_store_wt_fits((1 << 32) - 1) == 1
    assert lib.sr3_store_wt_fits(1 << 32) == 0          # the first size a 32-bit byte offset cannot cover
    assert lib.sr3_store_wt_fits((1 << 32) + 16) == 0 and lib.sr3_store_wt_fits(1 << 40) == 0
    # the flagship's largest output (batch 16, 128 x 128, 64 channels) and its largest slab set are far below it
    assert lib.sr3_store_wt_fits(16 * 128 * 128 * 64 * 4) == 1


def test_store_wt_is_a_mask_and_leaves_the_plan_alone():
    from sr3_hip import engine as E, lib as L
    p = E.Plan('sr3', 6, 3, 64, 32, [1, 2, 4, 8, 8], [16], 2, 128)
    derived = lambda: int(p.lib.sr3_plan_derived_bytes(p.handle))
    ops, ws, der = p.op_list(16), p.workspace_bytes(16), derived()
    prev = p.set_option('store_wt', 0)
    assert 0 <= prev <= 7                                # the default: whatever mask measured best
    for mask in (1, 2, 4, 7, 0):
        p.set_option('store_wt', mask)
        assert p.op_list(16) == ops and p.workspace_bytes(16) == ws and derived() == der
    assert p.set_option('store_wt', 5) == 0 and p.set_option('store_wt', prev) == 5      # returns the previous value
    for bad in (-1, 8, 16):
        with pytest.raises(L.Sr3Error, match='store_wt'):
            p.set_option('store_wt', bad)
    assert p.set_option('store_wt', prev) == prev        # a refused value changed nothing
