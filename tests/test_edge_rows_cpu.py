"""What keeps tests/edge_rows.py (the operand contract table) and gpu_util.halo_expected_refusal honest, without a device: the restated
halo rule against the library's own host query; every conv row's refusal rule says it runs and its scratch query returns what the row
names; every row's `check` passes on its own float64 reference rounded once to the output's type, and fails when one element is moved
by ten times the row's tolerance or is NaN."""
import numpy as np
import pytest
import torch

import gpu_util as G
from edge_rows import CONV_ROWS, ROWS, WGRAD_ROWS


def test_row_ids_are_unique_and_tiles_are_the_default_library_s():
    ids = [r.id for r in ROWS]
    assert len(set(ids)) == len(ids)
    for r in CONV_ROWS:
        assert not any(('_t%d_' % t) in r.id for t in (7, 8, 10)), r.id


@pytest.mark.parametrize('tile', [5, 6, 9])
def test_halo_rule_is_the_library_s(tile):
    """halo_expected_refusal(..., ksplit=1) is None exactly where the library's host query gives the un-split halo kernel statistics
    slices -- which it does where halo_geometry takes the map."""
    from sr3_hip import lib as L
    lib = L.load()
    Cin, Cout = 64, 128
    took = 0
    for ups in (0, 1):
        for B in (1, 2, 3, 4):
            for H in (4, 8, 10, 12, 16, 24, 32, 48):
                for W in (4, 8, 10, 12, 16, 24, 32, 48):
                    rule = G.halo_expected_refusal(B, Cin, H, W, ups, tile, 1)
                    fits = lib.sr3_conv_stats_slices(B, H, W, ups, Cin, Cout, tile, 1) > 0
                    assert (rule is None) == fits, (tile, B, H, W, ups, rule)
                    took += fits
    assert took > 0


def test_halo_rule_split_and_kernel_shape():
    assert G.halo_expected_refusal(2, 64, 16, 16, 0, 5, 1, k=1) == 'does not fit'
    assert G.halo_expected_refusal(2, 64, 16, 16, 0, 5, 1, stride=2) == 'does not fit'
    assert G.halo_expected_refusal(2, 32, 16, 16, 0, 5, 2) == 'empty split'          # one chunk over two splits
    assert G.halo_expected_refusal(2, 64, 16, 16, 0, 6, 3) == 'empty split'          # two chunks over three
    assert G.halo_expected_refusal(2, 96, 16, 16, 0, 9, 2) is None and G.halo_expected_refusal(2, 96, 16, 16, 0, 9, 0) is None
    assert G.halo_expected_refusal(3, 32, 8, 8, 0, 5, 1) is None and G.halo_expected_refusal(3, 32, 8, 8, 0, 6, 1) == 'does not fit'


@pytest.mark.parametrize('row', CONV_ROWS, ids=[r.id for r in CONV_ROWS])
def test_every_conv_row_must_run(row):
    from sr3_hip import lib as L
    lib = L.load()
    spec = row.spec()
    assert spec['refusal'](lib) is None, spec['refusal'](lib)
    nb = spec['query'](lib)
    if spec.get('expect') is not None:
        assert nb == spec['expect'], (nb, spec['expect'])


@pytest.mark.parametrize('row', WGRAD_ROWS, ids=[r.id for r in WGRAD_ROWS])
def test_every_wgrad_row_has_the_pixel_split_it_names(row):
    from sr3_hip import lib as L
    spec = row.spec()
    assert spec['expect'] > 0 and spec['query'](L.load()) == spec['expect']


def _moved(t, flat, delta):
    t = t.clone()
    v = t.view(-1)
    if delta is None:          # bit-exact: the next representable value
        v[flat] = torch.from_numpy(np.nextafter(v[flat:flat + 1].numpy(), np.array(np.inf, dtype=v.numpy().dtype)))[0]
    else:
        v[flat] = v[flat] + delta
    return t


@pytest.mark.parametrize('row', ROWS, ids=[r.id for r in ROWS])
def test_check_is_sound_and_has_teeth(row):
    spec = row.spec()
    exact = spec['exact']()
    assert set(exact) == set(spec['outs'])
    for k, o in spec['outs'].items():
        shape, dtype = (tuple(o.shape), o.dtype) if torch.is_tensor(o) else (tuple(o[0]), o[1])
        assert tuple(exact[k].shape) == shape and exact[k].dtype == dtype, k
    spec['check'](exact)                                  # sound: its own reference, rounded once
    assert spec['tol'], 'the row compares nothing'
    for k, tol in spec['tol'].items():
        at = int(exact[k].double().abs().argmax())
        for delta in ((None,) if tol is None else (10.0 * tol, -10.0 * tol)):
            bad = dict(exact)
            bad[k] = _moved(exact[k], at, delta)
            assert not torch.equal(bad[k], exact[k])
            with pytest.raises(AssertionError):
                spec['check'](bad)
        if exact[k].is_floating_point():
            bad = dict(exact)
            bad[k] = exact[k].clone()
            bad[k].view(-1)[at] = float('nan')
            with pytest.raises(AssertionError):
                spec['check'](bad)
