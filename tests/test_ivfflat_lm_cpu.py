"""CPU: which list-major form the IVFFLAT scan has for a row length (gamma_hip_ivfflat_lm_shape) -- read from
the library without a device call -- and the properties of the data that tests/test_gpu_ivfflat_lm_anyd.py relies on, examined
with the oracle so that those tests cannot pass vacuously."""
import numpy as np

from gamma_amd import api
from oracle import binding as B
from tests import ivfflat_lm_data as LM

FIXED = (16, 32, 64, 96, 128)


def test_lm_shape_over_every_row_length():
    for d in range(1, 4201):
        kind, slab, qtile = api.ivfflat_lm_shape(d)
        if d in FIXED:
            assert kind == 1, d
        elif d % 16 == 0 and d <= 4096:
            assert kind == 2, d
        else:
            assert kind == 0, d
        if kind:
            assert slab > 0 and qtile > 0 and slab % 16 == 0, (d, slab, qtile)
        if kind == 1:
            assert slab == d      # the whole row in registers


def test_lm_shape_of_lengths_that_are_no_row():
    for d in (0, -16, -1):
        assert api.ivfflat_lm_shape(d)[0] == 0


def test_the_sliced_tile_is_smaller_than_the_fixed_one_and_the_base_shapes_cross_the_slab():
    """the GPU cases d = 48, 144, 256, 272, 768 are: one partial slab; a full slab + 16; two full; two full + 16; six"""
    _, slab, qtile = api.ivfflat_lm_shape(144)
    assert (slab, qtile) == api.ivfflat_lm_shape(4096)[1:]      # one kernel shape for every sliced length
    assert [divmod(d, slab) for d in (48, 144, 256, 272, 768)] == [(0, 48), (1, 16), (2, 0), (2, 16), (6, 0)]
    assert qtile < 33      # the base shape's 33 queries x 4 probes can put more than one tile on a list


def test_many_queries_case_fills_one_tile_exactly_and_overflows_another():
    qtile = api.ivfflat_lm_shape(144)[2]
    c, q = LM.many_queries_case(qtile)
    cnt = LM.probes_per_list(c, q, LM.MANY_P)
    assert len(q) == 40 and (cnt > qtile).any() and (cnt == qtile).any()


def test_edge_case_has_lists_of_128_and_129_rows_and_an_empty_probed_list():
    c = LM.edge_case()
    assert len(c.lists[LM.EDGE_128]) == 128 and len(c.lists[LM.EDGE_129]) == 129 and len(c.lists[LM.EDGE_EMPTY]) == 0
    assert sum(len(l) for l in c.lists) == c.N
    cnt = LM.probes_per_list(c, c.q, 4)
    assert cnt[LM.EDGE_128] > 0 and cnt[LM.EDGE_129] > 0 and cnt[LM.EDGE_EMPTY] > 0


def test_tie_case_has_equal_distances_in_the_oracles_result():
    c = LM.tie_case()
    D, I = c.oracle(c.q, LM.TIE_K, 4)
    assert (I >= 0).all()
    assert np.array_equal(c.W, np.rint(c.W))      # integer-valued rows
    assert ((D[:, 1:] == D[:, :-1]) & (I[:, 1:] != I[:, :-1])).any(axis=1).all()      # every query has a tie among its results


def test_grid_stride_case_has_more_units_than_persistent_workgroups():
    c = LM.grid_case()
    assert LM.work_units(c, c.q, LM.GRID_P, api.ivfflat_lm_shape(c.d)[2]) > 2048
