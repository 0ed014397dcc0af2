"""CPU: which row lengths the list-major IVFFLAT scan with the scanner's tail steps serves, and with which load width
(gamma_hip_ivfflat_lm_tail_shape) -- read from the library without a device call."""
from math import gcd

from gamma_amd import api


def test_tail_shape_over_every_row_length_and_element_size():
    qtile = api.ivfflat_lm_shape(144)[2]
    for esz in (4, 2, 1):
        for d in range(1, 4201):
            kind, load, qt = api.ivfflat_lm_tail_shape(d, esz)
            assert kind == (3 if d <= 4096 and d % 16 else 0), (d, esz)
            assert load == gcd(16, d * esz), (d, esz)
            assert qt == qtile, (d, esz)
            assert not (kind and api.ivfflat_lm_shape(d)[0])      # a length has one list-major form
