"""CPU: which combinations of "raw_dtype", "devices", "placement" and "raw_placement" the HIPIVFPQ plugin takes
(HIPIVFPQModelParams::Parse + CheckRawKeys: what Init decides before it opens a device).  A narrow raw_dtype goes with several
devices only where the rows are sharded with their lists; sq8 keeps to one device."""
import pytest

from gamma_amd import plugin

BASE = '"ncentroids": 16, "nsubvector": 8'
OK, REJECTED = (0, 0), (0, -2)


def _check(extra=""):
    return plugin.check_raw_keys("{%s%s}" % (BASE, extra))   # (loads the host library: a missing one is a failure)


def _dt(dtype):
    return ', "raw_dtype": "%s"' % dtype


def test_one_device_takes_every_raw_dtype():
    for dtype in ("float32", "float16", "uint8", "int8", "sq8"):
        assert _check(_dt(dtype)) == OK
        assert _check(_dt(dtype) + ', "devices": "0"') == OK
    assert _check() == OK


@pytest.mark.parametrize("dtype", ["float16", "uint8", "int8"])
def test_narrow_rows_on_several_devices_only_sharded(dtype):
    assert _check(_dt(dtype) + ', "devices": "0,1", "raw_placement": "sharded"') == OK
    assert _check(_dt(dtype) + ', "devices": "0,1,2,3", "placement": "shard", "raw_placement": "sharded"') == OK
    assert _check(_dt(dtype.upper()) + ', "devices": "0,1", "raw_placement": "Sharded"') == OK
    # replicated rows stay fp32
    assert _check(_dt(dtype) + ', "devices": "0,1"') == REJECTED
    assert _check(_dt(dtype) + ', "devices": "0,1", "raw_placement": "replicated"') == REJECTED
    assert _check(_dt(dtype) + ', "devices": "0,1", "placement": "replicate"') == REJECTED
    # sharded rows need sharded lists and several devices, whatever the element type
    assert _check(_dt(dtype) + ', "devices": "0,1", "placement": "replicate", "raw_placement": "sharded"') == REJECTED
    assert _check(_dt(dtype) + ', "devices": "0", "raw_placement": "sharded"') == REJECTED
    assert _check(_dt(dtype) + ', "raw_placement": "sharded"') == REJECTED


def test_sq8_keeps_to_one_device():
    assert _check(_dt("sq8") + ', "devices": "0,1"') == REJECTED
    assert _check(_dt("sq8") + ', "devices": "0,1", "raw_placement": "sharded"') == REJECTED
    assert _check(_dt("sq8") + ', "devices": "0,1,2", "placement": "shard", "raw_placement": "sharded"') == REJECTED


def test_fp32_rows_are_as_before():
    assert _check(', "devices": "0,1"') == OK
    assert _check(', "devices": "0,1", "placement": "replicate"') == OK
    assert _check(', "devices": "0,1", "raw_placement": "sharded"') == OK
    assert _check(_dt("float32") + ', "devices": "0,1", "raw_placement": "sharded"') == OK
    assert _check(', "devices": "0,1", "placement": "replicate", "raw_placement": "sharded"') == REJECTED
    assert _check(', "raw_placement": "sharded"') == REJECTED


def test_a_bad_value_fails_the_parse():
    assert _check(_dt("uint4") + ', "devices": "0,1", "raw_placement": "sharded"') == (-1, -1)
    assert _check(_dt("uint8") + ', "devices": "0,1", "raw_placement": "shard"') == (-1, -1)
