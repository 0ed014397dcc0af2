"""CPU: the HIPIVFFLAT model's "group_rows" key (gamma_amd/host/gamma_index_ivfflat_group_rows_hip.cc) through
what Init decides before it opens a device (plugin.check_ivfflat_group_keys): "raw_dtype" means the members of a group hold their
rows in a narrow raw_dtype; without the key, or with "float32", a narrow raw_dtype beside several devices is rejected as it
always was.  Every rejection is one log line.  HIPIVFPQ ignores the key."""
import pytest

from gamma_amd import plugin

BASE = '"ncentroids": 16, "nprobe": 4, "metric_type": "L2"'
KEY = ', "group_rows": "raw_dtype"'
PLACEMENTS = [', "devices": "0,0,0"', ', "devices": "0,0,0", "raw_placement": "sharded"', ', "devices": "0,0,0", "placement": "replicate"']
NARROW = ["float16", "uint8", "int8"]


def _check(extra=""):
    return plugin.check_ivfflat_group_keys("{%s%s}" % (BASE, extra))   # (loads the host library: a missing one is a failure)


def _dt(dtype):
    return ', "raw_dtype": "%s"' % dtype


def _rejected_with_one_line(capfd, extra):
    capfd.readouterr()
    rc, several, narrow = _check(extra)
    err = capfd.readouterr().err
    assert rc != 0 and not several and not narrow, extra
    assert len([l for l in err.splitlines() if l.strip()]) == 1, (extra, err)
    return err


@pytest.mark.parametrize("dtype", NARROW)
@pytest.mark.parametrize("placement", PLACEMENTS, ids=["replicated-rows", "sharded-rows", "replicate"])
def test_narrow_members_in_every_placement_the_fp32_group_takes(capfd, placement, dtype):
    capfd.readouterr()
    assert _check(_dt(dtype) + placement + KEY) == (0, True, True)
    assert _check(_dt(dtype.upper()) + placement + ', "group_rows": "RAW_DTYPE"') == (0, True, True)
    assert _check(placement) == (0, True, False)                       # the fp32 group itself
    assert capfd.readouterr().err.strip() == ""


@pytest.mark.parametrize("dtype", NARROW)
def test_without_the_key_the_pinned_rejections_hold(capfd, dtype):
    for placement in PLACEMENTS:
        for key in ("", ', "group_rows": "float32"', ', "group_rows": "Float32"'):
            err = _rejected_with_one_line(capfd, _dt(dtype) + placement + key)
            assert "raw_dtype other than float32 with several devices is not supported" in err
    err = _rejected_with_one_line(capfd, _dt(dtype) + ', "devices": "0,0"')
    assert "the group's members hold fp32 rows" in err


def test_the_pinned_three(capfd):
    for extra in (', "devices": "0,0", "raw_dtype": "float16"', ', "devices": "0,0", "raw_dtype": "uint8"',
                  ', "raw_dtype": "uint8", "devices": "0,0,0", "raw_placement": "sharded"'):
        _rejected_with_one_line(capfd, extra)


def test_rejected_values_and_combinations(capfd):
    for v in ('"float16"', '"uint8"', '"yes"', '""', '"raw-dtype"', "1"):
        err = _rejected_with_one_line(capfd, _dt("uint8") + PLACEMENTS[0] + ', "group_rows": %s' % v)
        assert "invalid group_rows" in err
    # one device or none
    for dev in ("", ', "devices": "0"', ', "devices": 0'):
        for dtype in NARROW + ["float32"]:
            err = _rejected_with_one_line(capfd, _dt(dtype) + dev + KEY)
            assert "needs several devices" in err
        err = _rejected_with_one_line(capfd, dev + KEY)
        assert "needs several devices" in err
    # sq8: the trained ranges would have to reach every member
    for placement in PLACEMENTS:
        err = _rejected_with_one_line(capfd, ', "raw_dtype": "sq8", "sq8_ranges": "trained"' + placement + KEY)
        assert "sq8" in err
    # device_filters
    for dtype in NARROW:
        err = _rejected_with_one_line(capfd, _dt(dtype) + PLACEMENTS[0] + ', "device_filters": 1' + KEY)
        assert "device_filters" in err
    # what the fp32 group rejects stays rejected with the key
    _rejected_with_one_line(capfd, _dt("uint8") + ', "devices": "0,0", "placement": "replicate", "raw_placement": "sharded"' + KEY)
    _rejected_with_one_line(capfd, _dt("uint8") + ', "devices": "0,0", "placement": "elsewhere"' + KEY)
    _rejected_with_one_line(capfd, _dt("uint4") + PLACEMENTS[0] + KEY)


def test_the_key_beside_float32_rows_means_nothing(capfd):
    capfd.readouterr()
    for placement in PLACEMENTS:
        assert _check(placement + KEY) == (0, True, False)
        assert _check(_dt("float32") + placement + KEY) == (0, True, False)
    assert capfd.readouterr().err.strip() == ""


def test_one_device_is_as_before(capfd):
    capfd.readouterr()
    for dtype in NARROW + ["float32"]:
        assert _check(_dt(dtype)) == (0, False, False)
        assert _check(_dt(dtype) + ', "devices": "0"') == (0, False, False)
        assert _check(_dt(dtype) + ', "group_rows": "float32"') == (0, False, False)
    assert _check(', "raw_dtype": "sq8", "sq8_ranges": "trained"') == (0, False, False)
    assert _check() == (0, False, False)
    assert capfd.readouterr().err.strip() == ""


def test_hipivfpq_ignores_the_key():
    base = '"ncentroids": 16, "nsubvector": 8'
    for extra in ("", ', "devices": "0,1"', ', "raw_dtype": "uint8", "devices": "0,1"',
                  ', "raw_dtype": "uint8", "devices": "0,1", "raw_placement": "sharded"', ', "raw_dtype": "sq8", "devices": "0,1"',
                  ', "raw_dtype": "float16"', ', "raw_placement": "sharded"'):
        want = plugin.check_raw_keys("{%s%s}" % (base, extra))
        for key in (KEY, ', "group_rows": "float32"', ', "group_rows": "nonsense"'):
            assert plugin.check_raw_keys("{%s%s%s}" % (base, extra, key)) == want
    # ... and its own answers are the pinned ones
    assert plugin.check_raw_keys('{%s, "raw_dtype": "uint8", "devices": "0,1"%s}' % (base, KEY)) == (0, -2)
    assert plugin.check_raw_keys('{%s, "raw_dtype": "uint8", "devices": "0,1", "raw_placement": "sharded"%s}' % (base, KEY)) == (0, 0)
    assert plugin.check_raw_keys('{%s, "devices": "0,1"%s}' % (base, KEY)) == (0, 0)
