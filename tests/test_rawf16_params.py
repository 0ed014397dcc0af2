"""CPU: the HIP-only model key "raw_dtype" of HIPIVFPQ (HIPIVFPQModelParams::Parse): values, default, rejections."""
import pytest

from gamma_amd import plugin

BASE = '"ncentroids": 16, "nsubvector": 8'


def _parse(extra=""):
    return plugin.parse_raw_dtype("{%s%s}" % (BASE, extra))   # (loads the host library: a missing one is a failure)


def test_default_is_float32():
    assert _parse() == (0, "float32")
    assert _parse(', "raw_dtype": "float32"') == (0, "float32")


def test_float16_is_accepted_in_any_case():
    assert _parse(', "raw_dtype": "float16"') == (0, "float16")
    assert _parse(', "raw_dtype": "Float16"') == (0, "float16")


@pytest.mark.parametrize("value", ['"bfloat16"', '"half"', '"fp16"', '""', '"float64"'])
def test_other_strings_are_rejected(value):
    assert _parse(', "raw_dtype": %s' % value)[0] == -1


def test_the_other_keys_parse_beside_it():
    s = '{%s, "raw_dtype": "float16", "nprobe": 4, "metric_type": "L2"}' % BASE
    assert plugin.parse_raw_dtype(s) == (0, "float16")
    p = plugin.parse_model_params(s)
    assert p["rc"] == 0 and p["ncentroids"] == 16 and p["nsubvector"] == 8 and p["nprobe"] == 4
    # a bad value fails the whole parse, whatever stands beside it
    assert plugin.parse_model_params(s.replace("float16", "bfloat16"))["rc"] == -1
