"""CPU: HIPIVFPQ's model key "pq4_lm_scan" (HIPIVFPQModelParams::Parse, which Init runs first): beside "nbits_per_idx": 4 only."""
import pytest

from gamma_amd import plugin


@pytest.mark.parametrize("extra, rc", [
    (', "nbits_per_idx": 4, "pq4_lm_scan": 1', 0),
    (', "nbits_per_idx": 4, "pq4_lm_scan": 0', 0),
    (', "pq4_lm_scan": 0', 0),
    (', "pq4_lm_scan": 1', -1),                         # 8-bit codes (the default)
    (', "nbits_per_idx": 4, "pq4_lm_scan": 2', -1),
    (', "nbits_per_idx": 4, "pq4_lm_scan": "on"', -1),
])
def test_pq4_lm_scan_key(extra, rc):
    assert plugin.parse_model_params('{"ncentroids": 16, "nsubvector": 8%s}' % extra)["rc"] == rc   # (loads the host library)
