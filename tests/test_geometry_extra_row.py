"""Where the extra row (F = 32n+1) of the KL statistics runs, as describe() reports it (no device needed).

Full KL updates on the NK = 8, 4 + 4-wave loader geometry with at most two row groups (the headline, 257 x 100 000 at r = 256)
launch k_wstats_xg: the row runs behind P3's first W-fragment loads.  The deal of the row groups is unchanged, and so is the text
of every default plan (tests/golden/plan_geometry.json pins it byte for byte): it is the plan with SNMF_WSTATS_XG=0 -- the row
at the top of the tile, as before -- that names its placement, in the statistics' suffix.  Plans of any other shape do not
read the switch."""
import re

import numpy as np
import pytest

OFF = ", extra row at the top of the tile (SNMF_WSTATS_XG=0)"
C2 = ("F=257 T=100000 r=256 beta=1 | Fm=256(+1 VALU row) rp=256 Tp=100032 | hstep: k_hstep_rp (4 P1 + 4 P2 + 4 loader waves; 3072 of 3125 "
      "tiles pipelined, last round split 4 ways, grid 256), tile=32 frames, grid=256 x 768 thr, lds=136320 B | wstats: NK=8 waves=4+4 "
      "grid=(131 chunks,2 fgroups,1 kgroups; group-1 chunks 125) lds=154624 B%s | W finish (run loop): k_wfin | n_cu=256")
# four row groups / another statistics geometry: the whole text, with the switch at either value
OTHERS = {
    (513, 9001, 193): "F=513 T=9001 r=193 beta=1 | Fm=512(+1 VALU row) rp=224 Tp=9088 | hstep: k_hstep_rh (4 P1 + 4 P2 + 4 loader waves on "
                      "half tiles, P2 in wave pairs cut over the contraction + leftover columns as 4x4x1 MFMAs; 256 of 282 tiles pipelined, "
                      "last round split 4 ways, grid 256), tile=32 frames, grid=256 x 768 thr, lds=156064 B | wstats: NK=8 waves=4+4 "
                      "grid=(71 chunks,4 fgroups,1 kgroups; group-1 chunks 61) lds=153984 B | W finish (run loop): k_wfin | n_cu=256",
    (513, 9000, 193): "F=513 T=9000 r=193 beta=1 | Fm=512(+1 VALU row) rp=224 Tp=9088 | hstep: k_hstep_rh (4 P1 + 4 P2 + 4 loader waves on "
                      "half tiles, P2 in wave pairs cut over the contraction + leftover columns as 4x4x1 MFMAs; 256 of 282 tiles pipelined, "
                      "last round split 4 ways, grid 256), tile=32 frames, grid=256 x 768 thr, lds=156064 B | wstats: NK=8 waves=4+4 "
                      "grid=(71 chunks,4 fgroups,1 kgroups; group-1 chunks 61) lds=153984 B | W finish (run loop): k_wfin | n_cu=256",
    (513, 72000, 100): "F=513 T=72000 r=100 beta=1 | Fm=512(+1 VALU row) rp=128 Tp=72064 | hstep: k_hstep_rh (4 P1 + 4 P2 + 4 loader waves on "
                       "half tiles, P2 cut four ways over the contraction + leftover columns as 4x4x1 MFMAs; 2250 of 2250 tiles pipelined, "
                       "last round split 0 ways, grid 256), tile=32 frames, grid=256 x 768 thr, lds=154784 B | wstats: NK=4 waves=8+4 "
                       "grid=(133 chunks,2 fgroups,1 kgroups; group-1 chunks 123) lds=154112 B | W finish (run loop): k_wfin | n_cu=256",
}


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in ("SNMF_HSTEP_RP", "SNMF_HSTEP_SPLIT", "SNMF_WSTATS_NL", "SNMF_WSTATS_XG"):
        monkeypatch.delenv(k, raising=False)


def test_headline_text_and_deal_are_unchanged_and_the_switch_names_the_old_placement(lib, monkeypatch):
    from se_snmf_nat_amd.api import geometry_describe
    assert geometry_describe(257, 100000, 256, n_cu=256) == C2 % ""
    monkeypatch.setenv("SNMF_WSTATS_XG", "0")
    d = geometry_describe(257, 100000, 256, n_cu=256)
    assert d == C2 % OFF
    # the grid text keeps the form the element-wise bounds parse (tests/elementwise.chain_t)
    assert re.search(r"grid=\((\d+) chunks,(\d+) fgroups,(\d+) kgroups; group-1 chunks (\d+)\)", d)


@pytest.mark.parametrize("shape", sorted(OTHERS))
def test_other_geometries_keep_their_text(lib, shape, monkeypatch):
    from se_snmf_nat_amd.api import geometry_describe
    assert geometry_describe(*shape, n_cu=256) == OTHERS[shape]
    monkeypatch.setenv("SNMF_WSTATS_XG", "0")
    assert geometry_describe(*shape, n_cu=256) == OTHERS[shape]


def test_only_full_kl_updates_on_the_headline_geometry_read_the_switch(lib, monkeypatch):
    """The statistics launch of a W-only solve also sums the objective, other divergences, ranks and row counts run other
    instantiations: all of them keep the row at the top of the tile, so the switch changes nothing for them."""
    from se_snmf_nat_amd.api import geometry_describe
    monkeypatch.setenv("SNMF_WSTATS_XG", "0")
    assert OFF not in geometry_describe(257, 100000, 256, n_cu=256, h_update_ind=np.zeros(256, bool))  # W-only
    assert OFF not in geometry_describe(257, 100000, 256, beta=2.0, n_cu=256)
    assert OFF not in geometry_describe(256, 100000, 256, n_cu=256)   # no extra row
    assert OFF not in geometry_describe(257, 100000, 100, n_cu=256)   # NK = 4
    assert OFF not in geometry_describe(257, 1000, 256, n_cu=256)     # no loader waves
    for shape in ((129, 100000, 256), (257, 16411, 200), (161, 20000, 136), (193, 12345, 129)):  # one and two row groups
        assert OFF in geometry_describe(*shape, n_cu=256), shape
