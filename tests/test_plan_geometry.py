"""Kernel and geometry selection without a device: snmf_plan_geometry_describe must give, byte for byte, the describe()
text that real plans reported on an MI355X (n_cu = 256) -- the shapes of the pipelined / full-size / out-of-envelope tests,
the benchmark configurations, Euclidean and generic-beta plans, H-only / W-only masks, the T <= 32 online shapes and each
plan-creation switch at its "off" value (tests/golden/plan_geometry.json)."""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "plan_geometry.json")))
SWITCHES = ["SNMF_HSTEP_RP", "SNMF_HSTEP_SPLIT", "SNMF_WSTATS_NL", "SNMF_ITER_SF", "SNMF_GRAM_P", "SNMF_NO_SMALL", "SNMF_HFOLD"]
# switches that no longer exist: setting them must change nothing
RETIRED = {"SNMF_HSTEP_M": "1", "SNMF_HSTEP_SF": "0", "SNMF_WSTATS_SF": "0", "SNMF_HSTEP_SR": "0", "SNMF_WSTATS_SR": "0",
           "SNMF_RP_CUT": "0", "SNMF_RH_CUT2": "0", "SNMF_WSTATS_TIL": "1", "SNMF_WSTATS_NBUF": "2", "SNMF_WFIN_SPLIT": "0",
           "SNMF_WSTATS_X": "0.5", "SNMF_WSTAG": "500", "SNMF_SF_STAG": "0", "SNMF_SR_STAG": "0"}


def masks(mode, r):
    """(w_update_ind, h_update_ind) of a case's mode."""
    if mode == "h":
        return np.zeros(r), None
    if mode == "w":
        return None, np.zeros(r)
    if mode == "semi":
        w = np.ones(r)
        w[: r // 2] = 0
        return w, None
    return None, None


def describe(c, n_cu=256):
    from se_snmf_nat_amd.api import geometry_describe
    w, h = masks(c["mode"], c["r"])
    return geometry_describe(c["F"], c["T"], c["r"], beta=c["beta"], n_cu=n_cu, w_update_ind=w, h_update_ind=h)


@pytest.fixture
def clean_env(lib, monkeypatch):
    for k in SWITCHES + list(RETIRED):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def test_golden_covers_every_kernel_family():
    text = " ".join(c["describe"] for c in CASES)
    for k in ("k_hstep_rp", "k_hstep_rh", "k_hstep_sf", "k_iter_sf", "k_hstep_sr", "hstep: k_hstep,", "k_wstats_sf", "k_wstats_sr",
              "out-of-envelope", "Gram matrix"):
        assert k in text, k
    assert {k for c in CASES for k in c["env"]} == set(SWITCHES)


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: "%(F)dx%(T)d_r%(r)d_b%(beta)g_%(mode)s" % CASES[i]
                         + "".join("_%s=%s" % kv for kv in sorted(CASES[i]["env"].items())))
def test_geometry_describe_matches_recorded_plans(clean_env, i):
    c = CASES[i]
    for k, v in c["env"].items():
        clean_env.setenv(k, v)
    assert describe(c) == c["describe"]


def test_retired_switches_change_nothing(clean_env):
    for k, v in RETIRED.items():
        clean_env.setenv(k, v)
    for c in CASES:
        if not c["env"]:
            assert describe(c) == c["describe"]


def test_geometry_describe_validates_like_plan_create(lib):
    from se_snmf_nat_amd import SnmfError
    from se_snmf_nat_amd.api import geometry_describe
    with pytest.raises(SnmfError) as e:
        geometry_describe(257, 100, 40, h_update_ind=np.r_[np.ones(20), np.zeros(20)])
    assert e.value.status == 3  # SNMF_ERR_DIM: a partial h_update_ind
    with pytest.raises(SnmfError) as e:
        geometry_describe(0, 100, 40)
    assert e.value.status == 1
    with pytest.raises(SnmfError) as e:
        geometry_describe(257, 100, 40, n_cu=0)
    assert e.value.status == 1
    assert "n_cu=80" in geometry_describe(257, 100000, 256, n_cu=80)


@pytest.mark.gpu
@pytest.mark.parametrize("F,T,r,beta,mode", [
    (257, 100000, 256, 1.0, "full"), (257, 1000, 40, 1.0, "full"),                            # k_hstep_rp / k_hstep
    (513, 12000, 100, 1.0, "full"), (513, 9000, 200, 1.0, "h"),                               # k_hstep_rh
    (64, 20000, 100, 1.0, "full"), (64, 37000, 200, 1.0, "full"), (64, 12000, 40, 1.0, "w"),  # k_iter_sf / k_hstep_sf / k_wstats_sf
    (513, 12000, 20, 1.0, "full"), (513, 9000, 10, 1.0, "w"),                                 # k_hstep_sr / k_wstats_sr
    (513, 60000, 512, 2.0, "full"), (257, 30000, 256, 0.5, "full"), (2700, 700, 40, 1.0, "full"), (257, 1, 60, 1.0, "h"),
])
def test_plan_describe_equals_the_device_free_entry(gpu_ctx, clean_env, F, T, r, beta, mode):
    import re
    from se_snmf_nat_amd import Plan
    w, h = masks(mode, r)
    pl = Plan(gpu_ctx, F, T, r, beta=beta, max_iter=4, w_update_ind=w, h_update_ind=h)
    try:
        desc = pl.describe()
    finally:
        pl.close()
    n_cu = int(re.search(r"n_cu=(\d+)", desc).group(1))
    assert desc == describe(dict(F=F, T=T, r=r, beta=beta, mode=mode), n_cu=n_cu)
