"""Every solver kernel family judged element by element against an fp64 step taken from the device's own state.

Each case (tests/elementwise.CASES) creates a Plan (conv_eps = 0, cost_check on, the case's sparsity form and masks), uploads
V (fp32), W0, H0, calls init() and reads the state back: get_w() / get_h() after init return the normalised (W, H) of
src/sparse_nmf.m:157-160 (checked here against the oracle's normalisation).  Then three steps: run(1), read W_k (the fp64 master)
and H_k (the fp32 values), and judge

  - H_k against ref_hstep(W_{k-1}, H_{k-1}) and W_k against ref_wstep(W_{k-1}, H_k) -- the device's own H_k, so each kernel is
    judged alone -- per element with the one-step bounds tau_H / tau_W, region by region (tests/elementwise.py derives the bounds
    and parses the regions from describe());
  - the exact invariants: an H-only plan leaves W bit for bit, a W-only plan H; semi mode's fixed columns are only renormalised
    (already unit norm: within 4u);
  - the objective of every iterate against the fp64 divergence + sum(S .* H_k) on the device's (W_k, H_k), with test_gpu_parity's
    REL_COST and its 2e-7 * sum(V) floor (Itakura-Saito: eps_f32 per bin, as test_gpu_frame_solvers._check_solve).  The objective
    of iterate k is formed while step k + 1 runs (or by the final pass), so the three are read after the third step.

Three steps, because ping-pong H buffers, arrival counters and hand-off slots go wrong on the second and third iteration.

A second, tighter check per region: the RMS relative error of every step must stay within 4x of what this module measured on an
MI355X (fixed seeds are bitwise reproducible, test_gpu_parity.py::test_runs_are_bitwise_reproducible).  It catches a whole region
summed in a worse order than designed, which stays under the worst-case bound -- for the W statistics it is the only fine check,
tau_W being three orders above their rounding.  MEASURED below holds, per case and region, the largest worst-element and RMS
relative errors over the steps.  The limit is 4 x max(measured RMS, RMS_FLOOR): the floor, 1e-12, only matters for semi mode's
fixed columns, which are renormalised unit columns (~1e-16, and checked exactly against 4u besides); every other region measured
above 1e-9, so its limit is 4x its own value.

Measured on an MI355X at 4c62827 (the kernels this module judges are unchanged since).  The table gives, per case, the largest
value over the steps and the regions; MEASURED gives each region's.  The worst element sits one to two orders below its bound,
so a structural error of ~1/F stands out and rounding does not come near it.  The module runs in about 11 s of device and fp64
reference work (39 cases, 115 steps).

    case                        worst H / tau_H    RMS H   worst W / tau_W    RMS W
    rp_split2_F65              6.8e-07 / 1.3e-05  1.3e-07   3.4e-08 / 5.4e-05  6.4e-09
    rp_split4_F129             1.1e-06 / 2.1e-05  1.9e-07   3.3e-08 / 6.5e-05  6.0e-09
    rp_cut4_F289               4.8e-07 / 3.8e-05  9.7e-08   6.3e-08 / 1.1e-04  1.2e-08
    rp_pairs_F513              1.1e-06 / 6.5e-05  1.9e-07   6.6e-08 / 1.4e-04  9.4e-09
    rp_3tiles_semi_F65         6.8e-07 / 1.3e-05  1.3e-07   3.5e-08 / 6.9e-05  6.8e-09
    rp_3tiles_honly_F257       1.3e-06 / 4.7e-05  2.5e-07   -                        -
    rh_lx4_r97                 9.4e-07 / 6.8e-05  1.9e-07   5.3e-08 / 1.5e-04  9.2e-09
    rh_lx4_r100_honly          5.7e-07 / 6.8e-05  1.1e-07   -                        -
    rh_pairs_r193              9.6e-07 / 7.4e-05  1.9e-07   1.0e-07 / 1.9e-04  1.6e-08
    rh_pairs_r200_honly        9.3e-07 / 7.4e-05  1.8e-07   -                        -
    rh_plain_449               1.7e-06 / 6.9e-05  3.3e-07   1.0e-07 / 1.9e-04  1.5e-08
    plain_few_tiles            1.2e-06 / 3.4e-05  2.4e-07   7.7e-08 / 7.3e-05  1.4e-08
    plain_wonly                -                        -   5.6e-08 / 7.3e-05  1.2e-08
    plain_is_F33               7.4e-07 / 8.8e-06  1.4e-07   6.4e-08 / 3.4e-05  2.2e-08
    plain_b05_F64              8.8e-07 / 1.4e-05  1.8e-07   6.6e-08 / 4.4e-05  1.9e-08
    plain_b15_F257             1.7e-06 / 3.5e-05  3.4e-07   1.5e-07 / 7.1e-05  2.2e-08
    plain_ed_gram_F513         2.3e-06 / 6.8e-05  4.7e-07   2.0e-07 / 1.3e-04  3.3e-08
    wstats_nk16_gram           1.8e-06 / 5.6e-05  3.5e-07   2.0e-07 / 1.7e-04  3.1e-08
    wstats_nk16_kg2_kl         7.4e-07 / 4.5e-05  1.5e-07   6.1e-08 / 1.7e-04  9.8e-09
    wstats_gram_quiet          1.2e-06 / 2.2e-05  2.5e-07   1.6e-07 / 6.5e-05  3.1e-08
    isf_F64_r70                6.4e-07 / 1.3e-05  1.4e-07   2.6e-08 / 5.3e-05  5.3e-09
    isf_F64_r100               7.4e-07 / 1.5e-05  1.4e-07   2.6e-08 / 6.1e-05  5.3e-09
    isf_F64_r96                6.8e-07 / 1.4e-05  1.4e-07   2.7e-08 / 6.0e-05  5.0e-09
    isf_F48_r128               6.1e-07 / 1.4e-05  1.2e-07   2.9e-08 / 6.4e-05  5.3e-09
    hsf_shared_r200            7.3e-07 / 2.1e-05  1.4e-07   5.2e-08 / 1.1e-04  8.0e-09
    hsf_wsf_remainder          7.7e-07 / 1.1e-05  1.3e-07   2.7e-08 / 4.6e-05  6.1e-09
    hsf_honly_F32              6.3e-07 / 1.1e-05  1.1e-07   -                        -
    hsf_F40_r20                5.4e-07 / 7.0e-06  1.2e-07   2.9e-08 / 6.0e-05  9.4e-09
    sr_F513_r20                3.8e-07 / 6.3e-05  9.1e-08   3.9e-08 / 1.2e-04  8.1e-09
    sr_wonly_r10               -                        -   4.1e-08 / 1.2e-04  8.5e-09
    sr_honly_F257              4.2e-07 / 3.4e-05  8.3e-08   -                        -
    sr_F385_r10                4.7e-07 / 4.8e-05  1.6e-07   5.6e-08 / 9.6e-05  8.5e-09
    sr_semi_F422               4.5e-07 / 5.3e-05  9.2e-08   3.9e-08 / 1.2e-04  7.1e-09
    generic_2700               3.7e-06 / 3.3e-04  8.0e-07   2.2e-06 / 6.6e-04  3.6e-07
    generic_b15_2600           5.0e-06 / 3.1e-04  1.1e-06   2.0e-06 / 5.4e-04  3.1e-07
    generic_wonly_r1100        -                        -   2.3e-06 / 7.8e-04  2.7e-07
    generic_is_honly_kreduce   4.5e-06 / 3.4e-04  1.2e-06   -                        -
    generic_semi_2600          3.0e-06 / 3.1e-04  8.5e-07   1.0e-06 / 5.2e-04  1.7e-07
    headline_c2                1.4e-06 / 4.7e-05  2.4e-07   1.4e-07 / 3.1e-04  2.3e-08
"""
import time

import numpy as np
import pytest

from elementwise import (CASES, U, case_data, case_masks, chain_t, compare, cost_of, ref_hstep, ref_wstep, regions, tau_h,
                         tau_w)

pytestmark = pytest.mark.gpu

REL_COST = 1e-5  # test_gpu_parity.REL_COST

RMS_FLOOR = 1e-12  # (the module docstring: only the renormalised fixed columns of semi mode measure below it)
# Measured on an MI355X (n_cu = 256) at 4c62827.
MEASURED = {  # per case and region: (worst element, RMS) relative error, the largest over the steps, rounded up to two digits
    "rp_split2_F65": {"H": {"all": (6.8e-7, 1.3e-7), "comp.full_tiles": (6.8e-7, 1.3e-7), "comp.remainder": (6.2e-7, 1.3e-7),
        "frames.last_partial_tile": (2.6e-7, 9.5e-8), "frames.pipelined": (6.8e-7, 1.4e-7), "frames.split_round": (4.6e-7, 9.2e-8)},
        "W": {"all": (3.5e-8, 6.4e-9), "rows.mfma": (3.5e-8, 6.4e-9), "rows.extra_valu": (1.3e-8, 4.6e-9), "comp.full_tiles": (3.5e-8,
        6.4e-9), "comp.remainder": (2.1e-8, 5.5e-9)}},
    "rp_split4_F129": {"H": {"all": (1.1e-6, 1.8e-7), "comp.full_tiles": (1.1e-6, 1.8e-7), "comp.remainder": (8.7e-7, 1.7e-7),
        "frames.last_partial_tile": (3.6e-7, 8.9e-8), "frames.pipelined": (1.1e-6, 1.9e-7), "frames.split_round": (3.8e-7, 8.7e-8)},
        "W": {"all": (3.3e-8, 5.9e-9), "rows.mfma": (3.3e-8, 5.9e-9), "rows.extra_valu": (1.3e-8, 5.2e-9), "comp.full_tiles": (3.3e-8,
        6.0e-9), "comp.remainder": (2.0e-8, 4.4e-9)}},
    "rp_cut4_F289": {"H": {"all": (4.8e-7, 9.5e-8), "comp.full_tiles": (4.8e-7, 9.4e-8), "comp.remainder": (4.7e-7, 9.5e-8),
        "frames.last_tile": (3.6e-7, 9.8e-8), "frames.pipelined": (4.8e-7, 9.5e-8)}, "W": {"all": (6.3e-8, 1.2e-8), "rows.mfma":
        (6.3e-8, 1.2e-8), "rows.extra_valu": (2.1e-8, 7.8e-9), "comp.full_tiles": (6.3e-8, 1.3e-8), "comp.remainder": (6.3e-8,
        1.2e-8)}},
    "rp_pairs_F513": {"H": {"all": (1.1e-6, 1.9e-7), "comp.full_tiles": (1.1e-6, 1.9e-7), "comp.remainder": (8.9e-7, 1.9e-7),
        "frames.last_tile": (6.5e-7, 1.9e-7), "frames.pipelined": (1.1e-6, 1.9e-7)}, "W": {"all": (6.6e-8, 9.4e-9), "rows.mfma":
        (6.6e-8, 9.4e-9), "rows.extra_valu": (1.6e-8, 6.3e-9), "comp.full_tiles": (6.6e-8, 9.3e-9), "comp.remainder": (5.1e-8,
        9.5e-9)}},
    "rp_3tiles_semi_F65": {"H": {"all": (6.8e-7, 1.4e-7), "comp.full_tiles": (6.8e-7, 1.4e-7), "comp.remainder": (6.1e-7, 1.4e-7),
        "frames.last_partial_tile": (2.5e-7, 1.1e-7), "frames.pipelined": (6.8e-7, 1.4e-7), "frames.split_round": (2.5e-7, 1.1e-7)},
        "W": {"all": (3.5e-8, 4.9e-9), "rows.mfma": (3.5e-8, 4.9e-9), "rows.extra_valu": (9.8e-9, 2.4e-9), "comp.full_tiles": (3.5e-8,
        4.9e-9), "comp.remainder": (2.1e-8, 5.2e-9), "comp.fixed": (3.0e-16, 1.4e-16), "comp.updated": (3.5e-8, 6.9e-9)}},
    "rp_3tiles_honly_F257": {"H": {"all": (1.4e-6, 2.5e-7), "comp.full_tiles": (1.4e-6, 2.5e-7), "frames.last_partial_tile": (1.1e-6,
        2.5e-7), "frames.pipelined": (1.4e-6, 2.5e-7)}},
    "rh_lx4_r97": {"H": {"all": (9.4e-7, 1.4e-7), "comp.full_tiles": (9.4e-7, 1.4e-7), "comp.leftover_4x4x1": (6.7e-7, 1.4e-7),
        "frames.last_tile": (7.1e-7, 1.9e-7), "frames.pipelined": (5.4e-7, 1.1e-7), "frames.split_round": (9.4e-7, 1.9e-7)}, "W":
        {"all": (5.4e-8, 9.2e-9), "rows.mfma": (5.4e-8, 9.2e-9), "rows.extra_valu": (1.4e-8, 4.2e-9), "comp.full_tiles": (5.4e-8,
        9.2e-9), "comp.remainder": (2.7e-8, 6.8e-9)}},
    "rh_lx4_r100_honly": {"H": {"all": (5.7e-7, 1.2e-7), "comp.full_tiles": (5.7e-7, 1.2e-7), "comp.leftover_4x4x1": (4.0e-7, 8.4e-8),
        "frames.last_partial_tile": (4.4e-7, 1.2e-7), "frames.pipelined": (5.7e-7, 1.2e-7), "frames.split_round": (5.3e-7, 1.2e-7)}},
    "rh_pairs_r193": {"H": {"all": (9.6e-7, 1.9e-7), "comp.full_tiles": (9.6e-7, 1.9e-7), "comp.leftover_4x4x1": (4.7e-7, 1.3e-7),
        "frames.last_partial_tile": (4.9e-7, 1.2e-7), "frames.pipelined": (9.6e-7, 1.9e-7), "frames.split_round": (5.5e-7, 1.2e-7)},
        "W": {"all": (1.1e-7, 1.6e-8), "rows.mfma": (1.1e-7, 1.6e-8), "rows.extra_valu": (2.8e-8, 6.6e-9), "comp.full_tiles": (1.1e-7,
        1.6e-8), "comp.remainder": (6.3e-8, 1.7e-8)}},
    "rh_pairs_r200_honly": {"H": {"all": (9.3e-7, 1.8e-7), "comp.full_tiles": (9.3e-7, 1.9e-7), "comp.leftover_4x4x1": (5.3e-7,
        1.1e-7), "frames.last_partial_tile": (4.2e-7, 1.1e-7), "frames.pipelined": (9.3e-7, 1.9e-7), "frames.split_round": (5.4e-7,
        1.1e-7)}},
    "rh_plain_449": {"H": {"all": (1.8e-6, 3.3e-7), "comp.full_tiles": (1.8e-6, 3.3e-7), "comp.remainder": (1.6e-6, 3.3e-7),
        "frames.last_partial_tile": (1.2e-6, 3.3e-7), "frames.pipelined": (1.8e-6, 3.3e-7)}, "W": {"all": (1.1e-7, 1.6e-8),
        "rows.mfma": (1.1e-7, 1.6e-8), "rows.extra_valu": (3.4e-8, 6.9e-9), "comp.full_tiles": (1.1e-7, 1.6e-8), "comp.remainder":
        (8.7e-8, 1.6e-8)}},
    "plain_few_tiles": {"H": {"all": (1.3e-6, 2.5e-7), "comp.full_tiles": (1.3e-6, 2.5e-7), "comp.remainder": (1.1e-6, 2.5e-7),
        "frames.last_partial_tile": (9.0e-7, 2.5e-7)}, "W": {"all": (7.7e-8, 1.3e-8), "rows.mfma": (7.7e-8, 1.3e-8),
        "rows.extra_valu": (3.3e-8, 9.2e-9), "comp.full_tiles": (7.7e-8, 1.3e-8), "comp.remainder": (6.8e-8, 1.5e-8)}},
    "plain_wonly": {"W": {"all": (5.7e-8, 1.2e-8), "rows.mfma": (5.7e-8, 1.2e-8), "rows.extra_valu": (2.5e-8, 7.9e-9),
        "comp.full_tiles": (5.7e-8, 1.2e-8), "comp.remainder": (5.2e-8, 1.2e-8)}},
    "plain_is_F33": {"H": {"all": (7.4e-7, 1.4e-7), "comp.remainder": (7.4e-7, 1.4e-7), "frames.last_partial_tile": (5.4e-7, 1.4e-7)},
        "W": {"all": (6.4e-8, 2.2e-8), "rows.mfma": (6.4e-8, 2.2e-8), "rows.extra_valu": (2.3e-8, 1.1e-8), "comp.remainder": (6.4e-8,
        2.2e-8)}},
    "plain_b05_F64": {"H": {"all": (8.9e-7, 1.8e-7), "comp.full_tiles": (8.9e-7, 1.8e-7), "comp.remainder": (7.2e-7, 1.8e-7),
        "frames.last_partial_tile": (5.8e-7, 1.7e-7)}, "W": {"all": (6.7e-8, 1.8e-8), "rows.mfma": (6.7e-8, 1.8e-8),
        "comp.full_tiles": (6.7e-8, 1.8e-8), "comp.remainder": (6.1e-8, 1.9e-8)}},
    "plain_b15_F257": {"H": {"all": (1.7e-6, 3.4e-7), "comp.full_tiles": (1.6e-6, 3.4e-7), "comp.remainder": (1.7e-6, 3.5e-7),
        "frames.last_partial_tile": (1.4e-6, 3.5e-7)}, "W": {"all": (1.5e-7, 2.2e-8), "rows.mfma": (1.5e-7, 2.2e-8),
        "rows.extra_valu": (4.1e-8, 1.3e-8), "comp.full_tiles": (1.4e-7, 2.2e-8), "comp.remainder": (1.5e-7, 2.2e-8)}},
    "plain_ed_gram_F513": {"H": {"all": (2.4e-6, 4.7e-7), "comp.full_tiles": (2.4e-6, 4.7e-7), "comp.remainder": (1.8e-6, 4.7e-7),
        "frames.last_partial_tile": (1.7e-6, 4.7e-7)}, "W": {"all": (2.0e-7, 3.3e-8), "rows.mfma": (2.0e-7, 3.3e-8),
        "rows.extra_valu": (1.3e-7, 3.4e-8), "comp.full_tiles": (2.0e-7, 3.3e-8), "comp.remainder": (1.9e-7, 3.3e-8)}},
    "wstats_nk16_gram": {"H": {"all": (1.9e-6, 3.5e-7), "comp.full_tiles": (1.9e-6, 3.5e-7), "comp.remainder": (1.9e-6, 3.5e-7),
        "frames.last_tile": (1.4e-6, 3.5e-7)}, "W": {"all": (2.1e-7, 3.1e-8), "rows.mfma": (2.1e-7, 3.1e-8), "rows.extra_valu":
        (1.4e-7, 3.2e-8), "comp.full_tiles": (2.1e-7, 3.1e-8), "comp.remainder": (1.8e-7, 3.1e-8)}},
    "wstats_nk16_kg2_kl": {"H": {"all": (7.4e-7, 1.5e-7), "comp.full_tiles": (7.4e-7, 1.5e-7), "comp.remainder": (6.4e-7, 1.5e-7),
        "frames.last_partial_tile": (6.8e-7, 1.6e-7)}, "W": {"all": (6.1e-8, 9.8e-9), "rows.mfma": (6.1e-8, 9.8e-9),
        "rows.extra_valu": (2.7e-8, 5.7e-9), "comp.full_tiles": (6.1e-8, 9.8e-9), "comp.remainder": (5.3e-8, 9.7e-9)}},
    "wstats_gram_quiet": {"H": {"all": (1.2e-6, 2.4e-7), "comp.full_tiles": (1.2e-6, 2.4e-7), "comp.remainder": (1.1e-6, 2.4e-7),
        "frames.last_partial_tile": (9.3e-7, 2.5e-7)}, "W": {"all": (1.7e-7, 3.1e-8), "rows.mfma": (1.7e-7, 3.1e-8),
        "rows.extra_valu": (8.5e-8, 2.7e-8), "comp.full_tiles": (1.7e-7, 3.1e-8), "comp.remainder": (1.4e-7, 3.1e-8)}},
    "isf_F64_r70": {"H": {"all": (6.5e-7, 1.4e-7), "comp.full_tiles": (6.5e-7, 1.4e-7), "comp.remainder": (6.2e-7, 1.4e-7),
        "frames.last_partial_tile": (4.6e-7, 1.4e-7), "frames.shared_remainder": (6.5e-7, 1.4e-7)}, "W": {"all": (2.7e-8, 5.0e-9),
        "rows.mfma": (2.7e-8, 5.0e-9), "comp.full_tiles": (2.7e-8, 5.0e-9), "comp.remainder": (2.2e-8, 5.4e-9)}},
    "isf_F64_r100": {"H": {"all": (7.5e-7, 1.4e-7), "comp.full_tiles": (7.5e-7, 1.4e-7), "comp.remainder": (5.5e-7, 1.4e-7),
        "frames.last_partial_tile": (5.2e-7, 1.4e-7), "frames.shared_remainder": (7.5e-7, 1.4e-7)}, "W": {"all": (2.7e-8, 5.1e-9),
        "rows.mfma": (2.7e-8, 5.1e-9), "comp.full_tiles": (2.7e-8, 5.1e-9), "comp.remainder": (1.8e-8, 5.3e-9)}},
    "isf_F64_r96": {"H": {"all": (6.8e-7, 1.4e-7), "comp.full_tiles": (6.8e-7, 1.4e-7), "frames.last_partial_tile": (4.6e-7, 1.4e-7),
        "frames.shared_remainder": (6.8e-7, 1.4e-7)}, "W": {"all": (2.7e-8, 5.0e-9), "rows.mfma": (2.7e-8, 5.0e-9), "comp.full_tiles":
        (2.7e-8, 5.0e-9)}},
    "isf_F48_r128": {"H": {"all": (6.2e-7, 1.3e-7), "comp.full_tiles": (6.2e-7, 1.3e-7), "frames.last_tile": (4.7e-7, 1.3e-7),
        "frames.shared_remainder": (5.8e-7, 1.3e-7)}, "W": {"all": (2.9e-8, 5.2e-9), "rows.mfma": (2.9e-8, 5.2e-9),
        "rows.last_partial_tile": (2.6e-8, 5.3e-9), "comp.full_tiles": (2.9e-8, 5.2e-9)}},
    "hsf_shared_r200": {"H": {"all": (7.4e-7, 1.4e-7), "comp.full_tiles": (7.4e-7, 1.4e-7), "comp.remainder": (6.3e-7, 1.4e-7),
        "frames.last_partial_tile": (5.3e-7, 1.4e-7), "frames.whole_tiles": (7.4e-7, 1.4e-7), "frames.shared_tiles": (7.0e-7,
        1.4e-7)}, "W": {"all": (5.2e-8, 8.0e-9), "rows.mfma": (5.2e-8, 8.0e-9), "comp.full_tiles": (5.2e-8, 8.1e-9), "comp.remainder":
        (3.6e-8, 7.7e-9)}},
    "hsf_wsf_remainder": {"H": {"all": (7.8e-7, 1.4e-7), "comp.full_tiles": (7.8e-7, 1.4e-7), "comp.remainder": (6.3e-7, 1.4e-7),
        "frames.last_tile": (5.1e-7, 1.4e-7), "frames.whole_tiles": (7.8e-7, 1.4e-7)}, "W": {"all": (2.8e-8, 5.8e-9), "rows.mfma":
        (2.8e-8, 5.8e-9), "comp.full_tiles": (2.8e-8, 5.7e-9), "comp.remainder": (2.8e-8, 6.1e-9)}},
    "hsf_honly_F32": {"H": {"all": (6.3e-7, 1.2e-7), "comp.full_tiles": (6.3e-7, 1.1e-7), "comp.remainder": (5.0e-7, 1.2e-7),
        "frames.last_tile": (4.3e-7, 1.2e-7), "frames.whole_tiles": (6.3e-7, 1.2e-7)}},
    "hsf_F40_r20": {"H": {"all": (5.4e-7, 1.2e-7), "comp.remainder": (5.4e-7, 1.2e-7), "frames.last_partial_tile": (3.4e-7, 1.2e-7),
        "frames.whole_tiles": (5.4e-7, 1.2e-7)}, "W": {"all": (2.9e-8, 5.9e-9), "rows.mfma": (2.9e-8, 5.9e-9),
        "rows.last_partial_tile": (2.9e-8, 9.4e-9), "comp.remainder": (2.9e-8, 5.9e-9)}},
    "sr_F513_r20": {"H": {"all": (3.9e-7, 9.0e-8), "comp.remainder": (3.9e-7, 9.0e-8), "frames.last_tile": (2.9e-7, 9.1e-8)}, "W":
        {"all": (4.0e-8, 7.3e-9), "rows.mfma": (4.0e-8, 7.3e-9), "rows.extra_valu": (2.2e-8, 8.1e-9), "comp.remainder": (4.0e-8,
        7.3e-9)}},
    "sr_wonly_r10": {"W": {"all": (4.1e-8, 7.8e-9), "rows.mfma": (4.1e-8, 7.8e-9), "rows.extra_valu": (1.2e-8, 8.6e-9),
        "comp.remainder": (4.1e-8, 7.8e-9)}},
    "sr_honly_F257": {"H": {"all": (4.3e-7, 8.3e-8), "comp.full_tiles": (4.3e-7, 8.3e-8), "frames.last_tile": (2.8e-7, 8.3e-8)}},
    "sr_F385_r10": {"H": {"all": (4.7e-7, 9.8e-8), "comp.remainder": (4.7e-7, 9.8e-8), "frames.last_partial_tile": (3.3e-7, 1.6e-7)},
        "W": {"all": (5.7e-8, 8.5e-9), "rows.mfma": (5.7e-8, 8.5e-9), "rows.extra_valu": (6.8e-9, 4.8e-9), "comp.remainder": (5.7e-8,
        8.5e-9)}},
    "sr_semi_F422": {"H": {"all": (4.5e-7, 9.0e-8), "comp.full_tiles": (4.5e-7, 9.0e-8), "frames.last_partial_tile": (3.4e-7,
        9.2e-8)}, "W": {"all": (3.9e-8, 5.1e-9), "rows.mfma": (3.9e-8, 5.1e-9), "rows.last_partial_tile": (2.6e-8, 5.5e-9),
        "comp.full_tiles": (3.9e-8, 5.1e-9), "comp.fixed": (3.0e-16, 1.7e-16), "comp.updated": (3.9e-8, 7.1e-9)}},
    "generic_2700": {"H": {"all": (3.7e-6, 8.0e-7), "comp.full_tiles": (3.7e-6, 8.0e-7), "comp.remainder": (3.2e-6, 8.0e-7),
        "frames.last_partial_tile": (3.1e-6, 8.0e-7)}, "W": {"all": (2.2e-6, 3.5e-7), "comp.full_tiles": (2.2e-6, 3.4e-7),
        "comp.remainder": (2.0e-6, 3.6e-7)}},
    "generic_b15_2600": {"H": {"all": (5.0e-6, 1.1e-6), "comp.remainder": (5.0e-6, 1.1e-6), "frames.last_partial_tile": (3.4e-6,
        1.1e-6)}, "W": {"all": (2.1e-6, 3.2e-7), "comp.remainder": (2.1e-6, 3.2e-7)}},
    "generic_wonly_r1100": {"W": {"all": (2.4e-6, 2.8e-7), "comp.full_tiles": (2.4e-6, 2.8e-7), "comp.remainder": (1.6e-6, 2.7e-7)}},
    "generic_is_honly_kreduce": {"H": {"all": (4.6e-6, 1.1e-6), "comp.remainder": (4.6e-6, 1.1e-6), "frames.last_partial_tile":
        (4.2e-6, 1.3e-6)}},
    "generic_semi_2600": {"H": {"all": (3.1e-6, 7.9e-7), "comp.remainder": (3.1e-6, 7.9e-7), "frames.last_partial_tile": (2.4e-6,
        8.6e-7)}, "W": {"all": (1.1e-6, 1.3e-7), "comp.remainder": (1.1e-6, 1.3e-7), "comp.fixed": (8.9e-16, 4.5e-16), "comp.updated":
        (1.1e-6, 1.8e-7)}},
    "headline_c2": {"H": {"all": (1.5e-6, 2.5e-7), "comp.full_tiles": (1.5e-6, 2.5e-7), "frames.last_tile": (3.7e-7, 9.2e-8),
        "frames.pipelined": (1.5e-6, 2.5e-7), "frames.split_round": (4.1e-7, 9.2e-8)}, "W": {"all": (1.4e-7, 2.4e-8), "rows.mfma":
        (1.4e-7, 2.4e-8), "rows.extra_valu": (2.7e-8, 7.1e-9), "comp.full_tiles": (1.4e-7, 2.4e-8)}},
}


def run_case(ctx, case):
    """Run one case through its steps with every assertion of the module docstring; returns {"H"/"W": {region: (worst, rms)}}
    with the largest values over the steps, and the plan's describe() text."""
    from se_snmf_nat_amd import Plan
    F, T, r, beta, mode, steps = case["F"], case["T"], case["r"], case["beta"], case["mode"], case["steps"]
    V, W0, H0, S = case_data(case)
    w_ind, h_ind = case_masks(mode, r)
    upd_h, upd_w = mode != "w", mode != "h"
    pl = Plan(ctx, F, T, r, beta=beta, max_iter=steps, conv_eps=0.0, cost_check=True, sparsity=S, w_update_ind=w_ind,
              h_update_ind=h_ind)
    try:
        desc = pl.describe()
        for tok in case["tokens"]:
            assert tok in desc, (tok, desc)
        pl.set_v(V)
        pl.set_w(W0)
        pl.set_h(H0)
        pl.init()
        W, H = pl.get_w(), pl.get_h(np.float32)
        wn = np.sqrt((W0 ** 2).sum(0))
        np.testing.assert_allclose(W, W0 / wn, rtol=4 * 2.0 ** -52 * F)  # (the oracle's normalisation, :157-160)
        np.testing.assert_allclose(H, H0 * wn[:, None], rtol=4 * U)
        regs = regions(desc, F, T, r, mode)
        t_h = tau_h(F, r, beta, mode)
        t_w = tau_w(F, r, beta, chain_t(desc, T), mode)
        gram = "Gram matrix" in desc
        fixed = np.zeros(r, bool) if w_ind is None else ~w_ind
        stats = {"H": {}, "W": {}}
        iterates = []

        def keep(m, st):
            for name, (worst, _ij, rms) in st.items():
                w0, r0 = stats[m].get(name, (0.0, 0.0))
                stats[m][name] = (max(w0, worst), max(r0, rms))

        for k in range(1, steps + 1):
            pl.run(1)
            Wk, Hk = pl.get_w(), pl.get_h(np.float32)
            if upd_h:
                Hr, info = ref_hstep(V, W, H, beta, S)
                keep("H", compare(Hk, Hr, t_h, regs, "H", floors=info, what=f"{case['id']} step {k} H"))
            else:
                assert np.array_equal(Hk, H), f"step {k}: a W-only plan changed H"
            if upd_w:
                Wr, info = ref_wstep(V, W, Hk, beta, w_ind, gram=gram)
                keep("W", compare(Wk, Wr, t_w, regs, "W", floors=info, what=f"{case['id']} step {k} W"))
                if fixed.any():
                    d = np.abs(Wk[:, fixed] - W[:, fixed])
                    assert (d <= 4 * U * W[:, fixed]).all(), f"step {k}: fixed columns moved by {float((d / W[:, fixed]).max()):.3e}"
            else:
                assert np.array_equal(Wk, W), f"step {k}: an H-only plan changed W"
            W, H = Wk, Hk
            iterates.append((Wk, Hk))
        div, cost, n = pl.get_objective()
        assert n == steps, (n, steps)
        vsum = float(np.fmax(V.astype(np.float64), 1e-9).sum()) if beta != 0.0 else float(F * T)
        for k, (Wk, Hk) in enumerate(iterates):
            c = cost_of(V, Wk, Hk, beta, S)
            assert abs(cost[k] - c) <= REL_COST * abs(c) + 2e-7 * vsum, (k + 1, cost[k], c)
    finally:
        pl.close()
    return stats, desc


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_one_step_elementwise(gpu_ctx, case, monkeypatch):
    for k in ("SNMF_HSTEP_RP", "SNMF_HSTEP_SPLIT", "SNMF_WSTATS_NL", "SNMF_ITER_SF", "SNMF_GRAM_P", "SNMF_NO_SMALL", "SNMF_HFOLD"):
        monkeypatch.delenv(k, raising=False)  # default plans only
    t0 = time.perf_counter()
    stats, desc = run_case(gpu_ctx, case)
    measured = MEASURED.get(case["id"])
    assert measured is not None, f"nothing recorded for {case['id']}: {stats}"
    for m in ("H", "W"):
        assert set(stats[m]) == {m + "." + k for k in measured.get(m, {})}, (case["id"], m, sorted(stats[m]))
        for name, (_worst, rms) in stats[m].items():
            ref = measured[m][name.split(".", 1)[1]][1]
            assert rms <= 4 * max(ref, RMS_FLOOR), (f"{case['id']}: region {name} of {m}: RMS relative error {rms:.3e} against "
                                                    f"{ref:.3e} measured")
    print(f"{case['id']}: {time.perf_counter() - t0:.2f} s")
