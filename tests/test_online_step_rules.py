"""The rules of tests/online_step.py, proved on the CPU before any GPU run: the restatement of the frame step agrees with the oracle's
sep_frame in fp64, every case's pure oracle run reaches the frames the issue asks for (both sides of init_N_len and P_len_l,
triggered and untriggered frames, a wrapped ring, solves with 0 < n_up < R_a), both float32 emulations (sums in index order and
reversed) stay inside every derived bound on every case, and every planted error fails, naming its field and region.  The same
for the single-stream cases (SINGLE_CASES; a fixed-dictionary case has to reach both sides of init_N_len and P_len_l only), whose
driver is also run here on a simulated device -- the emulation behind OnlineSeparator's calls -- clean and with every plant.

Run with -s to see, per case, the oracle's counts and the emulations' worst / bound per field."""
import numpy as np
import pytest

import online_step as os_

_cache = {}
# every case of the batch and every single-stream case with a trajectory of its own (a case that differs from its base in the
# device's environment alone has the base's)
ALL_CASES = list(os_.CASES) + [n for n, c in os_.SINGLE_CASES.items() if c["base"] is None]


def _covered(name, cov):
    """The coverage rule of a case: coverage_ok, or without adaptation frames on both sides of init_N_len and of P_len_l."""
    return bool(cov["init_both"] and cov["pl_both"]) if os_.single_case(name)[2] else os_.coverage_ok(cov)


def _trajectory(name, kind):
    """A case's three streams stepped frame by frame on the CPU.  kind "oracle": the pure oracle run (the state advanced by the
    reference's own g_after), the fp64 restatement judged against it under the u = 2^-53 bounds.  kind "emulation": the state
    advanced by the float32 emulation in index order (what a device would hold), both emulations judged from it under the case's
    bounds.  Returns (tallies, records per stream, states per stream)."""
    if (name, kind) in _cache:
        return _cache[(name, kind)]
    p0, pcms, Bx0, Bds, H0s, Ads, precision, settings = os_.case_inputs(name)
    hop = p0["frameshift"]
    ps, Bxs = zip(*[os_.stream_view(p0, Bx0, settings, k) for k in range(3)])
    f32 = precision == "fp32" and kind == "emulation"  # (the fp64 twins: the same emulation in double under u = 2^-53)
    dt, u = (np.float32, os_.U) if f32 else (np.float64, os_.U64)
    tallies = (os_.Tally(), os_.Tally())
    records, states = [], []
    for k in range(3):
        p, Bx = ps[k], Bxs[k]
        g = os_.initial_state(p, Bx, Bds[k], H0s[k], Ads[k], dt, p["_B_Mel_ds"][k] if "_B_Mel_ds" in p else None)
        rec, sts = [], []
        for i in range(len(pcms[k]) // hop):
            y = os_.frame_buffer(g, pcms[k][i * hop:(i + 1) * hop])
            ref = os_.reference(g, y, p, Bx)
            bnd, margins = os_.case_bounds(g, y, p, Bx, ref, u)
            what = f"{name} stream {k} frame {g['l']}"
            first = None
            for rev, tally in zip((False, True), tallies):
                ga, fr, tr = os_.frame_step(g, y, g["l"], p, g["H0"], Bx, dt=dt, rev=rev, seq=kind == "emulation")
                dev = os_.after_state(g, ga, fr, p["framelength"])
                os_.judge(dev, tr, g, ref, bnd, margins, p, Bx, tally, what, u=u, pin_oracle=kind == "oracle")
                first = first or (ga, fr)
            sts.append((g, y))
            rec.append((g["l"], ref[2], ref[0]["n_push"], ref[0]["update_switch"]))
            g = os_.advance(g, ref[0], ref[1], y, p, dt) if kind == "oracle" else os_.advance(g, first[0], first[1], y, p, dt)
        records.append(rec)
        states.append(sts)
    _cache[(name, kind)] = (tallies, records, states, ps, Bxs)
    return _cache[(name, kind)]


@pytest.mark.parametrize("name", ALL_CASES)
def test_the_restatement_is_the_oracle_and_the_case_reaches_its_frames(name):
    tallies, records, _, ps, _ = _trajectory(name, "oracle")
    cov = os_.coverage(records, ps[0])
    t = tallies[0]
    print(f"\n{name}: pure oracle run: {t.frames} (frame, stream) pairs, triggered {t.triggered}, solved {t.solved}, left out {t.left_out}; {cov}")
    print("\n".join(t.lines()))
    assert not t.fails, "\n".join(t.fails[:10])
    assert _covered(name, cov), cov
    assert t.caps_ok(), (t.left_out, t.border_rows, t.elem_out)


@pytest.mark.parametrize("name", ALL_CASES)
def test_both_emulations_stay_inside_every_bound(name):
    (fwd, rev), records, _, ps, _ = _trajectory(name, "emulation")
    cov = os_.coverage(records, ps[0])
    print(f"\n{name}: emulated run: {fwd.frames} pairs, triggered {fwd.triggered}, solved {fwd.solved}, left out {fwd.left_out}; {cov}")
    print("index order:\n" + "\n".join(fwd.lines()))
    print("reversed:\n" + "\n".join(rev.lines()))
    assert not fwd.fails, "\n".join(fwd.fails[:10])
    assert not rev.fails, "\n".join(rev.fails[:10])
    assert _covered(name, cov), cov
    assert fwd.caps_ok() and rev.caps_ok(), (fwd.left_out, fwd.border_rows, fwd.elem_out, rev.left_out, rev.border_rows, rev.elem_out)


@pytest.mark.parametrize("plant", os_.PLANTS)
def test_a_planted_error_fails_and_names_its_field(plant):
    """The fp64 reference step, damaged, handed to the comparison as "the device" under the fp32 bounds of case 1: a failure must
    name the planted error's field AND region (PLANT_FIELDS; the init branch also its frame, init_N_len + 1 = 6)."""
    name = "c1_fft128_kl"
    _, _, states, ps, Bxs = _trajectory(name, "emulation")
    assert all(q is ps[0] for q in ps) and all(B is Bxs[0] for B in Bxs)  # (case 1 has one p and one Bx for all streams)
    p, Bx = ps[0], Bxs[0]
    want = os_.PLANT_FIELDS[plant]
    hits = []
    for k in range(3):
        for g, y in states[k]:
            ref = os_.reference(g, y, p, Bx)
            bnd, margins = os_.bounds(g, y, p, Bx, *ref, u=os_.U)
            ga, fr, tr = os_.frame_step(g, y, g["l"], p, g["H0"], Bx, plant=plant)
            dev = os_.after_state(g, ga, fr, p["framelength"])
            t = os_.Tally()
            os_.judge(dev, tr, g, ref, bnd, margins, p, Bx, t, f"stream {k} frame {g['l']}")
            hits += [f for f in t.fails if all(w in f for w in want)]
    print(f"\n{plant}: {len(hits)} failures naming {want}; first: {hits[0] if hits else None}")
    assert hits, f"planted error {plant} passed the comparison"


def _single_plant_hits(plant, name):
    """The single-stream driver (run_single) on a simulated device -- the float32 emulation behind OnlineSeparator's calls, with
    the planted error -- judged as the device test judges: the failures that name the plant's field and region."""
    views, precision, steps = os_.run_single(os_.sim_separator(plant=plant), name)
    assert precision == "fp32"
    want, hits, t = os_.PLANT_FIELDS[plant], [], os_.Tally()
    for k, ((p, Bx), sk) in enumerate(zip(views, steps)):
        for g, y, after, trace in sk:
            ref = os_.reference(g, y, p, Bx)
            bnd, margins = os_.bounds(g, y, p, Bx, *ref, u=os_.U)
            os_.judge(after, trace, g, ref, bnd, margins, p, Bx, t, f"stream {k} frame {g['l']}")
    hits = [f for f in t.fails if all(w in f for w in want)]
    return hits, t


# (the two plants of the single-stream adaptation also at s2's shape: 33 workgroups, m_a no multiple of 4)
@pytest.mark.parametrize("plant,name", [(pl, "c1_fft128_kl") for pl in os_.PLANTS] +
                         [(pl, "s2_fft512_ma21_wadapt") for pl in ("wg_partial", "r_up_shift")])
def test_a_planted_error_fails_through_the_single_stream_driver(plant, name):
    hits, _ = _single_plant_hits(plant, name)
    print(f"\n{plant} on {name}: {len(hits)} failures naming {os_.PLANT_FIELDS[plant]}; first: {hits[0] if hits else None}")
    assert hits, f"planted error {plant} passed the single-stream driver's comparison"


def test_the_single_stream_driver_passes_the_clean_emulation():
    """The same driver and comparison without a plant: no failure (what the plants are measured against), and the run judged
    as a device run is (judge_run: bounds, RMS, coverage, caps)."""
    views, precision, steps = os_.run_single(os_.sim_separator(), "c1_fft128_kl")
    dev = os_.judge_run("c1_fft128_kl (simulated device)", views, precision, steps)
    assert dev.solved >= 2 and not dev.fails


def test_s4_is_the_smallest_rank_past_the_persistent_kernel():
    """s4's frame solve must run through the ordinary plan loop at T = 1: its H-only plan has small_ok == false.  From the plan's
    describe text (Fm, the extra row, rp) and the LDS formula of plan_geometry, csrc/snmf_tu_geometry.hip: the persistent kernel
    needs (32 (ldh + ldr) + rp) 4 + 2 * 512 * 8 bytes with ldh = rp + 4, ldr = Fq + 4, Fq = Fm + 8 xr, against 160 KiB.  r = 161
    does not fit, r = 160 (one rank less: rp = 160) does."""
    import re
    from se_snmf_nat_amd.api import geometry_describe
    fft, _, _, Rx, Rd, _ = os_.GEO_S4
    F = fft // 2 + 1

    def small_ok(r):
        text = geometry_describe(F, 1, r, beta=1.0, w_update_ind=np.zeros(r))
        m = re.search(r"Fm=(\d+)\(\+(\d) VALU row\) rp=(\d+)", text)
        assert m, text
        Fm, xr, rp = (int(x) for x in m.groups())
        assert "hstep: k_hstep," in text  # (the plan loop's H step is the ordinary k_hstep at this shape)
        return (32 * ((rp + 4) + (Fm + 8 * xr + 4)) + rp) * 4 + 2 * 512 * 8 <= 160 * 1024

    assert Rx + Rd == 161 and not small_ok(Rx + Rd) and small_ok(Rx + Rd - 1)
    s3 = os_.GEO_S3
    assert small_ok(s3[3] + s3[4])  # s3 stays on k_hsolve_small


@pytest.mark.parametrize("name", list(os_.STOP_CASES))
def test_what_the_stop_armed_cases_reach_in_the_pure_oracle_run(name):
    """Cases 10 and 11 (shipped max_iter = 100, conv_eps = 1e-3): the reference run, the borderline rule of the issue (a relative
    cost change within 5 % of conv_eps) and the amplification over 8 draws at 1e-9, on the CPU.  The counts are the evidence that
    the rule and the cap on what may be left out (10 % of the pairs, no frame with `solved`) cannot both hold on these cases: the
    assertion on the cap below states what IS the case, and fails the day a restated rule makes the cases judgeable."""
    want = os_.STOP_CASES[name]
    recs = os_.stop_armed_oracle_run(name)
    border = [r["border_frame"] or r["border_adapt"] for r in recs]
    got = dict(pairs=len(recs), border_frame=sum(r["border_frame"] for r in recs), border_adapt=sum(r["border_adapt"] for r in recs),
               border=sum(border), solved=sum(r["solved"] for r in recs), solved_border=sum(r["solved"] and b for r, b in zip(recs, border)))
    judged = [r for r in recs if r["amp_max"] is not None]
    print(f"\n{name}: {got}; n_iter median {np.median([r['n_iter'] for r in recs]):.0f}, max {max(r['n_iter'] for r in recs)}, adapt_iters max "
          f"{max(r['adapt_iters'] for r in recs)}; {len(judged)} pairs left: amp max {max(r['amp_max'] for r in judged):.3g}, median of "
          f"the pairs' medians {np.median([r['amp_median'] for r in judged]):.3g}, draws that changed a decision "
          f"{sum(not r['linear'] for r in judged)}")
    assert got["pairs"] == want["pairs"] and got["solved"] == want["solved"], got
    for key in ("border_frame", "border_adapt", "border", "solved_border"):  # (an iterate on the band's edge may fall either way)
        assert abs(got[key] - want[key]) <= 2, (key, got)
    assert max(r["n_iter"] for r in recs) > 1 and max(r["adapt_iters"] for r in recs) > 1  # the stop is armed and fires
    assert all(r["linear"] and r["bound_ok"] for r in judged)  # on what is left the bound 4 n_iter tau max(1, amp) exists
    # the cap of the issue: at most 10 % of the pairs and no frame with `solved` may be left out.  It cannot hold:
    assert got["border"] > 0.5 * got["pairs"] and got["solved_border"] > 0.5 * got["solved"], got
