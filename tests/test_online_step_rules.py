"""The rules of tests/online_step.py, proved on the CPU before any GPU run: the restatement of the frame step agrees with the oracle's
sep_frame in fp64, every case's pure oracle run reaches the frames the issue asks for (both sides of init_N_len and P_len_l,
triggered and untriggered frames, a wrapped ring, solves with 0 < n_up < R_a), both float32 emulations (sums in index order and
reversed) stay inside every derived bound on every case, and every planted error fails, naming its field and region.

Run with -s to see, per case, the oracle's counts and the emulations' worst / bound per field."""
import numpy as np
import pytest

import online_step as os_

_cache = {}


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
            bnd, margins = os_.bounds(g, y, p, Bx, *ref, u=u)
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


@pytest.mark.parametrize("name", list(os_.CASES))
def test_the_restatement_is_the_oracle_and_the_case_reaches_its_frames(name):
    tallies, records, _, ps, _ = _trajectory(name, "oracle")
    cov = os_.coverage(records, ps[0])
    t = tallies[0]
    print(f"\n{name}: pure oracle run: {t.frames} (frame, stream) pairs, triggered {t.triggered}, solved {t.solved}, left out {t.left_out}; {cov}")
    print("\n".join(t.lines()))
    assert not t.fails, "\n".join(t.fails[:10])
    assert os_.coverage_ok(cov), cov
    assert t.caps_ok(), (t.left_out, t.border_rows, t.elem_out)


@pytest.mark.parametrize("name", list(os_.CASES))
def test_both_emulations_stay_inside_every_bound(name):
    (fwd, rev), records, _, ps, _ = _trajectory(name, "emulation")
    cov = os_.coverage(records, ps[0])
    print(f"\n{name}: emulated run: {fwd.frames} pairs, triggered {fwd.triggered}, solved {fwd.solved}, left out {fwd.left_out}; {cov}")
    print("index order:\n" + "\n".join(fwd.lines()))
    print("reversed:\n" + "\n".join(rev.lines()))
    assert not fwd.fails, "\n".join(fwd.fails[:10])
    assert not rev.fails, "\n".join(rev.fails[:10])
    assert os_.coverage_ok(cov), cov
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
