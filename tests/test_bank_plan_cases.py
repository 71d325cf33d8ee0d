"""tests/bank_plan.py held on the CPU: the model against the models the suite already trusts (bit for bit, one single-feature plan each), split
invariance of every plan, the coverage of the two tables as asserted conditions, and the levels of every plan.  No GPU: the tables and the
model are finished before tests/test_gpu_bank_plans*.py hold the library to them."""
import numpy as np
import pytest

import agc_model
import bank_plan as P
import cx_cases
import prefilter_model
import spectrum_model

Q15, F32 = P.plans_q15(), P.plans_f32()
ALL = Q15 + F32


def ident(p):
    return "%s%d" % ("f" if p.f32 else "q", p.seed)


def streams(plan, res):
    """per receiver the input it heard over the accepted calls of a plan whose map never changes: (xi [CH, n], xq [CH, n] or None, si, sq)"""
    ini = plan.initial()
    xs = [o.x for s, o in res if s[0] == "call" and o.status == P.OK]
    x = np.concatenate(xs, axis=1)
    n = x.shape[1]
    si, sq = P.Bank(ini["steps"], ini["phases"]).advance(n)
    heard = x[ini["rows"]]
    return (heard[..., 0], heard[..., 1], si, sq) if x.ndim == 3 else (heard, None, si, sq)


def gather(res, name):
    return np.concatenate([getattr(o, name) for s, o in res if s[0] == "call" and o.status == P.OK], axis=1)


# ------------------------------------------------------------------------------------------------ 1. the model against the trusted models
def test_the_bank_is_the_nco_tests_bank():
    from test_gpu_nco_per_channel import Bank
    rng = np.random.default_rng(5)
    steps, phases = P.off_grid_steps(rng, 4), rng.integers(0, 1 << 32, 4, dtype=np.uint64)
    a, b = P.Bank(steps, phases), Bank(steps, phases)
    for n in (7, 128, 33):
        for u, v in zip(a.advance(n), b.advance(n)):
            assert np.array_equal(u, v)
        a.retune(1, steps[:2] + np.uint64(2))
        b.retune(1, steps[:2] + np.uint64(2))
    assert np.array_equal(a.phi, b.phi)


def test_against_prefilter_model(orc):
    plan = P.Plan(901, [("prefilter", 1, 4, 16), ("decim", 2, 3), ("call", 3, 24, 1, None), ("call", 4, 8, 1, None), ("call", 5, 40, 1, None)])
    res, m = P.run_model(plan, orc)
    xi, _, si, sq = streams(plan, res)
    audio, pairs = gather(res, "audio"), gather(res, "pairs")
    for c in range(P.CH):
        a, fi, fq = prefilter_model.model_q15(orc, xi[c], si[c], sq[c], plan.prefilter_row(4, 16), 4, m.modes[c], m.ti[c], m.tq[c], 3)
        assert np.array_equal(audio[c], a) and np.array_equal(pairs[c, :, 0], fi) and np.array_equal(pairs[c, :, 1], fq), c
    assert np.abs(audio.astype(np.int32)).max() > 1000


@pytest.mark.parametrize("direction", [0, 1])
def test_against_the_complex_input_composition(orc, direction):
    plan = P.Plan(902, [("cx", 1, 1, direction), ("call", 2, 40, 1, None), ("call", 3, 8, 1, None), ("call", 4, 96, 1, None)])
    res, m = P.run_model(plan, orc)
    xi, xq, si, sq = streams(plan, res)
    audio, pairs = gather(res, "audio"), gather(res, "pairs")
    for c in range(P.CH):
        a, fi, fq, _, _ = cx_cases.compose_q15(orc, xi[c], xq[c], si[c], sq[c], direction, m.modes[c], m.ti[c], m.tq[c])
        assert np.array_equal(audio[c], a) and np.array_equal(pairs[c, :, 0], fi) and np.array_equal(pairs[c, :, 1], fq), c


def test_against_the_agc_model_over_thirty_calls(orc):
    """gain on, receivers 1 .. 3 at gains of their own, every AGC stepping: tests/agc_model.BankQ15 call by call -- audio, gained pairs, the
    ungained meter and all 32 words of every record"""
    calls = [("call", 10 + k, 64, 1, None) for k in range(30)]
    plan = P.Plan(903, [("gain", 1, 1), ("gainch", 2, 1, 3), ("agc", 3, (1, 1, 1, 1, 1)), ("decim", 4, 2)] + calls)
    res, m = P.run_model(plan, orc)
    ini = plan.initial()
    xi, _, si, sq = streams(plan, res)
    ref = agc_model.BankQ15(orc, xi, None, si, sq, ini["modes"], ini["ti"], ini["tq"])
    for c, g in enumerate(res[1][1].args[1]):
        ref.rx[1 + c].set_gain(g)
    for rx in ref.rx:
        rx.on = 1
    lo, moved = 0, set()
    m2 = P.BankModel(plan, orc)
    for s in plan.steps:
        o = m2.apply(s)
        if s[0] != "call":
            continue
        a, p, met = ref.call(lo, lo + o.n, 2)
        lo += o.n
        assert np.array_equal(o.audio, a) and np.array_equal(o.pairs, p) and np.array_equal(o.meter, met), s
        for c in range(P.CH):
            assert np.array_equal(m2.rx[c].words(), ref.rx[c].words()), (s, c)
            moved |= {t for tag in ref.rx[c].branches for t in tag}
    assert {"up", "dropped"} <= moved or len(moved) >= 2, moved          # (the trajectory moves the gains: thirty steps wrap the ring of 25)


def test_against_the_spectrum_model(orc):
    """every = 3 at D2 = 8: draws at calls 0, 3, 6; each window the last 64 of (zeros ++ every pair so far), its transform the oracle's"""
    calls = [("call", 10 + k, 16, 1, None) for k in range(8)]
    plan = P.Plan(904, [("decim", 1, 8), ("spectrum", 2, 1, 1, 3)] + calls)
    res, _ = P.run_model(plan, orc)
    tail, tick, k = spectrum_model.Tail(P.CH), spectrum_model.Tick(3), 0
    for s, o in res:
        if s[0] != "call":
            continue
        window = tail.push(o.pairs)
        assert o.drew == tick.tick() == (k in (0, 3, 6)), k
        if o.drew:
            for c in range(P.CH):
                b = spectrum_model.cfft64_q15(orc, window[c])
                assert np.array_equal(o.bins[c], b) and np.array_equal(o.power[c], spectrum_model.power_q15(b)), (k, c)
        else:
            assert o.bins is None and o.power is None
        k += 1


def test_against_the_decimation_tests_indexing(orc):
    """test_gpu_decim_per_channel.live_stream's expected value: the full-rate oracle_row over the stream, taken at o + D - 1 + D * arange per call,
    across a live change of D"""
    from test_gpu_osc_per_channel import oracle_row
    plan = P.Plan(905, [("decim", 1, 4), ("call", 2, 24, 1, None), ("call", 3, 40, 1, None), ("decim", 4, 3), ("call", 5, 64, 1, None), ("decim", 6, 1), ("call", 7, 96, 1, None)])
    res, m = P.run_model(plan, orc)
    xi, _, si, sq = streams(plan, res)
    n = xi.shape[1]
    n128 = (n + 127) // 128 * 128
    pad = lambda v: np.concatenate([v, np.zeros(n128 - n, v.dtype)])          # noqa: E731
    index, o, D = [], 0, 1
    for s, out in res:
        if s[0] == "decim":
            D = s[2]
        else:
            index.append(o + D - 1 + D * np.arange(out.n_out))
            o += out.n
    index, audio = np.concatenate(index), gather(res, "audio")
    for c in range(P.CH):
        want = oracle_row(orc, pad(xi[c]), pad(si[c]), pad(sq[c]), lambda b: (m.modes[c], m.ti[c], m.tq[c]), {})
        assert np.array_equal(audio[c], want[index]), c


# ------------------------------------------------------------------------------------------------ 2. the plans themselves
@pytest.mark.parametrize("plan", ALL, ids=ident)
def test_a_plan_prints_parses_and_shrinks(plan):
    assert str(P.Plan.parse(str(plan))) == str(plan)
    assert str(P.draw(plan.seed, plan.f32)) == str(plan)          # drawn from the seed by the rule, twice the same
    for i in range(len(plan.steps)):          # a plan with a step deleted is a plan: the host state machine runs it, refusing what the header refuses
        shorter = plan.without(i)
        assert len(shorter.steps) == len(plan.steps) - 1
        P.run_model(shorter)


@pytest.mark.parametrize("plan", ALL, ids=ident)
def test_a_refused_step_leaves_the_model_unchanged(plan, orc):
    m, refused = P.BankModel(plan, orc), 0
    for s in plan.steps:
        before = repr(m.state()) + repr((m.in_force(), m.clear, m.T, m.modes.tolist(), m.rows.tolist(), m.anr.tolist(), m.meter, m.iq, m.pitch, m.tick.counter))
        o = m.apply(s)
        if o.status != P.OK:
            refused += 1
            assert before == repr(m.state()) + repr((m.in_force(), m.clear, m.T, m.modes.tolist(), m.rows.tolist(), m.anr.tolist(), m.meter, m.iq, m.pitch, m.tick.counter)), s
    assert refused >= 1


@pytest.mark.parametrize("plan", [p for p in ALL if not any(s[0] in ("agc", "spectrum") for s in p.steps)], ids=ident)
def test_split_invariance(plan, orc):
    """cutting every call in two legal halves changes no audio or pair sample of the model"""
    whole, _ = P.run_model(plan, orc)
    halves, cuts = P.split(plan)
    parts, _ = P.run_model(halves, orc)
    calls = [o for s, o in whole if s[0] == "call" and o.status == P.OK]
    assert len(calls) == len(cuts) >= 6
    for o, (i, j) in zip(calls, cuts):
        a, b = parts[i][1], parts[j][1]
        assert a.status == b.status == P.OK and a.n + b.n == o.n
        assert np.array_equal(np.concatenate([a.pairs, b.pairs], axis=1), o.pairs)
        if o.audio_call:
            assert np.array_equal(np.concatenate([a.audio, b.audio], axis=1), o.audio)


@pytest.mark.parametrize("plan", ALL, ids=ident)
def test_levels(plan, orc):
    """neither silent nor saturated throughout: per receiver some call is above 1000 (of 32768), and some call stays inside the range"""
    res, _ = P.run_model(plan, orc)
    peak = np.array([np.abs(o.audio.astype(np.float64)).max(axis=1) * (32768.0 if plan.f32 else 1.0) for s, o in res if s[0] == "call" and o.status == P.OK and o.audio_call])
    assert (peak.max(axis=0) > 1000).all() and np.isfinite(peak).all(), peak
    if not plan.f32:          # (an fp32 chain has no range to saturate at)
        assert (peak.min(axis=0) < 32767).all(), peak


# ------------------------------------------------------------------------------------------------ 3. coverage, as conditions on the tables
SURVEYS = [P.survey(p) for p in ALL]


def total(key):
    return sum(d[key] for d in SURVEYS)


def test_the_shape_of_the_tables():
    assert len(Q15) == 32 and len(F32) == 10 and len({p.seed for p in Q15}) == 32 and len({p.seed for p in F32}) == 10
    assert sum(p.sections == 2 for p in F32) == 5 and not any(p.pll or p.post or p.nodes for p in F32)
    assert any(p.pll for p in Q15) and any(p.post and not p.pll for p in Q15) and any(p.nodes for p in Q15)
    for p in F32:          # "held gains (no AGC stepping) ... No PLL or LMS"
        assert not {s[0] for s in p.steps} - set(P.F32_KINDS)


@pytest.mark.parametrize("d", SURVEYS, ids=[ident(p) for p in ALL])
def test_every_plan_has_its_frame(d):
    assert 10 <= d["steps"] <= 14 and d["calls"] >= 6
    assert d["short"] >= 2          # "at least two calls per plan are shorter than the FIR history in force"
    assert d["refusals"] >= 1       # "every plan has its refusal"
    assert d["max_gen"] < 16        # "no plan reaches 16 generations in one history"


def test_every_step_kind_occurs_four_times():
    kinds = {}
    for d in SURVEYS:
        for k, n in d["kinds"].items():
            kinds[k] = kinds.get(k, 0) + n
    assert all(kinds.get(k, 0) >= 4 for k in P.KINDS + ("call_iq",)), kinds


def test_every_allowed_pair_of_switches_is_in_force_together_in_an_audio_call():
    pairs = set().union(*(d["pairs"] for d in SURVEYS))
    assert not P.wanted_pairs() - pairs, [tuple(p) for p in P.wanted_pairs() - pairs]
    assert not pairs & P.EXCLUDED


def test_both_orders_of_every_live_pair():
    orders = set().union(*(d["orders"] for d in SURVEYS))
    assert not P.wanted_orders() - orders, sorted(P.wanted_orders() - orders)


def test_the_history_gated_switches_go_on_behind_init_fir_and_reset_and_off():
    on, off = set().union(*(d["gated_on"] for d in SURVEYS)), set().union(*(d["gated_off"] for d in SURVEYS))
    assert P.WANTED_GATED_ON <= on and set(P.WANTED_GATED_OFF) <= off, (on, off)          # (msdr_chain_set_bank_post never goes off: "0 after 1 is MSDR_STATUS_ARGUMENT_ERROR")
    assert sum(p.post for p in Q15) >= 4


def test_every_refusal_the_header_names_occurs():
    kinds = {}
    for d in SURVEYS:
        for k, n in d["refusal_kinds"].items():
            kinds[k] = kinds.get(k, 0) + n
    assert not set(kinds) - set(P.REFUSALS), kinds          # (no refused step that is none of them)
    assert all(kinds.get(k, 0) >= n for k, n in P.WANTED_REFUSALS.items()), kinds


def test_generations_retunes_iq_only_calls_lms_and_agc():
    """P.WANTED_COUNTS: calls with three or more oscillator generations alive in their window; retunes directly behind an ACCEPTED set_decimation or
    tap change with a generation pending; two retunes with no call between them (not a generation); I/Q-only calls; and over the Q15 table resets
    that move the cadence (what mutant 7 changes), audio calls with the LMS filter on at D > 1, calls behind which an AGC steps"""
    for key, n in P.WANTED_COUNTS.items():
        over = SURVEYS[:32] if key in ("reset_mid_cadence", "lms_decimated", "agc_stepping") else SURVEYS
        assert sum(d[key] for d in over) >= n, (key, sum(d[key] for d in over), n)
    assert sum(d["phaseless"] > 0 for d in SURVEYS[:32]) >= 8          # (what mutant 6 changes)


# ------------------------------------------------------------------------------------------------ 4. the fp32 plans' reference is within reach
@pytest.mark.parametrize("plan", F32, ids=ident)
def test_the_fp32_composition_is_close_to_float64(plan, orc):
    """cx_cases.judge_f32 asks e_orc < 2e-6 of the reference itself before it judges the device: held here per call and receiver, without a GPU"""
    res, _ = P.run_model(plan, orc, truth=True)
    worst = 0.0
    for s, o in res:
        if s[0] == "call" and o.status == P.OK:
            for c in range(P.CH):
                worst = max(worst, cx_cases.rel(o.pairs[c], o.truth_pairs[c]), cx_cases.rel(o.audio[c], o.truth_audio[c]) if o.audio_call else 0.0)
    print("fp32 plan %d: e_orc at most %.3e" % (plan.seed, worst))
    assert worst < 2e-6
