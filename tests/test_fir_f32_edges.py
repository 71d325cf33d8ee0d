"""The judge of tests/fir_f32_edges.py bites, and what it asks can be met (no GPU): an index-level numpy emulation of the split-fp16
arithmetic the matrix-core kernels of msdr_fir_f32_process use -- scale per window from the Mw of include/msdr.h, hi piece rounded toward
zero, lo piece the fp16 of the exact remainder, the three products, sums in fp32 -- makes clauses (a) and (b) on every census case; three
mutants of it each miss a named case; the sequential fp32 arm_fir_f32 of the oracle clears the judge on every case (the reference alone
must not fail it); behind every level step a clause (b) stretch picks up again (the coverage condition)."""
import functools

import numpy as np
import pytest

import fir_f32_edges as E

SPECS = E.census()
BY_ID = {s.id: s for s in SPECS}


@functools.lru_cache(maxsize=4)
def _case(spec_id):
    case = E.build(BY_ID[spec_id])
    return case, E.case_references(case)


def _scale_exp(mw):
    """fm_scale_exp: k = 141 - biased exponent of the window's largest magnitude, |k| <= 100."""
    e = int(np.array(mw, np.float32).view(np.uint32) >> 23) & 0xFF
    return max(-100, min(100, 141 - e))


def _rtz16(v):
    h = v.astype(np.float16)
    up = np.abs(h.astype(np.float32)) > np.abs(v)
    h[up] = np.nextafter(h[up], np.float16(0))
    return h


def _conv32(a16, b16, n):
    return np.convolve(a16.astype(np.float32), b16.astype(np.float32)[::-1])[b16.size - 1:b16.size - 1 + n]


def emulate_row(kind, h, hist, x, pinned=None, mutant=None):
    N, n = h.size, x.size
    xe = np.concatenate([hist, x]).astype(np.float32)
    if kind == "plain":
        return np.convolve(xe, h[::-1])[N - 1:N - 1 + n].astype(np.float32)
    ex = 14 - int(np.frexp(float(np.abs(h).max()))[1])                      # largest tap 2^ex in [2^13, 2^14)
    hs = np.ldexp(h.astype(np.float64), ex)
    th = hs.astype(np.float16)
    tl = (hs - th.astype(np.float64)).astype(np.float16)
    y = np.empty(n, np.float32)
    prev = None
    for i in range((n + E.TILE - 1) // E.TILE):
        t0, t1 = i * E.TILE, min((i + 1) * E.TILE, n)
        lo = E.window_lo(kind, N, i)
        if mutant == "previous_tile":
            lo = max(t0 - E.TILE, -(N - 1))
        if pinned:
            k = max(-100, min(100, 15 - int(np.log2(E.pinned_mw(pinned)))))
        else:
            k = _scale_exp(np.abs(xe[N - 1 + lo:N - 1 + t1]).max())
        xs = np.ldexp(xe[t0:N - 1 + t1], k).astype(np.float32)              # the N - 1 samples before the tile, and the tile
        xh = _rtz16(xs)
        xl = (xs - xh.astype(np.float32)).astype(np.float16)
        if mutant == "halo_min15" and prev is not None and N > 1:
            pk, ph, pl = prev                                               # the halo keeps the previous tile's pieces, times 2^min(dk, 15)
            rs = np.float32(2.0 ** min(k - pk, 15))
            xh[:N - 1] = (ph[-(N - 1):].astype(np.float32) * rs).astype(np.float16)
            xl[:N - 1] = (pl[-(N - 1):].astype(np.float32) * rs).astype(np.float16)
        if mutant == "no_lo":
            xl[:] = 0
        prev = (k, xh, xl)
        m = t1 - t0
        acc = _conv32(xl, th, m) + _conv32(xh, th, m) + _conv32(xh, tl, m)
        y[t0:t1] = np.ldexp(acc, -k - ex).astype(np.float32)
    return y


def emulate_case(case, mutant=None):
    s = case.spec
    return [np.stack([emulate_row(s.kind, case.taps[r], hist[r], case.x[r, o:o + m], s.pinned, mutant) for r in range(E.CHANNELS)])
            for _, o, m, hist in E.calls(case)]


def test_census_covers_the_issue():
    assert len(SPECS) == len({s.id for s in SPECS}) == 12 * 2 * 10
    assert {(s.ntaps, s.per_channel, s.kind) for s in SPECS} == {(8, False, "plain"), (600, False, "plain"), (16, False, "tq"), (100, False, "tq"),
                                                                 (256, False, "tq"), (289, False, "tq"), (290, False, "mf"), (321, False, "mf"),
                                                                 (512, False, "mf"), (513, False, "mf"), (100, True, "plain"), (512, True, "plain")}
    profiles = {p for s in SPECS for p in s.rows}
    assert len(profiles) == 16 and "flat" in profiles
    assert E.window_lo("tq", 100, 2) == 2048 - 128 and E.window_lo("mf", 512, 2) == 1024 and E.window_lo("mf", 512, 0) == -511


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: s.id)
def test_emulation_and_oracle_clear_the_judge(orc, spec):
    case, refs = _case(spec.id)
    assert E.coverage_gaps(case, refs) == []
    if not spec.pinned:
        assert min(r.covered for row in refs for r in row[:1]) > 0.99          # the flat row: all of it under clause (b)
    viol = E.judge_case(case, refs, emulate_case(case))
    assert not viol, E.format_violations(spec, "emulation", viol)
    if spec.pinned:
        return                                                                # (the oracle has no input range to pin)
    seq = np.stack([orc.fir_f32_blocks(case.taps[r], case.x[r], 128) for r in range(E.CHANNELS)])
    viol = E.judge_case(case, refs, [seq[:, o:o + m] for _, o, m, _ in E.calls(case)])
    assert not viol, E.format_violations(spec, "arm_fir_f32 (oracle)", viol)


def _mutant_violations(spec_id, mutant):
    case, refs = _case(spec_id)
    return E.judge_case(case, refs, emulate_case(case, mutant))


@pytest.mark.parametrize("spec_id", ["512-aligned-drops-2^0", "290-odd-drops-2^-60", "100-aligned-spikes-2^90"])
def test_mutant_halo_rescaled_by_min_dk_15(spec_id):
    """The halo kept from the tile before and multiplied by 2^min(dk, 15): a drop by 2^-20 leaves it 32 times too small in the first
    window that is all quiet.  The 2^-12 drop is inside the clamp and passes."""
    viol = _mutant_violations(spec_id, "halo_min15")
    hit = {v["profile"] for v in viol}
    # (a spike's window, too, is followed by one whose scale is 2^20 up)
    assert hit and hit <= {"drop20@tile", "drop20@+500", "drop34@tile", "drop20@segment", "drop20@history", "spike@first", "spike@last", "spike@500"}, hit
    want = "drop20@segment" if "spikes" in spec_id else "drop20@tile"
    assert any(v["profile"] == want and v["clause"] == "a" for v in viol) and any(v["profile"] == want and v["clause"] == "b" for v in viol)


@pytest.mark.parametrize("spec_id", ["256-aligned-spikes-2^0", "513-odd-rises-2^-60"])
def test_mutant_lo_piece_dropped(spec_id):
    viol = _mutant_violations(spec_id, "no_lo")
    assert {v["profile"] for v in viol} >= {"flat"} and any(v["clause"] == "b" and v["rms"] > 1e-5 for v in viol)


@pytest.mark.parametrize("spec_id", ["256-odd-drops-2^0", "100-aligned-drops-2^0", "16-odd-drops-2^0"])
def test_mutant_scale_from_the_whole_previous_tile(spec_id):
    """At 16 .. 289 taps the header's window reaches numTaps - 1 (rounded up to 32) samples back: a drop by 2^-20 500 samples into a tile
    must not cost the tile behind it -- under the loud scale its quiet samples keep 2^-39 x 2^22 = 2^-17 of their level, and the tile's
    stretch misses 1e-6.  (At 290 .. 513 taps the header's window IS the whole previous tile: there the mutant is the kernel.)"""
    viol = _mutant_violations(spec_id, "previous_tile")
    assert any(v["clause"] == "b" and (v["profile"], v["call"], v["tile"]) == ("drop20@+500", 0, 2) for v in viol), viol
    assert not _mutant_violations(spec_id.replace("256", "512").replace("100", "321").replace("16-", "290-"), "previous_tile")
