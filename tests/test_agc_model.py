"""tests/agc_model.py pinned to the oracle.  CPU only.

1. The accumulators: at multiplier 65536 the gained pair is ssat16(acc >> 15), and that is orc.fir_q15_blocks of the mixed stream and the
   i_out / q_out of orc.chain_q15(..., want_iq=True) -- so `acc` is arm_fir_fast_q15's accumulator, wrapping included.
2. The rule: Rx.step against orc.agc_block on a block that is zero but for block[0] = absmax, from five start gains over six levels (silence
   among them) held long enough to fill the ring, then seeded random levels; the inputs are asserted to reach every branch.
3. The gain cases of the GPU tests are asserted to hold saturated outputs, a wrapped accumulator, a negative gain and a zero multiplier."""
import ctypes as C

import numpy as np

import agc_model as M
import orclib

NT = 102
LEVELS = (0, 16000, 18800, 21300, 24600, 32767)          # f = 16000 / d: +inf, 1.0 (dead zone), 0.851, 0.751, 0.650, 0.488
START = (0.05, 0.25, 1.0, 37.5, 39.9)


def taps(orc):
    return orc.calc_fir_coeffs(NT, 2800.0)[:NT].copy()


def test_unity_gain_is_the_oracles_fir_and_chain(orc):
    rng = np.random.default_rng(41)
    n = 4 * M.B
    t = taps(orc)
    for amp in (300, 30000):
        x = rng.integers(-amp, amp + 1, n).astype(np.int16)
        acc = M.acc_q15(x, t)
        rc, y = orc.fir_q15_blocks(t, x, M.B)
        assert rc == 0
        assert np.array_equal(M.pair_q15(acc, 65536), y) and np.array_equal(M.plain_q15(acc), y)
    si = np.round(32767 * np.sin(2 * np.pi * 0.21 * np.arange(n))).astype(np.int16)
    sq = np.round(32767 * np.cos(2 * np.pi * 0.21 * np.arange(n))).astype(np.int16)
    x = rng.integers(-30000, 30001, n).astype(np.int16)
    mi, mq = M.mixed_q15(orc, x, None, si, sq, 1)
    st = {}
    want = [np.concatenate(p) for p in zip(*[orc.chain_q15(x[o:o + M.B], orclib.LSB, t, t, mixer=1, osc_i=si[o:o + M.B], osc_q=sq[o:o + M.B], state=st, want_iq=True)
                                               for o in range(0, n, M.B)])]
    gi, gq = M.pair_q15(M.acc_q15(mi, t), 65536), M.pair_q15(M.acc_q15(mq, t), 65536)
    assert np.array_equal(gi, want[1]) and np.array_equal(gq, want[2])
    assert np.array_equal(orc.demod_q15(orclib.LSB, gi, gq), want[0])


def test_the_multiplier_is_the_oracles(orc):
    for g in (0.0, 1.0, -2.5, 0.25, 37.5, 40.0, 1e-6, -1e-6, 32767.0, 40000.0, -40000.0, 0.1, 1.0 / 3.0):
        assert M.multiplier(g) == orc.amp_multiplier(g), g
    assert M.multiplier(1.0) == 65536 and M.multiplier(1e-6) == 0


def oracle_agc(orc, gain):
    a = orclib.Agc()
    orc.lib.orc_agc_init(C.byref(a))
    a.AGC_val = gain
    a.multiplier = orc.amp_multiplier(gain)
    return a


def test_the_rule_is_orc_agc_block_and_every_branch_is_met(orc):
    rng = np.random.default_rng(42)
    seen, steps, mismatches = set(), 0, 0
    for g0 in START:
        a = oracle_agc(orc, g0)
        rx = M.Rx()
        rx.set_gain(g0)
        rx.on = 1
        seq = np.concatenate([np.full(60, lv) for lv in LEVELS] + [rng.choice(LEVELS, 200), np.full(400, 32767), np.zeros(200, np.int64)])
        for absmax in seq:
            block = np.zeros(M.B, np.int16)
            block[0] = absmax
            orc.agc_block(a, block)
            rx.after_call(int(absmax))
            steps += 1
            mismatches += not (a.agc_idx == rx.idx and M.bits(a.AGC_val) == M.bits(rx.val) and a.multiplier == rx.mult and
                               np.array_equal(np.array(a.agc_buffer[:], np.int32), rx.ring))
        for tag in rx.branches:
            seen.update(tag)
        assert rx.steps == seq.size
    assert mismatches == 0, (mismatches, steps)
    assert steps == len(START) * 1160
    # the five rules, the dead zone, the AGC_Max cap, the AGC_val <= 0.1 floor, d == 0, the dropped 26th store
    assert seen == {"up", "down50", "down200", "down2000", "down4000", "dead", "max", "floor", "d0", "dropped"}, seen


def test_the_clamp_to_32767_is_needed(orc):
    """AGC() fed a lone -32768 reads absmax 0 (orc_agc_block stores 0 in the ring under a full-scale sample); the bank's absmax is
    min(32767, |.|), so the same sample reads full scale"""
    a = oracle_agc(orc, 1.0)
    block = np.zeros(M.B, np.int16)
    block[0] = -32768
    orc.agc_block(a, block)
    assert a.agc_idx == 24 and a.agc_buffer[24] == 0
    block[0] = 32767
    orc.agc_block(a, block)
    assert a.agc_idx == 23 and a.agc_buffer[23] == 32767
    rx = M.Rx()
    assert rx.absmax_of(np.array([-32768], np.int16), np.array([0], np.int16)) == 32767


def gain_cases(orc):
    """(name, accumulators, multiplier) of the corners the GPU tests run: tests/test_gpu_agc_per_channel.py builds its inputs from these"""
    t = taps(orc)
    rng = np.random.default_rng(43)
    x = rng.integers(-300, 301, 512).astype(np.int16)
    loud = rng.integers(-30000, 30001, 512).astype(np.int16)
    full = np.full(NT, 32767, np.int16)
    edge = np.full(512, -32768, np.int16)
    return [("weak x 37.5", M.acc_q15(x, t), M.multiplier(37.5)),
            ("loud x 40: saturated", M.acc_q15(loud, t), M.multiplier(40.0)),
            ("all-32767 taps, -32768 input: wrapped", M.acc_q15(edge, full), M.multiplier(0.25)),
            ("negative gain", M.acc_q15(loud, t), M.multiplier(-2.5)),
            ("zero multiplier", M.acc_q15(loud, t), M.multiplier(0.0))]


def test_the_gain_cases_hold_the_corners(orc):
    cases = dict((n, (a, m)) for n, a, m in gain_cases(orc))
    a, m = cases["loud x 40: saturated"]
    g = M.pair_q15(a, m)
    assert (g == 32767).any() and (g == -32768).any()
    a, m = cases["all-32767 taps, -32768 input: wrapped"]
    exact = -32768 * 32767 * NT
    assert exact < -(1 << 31) and int(a[-1]) == ((exact + (1 << 31)) % (1 << 32)) - (1 << 31) != exact          # the accumulator wrapped
    a, m = cases["negative gain"]
    assert m < 0 and np.array_equal(np.sign(M.pair_q15(a, m)[np.abs(a) > (1 << 16)]), -np.sign(a[np.abs(a) > (1 << 16)]))
    a, m = cases["zero multiplier"]
    assert m == 0 and not M.pair_q15(a, m).any()
    # the amplifier on the accumulator keeps what the amplifier behind the shift has lost (the reason the gain lives in the kernels)
    a, m = cases["weak x 37.5"]
    before = M.pair_q15(a, m)
    after = orc.amp_update(m, M.plain_q15(a))
    assert np.unique(before).size > 1.5 * np.unique(after).size
    # and python's own integers agree with the vectorised form
    for acc in (int(a[5]), -(1 << 31), (1 << 31) - 1, -1, 0):
        for mm in (m, -163840, 0, 65536, 2147418112, -2147418112):
            want = max(-32768, min(32767, (acc * mm) >> 31))
            assert int(M.pair_q15(np.array([acc], np.int32), mm)[0]) == want, (acc, mm)


def test_the_corner_bank_of_the_gpu_tests_holds_the_corners(orc):
    """tests/test_gpu_agc_per_channel.py::test_the_corners runs agc_model.corners(): here its inputs are shown to be what they are meant to be"""
    assert (orclib.AM, orclib.LSB, orclib.USB) == (1, 2, 3)
    k = M.corners(taps(orc))
    si, sq = M.nco_rows(k["steps"], k["phases"], k["n"])
    assert (si[0, 0], sq[0, 0]) == (0, 32767) and (si[1, 0], sq[1, 0]) == (23170, 23170)
    bank = M.BankQ15(orc, k["x"], None, si, sq, k["modes"], k["taps"], k["taps"])
    for c, rx in enumerate(bank.rx):
        rx.set_gain(k["gains"][c])
    audio, pairs, _ = bank.call(0, k["n"])
    # 0, 1: the exact sums lie outside 32 bits, the accumulators are their low 32 bits
    mi, mq = M.mixed_q15(orc, k["x"][0], None, si[0], sq[0], 1)
    exact = int(mi[-1]) * 32767 * NT
    assert mi[-1] == -32767 and exact < -(1 << 31) and int(bank.acc[0][0][-1]) == ((exact + (1 << 31)) % (1 << 32)) - (1 << 31)
    mi, mq = M.mixed_q15(orc, k["x"][1], None, si[1], sq[1], 1)
    for stream, acc in ((mi, bank.acc[1][0]), (mq, bank.acc[1][1])):
        exact = int(stream[-1]) * 32767 * NT
        assert abs(exact) > (1 << 31) and int(acc[-1]) == ((exact + (1 << 31)) % (1 << 32)) - (1 << 31)
    assert bank.rx[1].mult < 0 and pairs[1].any()
    assert bank.rx[2].mult == 0 and not pairs[2].any() and not audio[2].any() and bank.rx[2].absmax == 0
    assert (pairs[3] == 32767).any() and (pairs[3] == -32768).any() and bank.rx[3].absmax == 32767
