"""The host layer's transfers are ordered on the context's stream ("Transfers"; profiles/host_transfers/README.md): two shapes in
which a bare copy on the null stream raced with work the chain's stream still held.

 1. The first input-row map of a process (profiles/pc_frame/README.md recorded it): the first msdr_chain_set_input_rows of a chain clears the
    new table on the stream and then uploads the rows.  One child process that creates no other chain first; fp32, NCO mixer, 13 taps,
    osc_len 24, seven receivers on three rows, the map set ONCE, one call of 128 samples.  Audio and FIR history are bit-identical to the
    same chain fed the replicated rows without a map.
 2. msdr_chain_reset directly behind a long call of an fp32 chain under msdr_chain_set_bank_post with the LMS filter on: the reset rewrites
    the LMS records the call's post_anr_f32_kernel is still stepping.  The next 256-sample call is bit-identical to a fresh chain's first.
    N_LONG: the smallest power of two at which the long call's GPU time clearly exceeds the reset's host time on the library before this
    change.  The chain's own kernel timing brackets the demodulator kernel only, 0.011 - 0.030 ms at every length from 2^5 to 2^18 and never
    above the reset's 0.04 - 0.05 ms (worst seen 0.081): the call's GPU time is the sequential LMS pass behind it, read as the call's wall
    time to an idle stream, 0.89 ms at 2^9 (of which some 0.07 ms are the host's) and 1.63 - 1.77 ms at 2^10, twenty times the reset's
    worst.  That library failed this test at every length from 2^5 to 2^18, 512 of 512 samples (profiles/host_transfers/README.md)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gpuhelp import ctx, msdr  # noqa: F401

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MAP = [0, 1, 0, 2, 1, 0, 2]
CH, NT, L, N = 7, 13, 24, 128
N_LONG = 1 << 10


def osc_tables(rng, rows):
    a = 2 * np.pi * rng.integers(1, L, rows)[:, None] * np.arange(L)[None, :] / L + rng.uniform(0, 6.28, rows)[:, None]
    oi, oq = np.round(32767 * np.sin(a)).astype(np.int16), np.round(32767 * np.cos(a)).astype(np.int16)
    return (oi / 32768.0).astype(np.float32), (oq / 32768.0).astype(np.float32)


def first_map_child():
    """runs in a process of its own: the chain with the map is the first chain the process makes"""
    ctx = msdr.Context(0)
    rng = np.random.default_rng(4100)
    ci, cq = ((rng.standard_normal((CH, NT)) * 0.08).astype(np.float32) for _ in range(2))
    oi, oq = osc_tables(rng, 1)
    modes = np.array([msdr.MODE_LSB, msdr.MODE_USB, msdr.MODE_AM, msdr.MODE_CW, msdr.MODE_AM, msdr.MODE_LSB, msdr.MODE_USB], np.int32)
    x = rng.integers(-20000, 20001, (max(MAP) + 1, N)).astype(np.int16)
    got = []
    for mapped in (True, False):
        chain = msdr.Chain(ctx, msdr.ARITH_F32, CH, ci[0], cq[0], mixer=msdr.MIXER_NCO, modes=modes, osc_i=oi[0], osc_q=oq[0])
        chain.set_taps_channels_f32(0, ci, cq)
        if mapped:
            chain.set_input_rows(np.array(MAP))          # once
        dy = ctx.array((CH, N), np.float32)
        chain.process(ctx.to_device(x if mapped else np.ascontiguousarray(x[MAP])), dy, N)
        got.append((dy.download(), np.stack([chain.fir_history(c) for c in range(CH)]), chain.info()["kernel"]))
        chain.close()
    (a0, h0, k0), (a1, h1, k1) = got
    assert k0 == k1, (k0, k1)
    assert np.isfinite(a1).all() and np.abs(a1).max() > 0
    bad = [c for c in range(CH) if not np.array_equal(a0[c], a1[c])]
    assert not bad, "receivers %s (rows %s) do not hear their mapped row" % (bad, [MAP[c] for c in bad])
    assert np.array_equal(h0, h1) and h0.any(), "FIR history"
    ctx.close()
    print("FIRST_MAP_OK")


def test_the_first_map_of_a_process_is_in_place_before_the_first_call():
    p = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import test_gpu_host_transfers as t; t.first_map_child()" % HERE],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "FIRST_MAP_OK" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])


def lms_chain(ctx, taps, oi, oq, steps):
    chain = msdr.Chain(ctx, msdr.ARITH_F32, 2, taps, taps, mixer=msdr.MIXER_NCO, mode=msdr.MODE_AM, osc_i=oi, osc_q=oq)
    chain.set_bank_post(True)
    chain.set_nco_channels(0, steps, np.zeros(2, np.uint32))          # (a reset puts every phase back to 0)
    chain.set_anr(np.ones(2, np.int32))
    return chain


def reset_behind_a_long_call(ctx, n_long):
    """-> (the 256-sample call behind long call + reset, a fresh chain's first 256-sample call, the long call's audio)"""
    rng = np.random.default_rng(4200)
    taps = (np.hanning(NT + 2)[1:-1] / np.hanning(NT + 2).sum()).astype(np.float32)
    oi, oq = osc_tables(rng, 1)
    steps = (rng.integers(1, 1 << 32, 2, dtype=np.uint64) | np.uint64(1)).astype(np.uint32)
    t = np.arange(n_long + 256)
    x = np.round(9000 * np.sin(2 * np.pi * 0.11 * t)[None, :] + rng.normal(0, 2500, (2, t.size))).astype(np.int16)
    short = ctx.to_device(np.ascontiguousarray(x[:, n_long:]))
    fresh = lms_chain(ctx, taps, oi[0], oq[0], steps)
    want = ctx.array((2, 256), np.float32)
    fresh.process(short, want, 256)
    want = want.download()
    assert fresh.info()["flavour"] & msdr.FLAVOUR_BANK_POST
    fresh.close()
    chain = lms_chain(ctx, taps, oi[0], oq[0], steps)
    long_in, long_out, got = ctx.to_device(np.ascontiguousarray(x[:, :n_long])), ctx.array((2, n_long), np.float32), ctx.array((2, 256), np.float32)
    ctx.synchronize()
    chain.process(long_in, long_out, n_long)
    chain.reset()          # at once: the long call is still running
    chain.process(short, got, 256)
    got, moved = got.download(), long_out.download()
    chain.close()
    return got, want, moved


def test_a_reset_behind_a_long_call_leaves_the_lms_records_at_their_start(ctx):
    got, want, moved = reset_behind_a_long_call(ctx, N_LONG)
    assert np.isfinite(moved).all() and np.abs(moved[:, -256:]).max() > 0          # (the long call ran, LMS and all)
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    assert np.array_equal(got, want), "after the reset: %d of %d samples differ from a fresh chain's, worst %.3g" % (
        int((got != want).sum()), got.size, float(np.abs(got - want).max()))
