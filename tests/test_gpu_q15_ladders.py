"""The census of the Q15 serial-recurrence ladders on the GPU (the table: tests/q15_ladder_cases.py; its CPU checks: tests/test_q15_ladder_cases.py).

Every entry -- one per branch and per fall-back edge of the node ladder behind a chain, the stand-alone node's and the front end's -- creates
its instance with the entry's switches in the environment (every one is read at create time), runs three or more consecutive calls so that
state is carried, and after EVERY call requires

  * the getter (Chain.node_kernel / BiquadQ15.last_kernel / Frontend.last_kernel) to name exactly the entry's kernel: all of these kernels
    give the same bits, so a silent fall-back to another of them passes every comparison of values;
  * every judged channel to equal the oracle bit for bit (orc.chain_q15 with its nodes, orc.biquad_teensy_update, orc.frontend_run);
  * the memory around the data to be untouched: the buffer has a guard of at least one row in front and one behind, filled with 0x5A5A, and the
    data pointer is the aligned pointer + the guard + the entry's alignment offset.  The kernels work in place with 16-byte loads and round
    channel counts up to workgroups: a wrong launch condition tramples a guard, not only a value.

At the end the state records (BiquadQ15.definition, Frontend.state) of the first channel, the last and one on each side of every 16-channel
boundary (16 divides every workgroup's channel count) meet the oracle's.  A chain has no getter for its nodes' records: they are held by
continuation -- the later calls start from them.

Inputs: uniform over the full int16 range, one row held at -32768, one at +32767, one full-scale square wave of period 80 -- saturation and the
14-bit residue together.  Coefficients: the reference's low-pass (5400 Hz x CORR, Q 0.54) and Q = 15 notch at 3000 Hz x CORR; multi-stage nodes:
the Linkwitz-Riley four and the high-shelf + notch."""
import numpy as np
import pytest

import orclib
import q15_ladder_cases as census
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_frontend import _adc, _check_state

pytestmark = pytest.mark.gpu
CORR = orclib.AUDIO_SAMPLE_RATE_EXACT / 24000.0
GUARD = 0x5A5A
ALL_CHANNELS_UP_TO = 130     # entries with more channels are judged on the first 16, the last 16 and 16 around every multiple of 64
SWITCHES = ("MSDR_Q15_NO_FUSE", "MSDR_BIQUAD_BLK", "MSDR_BIQUAD_PIPE_CH", "MSDR_FRONTEND_PIPE_CH", "MSDR_NO_BLOCK", "MSDR_MB_NW", "MSDR_MB_FILL")


def judged(ch):
    if ch <= ALL_CHANNELS_UP_TO:
        return list(range(ch))
    s = set(range(16)) | set(range(ch - 16, ch))
    for m in range(64, ch, 64):
        s |= set(range(m - 8, min(m + 8, ch)))
    return sorted(s)


def record_channels(ch):
    want = {0, ch - 1} | {c for m in range(16, ch, 16) for c in (m - 1, m)}
    return sorted(want & set(judged(ch)))


def set_switches(monkeypatch, e):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in e["env"].items():
        assert k in SWITCHES, k
        monkeypatch.setenv(k, v)


def int16_rows(ch, n, seed):
    x = np.random.default_rng(seed).integers(-32768, 32768, (ch, n)).astype(np.int16)
    x[1 % ch] = np.where((np.arange(n) // 40) % 2, 32767, -32768)
    x[3 % ch] = -32768
    x[5 % ch] = 32767
    return x


class Guarded:
    """[rows][n] 2-byte samples at (an aligned pointer + a guard of at least one row, a multiple of 16 bytes + `align`), one more row and 16 bytes behind"""

    def __init__(self, ctx, rows, n, align):
        assert align % 2 == 0
        front = -(-2 * n // 16) * 16
        self.first, self.count, self.shape = (front + align) // 2, rows * n, (rows, n)
        self.words = self.first + self.count + n + 8
        self.buf = ctx.array((self.words,), np.uint16)
        self.ptr = self.buf.offset(2 * self.first)
        assert (self.buf.ptr % 16 == 0) and (self.ptr.ptr - align) % 16 == 0

    def put(self, data=None):
        h = np.full(self.words, GUARD, np.uint16)
        if data is not None:
            h[self.first:self.first + self.count] = np.ascontiguousarray(data).view(np.uint16).reshape(-1)
        self.buf.upload(h)
        return self

    def get(self, what):
        h = self.buf.download()
        assert (h[:self.first] == GUARD).all(), (what, "the guard in front of the buffer", np.flatnonzero(h[:self.first] != GUARD)[:8])
        tail = h[self.first + self.count:]
        assert (tail == GUARD).all(), (what, "the guard behind the buffer", np.flatnonzero(tail != GUARD)[:8])
        return h[self.first:self.first + self.count].view(np.int16).reshape(self.shape)


def designs(orc):
    lp = orc.biquad_design(orclib.BQ_LOWPASS, np.float32(5400 * CORR), 0.54)
    nt = orc.biquad_design(orclib.BQ_NOTCH, np.float32(3000 * CORR), 15.0)
    lr = [orc.biquad_design(orclib.BQ_LOWPASS, np.float32(5400 * CORR), q) for q in (0.54, 1.3, 0.54, 1.3)]
    hs = orc.biquad_design(orclib.BQ_HIGHSHELF, np.float32(2000.0), 9.0, 0.8)
    return lp, nt, lr, hs


def node_stages(orc, e):
    """the uniform coefficients of every node of the entry: [node][stage] -> five words"""
    lp, nt, lr, hs = designs(orc)
    out = []
    for k, s in enumerate(e["nodes"]):
        out.append({1: [lp] if k == 0 else [nt], 2: [lr[0], lr[1]] if e["ladder"] == "node" else [hs, nt], 4: lr}[s])
    return out


def own_rows(orc, e, ch):
    """per-channel records: stage 0 of the LAST node, a row of five words per channel (a low-pass or a notch that moves with the channel)"""
    k = len(e["nodes"]) - 1
    if k == 0:
        return k, np.stack([orc.biquad_design(orclib.BQ_LOWPASS, np.float32((5400.0 - 20.0 * c) * CORR), 0.54) for c in range(ch)])
    return k, np.stack([orc.biquad_design(orclib.BQ_NOTCH, np.float32((3000.0 + 11.0 * c) * CORR), 15.0) for c in range(ch)])


def models(orc, e, stages, rows, c):
    """the oracle's nodes of channel c"""
    out = []
    for k, st in enumerate(stages):
        st = list(st)
        if rows is not None and k == rows[0]:
            st[0] = rows[1][c]
        out.append(orc.biquad_teensy_new(st))
    return out


CHAIN = [e["name"] for e in census.ENTRIES if e["ladder"] == "chain"]
NODE = [e["name"] for e in census.ENTRIES if e["ladder"] == "node"]
FRONTEND = [e["name"] for e in census.ENTRIES if e["ladder"] == "frontend"]


@pytest.mark.parametrize("name", CHAIN)
def test_chain_node_ladder(ctx, orc, golden, monkeypatch, name):
    e = census.BY_NAME[name]
    set_switches(monkeypatch, e)
    ch, lens = e["channels"], e["lengths"]
    total = sum(lens)
    x = int16_rows(ch, total, 7000 + census.NAMES.index(name))
    taps = golden["fir/taps_am102"]
    stages = node_stages(orc, e)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps, taps, mode=orclib.AM, biquad_nodes=stages)
    assert chain.node_kernel() == ""                                            # before the first call
    ti = None
    if e["pc_taps"]:
        ti = np.stack([msdr.calc_fir_coeffs(102, 1800.0 + 40.0 * c)[:102] for c in range(ch)])
        chain.set_taps_channels(0, ti, ti)
    rows = own_rows(orc, e, ch) if e["per_channel"] else None
    if rows is not None:
        chain.set_node_coefficients_channels(rows[0], 0, 0, rows[1])
    if e["block_kernel"]:
        chain.set_block_kernel_q15(1)
    got = np.empty((ch, total), np.int16)
    o = 0
    for k, n in enumerate(lens):
        dx = ctx.to_device(x[:, o:o + n])
        g = Guarded(ctx, ch, n, e["align"]).put()
        chain.process(dx, g.ptr, n)
        assert chain.node_kernel() == e["kernel"] == census.expected(e, n), (name, k, chain.node_kernel(), chain.info()["kernel"])
        got[:, o:o + n] = g.get((name, k))
        o += n
    pad = -total % 128                                                           # (the oracle runs whole 128-sample blocks; every stage is causal)
    for c in judged(ch):
        t = taps if ti is None else ti[c]
        want = orc.chain_q15(np.concatenate([x[c], np.zeros(pad, np.int16)]), orclib.AM, t, t, biquads=models(orc, e, stages, rows, c))[:total]
        assert np.array_equal(got[c], want), (name, c, int(np.flatnonzero(got[c] != want)[0]))
    assert int(np.abs(got.astype(np.int32)).max()) > 1000, name               # (not a comparison of silences)
    chain.close()


@pytest.mark.parametrize("name", NODE)
def test_standalone_node_ladder(ctx, orc, monkeypatch, name):
    e = census.BY_NAME[name]
    set_switches(monkeypatch, e)
    ch, lens = e["channels"], e["lengths"]
    x = int16_rows(ch, sum(lens), 8000 + census.NAMES.index(name))
    stages = node_stages(orc, e)
    node = msdr.BiquadQ15(ctx, ch)
    for s, coef in enumerate(stages[0]):
        node.set_coefficients(s, coef)
    rows = own_rows(orc, e, ch) if e["per_channel"] else None
    if rows is not None:
        node.set_coefficients_channels(0, 0, rows[1])
    assert node.last_kernel() == ""
    refs = {c: models(orc, e, stages, rows, c)[0] for c in judged(ch)}
    o = 0
    for k, n in enumerate(lens):
        g = Guarded(ctx, ch, n, e["align"]).put(x[:, o:o + n])
        node.update(g.ptr, n)
        assert node.last_kernel() == e["kernel"] == census.expected(e, n), (name, k, node.last_kernel())
        got = g.get((name, k))
        for c, ref in refs.items():
            want = orc.biquad_teensy_update(ref, x[c, o:o + n])
            assert np.array_equal(got[c], want), (name, k, c, int(np.flatnonzero(got[c] != want)[0]))
        o += n
    for c in record_channels(ch):
        assert list(node.definition(c)) == list(refs[c].definition), (name, c)
    node.close()


@pytest.mark.parametrize("name", FRONTEND)
def test_frontend_ladder(ctx, orc, monkeypatch, name):
    e = census.BY_NAME[name]
    set_switches(monkeypatch, e)
    ch, lens = e["channels"], e["lengths"]
    total = sum(lens)
    x = _adc(np.random.default_rng(9000 + census.NAMES.index(name)), ch, total // 128, 14000)
    x[1] = np.where((np.arange(total) // 40) % 2, 65535, 0)
    x[3] = 0
    x[5] = 65535
    x[7, 100:140] = 65535
    x[7, 140:220] = 0
    fe = msdr.Frontend(ctx, ch)
    fe.prime(x[:, 0])
    assert fe.last_kernel() == ""
    all_stages = e["fe_stages"] == "all"
    got = np.empty((ch, total), np.int16)
    o = 0
    for k, n in enumerate(lens):
        gin = Guarded(ctx, ch, n, e["align"][0]).put(x[:, o:o + n])
        gout = gin if e["in_place"] else Guarded(ctx, ch, n, e["align"][1]).put()
        fe.update(gin.ptr, gout.ptr, n, msdr.FE_ALL if all_stages else msdr.FE_DCBLOCK)
        assert fe.last_kernel() == e["kernel"] == census.expected(e, n), (name, k, fe.last_kernel())
        got[:, o:o + n] = gout.get((name, k, "output"))
        if not e["in_place"]:
            assert np.array_equal(gin.get((name, k, "input")).view(np.uint16), x[:, o:o + n]), (name, k, "the input was written")
        o += n
    for c in judged(ch):
        if all_stages:
            f = orc.frontend_new(first_conversion=int(x[c, 0]))
            want = orc.frontend_run(f, x[c])
        else:
            f = orclib.DcBlock(0, int(x[c, 0]) << 14)
            want = orc.dcblock(f, x[c])
        assert np.array_equal(got[c], want), (name, c, int(np.flatnonzero(got[c] != want)[0]))
        if c in record_channels(ch):
            if all_stages:
                _check_state(fe, f, c)
            else:
                st = fe.state(c)
                assert st[0] == f.hpf_y1 and st[1] == f.hpf_x1, (name, c)
    fe.close()


def test_graph_recording_names_what_it_enqueued(ctx, orc, golden, monkeypatch):
    """msdr_chain_graph_create records the launches of msdr_chain_process: the getter names the node kernel of the recorded calls, and a replay
    (which runs no host ladder) leaves it as it is."""
    e = census.BY_NAME["c_unfused"]
    set_switches(monkeypatch, e)
    ch, n = e["channels"], 128
    taps = golden["fir/taps_am102"]
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps, taps, mode=orclib.AM, biquad_nodes=node_stages(orc, e))
    x = int16_rows(ch, 2 * n, 11)
    dx = [ctx.to_device(x[:, k * n:(k + 1) * n]) for k in range(2)]
    dy = [ctx.array((ch, n), np.int16) for _ in range(2)]
    graph = chain.graph(dx, dy, n)
    assert chain.node_kernel() == e["kernel"]
    graph.launch()
    ctx.synchronize()
    assert chain.node_kernel() == e["kernel"]
    got = np.concatenate([d.download() for d in dy], axis=1)
    for c in (0, 1, 3, 5, 15, 16, ch - 1):
        want = orc.chain_q15(x[c], orclib.AM, taps, taps, biquads=models(orc, e, node_stages(orc, e), None, c))
        assert np.array_equal(got[c], want), c
    graph.close()
    chain.close()
