"""The batched 64-point complex FFT stage alone: msdr_cfft64_q15 / msdr_cfft64_f32 (bank_cfft64_q15_kernel / bank_cfft64_f32_kernel).

Q15 is compared with == against the oracle -- arm_cfft_q15 of length 64, what orc.rfft128_q15 leaves in `work` (tests/spectrum_model.py) --
and its power against re^2 + im^2 of those bins in int64, in display order.  F32 is judged against float64 numpy.fft.fft / 64 of the same
float inputs: ||dev - ref||_2 / ||ref||_2 <= 1e-5 per non-zero row (the project's fp32 bound), |p - p_ref| <= 2e-5 max_k p_ref per row, two
runs bit-identical.  nfft = 1, 4, 5, 16, 17, 67: one transform, a full wave, a partial wave, a full workgroup, a workgroup plus one, a partial
last group.  stride_pairs 64 and 72 (whole 16-byte slots per lane), 65 and a base one pair off a slot (pair by pair), seeded garbage between
the rows.  Every output buffer starts as a sentinel and has a guard row behind the last transform."""
import numpy as np
import pytest

import spectrum_model as M
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_iq_per_channel import bits, sentinel

pytestmark = pytest.mark.gpu
ARG = msdr.STATUS_ARGUMENT_ERROR
NFFT = (1, 4, 5, 16, 17, 67)
F = np.float32
SENT32 = 0x7B5A5B5C


@pytest.fixture(scope="module")
def rows(orc):
    """name -> (pairs [64, 2] int16, the oracle's bins [64, 2] int16); computed once and left alone"""
    r = M.stage_rows(np.random.default_rng(7100))
    out = {n: (p, M.cfft64_q15(orc, p)) for n, p in r.items()}
    for v in out.values():
        v[0].setflags(write=False); v[1].setflags(write=False)
    return out


def batch(rows, nfft, stride, rng, dtype=np.int16, scale=1.0, lead=0):
    """[lead + nfft * stride, 2] pairs: transform f = row f mod 12 at lead + f * stride, seeded garbage everywhere else"""
    names = list(rows)
    if dtype == np.int16:
        buf = rng.integers(-32768, 32768, (lead + nfft * stride, 2)).astype(np.int16)
    else:
        buf = (rng.standard_normal((lead + nfft * stride, 2)) * 1e4 * scale).astype(F)
    for f in range(nfft):
        p = rows[names[f % len(names)]][0]
        buf[lead + f * stride:lead + f * stride + 64] = p if dtype == np.int16 else (p.astype(np.float64) * scale).astype(F)
    return buf, [names[f % len(names)] for f in range(nfft)]


@pytest.mark.parametrize("stride, lead", [(64, 0), (72, 0), (65, 0), (64, 1)])
@pytest.mark.parametrize("nfft", NFFT)
def test_q15_is_the_oracles_transform(ctx, rows, nfft, stride, lead):
    rng = np.random.default_rng(7200 + nfft + stride + lead)
    buf, names = batch(rows, nfft, stride, rng, lead=lead)
    d_in = ctx.to_device(buf)
    src = d_in.offset(4 * lead)
    want_bins = np.stack([rows[n][1] for n in names])
    want_pow = np.stack([M.power_q15(rows[n][1]) for n in names])
    assert nfft < 3 or want_pow.max() == 2 ** 31          # the all-minimum row is transform 2
    for use_bins, use_pow in ((True, True), (True, False), (False, True)):
        d_bins = ctx.to_device(sentinel((nfft + 1, 64, 2), np.int16))
        d_pow = ctx.to_device(np.full((nfft + 1, 64), SENT32, np.uint32))
        ctx.cfft64_q15(src, stride, nfft, d_bins if use_bins else None, d_pow if use_pow else None)
        got_bins, got_pow = d_bins.download(), d_pow.download()
        if use_bins:
            assert np.array_equal(got_bins[:nfft], want_bins), [names[f] for f in range(nfft) if not np.array_equal(got_bins[f], want_bins[f])]
            assert np.array_equal(bits(got_bins[nfft:]), bits(sentinel((1, 64, 2), np.int16)))
        else:
            assert np.array_equal(bits(got_bins), bits(sentinel((nfft + 1, 64, 2), np.int16)))
        if use_pow:
            assert np.array_equal(got_pow[:nfft].astype(np.int64), want_pow), [names[f] for f in range(nfft) if not np.array_equal(got_pow[f], want_pow[f])]
            assert (got_pow[nfft:] == SENT32).all()
        else:
            assert (got_pow == SENT32).all()
    assert np.array_equal(d_in.download(), buf)          # the input is read-only


def test_q15_rows_cover_the_extremes(rows):
    """what the batches above contain from nfft = 17 on: every row of the set, the 2^31 power among them"""
    assert len(rows) == 12
    assert M.power_q15(rows["all_min"][1])[32] == 2 ** 31
    assert rows["tone5"][1][5].tolist() == [16382, -1]


WORST = {"bins": 0.0, "power": 0.0}


@pytest.mark.parametrize("scale", [1.0, 1.0 / 32768, 1e-3])
@pytest.mark.parametrize("stride, lead", [(64, 0), (72, 0), (65, 0), (64, 1)])
def test_f32_against_float64(ctx, rows, stride, lead, scale):
    rng = np.random.default_rng(7300 + stride + lead)
    for nfft in NFFT:
        buf, names = batch(rows, nfft, stride, rng, F, scale, lead)
        d_in = ctx.to_device(buf)
        src = d_in.offset(8 * lead)
        runs = []
        for use_bins, use_pow in ((True, True), (True, True), (True, False), (False, True)):
            d_bins = ctx.to_device(sentinel((nfft + 1, 64, 2), F))
            d_pow = ctx.to_device(sentinel((nfft + 1, 64), F))
            ctx.cfft64_f32(src, stride, nfft, d_bins if use_bins else None, d_pow if use_pow else None)
            got_bins, got_pow = d_bins.download(), d_pow.download()
            assert np.array_equal(bits(got_bins[nfft if use_bins else 0:]), bits(sentinel((1 if use_bins else nfft + 1, 64, 2), F)))
            assert np.array_equal(bits(got_pow[nfft if use_pow else 0:]), bits(sentinel((1 if use_pow else nfft + 1, 64), F)))
            runs.append((got_bins, got_pow))
            for f in range(nfft):
                ref = M.cfft64_f64(buf[lead + f * stride:lead + f * stride + 64])
                p_ref = M.display(ref.real ** 2 + ref.imag ** 2)
                assert np.abs(ref).max() > 0
                if use_bins:
                    dev = got_bins[f].astype(np.float64)
                    ratio = float(np.sqrt(((dev[:, 0] - ref.real) ** 2 + (dev[:, 1] - ref.imag) ** 2).sum()) / np.sqrt((np.abs(ref) ** 2).sum()))
                    WORST["bins"] = max(WORST["bins"], ratio)
                    assert ratio <= 1e-5, (names[f], nfft, ratio)
                if use_pow:
                    err = float(np.abs(got_pow[f].astype(np.float64) - p_ref).max() / p_ref.max())
                    WORST["power"] = max(WORST["power"], err)
                    assert err <= 2e-5, (names[f], nfft, err)
        assert np.array_equal(bits(runs[0][0]), bits(runs[1][0])) and np.array_equal(bits(runs[0][1]), bits(runs[1][1]))          # run to run
        assert np.array_equal(bits(runs[0][0][:nfft]), bits(runs[2][0][:nfft])) and np.array_equal(bits(runs[0][1][:nfft]), bits(runs[3][1][:nfft]))
    print("cfft64_f32 scale %g stride %d lead %d: worst relative L2 of bins %.3e, worst power error / max power %.3e" % (scale, stride, lead, WORST["bins"], WORST["power"]))


@pytest.mark.parametrize("f32", [False, True])
def test_refusals_write_nothing(ctx, rows, f32):
    dt, item = (F, 8) if f32 else (np.int16, 4)
    call = ctx.cfft64_f32 if f32 else ctx.cfft64_q15
    buf, _ = batch(rows, 4, 64, np.random.default_rng(7400), dt)
    d_in = ctx.to_device(np.concatenate([buf, buf]))
    d_bins = ctx.to_device(sentinel((6, 64, 2), dt))
    d_pow = ctx.to_device(sentinel((6, 64), F))
    cases = [(d_in, 64, None, None),                                     # both outputs NULL
             (d_in.offset(item // 2), 64, d_bins, d_pow),               # half a pair off
             (d_in, 64, d_bins.offset(4), d_pow), (d_in, 64, d_bins, d_pow.offset(8)),          # outputs off a 16-byte slot
             (d_in, 63, d_bins, d_pow)]                                  # rows that overlap
    for src, stride, b, p in cases:
        with pytest.raises(msdr.MsdrError) as e:
            call(src, stride, 4, b, p)
        assert e.value.status == ARG
    call(d_in, 64, 0, d_bins, d_pow)                                     # nfft == 0 does nothing
    ctx.synchronize()
    assert np.array_equal(bits(d_bins.download()), bits(sentinel((6, 64, 2), dt)))
    assert np.array_equal(bits(d_pow.download()), bits(sentinel((6, 64), F)))
