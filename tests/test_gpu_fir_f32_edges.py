"""msdr_fir_f32_process on the census of tests/fir_f32_edges.py: level steps by 2^-12 .. 2^-34 and 2^20 .. 2^30, a loud tile, isolated
spikes, base levels 2^-60 .. 2^90, a pinned input range, at every tap count where another kernel takes over (fir_kernel<FirF32>,
fir_f32tq_kernel, fir_f32mf_kernel, chain_f32pc_kernel) and under two call layouts (aligned rows; odd rows unaligned).  Every output of
every row is held to the precision clause of include/msdr.h (clause (a)), every stretch that lies under its own scale to 1e-6 relative RMS
against float64 (clause (b)).  Non-finite and out-of-range samples: their own channel, their own tile windows, and a NaN is never
turned into a number.

Findings at the commit before this module (profiles/fir_f32_edges/README.md has the figures): fir_f32mf_kernel (290 .. 513 taps) carried
its halo across a change of scale with the factor clamped to 2^-24 .. 2^15 -- behind a drop by 2^-20 the first numTaps - 1 outputs of the
first all-quiet window were wrong by a factor of order one, behind a rise by 2^30 the quiet halo came out 2^6 too large; and both
matrix-core kernels rounded the lo pieces toward zero, up to twice the header's 2^-39 Mw."""
import numpy as np
import pytest

import fir_f32_edges as E
from gpuhelp import ctx, msdr  # noqa: F401

pytestmark = pytest.mark.gpu

SPECS = E.census()


def _run(ctx, case, pinned=None):
    """Every call of the case's layout through one FirF32 -> (outputs[call] = [6][m], the kernel it reports).  Outputs start as NaN and
    have one guard row behind the last channel."""
    s = case.spec
    fir = msdr.FirF32(ctx, case.taps[0], E.CHANNELS)
    try:
        if s.per_channel:
            fir.set_coeffs_channels(0, case.taps)
        if pinned:
            fir.set_input_range(pinned)
        outs, name = [], None
        for _, o, m, _ in E.calls(case):
            dx = ctx.to_device(np.ascontiguousarray(case.x[:, o:o + m]))
            dy = ctx.to_device(np.full((E.CHANNELS + 1, m), np.nan, np.float32))
            fir.process(dx, dy, m)
            y = dy.download()
            name = fir.kernel_name()
            assert E.kernel_name_ok(s.kernel, name), (s.id, name)
            assert np.isnan(y[E.CHANNELS]).all(), (s.id, "the row behind the last channel was written")
            outs.append(y[:E.CHANNELS])
            dx.free()
            dy.free()
        return outs, name
    finally:
        fir.close()


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: s.id)
def test_fir_f32_census(ctx, spec):
    case = E.build(spec)
    refs = E.case_references(case)
    outs, name = _run(ctx, case, spec.pinned)
    viol = E.judge_case(case, refs, outs)
    if viol:
        print(E.format_violations(spec, name, viol))
    assert not viol, E.format_violations(spec, name, viol, limit=6)


def _flat(ntaps, layout):
    kind, kernel = [(k, n) for t, pc, k, n in E.TAP_CONFIGS if t == ntaps and not pc][0]
    return E.build(E.Spec(ntaps, False, kind, kernel, layout, "flat", 0))


def _contained(ctx, case, struck):
    """The struck samples cost their own channel's tile windows and nothing else; -> the outputs."""
    dirty, clean, exclude = E.strike(case, struck)
    outs, name = _run(ctx, dirty)
    viol = E.judge_case(clean, E.case_references(clean), outs, exclude)
    if viol:
        print(E.format_violations(case.spec, name, viol))
    assert not viol, E.format_violations(case.spec, name, viol, limit=6)
    for r in range(E.CHANNELS):
        if r not in struck:
            assert all(e[r] is None for e in exclude)                  # clean channels: judged in full
    assert not exclude[1][1].any() and not exclude[1][3].any()         # the next call: the history has passed the sample
    return outs


@pytest.mark.parametrize("layout", list(E.LAYOUTS))
@pytest.mark.parametrize("ntaps", [256, 512])
def test_fir_f32_non_finite_samples_stay_in_their_windows(ctx, ntaps, layout):
    """One NaN (channel 1, +300 of tile 2) and one +Inf (channel 3, the last sample of tile 1): the four clean channels make clauses
    (a) and (b) in full, the struck channels everywhere but in the tile windows that hold the sample, the next call is clean, and the
    numTaps outputs arm_fir_f32 would lose are non-finite (every tap is non-zero)."""
    case = _flat(ntaps, layout)
    assert (case.taps != 0).all()
    struck = {1: {2 * 1024 + 300: np.nan}, 3: {2 * 1024 - 1: np.inf}}
    outs = _contained(ctx, case, struck)
    for r, hits in struck.items():
        for p in hits:
            assert not np.isfinite(outs[0][r, p:p + ntaps]).any(), (r, p)


@pytest.mark.parametrize("ntaps", [256, 512])
@pytest.mark.parametrize("peak", [120, -120])
def test_fir_f32_out_of_range_magnitudes_stay_in_their_windows(ctx, ntaps, peak):
    """Samples outside the magnitude range of include/msdr.h (peaks of 2^120: fp16 infinities after the limited scale; 2^-120: flushed):
    containment only -- other channels and other tile windows make clauses (a) and (b)."""
    case = _flat(ntaps, "aligned")
    rng = np.random.default_rng(abs(peak) + ntaps)
    pos = np.arange(1024 + 200, 1024 + 700)
    vals = (rng.standard_normal(pos.size) * 2.0 ** (peak - 3)).astype(np.float32)
    vals[7] = np.float32(2.0 ** peak)
    struck = {1: dict(zip(pos.tolist(), vals.tolist())), 3: {2 * 1024 - 1: float(np.float32(2.0 ** peak))}}
    _contained(ctx, case, struck)
