"""The conditions on the cases of tests/test_gpu_taps_per_channel_f32.py, checked without a GPU (oracle, float64 and the library's host-side
msdr_biquad_df1_f32_cascade_info only): for every (taps, mode, cascade, oscillator) combination a judged GPU row uses,
bound = 2 e_orc + fp32_noise + 1e-6 stays at or below 2e-5 and the contract's level, max(1, input rms / output rms), below 1.1 -- so the GPU
tests assert e_gpu <= 2 e_orc + fp32_noise + 1e-6 with the level taken as 1, and the float64 clause stays as tight as the plain 1e-5 it
stands for.  The cascades are the reference's own: low-pass Q 0.54, notch Q 15."""
import numpy as np
import pytest

import f32pc_cases as pc
from f32judge import fp32_noise, level, references
from gpuhelp import msdr, rel_rms

CASES = pc.cases()


def test_cases_cover_the_tap_counts_and_flavours_the_gpu_tests_use():
    import ast
    import os
    assert {c[0].size for c in CASES.values()} == {pc.NT} | set(pc.LONG_TAPS)
    assert {c[2] for c in CASES.values()} == {pc.orclib.AM, pc.orclib.LSB, pc.orclib.USB, pc.orclib.CW}
    assert {c[3] for c in CASES.values()} == {None, "lp", "lp+notch"}
    for n in (pc.NT,) + pc.LONG_TAPS:          # every tap count under every mode family and both mixers
        have = {(c[2], c[4] is pc.FS4) for c in CASES.values() if c[0].size == n}
        assert have >= {(m, f) for m in (pc.orclib.AM, pc.orclib.LSB, pc.orclib.USB) for f in (True, False)}, (n, have)
    assert len({c.tobytes() for c in pc.bank_taps(64)}) == 64 and len({c.tobytes() for c in pc.bank_taps(4096)}) == 196
    # the GPU test's own parameters, read from its source: the long tap counts and the cascades it names are the table's
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_taps_per_channel_f32.py")).read()
    tree = ast.parse(src)
    params = [ast.literal_eval(d.args[1]) for f in ast.walk(tree) if isinstance(f, ast.FunctionDef) and f.name == "test_long_tap_counts"
              for d in f.decorator_list if isinstance(d, ast.Call)]
    assert params == [list(pc.LONG_TAPS)], params
    import re
    assert set(re.findall(r'cascade\("([^"]+)"\)', src)) == {"lp", "lp+notch"}


def test_the_cascades_are_the_reference_s_own_and_well_conditioned_enough():
    s = pc.sections()
    lp, notch = s["lp"].astype(np.float64), s["notch"].astype(np.float64)
    assert abs(lp[:3].sum() / (1 - lp[3] - lp[4]) - 1.0) < 1e-3                     # unit gain at DC
    assert abs(notch[:3].sum() / (1 - notch[3] - notch[4]) - 1.0) < 1e-3
    for key in ("lp", "lp+notch"):
        kappa, noise, _ = msdr.biquad_cascade_info(pc.cascade(key))
        print(key, "kappa %.2f fp32_noise %.2e" % (kappa, noise))
        assert noise < 5e-6, (key, noise)


@pytest.mark.parametrize("name", sorted(CASES))
def test_bound_at_level_one_is_at_most_2e_5(name):
    hi, hq, mode, key, osc = CASES[name]
    rng = np.random.default_rng([77, len(name), sum(map(ord, name))])
    x = rng.integers(-20000, 20001, 6000 + 8 * hi.size).astype(np.int16)
    case = dict(mode=int(mode), hi=hi, hq=hq, oi=osc[0], oq=osc[1], bq=pc.cascade(key))
    want, truth, pre = references(x, case)
    for wname, w in (("all", slice(0, x.size)), ("settled", slice(4 * hi.size, x.size)), ("tail", slice(x.size - 1500, x.size))):
        e_orc = rel_rms(want[w], truth[w])
        bound = 2 * e_orc + fp32_noise(case["bq"]) + 1e-6
        lvl = level(want[w], pre[w])
        print("%s %-8s e_orc %.3e fp32_noise %.2e bound %.3e level %.3f" % (name, wname, e_orc, fp32_noise(case["bq"]), bound, lvl))
        assert bound <= 2e-5, (name, wname, bound)
        assert lvl < 1.1, (name, wname, lvl)
