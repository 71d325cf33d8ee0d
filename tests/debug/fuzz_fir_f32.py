"""Randomised differential test of the arm_fir_f32 stage (fir_f32tq_kernel / fir_f32mf_kernel / fir_kernel<FirF32>) against a float64
convolution: every channel, every output, held to the per-output bound of include/msdr.h (clause (a) of tests/fir_f32_edges.py: a quiet
stretch is judged at its own level, not against the row's energy); on a mismatch the (call, channel, tile) map of the error is printed.
    python tests/debug/fuzz_fir_f32.py [seconds] [seed]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpuhelp import msdr  # noqa: E402  (imports torch first)
import fir_f32_edges as E  # noqa: E402

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rng = np.random.default_rng(seed)
ctx = msdr.Context(0)
B = 128
t_end = time.time() + budget
cases = bad = 0
while time.time() < t_end:
    cases += 1
    ntaps = int(rng.integers(1, 514))
    ch = int(rng.choice([1, 5, 70, 70, 70, 300]))
    n = int(rng.integers(1, 80)) * B
    h = (rng.standard_normal(ntaps) * 10.0 ** rng.uniform(-3, 1)).astype(np.float32)
    x = (rng.standard_normal((ch, n)) * 10.0 ** rng.uniform(-6, 6)).astype(np.float32)
    if rng.integers(0, 2):
        x[:, int(rng.integers(0, n)):] *= np.float32(10.0 ** rng.uniform(-8, 8))
    cuts = sorted(set([0, n] + [int(c) * B for c in rng.integers(1, max(2, n // B), int(rng.integers(0, 4)))]))
    fir = msdr.FirF32(ctx, h, ch)
    got = np.empty_like(x)
    for o, e in zip(cuts[:-1], cuts[1:]):
        m = e - o
        dx, dy = ctx.to_device(np.ascontiguousarray(x[:, o:e])), ctx.to_device(np.full((ch, m), np.nan, np.float32))    # (outputs never written stay NaN)
        fir.process(dx, dy, m)
        got[:, o:e] = dy.download()
    name = fir.kernel_name()
    kind = "tq" if name.startswith("fir_f32tq") else "mf" if name.startswith("fir_f32mf") else "plain"
    shown = rows = 0
    lines = []
    worst = 0.0
    for c in range(ch):                                         # every row (a few ms each; the judge draws nothing from rng)
        for o, e in zip(cuts[:-1], cuts[1:]):
            hist = np.zeros(ntaps - 1, np.float32)
            have = min(o, ntaps - 1)
            if have:
                hist[ntaps - 1 - have:] = x[c, o - have:o]
            ref = E.row_reference(kind, h, hist, x[c, o:e], np.zeros(e - o, np.int64), pinned=None)
            miss, _, over = E.judge_row(ref, got[c, o:e])
            worst = max(worst, over)
            if miss.any():
                rows += 1
                for t in range(0, e - o, E.TILE):
                    idx = np.nonzero(miss[t:t + E.TILE])[0]
                    if idx.size and shown < 40:
                        shown += 1
                        k = t + idx[0]
                        lines.append("   channel %d call [%d, %d) tile at %d: %d bad samples in +%d .. +%d, %d of them NaN (never written); got %.6g want %.6g bound %.3g" % (
                            c, o, e, o + t, idx.size, idx[0], idx[-1], int(np.isnan(got[c, o + t:o + t + E.TILE][idx]).sum()), got[c, o + k], ref.truth[k], ref.bound[k]))
    if rows:
        bad += 1
        print("MISMATCH", dict(seed=seed, case=cases, ntaps=ntaps, ch=ch, n=n, cuts=cuts, kernel=name, rows=rows, worst_over_bound=worst), flush=True)
        print("\n".join(lines), flush=True)
    fir.close()
    if cases % 200 == 0:
        print("cases", cases, "bad", bad, flush=True)
print("fuzz done: %d cases, %d mismatches (seed %d)" % (cases, bad, seed))
sys.exit(1 if bad else 0)
