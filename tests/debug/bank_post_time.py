"""tests/debug/bank_post_time.py -- what synchronous AM behind the down-converter bank costs on one MI355X (not collected by pytest).

4096 receivers x 2^14 samples on ONE antenna row (msdr_chain_set_input_rows, n_inputs 1), 102 taps, a quarter of the receivers on SYNCAM, chains
created with MSDR_CHAIN_SYNCAM_PLL, Q15 and F32 (no cascade, no nodes, no LMS channel), decimation 1 and 8:

  parent   Q15 D = 1: the chain on a build of the PARENT commit (--parent-lib): the syncam_q hand-over and syncam_pll_kernel
           F32 D = 1: the parent's only route for such a chain, the table mixer with the auxiliary chain behind it (no phase accumulator)
  off      the same two chains on this build, msdr_chain_set_bank_post never called                                                      (a)
  on       msdr_chain_set_bank_post(1), then phase-accumulator mode (F32: steps on the 128 grid, k 2^25): the I/Q twin stores the pairs into
           the chain's own buffer and bank_pll_*_kernel runs over them                                                                   (b) (c)
  on_am    ... with every receiver on AM: the same launches without the pair store and the PLL pass; on - on_am is the pass and its store (d)

Per arithmetic and factor, `spread` being the parent's own run-to-run spread (its largest minus its smallest step over the rounds):
  (a)  main kernel, off <= parent + spread                  (the existing kernels' machine code is the parent's, byte for byte)
  (b)  Q15 D = 1, whole call: on <= parent + spread + the added pair bytes at 0.82 x 8 TB/s   (4096 x 2^14 x 4 bytes written and a quarter read)
  (c)  F32 D = 1, whole call: on against parent (the expectation: one pass over stored pairs beats a second FIR chain); recorded either way
  (d)  (on - on_am) at D = 8 as a fraction of the same at D = 1: the expectation is about 1 / 8, the recurrence is per output
The configurations ALTERNATE, each step in a child process of its own under its own time limit, and the run stops at the first step that
fails.  Per step: device time over `reps` calls behind two warm-up calls -- of the main kernel (msdr_chain_enable_timing) and of the whole
call (events around the loop) -- the fastest and the median of three runs.

usage: python tests/debug/bank_post_time.py [--parent-lib PATH/libmsdr.so] [--out FILE.json] [--rounds N] [--reps N] [--kinds a,b,...]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KINDS = ["parent", "off", "on", "on_am"]
ARITHS = ["q15", "f32"]
DECS = [1, 8]
LIMIT_S = 150
PAIR_GBPS = 0.82 * 8000.0


def applies(arith, kind, D):
    """parent / off: D = 1 only (without the switch such a chain does not decimate; an fp32 one does not even enter the mode)"""
    return kind in ("on", "on_am") or D == 1


def step(arith, kind, D, reps):
    import numpy as np
    import torch                                   # first: the library binds to the HIP runtime torch initialised
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    ch, n, nt, L, D = 4096, 1 << 14, 102, 128, int(D)
    f32 = arith == "f32"
    bank = kind in ("on", "on_am")
    stream = torch.cuda.Stream()
    ctx = msdr.Context(0, stream=stream.cuda_stream)
    q = msdr.calc_fir_coeffs(nt, 2400.0)[:nt].copy()
    taps = (q.astype(np.float64) / 32768.0).astype(np.float32) if f32 else q
    a = 2 * np.pi * 5 * np.arange(L) / L
    oi, oq = np.round(32767 * np.sin(a)).astype(np.int16), np.round(32767 * np.cos(a)).astype(np.int16)
    if f32:
        oi, oq = (oi / 32768.0).astype(np.float32), (oq / 32768.0).astype(np.float32)
    modes = np.full(ch, msdr.MODE_AM, np.int32)
    if kind != "on_am":
        modes[::4] = msdr.MODE_SYNCAM
    chain = msdr.Chain(ctx, msdr.ARITH_F32 if f32 else msdr.ARITH_Q15, ch, taps, taps, mixer=msdr.MIXER_NCO, modes=modes, osc_i=oi, osc_q=oq, flags=msdr.CHAIN_SYNCAM_PLL)
    if bank:
        chain.set_bank_post(True)
    rows = 1
    if bank or not f32:
        (chain.set_taps_channels_f32 if f32 else chain.set_taps_channels)(0, np.tile(taps, (ch, 1)))
        k = np.random.default_rng(7).integers(1, 64, ch, dtype=np.uint64)
        steps = (k << np.uint64(25)) if f32 else np.random.default_rng(7).integers(0, 1 << 32, ch, dtype=np.uint64)
        chain.set_nco_channels(0, steps.astype(np.uint32))
        chain.set_input_rows(np.zeros(ch, np.int64), 1)
    else:
        rows = ch          # (the auxiliary chain gathers d_if by channel: no input map on such a chain)
    if D > 1:
        chain.set_decimation(D)
    nout = n // D
    t = torch.arange(n, device="cuda", dtype=torch.float64)
    x = (9000 * torch.cos(2 * 3.141592653589793 * (5.0 / 128 + 60.0 / 24000.0) * t)).round().to(torch.int16).reshape(1, n).repeat(rows, 1).contiguous()
    y = torch.empty(ch * nout, dtype=torch.float32 if f32 else torch.int16, device="cuda")
    dst = y.data_ptr()
    with torch.cuda.stream(stream):
        for _ in range(2):
            chain.process(x.data_ptr(), dst, n)
        torch.cuda.synchronize()
        chain.enable_timing(True)
        runs, calls = [], []
        for _ in range(3):
            chain.kernel_time()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                chain.process(x.data_ptr(), dst, n)
            e1.record(stream)
            ms, launches = chain.kernel_time()
            runs.append(ms / max(launches, 1))
            calls.append(e0.elapsed_time(e1) / reps)
    info = chain.info()
    print(json.dumps({"arith": arith, "kind": kind, "D": D, "kernel_ms": min(runs), "kernel_ms_median": sorted(runs)[1], "call_ms": min(calls),
                      "call_ms_median": sorted(calls)[1], "kernel": info["kernel"], "grid": info["grid"], "block": info["block"],
                      "post_kernel": chain.post_kernel() if hasattr(ctx.lib, "msdr_chain_post_kernel") else None,
                      "time_segments": info["time_segments"], "channels": ch, "samples": n, "taps": nt, "reps": reps, "flavour": info["flavour"],
                      "audio_nonzero": int((y != 0).sum().item()), "device": torch.cuda.get_device_name(0), "lib": os.environ.get("MSDR_LIB", "")}), flush=True)
    ctx.close()


def verdicts(res):
    out = []
    med, spread = {}, {}
    for r in res:
        med.setdefault((r["arith"], r["D"], r["kind"]), {"kernel": [], "call": []})
        med[(r["arith"], r["D"], r["kind"])]["kernel"].append(r["kernel_ms"])
        med[(r["arith"], r["D"], r["kind"])]["call"].append(r["call_ms"])
    m = {k: {w: statistics.median(v[w]) for w in v} for k, v in med.items()}
    for k, v in med.items():
        spread[k] = {w: max(v[w]) - min(v[w]) for w in v}
    pair_ms = 4096 * (1 << 14) * 4 * 1.25 / (PAIR_GBPS * 1e9) * 1e3
    for arith in ARITHS:
        p, off, on = m.get((arith, 1, "parent")), m.get((arith, 1, "off")), m.get((arith, 1, "on"))
        sp = spread.get((arith, 1, "parent"))
        if p and off:
            out.append("(a) %s D 1 main kernel: off %.4f parent %.4f spread %.4f ms: %s" % (arith, off["kernel"], p["kernel"], sp["kernel"],
                       "met" if off["kernel"] <= p["kernel"] + sp["kernel"] else "**MISSED** by %.4f" % (off["kernel"] - p["kernel"] - sp["kernel"])))
        if p and on and arith == "q15":
            lim = p["call"] + sp["call"] + pair_ms
            out.append("(b) q15 D 1 whole call: on %.4f parent %.4f spread %.4f pair bytes %.4f ms: %s" % (on["call"], p["call"], sp["call"], pair_ms,
                       "met" if on["call"] <= lim else "**MISSED** by %.4f" % (on["call"] - lim)))
        if p and on and arith == "f32":
            out.append("(c) f32 D 1 whole call: on %.4f, the parent's auxiliary-chain route %.4f ms: %s" % (on["call"], p["call"],
                       "met" if on["call"] <= p["call"] else "**MISSED** by %.4f" % (on["call"] - p["call"])))
        d = {D: m[(arith, D, "on")]["call"] - m[(arith, D, "on_am")]["call"] for D in DECS if (arith, D, "on") in m and (arith, D, "on_am") in m}
        if len(d) == 2:
            out.append("(d) %s PLL pass and pair store: D 1 %.4f ms, D 8 %.4f ms, fraction %.3f (expected about 0.125)" % (arith, d[1], d[8], d[8] / d[1] if d[1] else float("nan")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--parent-lib", help="libmsdr.so of the parent commit (case parent); without it that case is left out")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--step", help="arith:kind:D -- run this one step in this process")
    args = ap.parse_args()
    if args.step:
        return step(*args.step.split(":"), args.reps)
    kinds = [kd for kd in args.kinds.split(",") if kd != "parent" or args.parent_lib]
    res, rc = [], 0
    for r in range(args.rounds):
        for arith, D, kind in [(a, d, k) for a in ARITHS for d in DECS for k in kinds if applies(a, k, d)]:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", "%s:%s:%d" % (arith, kind, D), "--reps", str(args.reps)]
            env = dict(os.environ)
            if kind == "parent":
                env["MSDR_LIB"] = os.path.abspath(args.parent_lib)
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=LIMIT_S, env=env)
            except subprocess.TimeoutExpired:
                print("round %d %s %s D %d ran over its %d s: stopping" % (r, arith, kind, D, LIMIT_S), flush=True)
                rc = 1
                break
            if p.returncode != 0:
                print("round %d %s %s D %d failed (exit %d): stopping\n%s" % (r, arith, kind, D, p.returncode, p.stderr[-2000:]), flush=True)
                rc = 1
                break
            rec = json.loads(p.stdout.strip().splitlines()[-1])
            rec["round"] = r
            res.append(rec)
            print("round %d %s D %d %-7s kernel %8.4f ms  call %8.4f ms (median %8.4f)  %s + %s  segments %d" %
                  (r, arith, D, kind, rec["kernel_ms"], rec["call_ms"], rec["call_ms_median"], rec["kernel"], rec["post_kernel"], rec["time_segments"]), flush=True)
        if rc:
            break
    for line in verdicts(res):
        print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return rc


if __name__ == "__main__":
    sys.exit(main())
