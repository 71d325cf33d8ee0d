"""tests/debug/spectrum_pc_time.py -- what the per-receiver spectrum display costs on one MI355X (not collected by pytest).

4096 receivers x 2^14 samples on ONE antenna row (msdr_chain_set_input_rows, n_inputs 1), 102 taps, every receiver on AM, Q15 and F32 (no
cascade, no nodes), decimation 1 and 8:

  parent   the chain in phase-accumulator mode on a build of the PARENT commit (--parent-lib)
  off      the same chain on this build, msdr_chain_set_spectrum never called                                                 (a)
  iq       ... with a caller's d_iq (msdr_chain_set_iq_out) and the spectrum off
  iq_on    ... with the same d_iq and the spectrum on, every = 1: iq_on - iq is the spectrum's launch alone                     (b)
  on       the spectrum on, every = 1, without a d_iq: the main launch picks its I/Q twin and stores into the chain's own buffer  (c)
and the stage alone:
  stage    msdr_cfft64_* over 4096 transforms, both outputs (the bound of (b)); Q15 also at nfft = 2^20, both outputs, against
           msdr_rfft128_q15 (both outputs) at the same nfft in the same process                                               (d)

Per arithmetic and factor, `spread` being the parent's own run-to-run spread (its largest minus its smallest step over the rounds):
  (a)  main kernel, off <= parent + spread           (the existing kernels' machine code is the parent's, byte for byte)
  (b)  whole call, iq_on - iq <= the stand-alone stage over 4096 transforms + the iq step's own spread; the absolute microseconds are reported
  (c)  on against off, main kernel and whole call: the I/Q twin where the plain kernel ran before -- the tap's known cost, reported apart
  (d)  algorithmic bytes per second of msdr_cfft64_q15 (768 per transform) >= msdr_rfft128_q15's (895 per transform) minus the spread
The configurations ALTERNATE, each step in a child process of its own under its own time limit, and the run stops at the first step that
fails.  Per step: device time over `reps` calls behind two warm-up calls -- of the main kernel (msdr_chain_enable_timing) and of the whole
call (events around the loop) -- the fastest and the median of three runs.

usage: python tests/debug/spectrum_pc_time.py [--parent-lib PATH/libmsdr.so] [--out FILE.json] [--rounds N] [--reps N] [--kinds a,b,...]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KINDS = ["parent", "off", "iq", "iq_on", "on", "stage"]
ARITHS = ["q15", "f32"]
DECS = [1, 8]
LIMIT_S = 150


def applies(kind, D):
    return kind != "stage" or D == 1


def timed(stream, torch, fn, reps):
    """ms per call of fn over `reps` calls behind two warm-up calls: [three runs]"""
    out = []
    with torch.cuda.stream(stream):
        fn(); fn()
        torch.cuda.synchronize()
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                fn()
            e1.record(stream)
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / reps)
    return out


def stage_step(arith, reps):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    f32 = arith == "f32"
    stream = torch.cuda.Stream()
    ctx = msdr.Context(0, stream=stream.cuda_stream)
    rec = {"arith": arith, "kind": "stage", "D": 1, "device": torch.cuda.get_device_name(0)}
    for nfft in (4096,) + (() if f32 else (1 << 20,)):
        g = torch.Generator(device="cuda").manual_seed(1)
        if f32:
            pairs = torch.randn(nfft * 128, device="cuda", generator=g, dtype=torch.float32)
        else:
            pairs = torch.randint(-32768, 32768, (nfft * 128,), device="cuda", generator=g, dtype=torch.int16)
        bins = torch.empty(nfft * 128, device="cuda", dtype=pairs.dtype)
        power = torch.empty(nfft * 64, device="cuda", dtype=torch.float32 if f32 else torch.int32)
        call = ctx.cfft64_f32 if f32 else ctx.cfft64_q15
        runs = timed(stream, torch, lambda: call(pairs.data_ptr(), 64, nfft, bins.data_ptr(), power.data_ptr()), reps)
        rec["cfft64_ms_%d" % nfft] = min(runs)
        rec["cfft64_ms_median_%d" % nfft] = sorted(runs)[1]
        if not f32 and nfft == 1 << 20:
            fft_out = torch.empty(nfft * 256, device="cuda", dtype=torch.int16)
            cols = torch.empty(nfft * 128, device="cuda", dtype=torch.uint8)
            lib = ctx.lib
            runs = timed(stream, torch, lambda: msdr._ck(lib.msdr_rfft128_q15(ctx.h, pairs.data_ptr(), 128, fft_out.data_ptr(), cols.data_ptr(), nfft)), reps)
            rec["rfft128_ms_%d" % nfft] = min(runs)
            rec["rfft128_ms_median_%d" % nfft] = sorted(runs)[1]
            rec["cfft64_gbps"] = 768.0 * nfft / (rec["cfft64_ms_%d" % nfft] * 1e-3) / 1e9
            rec["rfft128_gbps"] = 895.0 * nfft / (rec["rfft128_ms_%d" % nfft] * 1e-3) / 1e9
    print(json.dumps(rec), flush=True)
    ctx.close()


def step(arith, kind, D, reps):
    if kind == "stage":
        return stage_step(arith, reps)
    import numpy as np
    import torch                                   # first: the library binds to the HIP runtime torch initialised
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    ch, n, nt, L, D = 4096, 1 << 14, 102, 128, int(D)
    f32 = arith == "f32"
    stream = torch.cuda.Stream()
    ctx = msdr.Context(0, stream=stream.cuda_stream)
    q = msdr.calc_fir_coeffs(nt, 2400.0)[:nt].copy()
    taps = (q.astype(np.float64) / 32768.0).astype(np.float32) if f32 else q
    a = 2 * np.pi * 5 * np.arange(L) / L
    oi, oq = np.round(32767 * np.sin(a)).astype(np.int16), np.round(32767 * np.cos(a)).astype(np.int16)
    if f32:
        oi, oq = (oi / 32768.0).astype(np.float32), (oq / 32768.0).astype(np.float32)
    modes = np.full(ch, msdr.MODE_AM, np.int32)
    chain = msdr.Chain(ctx, msdr.ARITH_F32 if f32 else msdr.ARITH_Q15, ch, taps, taps, mixer=msdr.MIXER_NCO, modes=modes, osc_i=oi, osc_q=oq)
    (chain.set_taps_channels_f32 if f32 else chain.set_taps_channels)(0, np.tile(taps, (ch, 1)))
    chain.set_nco_channels(0, np.random.default_rng(7).integers(0, 1 << 32, ch, dtype=np.uint64).astype(np.uint32))
    chain.set_input_rows(np.zeros(ch, np.int64), 1)
    if D > 1:
        chain.set_decimation(D)
    nout = n // D
    keep = []
    if kind in ("iq", "iq_on"):
        iq = torch.empty(ch * nout * 2, dtype=torch.float32 if f32 else torch.int16, device="cuda")
        chain.set_iq_out(iq.data_ptr(), nout)
        keep.append(iq)
    if kind in ("iq_on", "on"):
        bins = torch.empty(ch * 128, dtype=torch.float32 if f32 else torch.int16, device="cuda")
        power = torch.zeros(ch * 64, dtype=torch.float32 if f32 else torch.int32, device="cuda")
        chain.set_spectrum(bins.data_ptr(), power.data_ptr(), 1)
        keep += [bins, power]
    t = torch.arange(n, device="cuda", dtype=torch.float64)
    x = (9000 * torch.cos(2 * 3.141592653589793 * (5.0 / 128 + 60.0 / 24000.0) * t)).round().to(torch.int16).reshape(1, n).contiguous()
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
    drawn = chain.spectrum()[3] if kind in ("iq_on", "on") else 0
    print(json.dumps({"arith": arith, "kind": kind, "D": D, "kernel_ms": min(runs), "kernel_ms_median": sorted(runs)[1], "call_ms": min(calls),
                      "call_ms_median": sorted(calls)[1], "kernel": info["kernel"], "grid": info["grid"], "block": info["block"],
                      "time_segments": info["time_segments"], "channels": ch, "samples": n, "taps": nt, "reps": reps, "flavour": info["flavour"],
                      "drawn": drawn, "power_nonzero": int((keep[-1] != 0).sum().item()) if drawn else 0,
                      "audio_nonzero": int((y != 0).sum().item()), "device": torch.cuda.get_device_name(0), "lib": os.environ.get("MSDR_LIB", "")}), flush=True)
    ctx.close()


def verdicts(res):
    out = []
    vals = {}
    for r in res:
        if r["kind"] == "stage":
            for k, v in r.items():
                if k.startswith(("cfft64_", "rfft128_")) and "median" not in k:
                    vals.setdefault((r["arith"], 1, "stage", k), []).append(v)
            continue
        vals.setdefault((r["arith"], r["D"], r["kind"], "kernel"), []).append(r["kernel_ms"])
        vals.setdefault((r["arith"], r["D"], r["kind"], "call"), []).append(r["call_ms"])
    m = {k: statistics.median(v) for k, v in vals.items()}
    sp = {k: max(v) - min(v) for k, v in vals.items()}
    for arith in ARITHS:
        for D in DECS:
            g = lambda kind, w: m.get((arith, D, kind, w))
            if g("parent", "kernel") is not None and g("off", "kernel") is not None:
                s = sp[(arith, D, "parent", "kernel")]
                out.append("(a) %s D %d main kernel: off %.4f parent %.4f spread %.4f ms: %s" % (arith, D, g("off", "kernel"), g("parent", "kernel"), s,
                           "met" if g("off", "kernel") <= g("parent", "kernel") + s else "**MISSED** by %.4f" % (g("off", "kernel") - g("parent", "kernel") - s)))
            st = m.get((arith, 1, "stage", "cfft64_ms_4096"))
            if g("iq", "call") is not None and g("iq_on", "call") is not None and st is not None:
                s = sp[(arith, D, "iq", "call")]
                d = g("iq_on", "call") - g("iq", "call")
                out.append("(b) %s D %d whole call: spectrum on %.4f, off %.4f (both with a d_iq): +%.1f us; stage alone over 4096 transforms %.1f us, spread %.1f us: %s" %
                           (arith, D, g("iq_on", "call"), g("iq", "call"), 1e3 * d, 1e3 * st, 1e3 * s, "met" if d <= st + s else "**MISSED** by %.1f us" % (1e3 * (d - st - s))))
            if g("on", "call") is not None and g("off", "call") is not None:
                out.append("(c) %s D %d spectrum on without a d_iq against off: main kernel %.4f vs %.4f ms (the I/Q twin), whole call %.4f vs %.4f ms" %
                           (arith, D, g("on", "kernel"), g("off", "kernel"), g("on", "call"), g("off", "call")))
    a, b = vals.get(("q15", 1, "stage", "cfft64_gbps")), vals.get(("q15", 1, "stage", "rfft128_gbps"))
    if a and b:
        ma, mb, s = statistics.median(a), statistics.median(b), max(b) - min(b)
        out.append("(d) nfft 2^20, both outputs: msdr_cfft64_q15 %.0f GB/s (%.4f ms), msdr_rfft128_q15 %.0f GB/s (%.4f ms), spread %.0f GB/s: %s" %
                   (ma, m[("q15", 1, "stage", "cfft64_ms_%d" % (1 << 20))], mb, m[("q15", 1, "stage", "rfft128_ms_%d" % (1 << 20))], s,
                    "met" if ma >= mb - s else "**MISSED** by %.0f GB/s" % (mb - s - ma)))
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
        for arith, D, kind in [(a, d, k) for a in ARITHS for d in DECS for k in kinds if applies(k, d)]:
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
            if kind == "stage":
                print("round %d %s stage  %s" % (r, arith, "  ".join("%s %.4f" % (k, v) for k, v in sorted(rec.items()) if isinstance(v, float))), flush=True)
            else:
                print("round %d %s D %d %-6s kernel %8.4f ms  call %8.4f ms (median %8.4f)  %s  segments %d  drawn %d" %
                      (r, arith, D, kind, rec["kernel_ms"], rec["call_ms"], rec["call_ms_median"], rec["kernel"], rec["time_segments"], rec["drawn"]), flush=True)
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
