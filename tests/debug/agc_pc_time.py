"""tests/debug/agc_pc_time.py -- what the per-receiver gain and AGC cost a per-receiver chain on one MI355X (not collected by pytest).

4096 AM channels x 2^14 samples, 102 taps, phase-accumulator oscillators with seeded random steps, one shared IF row (msdr_chain_set_input_rows,
n_inputs 1), Q15 and F32 (no cascade, no nodes: the demodulator kernel alone), decimation 1 and 8:

  parent   the chain on a build of the PARENT commit (--parent-lib), which has no gain
  off      the same chain on this build, msdr_chain_set_gain never called: the plain kernels                                          (a)
  meter    ... with msdr_chain_set_meter: the metered twin, the yardstick of comparable extra work per output
  held     ... with msdr_chain_set_gain(1) and seeded gains, every AGC held: the gain twin                                             (b)
  agc      ... with msdr_chain_set_agc(all on) as well: the same kernel, and agc_step_kernel steps every receiver behind every call     (b)

Per arithmetic and factor, on the main kernel's ms per call (the median over the rounds of each step's fastest run), `spread` being the
parent's own run-to-run spread (its largest minus its smallest step over the rounds):
  (a) condition   off <= parent + spread           (the plain kernels' machine code is the parent's, byte for byte)
  (b) condition   held, agc <= meter + spread      (two multiplies and a max per output against two multiplies and an add)
The step kernel is not in the main kernel's time: it shows in the whole call's (call_ms of agc against held).
The configurations ALTERNATE, each step in a child process of its own under its own time limit, and the run stops at the first step that
fails.  Per step: device time over `reps` calls behind two warm-up calls -- of the main kernel (msdr_chain_enable_timing: HIP events around
its launch) and of the whole call (events around the loop, so the history kernel and the step kernel count) -- the fastest and the median of
three runs, with the clocks rocm-smi reports read at the end of the step.

usage: python tests/debug/agc_pc_time.py --parent-lib PATH/libmsdr.so [--out FILE.json] [--rounds N] [--reps N] [--kinds a,b,...]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KINDS = ["parent", "off", "meter", "held", "agc"]
ARITHS = ["q15", "f32"]
DECS = [1, 8]
LIMIT_S = 120


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=20).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln]
    except Exception as e:          # the tool may be missing: the timing stands without it
        return ["rocm-smi: %s" % e]


def step(arith, kind, D, reps):
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
    a = 2 * np.pi * np.arange(L) / L
    oi, oq = np.round(32767 * np.sin(a)).astype(np.int16), np.round(32767 * np.cos(a)).astype(np.int16)
    if f32:
        oi, oq = (oi / 32768.0).astype(np.float32), (oq / 32768.0).astype(np.float32)
    chain = msdr.Chain(ctx, msdr.ARITH_F32 if f32 else msdr.ARITH_Q15, ch, taps, taps, mixer=msdr.MIXER_NCO, mode=msdr.MODE_AM, osc_i=oi, osc_q=oq)
    (chain.set_taps_channels_f32 if f32 else chain.set_taps_channels)(0, np.tile(taps, (ch, 1)))
    chain.set_nco_channels(0, np.random.default_rng(7).integers(0, 1 << 32, ch, dtype=np.uint64).astype(np.uint32))
    chain.set_input_rows(np.zeros(ch, np.int64), 1)
    if D > 1:
        chain.set_decimation(D)
    nout = n // D
    meter = None
    if kind == "meter":
        meter = torch.zeros(ch, dtype=torch.float64 if f32 else torch.int64, device="cuda")
        chain.set_meter(meter.data_ptr())
    if kind in ("held", "agc"):
        chain.set_gain(True)
        chain.set_gain_channels(0, np.random.default_rng(8).uniform(0.25, 8.0, ch).astype(np.float32))
        chain.set_agc(None, 1 if kind == "agc" else 0)
    x = torch.randint(-12000, 12001, (1, n), dtype=torch.int16, device="cuda")
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
                      "lds_bytes": info["lds_bytes"], "time_segments": info["time_segments"], "channels": ch, "samples": n, "taps": nt, "reps": reps,
                      "flavour": info["flavour"], "audio_nonzero": int((y != 0).sum().item()),
                      "agc_steps": chain.agc_state(0)["steps"] if kind in ("held", "agc") else None,
                      "clocks": clocks(), "device": torch.cuda.get_device_name(0), "lib": os.environ.get("MSDR_LIB", "")}), flush=True)
    ctx.close()


def verdicts(res):
    """the condition and the ratio per arithmetic and factor, as lines"""
    out = []
    for arith in ARITHS:
        for D in DECS:
            ms = {k: [r["kernel_ms"] for r in res if (r["arith"], r["D"], r["kind"]) == (arith, D, k)] for k in KINDS}
            if not ms["off"]:
                continue
            med = {k: statistics.median(v) for k, v in ms.items() if v}
            spread = max(ms["parent"]) - min(ms["parent"]) if ms["parent"] else float("nan")
            line = "%s D %d: %s   spread %.4f ms" % (arith, D, "  ".join("%s %.4f" % (k, med[k]) for k in KINDS if k in med), spread)
            if "parent" in med:
                line += "   (a) off %s" % ("met" if med["off"] <= med["parent"] + spread else "MISSED by %.4f" % (med["off"] - med["parent"] - spread))
            for k in ("held", "agc"):
                if k in med and "meter" in med and spread == spread:
                    line += "   (b) %s / meter %.3f %s" % (k, med[k] / med["meter"], "met" if med[k] <= med["meter"] + spread else "MISSED by %.4f" % (med[k] - med["meter"] - spread))
            out.append(line)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--parent-lib", help="libmsdr.so of the parent commit (case parent); without it that case is left out")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--step", help="arith:kind:D -- run this one step in this process")
    args = ap.parse_args()
    if args.step:
        return step(*args.step.split(":"), args.reps)
    kinds = [kd for kd in args.kinds.split(",") if kd != "parent" or args.parent_lib]
    res, rc = [], 0
    for r in range(args.rounds):
        for arith, D, kind in [(a, d, k) for a in ARITHS for d in DECS for k in kinds]:
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
            print("round %d %s D %d %-7s kernel %8.4f ms (median %8.4f)  call %8.4f ms (median %8.4f)  %s  segments %d   %s" %
                  (r, arith, D, kind, rec["kernel_ms"], rec["kernel_ms_median"], rec["call_ms"], rec["call_ms_median"], rec["kernel"], rec["time_segments"],
                   "; ".join(rec["clocks"])), flush=True)
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
