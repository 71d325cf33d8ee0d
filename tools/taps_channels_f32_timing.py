"""tools/taps_channels_f32_timing.py -- what per-channel FIR coefficients cost an fp32 chain on one MI355X.

An fp32 chain (Fs/4 mix, AM, two-stage cascade: the reference's low-pass Q 0.54 and notch Q 15) is timed with its channels on ONE shared tap
set (the uniform kernels) and with every channel on taps of its own (msdr_chain_set_taps_channels_f32: chain_f32pc_kernel, the CMSIS-order
cascade and the history kernel behind it):

  long102_*   4096 channels x 2^18 samples, 102 taps, one call per step
  long256_*   the c3 shape: the same with 256 taps
  tick4096_*  one 128-sample block per call, 4096 channels, 102 taps
  tick1_*     the same with ONE receiver
  *_valu      the yardstick of the long calls: the uniform chain on the vector ALU (MSDR_CHAIN_NO_MFMA: chain_fold_kernel), same shape

Every step runs in a child process of its own under its own time limit, and the run stops at the first step that fails.  Device time per
call from HIP events around a run of back-to-back calls, and the demodulator kernel alone from msdr_chain_enable_timing.  The per-kernel
split of a step comes from running that step under a profiler:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/taps_channels_f32_timing.py --step long256_per_channel --quick

usage: python tools/taps_channels_f32_timing.py [--out FILE.json] [--quick] [--parent-lib LIBMSDR_SO] [--only PREFIX]
  --parent-lib: the uniform and yardstick steps are also run on that build of the library (the commit before this path), same process
  order, same box: `*@parent`."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ["long102_uniform", "long102_valu", "long102_per_channel", "long256_uniform", "long256_valu", "long256_per_channel",
         "tick4096_uniform", "tick4096_per_channel", "tick1_uniform", "tick1_per_channel"]
LIMIT_S = 300


def step(name, quick):
    import numpy as np
    import torch                                   # first: the library binds to the HIP runtime torch initialised
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    shape, kind = name.split("_", 1)
    ch, n, nt, reps = {"long102": (4096, 1 << 18, 102, 5), "long256": (4096, 1 << 18, 256, 5), "tick4096": (4096, 128, 102, 2000),
                       "tick1": (1, 128, 102, 2000)}[shape]
    if quick:
        reps = max(2, reps // 10)
    stream = torch.cuda.Stream()
    ctx = msdr.Context(0, stream=stream.cuda_stream)
    corr = msdr.AUDIO_SAMPLE_RATE_EXACT / 24000.0

    def taps_of(bw):
        return (msdr.calc_fir_coeffs(nt, bw)[:nt].astype(np.float64) / 32768.0).astype(np.float32)

    def section(kind_, f, q):
        c = np.asarray(msdr.biquad_design(kind_, np.float32(f * corr), q), np.float64) / 1073741824.0
        return [c[0], c[1], c[2], -c[3], -c[4]]
    bq = np.array([section(msdr.BQ_LOWPASS, 5400.0, 0.54), section(msdr.BQ_NOTCH, 3000.0, 15.0)], np.float32)
    taps = taps_of(2400.0)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, taps, taps, mode=msdr.MODE_AM, biquad_coeffs=bq, flags=msdr.CHAIN_NO_MFMA if kind == "valu" else 0)
    if kind == "per_channel":                      # the bandwidth menu's 196 values (125 .. 5000 Hz in steps of 25), dealt round the bank
        menu = [taps_of(125.0 + 25.0 * k) for k in range(196)]
        chain.set_taps_channels_f32(0, np.stack([menu[c % 196] for c in range(ch)]))
    x = torch.randint(-12000, 12001, (ch, n), dtype=torch.int16, device="cuda")
    y = torch.empty(ch * n, dtype=torch.float32, device="cuda")
    for _ in range(3):
        chain.process(x.data_ptr(), y.data_ptr(), n)
    torch.cuda.synchronize()
    best = None
    for _ in range(3):                             # three runs of `reps` calls, the fastest (clocks settle during the first)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            chain.process(x.data_ptr(), y.data_ptr(), n)
        e1.record(stream)
        e1.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / reps
        best = us if best is None else min(best, us)
    chain.enable_timing(True)                      # the demodulator kernel alone
    for _ in range(min(reps, 200)):
        chain.process(x.data_ptr(), y.data_ptr(), n)
    ms, launches = chain.kernel_time()
    info = chain.info()
    print(json.dumps({"step": name, "us_per_call": best, "main_kernel_us": ms * 1e3 / max(launches, 1), "kernel": info["kernel"], "flavour": info["flavour"],
                      "grid": info["grid"], "block": info["block"], "lds_bytes": info["lds_bytes"], "time_segments": info["time_segments"], "channels": ch,
                      "samples": n, "taps": nt, "device": torch.cuda.get_device_name(0)}), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="a tenth of the repetitions (for a profiler run)")
    ap.add_argument("--step", choices=STEPS, help="run this one step in this process")
    ap.add_argument("--parent-lib")
    ap.add_argument("--only", help="only the steps whose name starts with this")
    args = ap.parse_args()
    if args.step:
        return step(args.step, args.quick)
    plan = []
    for s in STEPS:
        if args.only and not s.startswith(args.only):
            continue
        if args.parent_lib and "per_channel" not in s:
            plan.append((s + "@parent", s, args.parent_lib))
        plan.append((s, s, None))
    res = {}
    rc = 0
    for key, s, lib in plan:
        env = dict(os.environ)
        if lib:
            env["MSDR_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--step", s] + (["--quick"] if args.quick else [])
        try:
            r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            print("step %s ran over its %d s: stopping" % (key, LIMIT_S), flush=True)
            rc = 1
            break
        if r.returncode != 0:
            print("step %s failed (exit %d): stopping\n%s" % (key, r.returncode, r.stderr[-2000:]), flush=True)
            rc = 1
            break
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        res[key] = rec
        print("%-32s %12.2f us per call  (main kernel %10.2f)   %s" % (key, rec["us_per_call"], rec["main_kernel_us"], rec["kernel"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return rc


if __name__ == "__main__":
    sys.exit(main())
