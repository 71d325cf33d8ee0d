"""tools/taps_channels_timing.py -- what per-channel FIR coefficients cost on one MI355X.

A Q15 chain (Fs/4 mix, AM, both biquad nodes with one stage each: low-pass and notch) is timed with its channels on ONE shared tap set
(the uniform kernels: chain_q15mf_kernel on long calls, the fused chain_q15mb_kernel tick at 128 samples) and with every channel on taps
of its own (msdr_chain_set_taps_channels: chain_q15pc_kernel, the node kernel and the history kernel behind it):

  long102_*   4096 channels x 2^18 samples, 102 taps, one call per step
  long256_*   the q15_c3 shape: the same with 256 taps
  tick4096_*  one 128-sample block per call, 4096 channels, 102 taps
  tick1_*     the same with ONE receiver

Every step runs in a child process of its own under its own time limit, and the run stops at the first step that fails.  Device time per
call from HIP events around a run of back-to-back calls; for the per-channel steps also the demodulator kernel alone
(msdr_chain_enable_timing).  The per-kernel split of a step comes from running that step under a profiler:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/taps_channels_timing.py --step long102_per_channel --quick

usage: python tools/taps_channels_timing.py [--out FILE.json] [--quick] [--parent-lib LIBMSDR_SO]
  --parent-lib: the uniform steps are also run on that build of the library (the commit before per-channel taps), same process
  order, same box: `*_uniform@parent`."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ["long102_uniform", "long102_per_channel", "long256_uniform", "long256_per_channel", "tick4096_uniform", "tick4096_per_channel",
         "tick1_uniform", "tick1_per_channel"]
LIMIT_S = 240


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
    taps = msdr.calc_fir_coeffs(nt, 2400)[:nt]
    lp = msdr.biquad_design(msdr.BQ_LOWPASS, np.float32(6000 * 0.9 * corr), 0.54)
    notch = msdr.biquad_design(msdr.BQ_NOTCH, np.float32(3000 * corr), 15.0)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps, taps, mode=msdr.MODE_AM, biquad_nodes=[[lp], [notch]])
    if kind == "per_channel":                      # the bandwidth menu's 196 values (125 .. 5000 Hz in steps of 25), dealt round the bank
        menu = [msdr.calc_fir_coeffs(nt, 125.0 + 25.0 * k)[:nt] for k in range(196)]
        chain.set_taps_channels(0, np.stack([menu[c % 196] for c in range(ch)]))
    x = torch.randint(-12000, 12001, (ch, n), dtype=torch.int16, device="cuda")
    y = torch.empty(ch * n, dtype=torch.int16, device="cuda")
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
    print(json.dumps({"step": name, "us_per_call": best, "main_kernel_us": ms * 1e3 / max(launches, 1), "kernel": info["kernel"], "grid": info["grid"],
                      "block": info["block"], "lds_bytes": info["lds_bytes"], "channels": ch, "samples": n, "taps": nt,
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    ctx.close()

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="a tenth of the repetitions (for a profiler run)")
    ap.add_argument("--step", choices=STEPS, help="run this one step in this process")
    ap.add_argument("--parent-lib")
    args = ap.parse_args()
    if args.step:
        return step(args.step, args.quick)
    plan = []
    for s in STEPS:
        if args.parent_lib and "uniform" in s:
            plan.append((s + "@parent", s, args.parent_lib))
        plan.append((s, s, None))
    res = {}
    for key, s, lib in plan:
        env = dict(os.environ)
        if lib:
            env["MSDR_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--step", s] + (["--quick"] if args.quick else [])
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=LIMIT_S)
        if r.returncode != 0:
            print("step %s failed (exit %d): stopping\n%s" % (key, r.returncode, r.stderr[-2000:]), flush=True)
            return 1
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        res[key] = rec
        print("%-32s %12.2f us per call  (main kernel %10.2f)   %s" % (key, rec["us_per_call"], rec["main_kernel_us"], rec["kernel"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
