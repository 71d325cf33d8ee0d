"""tests/debug/cascade_pc_time.py -- what per-channel cascade coefficients cost an fp32 chain on one MI355X (not collected by pytest).

4096 channels x 2^18 samples, AM, Fs/4, 256 taps, a two-stage cascade (the reference's low-pass Q 0.54 + notch Q 15), every channel on FIR
taps of its own (chain_f32pc_kernel), the cascade in CMSIS order behind it:

  uniform      one cascade for the bank: biquad_df1_seq_kernel (the configuration profiles/taps_per_channel_f32/ recorded)
  per_channel  every channel its own notch (3000 Hz + 1 Hz x channel % 1000): biquad_df1_seq_pc_kernel

The two configurations ALTERNATE, each round in a child process of its own under its own time limit, and the run stops at the first step
that fails.  Per step: device time of the whole msdr_chain_process call (HIP events around a run of back-to-back calls, the fastest of three
runs) and of the cascade pass alone (msdr_ctx_get_kernel_time: the context's timer brackets the CMSIS-order cascade launch), with the
clocks rocm-smi reports read once at the end of the step.

usage: python tests/debug/cascade_pc_time.py [--out FILE.json] [--rounds N] [--reps N]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KINDS = ["uniform", "per_channel"]
LIMIT_S = 240


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=20).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln]
    except Exception as e:          # the tool may be missing: the timing stands without it
        return ["rocm-smi: %s" % e]


def step(kind, reps):
    import numpy as np
    import torch                                   # first: the library binds to the HIP runtime torch initialised
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    ch, n, nt = 4096, 1 << 18, 256
    stream = torch.cuda.Stream()
    ctx = msdr.Context(0, stream=stream.cuda_stream)
    corr = msdr.AUDIO_SAMPLE_RATE_EXACT / 24000.0

    def taps_of(bw):
        return (msdr.calc_fir_coeffs(nt, bw)[:nt].astype(np.float64) / 32768.0).astype(np.float32)

    def section(kind_, f, q):
        c = np.asarray(msdr.biquad_design(kind_, np.float32(f * corr), q), np.float64) / 1073741824.0
        return [c[0], c[1], c[2], -c[3], -c[4]]
    lp = section(msdr.BQ_LOWPASS, 5400.0, 0.54)
    bq = np.array([lp, section(msdr.BQ_NOTCH, 3000.0, 15.0)], np.float32)
    taps = taps_of(2400.0)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, taps, taps, mode=msdr.MODE_AM, biquad_coeffs=bq)
    menu = [taps_of(125.0 + 25.0 * k) for k in range(196)]
    chain.set_taps_channels_f32(0, np.stack([menu[c % 196] for c in range(ch)]))
    if kind == "per_channel":
        notches = [section(msdr.BQ_NOTCH, 3000.0 + k, 15.0) for k in range(1000)]
        chain.set_biquad_coeffs_channels(0, np.array([[lp, notches[c % 1000]] for c in range(ch)], np.float32))
    x = torch.randint(-12000, 12001, (ch, n), dtype=torch.int16, device="cuda")
    y = torch.empty(ch * n, dtype=torch.float32, device="cuda")
    for _ in range(2):
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
        ms = e0.elapsed_time(e1) / reps
        best = ms if best is None else min(best, ms)
    ctx.enable_kernel_timing(True)                 # the cascade pass alone
    ctx.kernel_time()
    for _ in range(reps):
        chain.process(x.data_ptr(), y.data_ptr(), n)
    cas_ms, launches = ctx.kernel_time()
    info = chain.info()
    print(json.dumps({"kind": kind, "call_ms": best, "cascade_ms": cas_ms / max(launches, 1), "cascade_launches": launches, "kernel": info["kernel"],
                      "flavour": info["flavour"], "channels": ch, "samples": n, "taps": nt, "reps": reps, "clocks": clocks(),
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--step", choices=KINDS, help="run this one step in this process")
    args = ap.parse_args()
    if args.step:
        return step(args.step, args.reps)
    res, rc = [], 0
    for r in range(args.rounds):
        for kind in KINDS:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", kind, "--reps", str(args.reps)]
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=LIMIT_S)
            except subprocess.TimeoutExpired:
                print("round %d %s ran over its %d s: stopping" % (r, kind, LIMIT_S), flush=True)
                rc = 1
                break
            if p.returncode != 0:
                print("round %d %s failed (exit %d): stopping\n%s" % (r, kind, p.returncode, p.stderr[-2000:]), flush=True)
                rc = 1
                break
            rec = json.loads(p.stdout.strip().splitlines()[-1])
            rec["round"] = r
            res.append(rec)
            print("round %d %-12s call %8.3f ms  cascade pass %8.3f ms   %s   %s" % (r, kind, rec["call_ms"], rec["cascade_ms"], rec["kernel"], "; ".join(rec["clocks"])), flush=True)
        if rc:
            break
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return rc


if __name__ == "__main__":
    sys.exit(main())
