"""tests/debug/prefilter_pc_time.py -- what two-stage decimation costs a bank of receivers on one MI355X (not collected by pytest).

4096 AM channels x 2^14 INPUT samples, one shared IF row (msdr_chain_set_input_rows, n_inputs 1), seeded random oscillator steps, Q15 and F32
(no cascade, no nodes: the demodulator kernel alone), every case at fs / 32:

  parent_d32_832   msdr_chain_set_decimation(32) with an 832-tap channel filter on a build of the PARENT commit (--parent-lib):
                   chain_q15pcnd_kernel / chain_f32pcnd_kernel -- the one-stage filter as selective as (c)                                  (a)
  d32_832          the same chain on this build, prefilter off: the same kernels, which this change does not touch                          (b)
  pre_8_4          msdr_chain_set_prefilter(8, 32 taps), msdr_chain_set_decimation(4), 104 channel taps: chain_q15pcn2_kernel /
                   chain_f32pcn2_kernel                                                                                                     (c)
  parent_d32_104   the parent's D = 32 with 104 taps: NOT the same filter as (c) -- it cannot reject what folds into fs / 32 --, for the reader

The configurations ALTERNATE, each step in a child process of its own under its own time limit, and the run stops at the first step that
fails.  Per step: device time of the main kernel (msdr_chain_enable_timing: HIP events around its launch) over `reps` calls behind two
warm-up calls, the fastest and the median of three runs, with the clocks rocm-smi reports read at the end of the step.

usage: python tests/debug/prefilter_pc_time.py [--parent-lib PATH/libmsdr.so] [--out FILE.json] [--rounds N] [--reps N] [--kinds a,b,...]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KINDS = ["parent_d32_832", "d32_832", "pre_8_4", "parent_d32_104"]
ARITHS = ["q15", "f32"]
LIMIT_S = 120


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=20).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln]
    except Exception as e:          # the tool may be missing: the timing stands without it
        return ["rocm-smi: %s" % e]


def step(arith, kind, reps):
    import numpy as np
    import torch                                   # first: the library binds to the HIP runtime torch initialised
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    ch, n = 4096, 1 << 14
    f32 = arith == "f32"
    pre = kind == "pre_8_4"
    nt = 104 if pre else int(kind.split("_")[-1])
    D1, D = (8, 4) if pre else (1, 32)
    stream = torch.cuda.Stream()
    ctx = msdr.Context(0, stream=stream.cuda_stream)

    def lowpass(count, cutoff):          # a windowed sinc of unit DC gain, cutoff in cycles per sample of the rate it runs at
        k = np.arange(count) - (count - 1) / 2.0
        h = np.sinc(2.0 * cutoff * k) * np.kaiser(count, 6.0)
        h /= h.sum()
        return h.astype(np.float32) if f32 else np.round(h * 32767.0).astype(np.int16)

    taps = lowpass(nt, 0.4 / 32 * D1)          # the channel filter: 0.4 of the output rate, designed at fs / D1
    tab = np.zeros(128, np.float32 if f32 else np.int16)          # (the tables a table-mixer chain is created with; nothing reads them in this mode)
    chain = msdr.Chain(ctx, msdr.ARITH_F32 if f32 else msdr.ARITH_Q15, ch, taps, taps, mixer=msdr.MIXER_NCO, mode=msdr.MODE_AM, osc_i=tab, osc_q=tab)
    (chain.set_taps_channels_f32 if f32 else chain.set_taps_channels)(0, np.tile(taps, (ch, 1)))
    chain.set_nco_channels(0, np.random.default_rng(7).integers(0, 1 << 32, ch, dtype=np.uint64).astype(np.uint32))
    chain.set_input_rows(np.zeros(ch, np.int64), 1)
    if pre:
        chain.set_prefilter(D1, lowpass(32, 0.4 / D1))
    chain.set_decimation(D)
    D *= D1
    x = torch.randint(-12000, 12001, (1, n), dtype=torch.int16, device="cuda")
    y = torch.empty(ch * (n // D), dtype=torch.float32 if f32 else torch.int16, device="cuda")
    for _ in range(2):
        chain.process(x.data_ptr(), y.data_ptr(), n)
    torch.cuda.synchronize()
    chain.enable_timing(True)
    runs = []
    for _ in range(3):
        chain.kernel_time()
        for _ in range(reps):
            chain.process(x.data_ptr(), y.data_ptr(), n)
        ms, launches = chain.kernel_time()
        runs.append(ms / max(launches, 1))
    info = chain.info()
    print(json.dumps({"arith": arith, "kind": kind, "decimation": D, "prefilter": D1, "kernel_ms": min(runs), "kernel_ms_median": sorted(runs)[1], "kernel": info["kernel"],
                      "grid": info["grid"], "block": info["block"], "lds_bytes": info["lds_bytes"], "tile": info["tile"], "time_segments": info["time_segments"],
                      "channels": ch, "samples": n, "taps": nt, "reps": reps, "clocks": clocks(), "device": torch.cuda.get_device_name(0),
                      "lib": os.environ.get("MSDR_LIB", "")}), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--parent-lib", help="libmsdr.so of the parent commit (the parent_* cases); without it those cases are left out")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--step", help="arith:kind -- run this one step in this process")
    args = ap.parse_args()
    if args.step:
        return step(*args.step.split(":"), args.reps)
    kinds = [kd for kd in args.kinds.split(",") if not kd.startswith("parent_") or args.parent_lib]
    res, rc = [], 0
    for r in range(args.rounds):
        for arith in ARITHS:
            for kind in kinds:
                cmd = [sys.executable, os.path.abspath(__file__), "--step", "%s:%s" % (arith, kind), "--reps", str(args.reps)]
                env = dict(os.environ)
                if kind.startswith("parent_"):
                    env["MSDR_LIB"] = os.path.abspath(args.parent_lib)
                try:
                    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=LIMIT_S, env=env)
                except subprocess.TimeoutExpired:
                    print("round %d %s %s ran over its %d s: stopping" % (r, arith, kind, LIMIT_S), flush=True)
                    rc = 1
                    break
                if p.returncode != 0:
                    print("round %d %s %s failed (exit %d): stopping\n%s" % (r, arith, kind, p.returncode, p.stderr[-2000:]), flush=True)
                    rc = 1
                    break
                rec = json.loads(p.stdout.strip().splitlines()[-1])
                rec["round"] = r
                res.append(rec)
                print("round %d %s %-15s kernel %8.4f ms (median %8.4f)  %s  tile %d  lds %d   %s" % (r, arith, kind, rec["kernel_ms"], rec["kernel_ms_median"], rec["kernel"],
                                                                                                  rec["tile"], rec["lds_bytes"], "; ".join(rec["clocks"])), flush=True)
            if rc:
                break
        if rc:
            break
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return rc


if __name__ == "__main__":
    sys.exit(main())
