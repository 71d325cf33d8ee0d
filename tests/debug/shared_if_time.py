"""tests/debug/shared_if_time.py -- what the input map (msdr_chain_set_input_rows) costs a chain on one MI355X (not collected by pytest).

4096 AM channels x 2^14 samples, 102 taps, NCO mixer with osc_len 128 and 4096 distinct oscillator rows (msdr_chain_set_osc_channels), Q15
and F32, no cascade and no nodes: chain_q15pco_kernel / chain_f32pco_kernel and the history kernel behind it.

  parent      a build of the PARENT commit (--parent-lib), replicated input [4096][n]                                   (a)
  replicated  this build, the setter never called, replicated input                                                       (b)
  shared1     this build, msdr_chain_set_input_rows with n_inputs = 1: every receiver hears the one row                   (c)
  shared64    ... with n_inputs = 64: receiver c hears row c % 64                                                          (c)

Per round the steps run as  parent, replicated, parent, shared1, shared64  -- (a) and (b) alternate and (a) repeats, so that the spread of
(a) over the session is what (b) and (c) are held against.  Each step is a child process of its own under its own time limit, and the run
stops at the first step that fails.  Per step: milliseconds per msdr_chain_process call (events on the chain's stream around `reps` calls
behind two warm-up calls -- more than one history length, so no oscillator generation is pending), the fastest and the median of three
runs; the main kernel's own time (msdr_chain_enable_timing) beside it; the clocks rocm-smi reports at the end of the step; msdr_build_rev().

usage: python tests/debug/shared_if_time.py --parent-lib PATH/libmsdr.so [--out FILE.json] [--rounds N] [--reps N]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ORDER = ["parent", "replicated", "parent", "shared1", "shared64"]
ARITHS = ["q15", "f32"]
LIMIT_S = 150


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
    ch, n, nt, L = 4096, 1 << 14, 102, 128
    f32 = arith == "f32"
    n_inputs = {"shared1": 1, "shared64": 64}.get(kind, 0)
    stream = torch.cuda.Stream()
    ctx = msdr.Context(0, stream=stream.cuda_stream)
    lib = msdr.load_library()
    lib.msdr_build_rev.restype = ctypes.c_char_p
    q = msdr.calc_fir_coeffs(nt, 2400.0)[:nt].copy()
    taps = (q.astype(np.float64) / 32768.0).astype(np.float32) if f32 else q
    k = (1 + 3 * np.arange(ch)) % L
    a = 2 * np.pi * k[:, None] * np.arange(L)[None, :] / L + 0.61 * np.arange(ch)[:, None]
    oi, oq = np.round(32767 * np.sin(a)).astype(np.int16), np.round(32767 * np.cos(a)).astype(np.int16)
    if f32:
        oi, oq = (oi / 32768.0).astype(np.float32), (oq / 32768.0).astype(np.float32)
    chain = msdr.Chain(ctx, msdr.ARITH_F32 if f32 else msdr.ARITH_Q15, ch, taps, taps, mixer=msdr.MIXER_NCO, mode=msdr.MODE_AM, osc_i=oi[0], osc_q=oq[0])
    chain.set_osc_channels(0, oi, oq)
    if n_inputs:
        chain.set_input_rows(np.arange(ch) % n_inputs, n_inputs=n_inputs)
    x = torch.randint(-12000, 12001, (n_inputs or ch, n), dtype=torch.int16, device="cuda")
    y = torch.empty(ch * n, dtype=torch.float32 if f32 else torch.int16, device="cuda")
    for _ in range(2):
        chain.process(x.data_ptr(), y.data_ptr(), n)
    torch.cuda.synchronize()
    chain.enable_timing(True)
    calls, kernels = [], []
    for _ in range(3):
        chain.kernel_time()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            chain.process(x.data_ptr(), y.data_ptr(), n)
        e1.record(stream)
        e1.synchronize()
        calls.append(e0.elapsed_time(e1) / reps)
        ms, launches = chain.kernel_time()
        kernels.append(ms / max(launches, 1))
    info = chain.info()
    print(json.dumps({"arith": arith, "kind": kind, "call_ms": min(calls), "call_ms_median": sorted(calls)[1], "kernel_ms": min(kernels), "kernel": info["kernel"],
                      "grid": info["grid"], "block": info["block"], "lds_bytes": info["lds_bytes"], "flavour": info["flavour"], "channels": ch, "samples": n, "taps": nt,
                      "osc_len": L, "n_inputs": n_inputs, "reps": reps, "clocks": clocks(), "device": torch.cuda.get_device_name(0),
                      "build_rev": lib.msdr_build_rev().decode(), "lib": os.environ.get("MSDR_LIB", "")}), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libmsdr.so built from the parent commit: yardstick (a)")
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step", help="arith:kind -- run this one step in this process")
    args = ap.parse_args()
    if args.step:
        return step(*args.step.split(":"), args.reps)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        print("--parent-lib: a build of the parent commit is needed for yardstick (a)")
        return 2
    res, rc = [], 0
    for r in range(args.rounds):
        for arith in ARITHS:
            for kind in ORDER:
                env = dict(os.environ)
                env.pop("MSDR_LIB", None)
                if kind == "parent":
                    env["MSDR_LIB"] = os.path.abspath(args.parent_lib)
                cmd = [sys.executable, os.path.abspath(__file__), "--step", "%s:%s" % (arith, "replicated" if kind == "parent" else kind), "--reps", str(args.reps)]
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
                rec["round"], rec["kind"] = r, kind
                res.append(rec)
                print("round %d %s %-10s call %8.4f ms (median %8.4f)  kernel %8.4f ms  %s  rev %s   %s" % (r, arith, kind, rec["call_ms"], rec["call_ms_median"], rec["kernel_ms"],
                                                                                                          rec["kernel"], rec["build_rev"], "; ".join(rec["clocks"])), flush=True)
            if rc:
                break
        if rc:
            break
    for arith in ARITHS:
        a = [x["call_ms"] for x in res if x["arith"] == arith and x["kind"] == "parent"]
        if len(a) < 2:
            continue
        spread = max(a) - min(a)
        print("%s (a) parent %s: spread %.4f ms" % (arith, ", ".join("%.4f" % v for v in a), spread))
        for kind in ("replicated", "shared1", "shared64"):
            v = [x["call_ms"] for x in res if x["arith"] == arith and x["kind"] == kind]
            if v:
                print("%s %-10s %s" % (arith, kind, ", ".join("%.4f" % t for t in v)))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return rc


if __name__ == "__main__":
    sys.exit(main())
