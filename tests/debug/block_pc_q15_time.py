"""tests/debug/block_pc_q15_time.py -- what one launch per tick is worth to a per-receiver Q15 chain on one MI355X (not collected by pytest).

4096 AM channels x 128 samples per call, 102 taps, NCO mixer with osc_len 128 and 4096 distinct per-channel rows, two one-stage
AudioFilterBiquad nodes with per-channel records -- microseconds per tick, GPU time between two events on the chain's stream around `ticks`
consecutive calls:

  parent_off   (with --parent-lib PATH) off_direct on another build of the library: the commit before the block kernel
  off_direct   the block kernel off: chain_q15pco_kernel + biquad_teensy_pc_kernel<2> + history_kernel per tick
  on_direct    msdr_chain_set_block_kernel_q15(1): chain_q15pcb_kernel, one launch per tick
  on_graph     the same as a 64-tick HIP graph (msdr_chain_graph_create), replayed

The configurations ALTERNATE, each step in a child process of its own under its own time limit, and the run stops at the first step that
fails.  Per step the fastest and the median of five runs behind a warm-up run, with the clocks rocm-smi reports read at the end of the step.

usage: python tests/debug/block_pc_q15_time.py [--out FILE.json] [--rounds N] [--ticks N] [--kinds off_direct,on_direct,on_graph] [--parent-lib PATH] [--tag NAME]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KINDS = ["off_direct", "on_direct", "on_graph"]
LIMIT_S = 120
GRAPH_TICKS = 64


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=20).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln]
    except Exception as e:          # the tool may be missing: the timing stands without it
        return ["rocm-smi: %s" % e]


def step(kind, ticks):
    import numpy as np
    import torch                                   # first: the library binds to the HIP runtime torch initialised
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import msdr
    ch, n, nt, L = 4096, 128, 102, 128
    ticks = (ticks + GRAPH_TICKS - 1) // GRAPH_TICKS * GRAPH_TICKS
    stream = torch.cuda.Stream()
    ctx = msdr.Context(0, stream=stream.cuda_stream)
    taps = msdr.calc_fir_coeffs(nt, 2400.0)[:nt].copy()
    k = (1 + 3 * np.arange(ch)) % L
    a = 2 * np.pi * k[:, None] * np.arange(L)[None, :] / L + 0.61 * np.arange(ch)[:, None]
    oi, oq = np.round(32767 * np.sin(a)).astype(np.int16), np.round(32767 * np.cos(a)).astype(np.int16)
    assert len({r.tobytes() for r in oi}) == ch
    corr = msdr.AUDIO_SAMPLE_RATE_EXACT / 24000.0
    lp = msdr.biquad_design(msdr.BQ_LOWPASS, np.float32(5400.0 * corr), 0.54)
    notches = np.stack([msdr.biquad_design(msdr.BQ_NOTCH, np.float32((2500.0 + 0.25 * c) * corr), 15.0) for c in range(ch)])
    lows = np.stack([msdr.biquad_design(msdr.BQ_LOWPASS, np.float32((4400.0 + 0.25 * c) * corr), 0.54) for c in range(ch)])
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps, taps, mixer=msdr.MIXER_NCO, mode=msdr.MODE_AM, osc_i=oi[0], osc_q=oq[0], biquad_nodes=[[lp], [notches[0]]])
    chain.set_taps_channels(0, np.tile(taps, (ch, 1)))
    chain.set_node_coefficients_channels(0, 0, 0, lows)
    chain.set_node_coefficients_channels(1, 0, 0, notches)
    chain.set_osc_channels(0, oi, oq)
    if kind in ("on_direct", "on_graph"):
        chain.set_block_kernel_q15(1)
    xs = [torch.randint(-12000, 12001, (ch, n), dtype=torch.int16, device="cuda") for _ in range(GRAPH_TICKS)]
    ys = [torch.empty(ch * n, dtype=torch.int16, device="cuda") for _ in range(GRAPH_TICKS)]
    torch.cuda.synchronize()
    for t in range(4):                              # the pending generation of set_osc_channels leaves with the first history length
        chain.process(xs[t].data_ptr(), ys[t].data_ptr(), n)
    graph = chain.graph([x.data_ptr() for x in xs], [y.data_ptr() for y in ys], n) if kind == "on_graph" else None

    def run():
        if graph:
            for _ in range(ticks // GRAPH_TICKS):
                graph.launch()
        else:
            for t in range(ticks):
                chain.process(xs[t % GRAPH_TICKS].data_ptr(), ys[t % GRAPH_TICKS].data_ptr(), n)

    runs = []
    with torch.cuda.stream(stream):
        run()
        stream.synchronize()
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            run()
            e1.record(stream)
            stream.synchronize()
            runs.append(e0.elapsed_time(e1) * 1000.0 / ticks)
    info = chain.info()
    print(json.dumps({"kind": kind, "us_per_tick": min(runs), "us_per_tick_median": sorted(runs)[2], "kernel": info["kernel"], "grid": info["grid"],
                      "block": info["block"], "lds_bytes": info["lds_bytes"], "channels": ch, "samples": n, "taps": nt, "osc_len": L, "nodes": 2,
                      "ticks": ticks, "clocks": clocks(), "device": torch.cuda.get_device_name(0), "lib": os.environ.get("MSDR_LIB", "")}), flush=True)
    if graph:
        graph.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ticks", type=int, default=512)
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--tag", default="")
    ap.add_argument("--parent-lib", help="libmsdr.so of the commit before the block kernel: adds the step parent_off in front of every round")
    ap.add_argument("--step", help="kind -- run this one step in this process")
    args = ap.parse_args()
    if args.step:
        return step(args.step, args.ticks)
    res, rc = [], 0
    for r in range(args.rounds):
        for kind in (["parent_off"] if args.parent_lib else []) + args.kinds.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", kind, "--ticks", str(args.ticks)]
            env = dict(os.environ, MSDR_LIB=os.path.abspath(args.parent_lib)) if kind == "parent_off" else None
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=LIMIT_S, env=env)
            except subprocess.TimeoutExpired:
                print("round %d %s ran over its %d s: stopping" % (r, kind, LIMIT_S), flush=True)
                rc = 1
                break
            if p.returncode != 0:
                print("round %d %s failed (exit %d): stopping\n%s" % (r, kind, p.returncode, p.stderr[-2000:]), flush=True)
                rc = 1
                break
            rec = json.loads(p.stdout.strip().splitlines()[-1])
            rec["round"], rec["tag"] = r, args.tag
            res.append(rec)
            print("round %d %-10s %8.2f us per tick (median %8.2f)  %s  lds %d   %s" % (r, kind, rec["us_per_tick"], rec["us_per_tick_median"], rec["kernel"],
                                                                                       rec["lds_bytes"], "; ".join(rec["clocks"])), flush=True)
        if rc:
            break
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return rc


if __name__ == "__main__":
    sys.exit(main())
