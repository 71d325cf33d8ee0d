#!/usr/bin/env python3
"""tools/pc_kernels_digest.py -- what the per-receiver chain kernels compute and how they are launched, as digests (not collected by pytest).

Runs against the library MSDR_LIB names (default: this tree's build).  Run it once against a build of one commit and once against a build of
another: the two JSON files are byte-identical exactly when every case gives the same output bits from the same launches.  --out holds
one line per case (the SHA-256 over the case's records); --records FILE keeps the records themselves, to find the shape that differs.

Cases reach every instantiation and every oscillator policy of chain_q15pc / chain_f32pc / chain_q15pco / chain_f32pco / chain_q15pcn /
chain_f32pcn / chain_q15pcnd / chain_f32pcnd and the block kernels chain_f32pcb / chain_q15pcb:
per-channel taps (Fs/4, the shared NCO table, the table with a pending generation; LSB / USB / AM, both square roots and a SYNCAM channel
under the PLL on Q15), per-channel oscillator rows with and without a pending generation, a set_input_rows map (on the taps, the rows, the
phase accumulator and the block kernels), the phase-accumulator oscillator (*_nco_steps: set_nco_channels with steps off the 128 grid;
*_nco_pending: some channels retuned between the priming call and the calls that count; *_nco_map: behind a set_input_rows map; the table
mixer's cases have the names *_nco and *_pending), decimation by 2, 3, 4 and 8 (*_dec: every read width AL of both kernels),
the two FIR stages with per-channel coefficients, block-kernel ticks (Fs/4, shared table, bank; 0 and 2 cascade stages, shared and per-channel rows; fp32 and int16),
and one long call with time segments.  7 channels; n in {128, 256, 1003} (block kernel: 128, 256, 512; decimation: 64, 250 and 1003 OUTPUTS,
n = outputs x factor, so that every factor meets 4, 2 and 1 channels per wave); 13, 21 and 30 taps (padded rows of 16,
24 and 32; Q15: 14, 22 and 30 taps, the same rows -- arm_fir_init_q15 takes even counts only); osc_len 24.

Every shape of a case: a priming call of 37 samples (36 with 21 taps: the calls that count start with a full history at a non-zero phase, odd
and even, so that both arrangements of the Fs/4 flavour's rows and accumulators run at every n), the
case's pending change if it has one (decimation is set here: the priming call runs undecimated), then TWO calls of n samples; the record holds the SHA-256 of the two outputs' bytes and what
msdr_chain_get_info reports behind the second.  Each case runs in a child process under its own time limit; the run stops at the first failure.

usage: python tools/pc_kernels_digest.py [--out FILE.json] [--records FILE.json] [--cases a,b,...]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 120
CH, L = 7, 24
NS, NTS = (128, 256, 1003), (13, 21, 30)
NOUTS = (64, 250, 1003)          # outputs of a decimated call
INFO = ("kernel", "grid", "block", "lds_bytes", "time_segments", "tile")
MAP = [0, 1, 0, 2, 1, 0, 2]          # set_input_rows: 7 receivers on 3 input rows


def ntaps(nt, f32):
    return nt if f32 else nt + (nt & 1)


def prime(nt):
    """length of the priming call: odd for 13 and 30 taps, even for 21, so that every n meets both parities of phase0 (the Fs/4 row swap)"""
    return 36 if nt == 21 else 37


def osc(rng, rows, f32):
    a = 2 * np.pi * rng.integers(1, L, rows)[:, None] * np.arange(L)[None, :] / L + rng.uniform(0, 6.28, rows)[:, None]
    oi, oq = np.round(32767 * np.sin(a)).astype(np.int16), np.round(32767 * np.cos(a)).astype(np.int16)
    return ((oi / 32768.0).astype(np.float32), (oq / 32768.0).astype(np.float32)) if f32 else (oi, oq)


def taps(rng, rows, nt, f32):
    return (rng.standard_normal((rows, nt)) * 0.08).astype(np.float32) if f32 else rng.integers(-2500, 2501, (rows, nt)).astype(np.int16)


def set_map(chain):
    chain.set_input_rows(np.array(MAP))


def record(obj, channels, calls, out_dtype, in_dtype=np.int16):
    """calls: the inputs of the priming call and of the two calls that count, in order; a callable among them runs between two calls"""
    h, k = hashlib.sha256(), 0
    for c in calls:
        if callable(c):
            c()
            continue
        dx, dy = ctx.to_device(np.ascontiguousarray(c, in_dtype)), ctx.array((channels, c.shape[1] // getattr(obj, "decimation", lambda: 1)()), out_dtype)
        obj.process(dx, dy, c.shape[1])
        if k:
            h.update(dy.download().tobytes())
        k += 1
    return h.hexdigest()


def chain_case(name):
    """per-channel taps / oscillator rows / input rows: name = <arith>_<what>"""
    arith, what = name.split("_", 1)
    f32 = arith == "f32"
    out = []
    for n in NS:
        for nt in NTS:
            rng = np.random.default_rng([n, nt, len(name)])
            ci, cq = taps(rng, CH, ntaps(nt, f32), f32), taps(rng, CH, ntaps(nt, f32), f32)
            oi, oq = osc(rng, CH, f32)
            ni, nq = osc(rng, CH, f32)
            modes = np.array([msdr.MODE_LSB, msdr.MODE_USB, msdr.MODE_AM, msdr.MODE_SYNCAM if what == "pll" else msdr.MODE_CW, msdr.MODE_AM, msdr.MODE_LSB, msdr.MODE_USB], np.int32)
            nco = what != "fs4"
            chain = msdr.Chain(ctx, msdr.ARITH_F32 if f32 else msdr.ARITH_Q15, CH, ci[0], cq[0], mixer=msdr.MIXER_NCO if nco else msdr.MIXER_FS4, modes=modes,
                               osc_i=oi[0] if nco else None, osc_q=oq[0] if nco else None, sqrt_kind=msdr.SQRT_Q31 if what == "nco_q31" else msdr.SQRT_F32,
                               flags=msdr.CHAIN_SYNCAM_PLL if what == "pll" else 0)
            (chain.set_taps_channels_f32 if f32 else chain.set_taps_channels)(0, ci, cq)
            change, rows = None, CH
            if what in ("rows", "rows_pending", "rows_map"):
                chain.set_osc_channels(0, oi, oq)
            if what == "pending":
                change = lambda: chain.set_osc(ni[0], nq[0])          # noqa: E731
            if what == "rows_pending":
                change = lambda: chain.set_osc_channels(2, ni[:4], nq[:4])          # noqa: E731
            if what in ("map", "rows_map"):
                set_map(chain)
                rows = max(MAP) + 1
            x = [rng.integers(-20000, 20001, (rows, m)).astype(np.int16) for m in (prime(nt), n, n)]
            sha = record(chain, CH, [x[0]] + ([change] if change else []) + x[1:], np.float32 if f32 else np.int16)
            info = chain.info()
            out.append(dict(n=n, taps=nt, sha256=sha, **{k: info[k] for k in INFO}))
            chain.close()
    return out


def nco_case(name):
    """the phase-accumulator oscillator: name = <arith>_<nco_steps | nco_pending | nco_map | dec>"""
    arith, what = name.split("_", 1)
    f32 = arith == "f32"
    out = []
    for D in ((2, 3, 4, 8) if what == "dec" else (1,)):
        for n in (NOUTS if what == "dec" else NS):
            for nt in NTS:
                rng = np.random.default_rng([D, n, nt, len(name)])
                ci, cq = taps(rng, CH, ntaps(nt, f32), f32), taps(rng, CH, ntaps(nt, f32), f32)
                oi, oq = osc(rng, 1, f32)
                steps, phases = [(rng.integers(1, 1 << 32, CH, dtype=np.uint64) | np.uint64(1)).astype(np.uint32) for _ in range(2)], [rng.integers(0, 1 << 32, CH, dtype=np.uint64).astype(np.uint32) for _ in range(2)]
                modes = np.array([msdr.MODE_LSB, msdr.MODE_USB, msdr.MODE_AM, msdr.MODE_CW, msdr.MODE_AM, msdr.MODE_LSB, msdr.MODE_USB], np.int32)
                chain = msdr.Chain(ctx, msdr.ARITH_F32 if f32 else msdr.ARITH_Q15, CH, ci[0], cq[0], mixer=msdr.MIXER_NCO, modes=modes, osc_i=oi[0], osc_q=oq[0])
                (chain.set_taps_channels_f32 if f32 else chain.set_taps_channels)(0, ci, cq)
                chain.set_nco_channels(0, steps[0], phases[0])
                change, rows = None, CH
                if what == "nco_pending":
                    change = lambda: chain.set_nco_channels(2, steps[1][:4], phases[1][:4])          # noqa: E731
                if what == "dec":
                    change = lambda: chain.set_decimation(D)          # noqa: E731
                if what == "nco_map":
                    set_map(chain)
                    rows = max(MAP) + 1
                x = [rng.integers(-20000, 20001, (rows, m)).astype(np.int16) for m in (prime(nt), n * D, n * D)]
                sha = record(chain, CH, [x[0]] + ([change] if change else []) + x[1:], np.float32 if f32 else np.int16)
                info = chain.info()
                out.append(dict(n=n * D, taps=nt, sha256=sha, **({"decimation": D} if what == "dec" else {}), **{k: info[k] for k in INFO}))
                chain.close()
    return out


def fir_case(name):
    f32 = name == "f32_fir"
    out = []
    for n in NS:
        for nt in NTS:
            rng = np.random.default_rng([n, nt, 99])
            c = taps(rng, CH, ntaps(nt, f32), f32)
            fir = (msdr.FirF32 if f32 else msdr.FirQ15)(ctx, c[0], CH)
            fir.set_coeffs_channels(0, c)
            dt = np.float32 if f32 else np.int16
            x = [(rng.standard_normal((CH, m)) * 0.3).astype(np.float32) if f32 else rng.integers(-20000, 20001, (CH, m)).astype(np.int16) for m in (prime(nt), n, n)]
            rec = dict(n=n, taps=nt, sha256=record(fir, CH, x, dt, dt))
            if f32:
                rec["kernel"] = fir.kernel_name()
            out.append(rec)
            fir.close()
    return out


def block_case(name):
    """block-kernel ticks: name = block_<fs4 | shared | bank | map> (map: the bank behind a set_input_rows map)"""
    what = name.split("_", 1)[1]
    out = []
    bq = np.array([[0.2066, 0.4131, 0.2066, 0.3695, -0.1958], [0.9766, -1.3815, 0.9766, 1.3815, -0.9533]], np.float32)
    for n in (128, 256, 512):
        for nt in NTS:
            for stages, pc_rows in ((0, False), (2, False), (2, True)):
                for i16 in (False, True):
                    rng = np.random.default_rng([n, nt, stages, int(pc_rows), int(i16)])
                    ci, cq = taps(rng, CH, nt, True), taps(rng, CH, nt, True)
                    oi, oq = osc(rng, CH, True)
                    modes = np.array([(msdr.MODE_AM, msdr.MODE_LSB, msdr.MODE_USB)[c % 3] for c in range(CH)], np.int32)
                    nco = what != "fs4"
                    chain = msdr.Chain(ctx, msdr.ARITH_F32, CH, ci[0], cq[0], mixer=msdr.MIXER_NCO if nco else msdr.MIXER_FS4, modes=modes, osc_i=oi[0] if nco else None,
                                       osc_q=oq[0] if nco else None, biquad_coeffs=bq if stages else None, flags=msdr.CHAIN_OUT_I16 if i16 else 0)
                    chain.set_taps_channels_f32(0, ci, cq)
                    if pc_rows:
                        chain.set_biquad_coeffs_channels(0, np.stack([bq * np.float32([1.0, 1.0 - 0.002 * c, 1.0, 1.0 - 0.002 * c, 1.0]) for c in range(CH)]))
                    if what in ("bank", "map"):
                        chain.set_osc_channels(0, oi, oq)
                    if what == "map":
                        set_map(chain)
                    chain.set_block_kernel(1)
                    x = [rng.integers(-20000, 20001, (max(MAP) + 1 if what == "map" else CH, m)).astype(np.int16) for m in (prime(nt), n, n)]
                    sha = record(chain, CH, x, np.int16 if i16 else np.float32)
                    info = chain.info()
                    out.append(dict(n=n, taps=nt, stages=stages, rows_per_channel=pc_rows, out_i16=i16, sha256=sha, **{k: info[k] for k in INFO}))
                    chain.close()
    return out


def long_case(name):
    """64 channels x 2^16 samples: time segments"""
    out = []
    ch, n, nt = 64, 1 << 16, 30
    for arith in ("q15", "f32"):
        for rows in (False, True):
            f32 = arith == "f32"
            rng = np.random.default_rng([7, int(f32), int(rows)])
            ci, cq = taps(rng, ch, nt, f32), taps(rng, ch, nt, f32)
            oi, oq = osc(rng, ch, f32)
            chain = msdr.Chain(ctx, msdr.ARITH_F32 if f32 else msdr.ARITH_Q15, ch, ci[0], cq[0], mixer=msdr.MIXER_NCO, mode=msdr.MODE_LSB, osc_i=oi[0], osc_q=oq[0])
            (chain.set_taps_channels_f32 if f32 else chain.set_taps_channels)(0, ci, cq)
            if rows:
                chain.set_osc_channels(0, oi, oq)
            x = [rng.integers(-20000, 20001, (ch, m)).astype(np.int16) for m in (prime(nt), n, n)]
            sha = record(chain, ch, x, np.float32 if f32 else np.int16)
            info = chain.info()
            out.append(dict(arith=arith, osc_rows=rows, n=n, taps=nt, sha256=sha, **{k: info[k] for k in INFO}))
            chain.close()
    return out


CASES = {}
for _a in ("q15", "f32"):
    for _w in ("fs4", "nco", "pending", "rows", "rows_pending", "map", "rows_map"):
        CASES["%s_%s" % (_a, _w)] = chain_case
    for _w in ("nco_steps", "nco_pending", "nco_map", "dec"):
        CASES["%s_%s" % (_a, _w)] = nco_case
    CASES["%s_fir" % _a] = fir_case
CASES.update({"q15_nco_q31": chain_case, "q15_pll": chain_case, "block_fs4": block_case, "block_shared": block_case, "block_bank": block_case, "block_map": block_case, "long": long_case})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="one line per case: its records folded into one SHA-256 (default: to stdout)")
    ap.add_argument("--records", help="every record of every case, to see which shape differs when two runs do")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--case", help="run this one case in this process")
    args = ap.parse_args()
    if args.case:
        global msdr, ctx
        sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
        import msdr
        ctx = msdr.Context(0)
        print(json.dumps(CASES[args.case](args.case)), flush=True)
        ctx.close()
        return 0
    res, rc = {}, 0
    for name in args.cases.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            print("%s ran over its %d s: stopping" % (name, LIMIT_S), file=sys.stderr, flush=True)
            rc = 1
            break
        if p.returncode != 0:
            print("%s failed (exit %d): stopping\n%s" % (name, p.returncode, p.stderr[-3000:]), file=sys.stderr, flush=True)
            rc = 1
            break
        res[name] = json.loads(p.stdout.strip().splitlines()[-1])
        print("%s: %d records" % (name, len(res[name])), file=sys.stderr, flush=True)
    if args.records:
        with open(args.records, "w") as f:
            f.write(json.dumps(res, indent=1, sort_keys=True) + "\n")
    # one line per case: the SHA-256 over its records (each: shape, output digest, launch), so that two runs compare at a glance
    text = "{\n" + ",\n".join(' "%s": %s' % (name, json.dumps({"records": len(recs), "kernels": sorted({r["kernel"] for r in recs if "kernel" in r}),
                                                             "sha256": hashlib.sha256(json.dumps(recs, sort_keys=True).encode()).hexdigest()}, sort_keys=True))
                             for name, recs in sorted(res.items())) + "\n}\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    return rc


if __name__ == "__main__":
    sys.exit(main())
