"""tools/cmsis_elementwise_timing.py -- what the q15 element-wise CMSIS shims and the in-place FFT cost on one MI355X.

  1. arm_add_q15 on one 128-sample block (channels = 1) under msdr_cmsis_bind: device time per call (HIP events around a run of
     back-to-back calls on the context's stream) and host wall time per call (pointer classification + enqueue); next to it an empty
     kernel launch (torch.cuda._sleep(0)) and the same call under msdr_cmsis_bind_host (wall time: each call returns with the result)
  2. effective bandwidth of the batched add and mult at >= 1 GB of traffic per call (operands beyond the 256 MiB Infinity Cache),
     next to a device-to-device copy of the same traffic in the same run (hipMemcpyAsync and msdr_copy_q15)
  3. freq_conv.cpp's six calls (4 x arm_mult_q15, arm_add_q15, arm_sub_q15 with the host-global oscillator tables) against the native
     one-kernel AudioEffectFreqConv (msdr_freqconv_q15) at 4096 channels x 128
  4. arm_rfft_q15 (in place) against msdr_rfft128_q15 at 4096 transforms

usage: python tools/cmsis_elementwise_timing.py [--out FILE.json] [--quick]
Prints one line per figure and, with --out, writes them as JSON."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402  (first: the library binds to the HIP runtime torch initialised)

sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
import msdr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="fewer repetitions (for a profiler run)")
    args = ap.parse_args()
    reps = 200 if args.quick else 2000
    stream = torch.cuda.Stream()
    ctx = msdr.Context(0, stream=stream.cuda_stream)
    lib = ctx.lib
    for n in ("mult", "add", "sub"):
        getattr(lib, "msdr_arm_%s_q15" % n).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        getattr(lib, "msdr_arm_%s_q15" % n).restype = None
    lib.msdr_cmsis_bind.argtypes = lib.msdr_cmsis_bind_host.argtypes = [C.c_void_p, C.c_uint32]
    lib.msdr_memcpy_d2d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    res = {"device": torch.cuda.get_device_name(0)}

    def events(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        for _ in range(k):
            fn()
        e1.record(stream)
        wall = time.perf_counter() - t0
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / k, wall * 1e6 / k        # us per call: device, host enqueue

    def say(key, value, unit):
        res[key] = value
        print("%-58s %10.2f %s" % (key, value, unit), flush=True)

    # ---- 1. one 128-sample block ------------------------------------------------------------------------------------------------
    B = 128
    rng = np.random.default_rng(0)
    a, b = rng.integers(-32768, 32768, (2, B)).astype(np.int16)
    assert lib.msdr_cmsis_bind(ctx.h, 1) == 0
    da, db, dd = ctx.to_device(a), ctx.to_device(b), ctx.array(B, np.int16)
    dev, host = events(lambda: lib.msdr_arm_add_q15(da.ptr, db.ptr, dd.ptr, B), reps)
    say("add_1x128_device_binding_device_us_per_call", dev, "us")
    say("add_1x128_device_binding_host_us_per_call", host, "us")
    osc = np.ascontiguousarray(b)
    dev, host = events(lambda: lib.msdr_arm_add_q15(da.ptr, osc.ctypes.data, dd.ptr, B), reps)
    say("add_1x128_shared_host_row_device_us_per_call", dev, "us")
    say("add_1x128_shared_host_row_host_us_per_call", host, "us")
    with torch.cuda.stream(stream):
        dev, host = events(lambda: torch.cuda._sleep(0), reps)
    say("empty_kernel_device_us_per_launch", dev, "us")
    say("empty_kernel_host_us_per_launch", host, "us")
    assert lib.msdr_cmsis_bind_host(ctx.h, 1) == 0
    y = np.empty(B, np.int16)
    for _ in range(50):
        lib.msdr_arm_add_q15(a.ctypes.data, b.ctypes.data, y.ctypes.data, B)
    t0 = time.perf_counter()
    for _ in range(reps):
        lib.msdr_arm_add_q15(a.ctypes.data, b.ctypes.data, y.ctypes.data, B)
    say("add_1x128_host_binding_wall_us_per_call", (time.perf_counter() - t0) * 1e6 / reps, "us")

    # ---- 2. bandwidth beyond the Infinity Cache ---------------------------------------------------------------------------------
    assert lib.msdr_cmsis_bind(ctx.h, 1) == 0
    ch = 1 << 21 if not args.quick else 1 << 20        # 2 Mi x 128 samples = 512 MiB per operand: 1.5 GiB moved per add / mult
    n_bytes = ch * B * 2
    x = torch.randint(-32768, 32768, (ch, B), dtype=torch.int16, device="cuda")
    z = torch.randint(-32768, 32768, (ch, B), dtype=torch.int16, device="cuda")
    o = torch.empty_like(x)
    k = 10 if not args.quick else 3
    for name, fn in (("add", ctx.add_q15), ("mult", ctx.mult_q15)):
        dev, _ = events(lambda: fn(_Ptr(x), _Ptr(z), _Ptr(o), ch, B), k)
        say("%s_%dx128_GBps" % (name, ch), 3 * n_bytes / dev / 1e3, "GB/s")
    # a plain copy with the same traffic (1.5x the bytes of one operand, read and written)
    big = torch.empty(3 * n_bytes // 4, dtype=torch.int16, device="cuda")
    big2 = torch.empty_like(big)
    assert lib.msdr_memcpy_d2d(ctx.h, big2.data_ptr(), big.data_ptr(), big.numel() * 2) == 0
    dev, _ = events(lambda: lib.msdr_memcpy_d2d(ctx.h, big2.data_ptr(), big.data_ptr(), big.numel() * 2), k)
    say("hipMemcpyAsync_d2d_GBps", 2 * big.numel() * 2 / dev / 1e3, "GB/s")
    rows = big.numel() // B
    dev, _ = events(lambda: ctx.copy_q15(_Ptr(big), _Ptr(big2), rows, B), k)
    say("copy_q15_kernel_GBps", 2 * rows * B * 2 / dev / 1e3, "GB/s")
    del x, z, o, big, big2
    torch.cuda.empty_cache()

    # ---- 3. freq_conv.cpp's six calls vs the native node at 4096 x 128 ------------------------------------------------------------
    ch = 4096
    assert lib.msdr_cmsis_bind(ctx.h, ch) == 0
    I, Q = (ctx.to_device(rng.integers(-32768, 32768, (ch, B)).astype(np.int16)) for _ in range(2))
    A, Bk, Cc, D = (ctx.array((ch, B), np.int16) for _ in range(4))
    osc_i = np.round(32767 * np.sin(2 * np.pi * 32 * np.arange(B) / B)).astype(np.int16)
    osc_q = np.round(32767 * np.cos(2 * np.pi * 32 * np.arange(B) / B)).astype(np.int16)
    pi, pq = osc_i.ctypes.data, osc_q.ctypes.data

    def six():
        lib.msdr_arm_mult_q15(I.ptr, pq, A.ptr, B)
        lib.msdr_arm_mult_q15(Q.ptr, pi, Bk.ptr, B)
        lib.msdr_arm_mult_q15(Q.ptr, pq, Cc.ptr, B)
        lib.msdr_arm_mult_q15(I.ptr, pi, D.ptr, B)
        lib.msdr_arm_add_q15(A.ptr, Bk.ptr, I.ptr, B)
        lib.msdr_arm_sub_q15(Cc.ptr, D.ptr, Q.ptr, B)
    dev, host = events(six, reps // 4)
    say("freq_conv_six_calls_4096x128_device_us", dev, "us")
    say("freq_conv_six_calls_4096x128_host_us", host, "us")
    dev, host = events(lambda: ctx.freqconv_q15(I, Q, osc_i, osc_q, 0, 1, ch, B), reps // 4)
    say("freq_conv_native_node_4096x128_device_us", dev, "us")
    say("freq_conv_native_node_4096x128_host_us", host, "us")

    # ---- 4. the spectrum transform, in place vs read-only ---------------------------------------------------------------------------
    src, out = ctx.to_device(rng.integers(-32768, 32768, (ch, 128)).astype(np.int16)), ctx.array((ch, 256), np.int16)
    dev, _ = events(lambda: msdr.rfft128_q15(ctx, src, 128, ch, out), reps // 4)
    say("rfft128_4096_read_only_device_us", dev, "us")
    dev, _ = events(lambda: msdr.rfft128_q15_inplace(ctx, src, 128, ch, out), reps // 4)
    say("rfft128_4096_in_place_device_us", dev, "us")
    lib.msdr_cmsis_bind(None, 0)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


class _Ptr:
    """a torch tensor as the Context wrappers take device buffers (.ptr)"""

    def __init__(self, t):
        self.ptr = t.data_ptr()


if __name__ == "__main__":
    main()
