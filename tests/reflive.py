"""The compiled reference's answers to the inputs of the `*_live` tests (tests/test_oracle_pinned.py, tests/test_abi.py), recorded
in tests/golden/ref_live.npz and tests/golden/ref_live_dspinst.npz so that those tests also run where oracle/_ref/libmsdr_ref.so
cannot be built.

Each case function draws its inputs from a fixed seed, asks an orclib.Reference for the answers and returns inputs and answers
as one dict of arrays.  answers(name) gives the recorded dict and, where the reference is built, the same case asked of it
now; the tests hold the oracle (or the product) to every dict they get.  Recorded again where the reference is present:
    python tests/reflive.py
"""
import ctypes as C
import os

import numpy as np

import orclib

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PI = {False: "pif", True: "pid"}
SSAT_SHIFTS = (0, 1, 14, 15, 16)


def _designer(ref, seed, n_hi, types, stops):
    rng = np.random.default_rng(seed)
    d, params = {}, []
    for i in range(60):
        n = int(rng.integers(4, n_hi)) & ~1
        fc, a = float(rng.integers(100, 9000)), float(rng.choice(stops))
        t, dfc = int(rng.integers(0, types)), float(rng.integers(50, 2000))
        params.append((n, fc, a, t, dfc))
        for pid in (False, True):
            d["c%d_%s" % (i, PI[pid])] = ref.calc_fir_coeffs(n, fc, a, t, dfc, 24000.0, pi_double=pid)
    d["params"] = np.array(params, np.float64)
    return d


def designer(ref):
    """calc_FIR_coeffs, 60 random designs with both PIs, and the Hilbert branch (type 4) at 8, 32, 64 taps."""
    d = _designer(ref, 11, 300, 4, [10.0, 30.0, 45.5, 50.0, 70.0, 90.0])
    for n in (8, 32, 64):
        d["hilbert_n%d" % n] = ref.calc_fir_coeffs(n, 0, 70, 4)
    return d


def designer_wide(ref):
    """calc_FIR_coeffs up to 518 taps and filter types 0..4, both PIs."""
    return _designer(ref, 22, 520, 5, [20.0, 45.5, 70.0, 90.0])


def izero_msinc(ref):
    x = np.linspace(0, 12, 97, dtype=np.float32)
    m = np.arange(-40, 41, 2)
    fc = np.array([0.01, 0.2333, 0.5])
    return {"x": x, "izero": np.array([ref.lib.Izero(float(v)) for v in x], np.float32), "m": m, "fc": fc,
            "m_sinc": np.array([[ref.lib.m_sinc(int(k), float(f)) for f in fc] for k in m], np.float32)}


def fir_q15(ref):
    """arm_fir_fast_q15 in consecutive blocks: 40 random tap sets, amplitudes and block lengths."""
    rng = np.random.default_rng(5)
    d = {"cases": np.array(40)}
    for i in range(40):
        n = int(rng.integers(2, 140)) * 2
        amp = int(rng.choice([300, 8000, 32767]))
        taps = rng.integers(-amp, amp + 1, n).astype(np.int16)
        blk = int(rng.choice([1, 2, 3, 4, 5, 64, 127, 128, 129, 256]))
        x = rng.integers(-32768, 32768, blk * int(rng.integers(1, 5))).astype(np.int16)
        rc, y = ref.fir_q15_blocks(taps, x, blk)
        assert rc == 0
        d.update({"c%d_taps" % i: taps, "c%d_x" % i: x, "c%d_block" % i: np.array(blk), "c%d_y" % i: y})
    return d


def sqrt_q31(ref):
    rng = np.random.default_rng(9)
    vals = list(rng.integers(-5, 2 ** 31, 3000)) + [2 ** 31 - 1, 1, 0, -2 ** 31] + [2 ** k for k in range(31)]
    v = np.array([int(x) for x in vals], np.int64)
    res = [ref.sqrt_q31(int(x)) for x in v]
    return {"in": v, "rc": np.array([r[0] for r in res], np.int32), "out": np.array([r[1] for r in res], np.int32)}


def rfft128(ref):
    rng = np.random.default_rng(128)
    xs, outs, works = [], [], []
    for case in range(300):
        amp = (300, 8000, 32767, 32767)[case % 4]
        x = rng.integers(-amp, amp + 1, 128).astype(np.int16)
        if case % 4 == 3:
            x[rng.integers(0, 128, 40)] = -32768
            x[rng.integers(0, 128, 40)] = 32767
        out, work = ref.rfft128_q15(x)
        xs.append(x)
        outs.append(out)
        works.append(work)
    return {"x": np.array(xs), "out": np.array(outs), "work": np.array(works)}


def dspinst(ref):
    """signed_multiply_32x16b/t, signed_saturate_rshift (16 bits, shifts SSAT_SHIFTS), pack_16b_16b on 30000 random pairs."""
    R = ref.lib
    for n in ("dspinst_signed_multiply_32x16b", "dspinst_signed_multiply_32x16t"):
        getattr(R, n).restype = C.c_int32
        getattr(R, n).argtypes = [C.c_int32, C.c_uint32]
    R.dspinst_signed_saturate_rshift.restype = C.c_int32
    R.dspinst_signed_saturate_rshift.argtypes = [C.c_int32, C.c_int, C.c_int]
    R.dspinst_pack_16b_16b.restype = C.c_uint32
    R.dspinst_pack_16b_16b.argtypes = [C.c_int32, C.c_int32]
    rng = np.random.default_rng(77)
    a = rng.integers(-2 ** 31, 2 ** 31, 30000).astype(np.int32)
    b = rng.integers(-2 ** 31, 2 ** 31, 30000).astype(np.int32)
    a[:8] = [0x7FFFFFFF, -0x80000000, 0x40000000, -0x40000000, -1, 1, 0x3FFF, -0x4000]
    b[:8] = [-0x80000000, 0x7FFFFFFF, 0x80008000 - (1 << 32), 0x7FFF7FFF, -1, 0x00010001, 0x8000, 0x7FFF]
    ai, bi = [int(x) for x in a], [int(y) for y in b]
    return {"a": a, "b": b,
            "mulwb": np.array([R.dspinst_signed_multiply_32x16b(x, y & 0xFFFFFFFF) for x, y in zip(ai, bi)], np.int32),
            "mulwt": np.array([R.dspinst_signed_multiply_32x16t(x, y & 0xFFFFFFFF) for x, y in zip(ai, bi)], np.int32),
            "ssat16": np.array([[R.dspinst_signed_saturate_rshift(x, 16, sh) for x in ai] for sh in SSAT_SHIFTS], np.int16),
            "pack_bb": np.array([R.dspinst_pack_16b_16b(x, y) for x, y in zip(ai, bi)], np.uint32)}


def am_sqrt_f32(ref):
    """arm_sqrt_f32 on every kind of int32 sum the AM / CW branch can hand it, converted to float."""
    ref.lib.cmsis_arm_sqrt_f32.restype = C.c_int
    ref.lib.cmsis_arm_sqrt_f32.argtypes = [C.c_float, C.POINTER(C.c_float)]
    rng = np.random.default_rng(5)
    vals = np.concatenate([rng.integers(-2 ** 31, 2 ** 31, 20000).astype(np.float32), np.arange(0, 4096, dtype=np.float32) ** 2,
                           np.array([0.0, -0.0, 1e-45, -1e-45, 2147483648.0, -2147483648.0, 2.0 * 32768.0 ** 2, np.inf], np.float32)])
    outs, rcs = [], []
    for v in vals:
        out = C.c_float(-1.0)
        rcs.append(ref.lib.cmsis_arm_sqrt_f32(float(v), C.byref(out)))
        outs.append(np.float32(out.value))
    return {"in": vals, "out": np.array(outs, np.float32), "rc": np.array(rcs, np.int32)}


CASES = {"designer": designer, "designer_wide": designer_wide, "izero_msinc": izero_msinc, "fir_q15": fir_q15, "sqrt_q31": sqrt_q31,
         "rfft128": rfft128, "dspinst": dspinst, "am_sqrt_f32": am_sqrt_f32}


def _file(name):
    return os.path.join(HERE, "ref_live_dspinst.npz" if name == "dspinst" else "ref_live.npz")


def recorded(name):
    z = np.load(_file(name))
    pre = name + "/"
    d = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    assert d, "%s: no case %r recorded" % (_file(name), name)
    return d


def answers(name):
    """[recorded answers] + [the compiled reference's answers now, where oracle/_ref/libmsdr_ref.so is built]."""
    out = [recorded(name)]
    if orclib.Reference.available():
        out.append(CASES[name](orclib.Reference()))
    return out


def record():
    ref = orclib.Reference()
    files = {}
    for name, fn in CASES.items():
        files.setdefault(_file(name), {}).update({name + "/" + k: v for k, v in fn(ref).items()})
    for path, arrays in files.items():
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    record()
