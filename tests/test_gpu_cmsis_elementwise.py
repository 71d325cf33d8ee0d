"""include/msdr_cmsis.h on the GPU: arm_mult_q15 / arm_add_q15 / arm_sub_q15 / arm_copy_q15 (arm_math.h:1898, 2412, 2468, 2831) with
their own argument lists, called through ctypes as a relinked freq_conv.cpp (:70-103) or demodulation() (Minimal-SDR.ino:577-578) calls
them; both bindings, the operand rules and the refusals.  Every check is bit-exact against a numpy restatement of the CMSIS arithmetic:
mult = ssat16((a * b) >> 15), add / sub = ssat16(a +/- b) (__QADD16 / __QSUB16), copy = a."""
import ctypes as C

import numpy as np
import pytest

from gpuhelp import ctx, msdr  # noqa: F401

pytestmark = pytest.mark.gpu

OPS = ("mult", "add", "sub", "copy")
EDGES = np.array([32767, -32768, -32767, -1, 0, 1, 16384, -16384], np.int16)


def model(op, a, b=None):
    a32 = a.astype(np.int32)
    if op == "copy":
        return a.copy()
    b32 = np.broadcast_to(b, a.shape).astype(np.int32)
    r = {"mult": (a32 * b32) >> 15, "add": a32 + b32, "sub": a32 - b32}[op]
    return np.clip(r, -32768, 32767).astype(np.int16)


def lib_of(ctx):
    lib = ctx.lib
    for n in ("mult", "add", "sub"):
        f = getattr(lib, "msdr_arm_%s_q15" % n)
        f.argtypes, f.restype = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32], None
    lib.msdr_arm_copy_q15.argtypes, lib.msdr_arm_copy_q15.restype = [C.c_void_p, C.c_void_p, C.c_uint32], None
    lib.msdr_cmsis_bind.argtypes = lib.msdr_cmsis_bind_host.argtypes = [C.c_void_p, C.c_uint32]
    return lib


def call(lib, op, a, b, dst, n):
    """a, b, dst: raw addresses (int) or numpy arrays (host)"""
    addr = [x.ctypes.data if isinstance(x, np.ndarray) else x for x in (a, b, dst)]
    if op == "copy":
        lib.msdr_arm_copy_q15(addr[0], addr[2], n)
    else:
        getattr(lib, "msdr_arm_%s_q15" % op)(addr[0], addr[1], addr[2], n)


def last_error(lib):
    return lib.msdr_last_error().decode()


def operands(rng, shape):
    """random q15 with the saturation edges mixed in: +/-32767, -32768 (and so -32768 x -32768), -1, 0"""
    a = rng.integers(-32768, 32768, shape).astype(np.int16)
    b = rng.integers(-32768, 32768, shape).astype(np.int16)
    m = rng.random(shape) < 0.3
    a[m] = rng.choice(EDGES, int(m.sum()))
    m = rng.random(shape) < 0.3
    b[m] = rng.choice(EDGES, int(m.sum()))
    k = min(4, a.size)
    a.reshape(-1)[:k] = [-32768, -32768, 32767, -32768][:k]
    b.reshape(-1)[:k] = [-32768, 32767, 32767, 1][:k]
    return a, b


@pytest.fixture
def unbind(ctx):
    yield
    lib_of(ctx).msdr_cmsis_bind(None, 0)


@pytest.mark.parametrize("channels", [1, 3, 4096])
@pytest.mark.parametrize("n", [1, 7, 128, 129, 1000])
def test_device_batch(ctx, unbind, channels, n):
    lib = lib_of(ctx)
    assert lib.msdr_cmsis_bind(ctx.h, channels) == 0
    a, b = operands(np.random.default_rng(channels * 1000 + n), (channels, n))
    da, db = ctx.to_device(a), ctx.to_device(b)
    for op in OPS:
        dd = ctx.array((channels, n), np.int16).fill(0x5a)
        call(lib, op, da.ptr, db.ptr, dd.ptr, n)
        assert np.array_equal(dd.download(), model(op, a, b)), (op, channels, n)


@pytest.mark.parametrize("n", [7, 128, 129])
def test_device_pointers_one_sample_off(ctx, unbind, n):
    """Sources and destination one sample past a 16-byte boundary (and each combination with aligned ones): the 2-byte-aligned path."""
    channels = 5
    lib = lib_of(ctx)
    assert lib.msdr_cmsis_bind(ctx.h, channels) == 0
    a, b = operands(np.random.default_rng(n), (channels, n))
    total = channels * n
    for offs in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (3, 1, 2)):
        bufs = []
        for k, (x, o) in enumerate(zip((a, b, None), offs)):
            full = np.zeros(total + 8, np.int16)
            if x is not None:
                full[o:o + total] = x.reshape(-1)
            bufs.append(ctx.to_device(full))
        for op in OPS:
            bufs[2].upload(np.full(total + 8, 1234, np.int16))
            call(lib, op, bufs[0].ptr + 2 * offs[0], bufs[1].ptr + 2 * offs[1], bufs[2].ptr + 2 * offs[2], n)
            got = bufs[2].download()
            o = offs[2]
            assert np.array_equal(got[o:o + total].reshape(channels, n), model(op, a, b)), (op, offs)
            assert (got[:o] == 1234).all() and (got[o + total:] == 1234).all(), (op, offs)     # nothing outside pDst


@pytest.mark.parametrize("n", [128, 129])
def test_device_destination_aliases_a_source(ctx, unbind, n):
    """pDst == pSrcA and pDst == pSrcB (the commented-out forms of freq_conv.cpp:75, :91)."""
    channels = 64
    lib = lib_of(ctx)
    assert lib.msdr_cmsis_bind(ctx.h, channels) == 0
    a, b = operands(np.random.default_rng(3 + n), (channels, n))
    for op in ("mult", "add", "sub"):
        da, db = ctx.to_device(a), ctx.to_device(b)
        call(lib, op, da.ptr, db.ptr, da.ptr, n)
        assert np.array_equal(da.download(), model(op, a, b)), op
        da, db = ctx.to_device(a), ctx.to_device(b)
        call(lib, op, da.ptr, db.ptr, db.ptr, n)
        assert np.array_equal(db.download(), model(op, a, b)), op
    da = ctx.to_device(a)
    call(lib, "copy", da.ptr, None, da.ptr, n)
    assert np.array_equal(da.download(), a)


@pytest.mark.parametrize("n", [128, 7])
def test_device_binding_shared_host_row(ctx, unbind, n):
    """A host source under msdr_cmsis_bind is ONE row shared by every channel (freq_conv.cpp's `(q15_t *) Osc_Q_buffer_i`); rewritten in
    place between two calls, each call sees the bytes it was made with (the first result is read only after the second call)."""
    channels = 96
    lib = lib_of(ctx)
    assert lib.msdr_cmsis_bind(ctx.h, channels) == 0
    rng = np.random.default_rng(11 + n)
    x, _ = operands(rng, (channels, n))
    row = np.round(32767 * np.sin(2 * np.pi * np.arange(n) / 16)).astype(np.int16)
    row[:2] = [-32768, 32767]
    first = row.copy()
    dx = ctx.to_device(x)
    for op in ("mult", "add", "sub"):
        d1, d2, d3 = (ctx.array((channels, n), np.int16) for _ in range(3))
        row[:] = first
        call(lib, op, dx.ptr, row, d1.ptr, n)
        row[:] = np.round(32767 * np.cos(2 * np.pi * np.arange(n) / 16)).astype(np.int16)       # the table rewritten in place
        second = row.copy()
        call(lib, op, dx.ptr, row, d2.ptr, n)
        call(lib, op, row, dx.ptr, d3.ptr, n)                                                     # the shared row as pSrcA
        assert np.array_equal(d1.download(), model(op, x, first[None, :])), op
        assert np.array_equal(d2.download(), model(op, x, second[None, :])), op
        assert np.array_equal(d3.download(), model(op, np.broadcast_to(second, x.shape), x)), op
    d4 = ctx.array((channels, n), np.int16)
    call(lib, "copy", row, None, d4.ptr, n)                                                       # a host row copied to every channel
    assert np.array_equal(d4.download(), np.broadcast_to(row, (channels, n)))


@pytest.mark.parametrize("channels,n", [(1, 128), (1, 7), (3, 129), (64, 128)])
def test_host_binding(ctx, unbind, channels, n):
    lib = lib_of(ctx)
    assert lib.msdr_cmsis_bind_host(ctx.h, channels) == 0
    a, b = operands(np.random.default_rng(channels + n), (channels, n))
    for op in OPS:
        dst = np.full((channels, n), 77, np.int16)
        call(lib, op, a, b, dst, n)
        assert np.array_equal(dst, model(op, a, b)), op
    for op in ("mult", "add", "sub"):              # pDst aliasing a source
        a2, b2 = a.copy(), b.copy()
        call(lib, op, a2, b2, a2, n)
        call(lib, op, a, b2, b2, n)
        assert np.array_equal(a2, model(op, a, b)) and np.array_equal(b2, model(op, a, b)), op


def test_copy_matches_pinned_golden(ctx, unbind, golden):
    """arm_copy_q15 on the compiled reference's answer (copy_q15/out: 131 samples of fir/x_full), under both bindings."""
    lib = lib_of(ctx)
    x = golden["fir/x_full"][:131].copy()
    want = golden["copy_q15/out"]
    assert lib.msdr_cmsis_bind_host(ctx.h, 1) == 0
    out = np.zeros(131, np.int16)
    call(lib, "copy", x, None, out, 131)
    assert np.array_equal(out, want)
    assert lib.msdr_cmsis_bind(ctx.h, 1) == 0
    dx, dd = ctx.to_device(x), ctx.array(131, np.int16)
    call(lib, "copy", dx.ptr, None, dd.ptr, 131)
    assert np.array_equal(dd.download(), want)


def test_refusals_leave_destination_unchanged(ctx, unbind):
    lib = lib_of(ctx)
    channels, n = 4, 128
    a, b = operands(np.random.default_rng(5), (channels, n))
    da, db = ctx.to_device(a), ctx.to_device(b)
    # a host pDst under the device binding
    assert lib.msdr_cmsis_bind(ctx.h, channels) == 0
    for op in OPS:
        dst = np.full((channels, n), 321, np.int16)
        call(lib, op, da.ptr, db.ptr, dst, n)
        assert (dst == 321).all() and "pDst" in last_error(lib), op
    # a device pointer under the host binding (as source and as destination)
    assert lib.msdr_cmsis_bind_host(ctx.h, channels) == 0
    for op in OPS:
        dst = np.full((channels, n), 321, np.int16)
        call(lib, op, da.ptr, b, dst, n)
        assert (dst == 321).all() and "device pointer" in last_error(lib), op
        dd = ctx.to_device(np.full((channels, n), 321, np.int16))
        call(lib, op, a, b, dd.ptr, n)
        assert (dd.download() == 321).all() and "device pointer" in last_error(lib), op
    # not bound
    assert lib.msdr_cmsis_bind(None, 0) == 0
    for op in OPS:
        dst = np.full((channels, n), 321, np.int16)
        call(lib, op, a, b, dst, n)
        assert (dst == 321).all() and "no context bound" in last_error(lib), op
        dd = ctx.to_device(np.full((channels, n), 321, np.int16))
        call(lib, op, da.ptr, db.ptr, dd.ptr, n)
        assert (dd.download() == 321).all() and last_error(lib) != "", op
    # blockSize 0 writes nothing
    assert lib.msdr_cmsis_bind_host(ctx.h, channels) == 0
    dst = np.full((channels, n), 321, np.int16)
    call(lib, "add", a, b, dst, 0)
    assert (dst == 321).all()


def test_c_abi_strides(ctx):
    """The batched entry points behind the shims (include/msdr.h): explicit row strides, stride 0 = a shared row, a padded source."""
    rng = np.random.default_rng(9)
    channels, n, pitch = 6, 129, 136
    a, b = operands(rng, (channels, pitch))
    row = rng.integers(-32768, 32768, n).astype(np.int16)
    da, db, drow = ctx.to_device(a), ctx.to_device(b), ctx.to_device(row)
    for op in ("mult", "add", "sub"):
        dd = ctx.array((channels, n), np.int16)
        getattr(ctx, op + "_q15")(da, drow, dd, channels, n, a_stride=pitch, b_stride=0)
        assert np.array_equal(dd.download(), model(op, a[:, :n], row[None, :])), op
        getattr(ctx, op + "_q15")(drow, db, dd, channels, n, a_stride=0, b_stride=pitch)
        assert np.array_equal(dd.download(), model(op, np.broadcast_to(row, (channels, n)), b[:, :n])), op
    dd = ctx.array((channels, 128), np.int16)
    ctx.copy_q15(da, dd, channels, 128, src_stride=pitch)
    assert np.array_equal(dd.download(), a[:, :128])
