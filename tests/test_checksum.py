"""The per-tile checksum of include/dswx_hip.h (ABI v7) without a GPU: its numpy statement (proteus_amd/checksum.py)
against a scalar loop written here, the library's scalar statement (dswx_checksum_host) against the numpy one, the
properties the header promises, and every error path of the three entries that needs no device."""
import ctypes

import numpy as np
import pytest

from proteus_amd import _capi
from proteus_amd.checksum import checksum, checksum_tiles

M64 = (1 << 64) - 1
# the header's numbers, written out again: the test shares no constant with the code under test
K, M1, M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def scalar_checksum(raw):
    """The definition, word by word, in Python integers."""
    def mix(x):
        x ^= x >> 30
        x = (x * M1) & M64
        x ^= x >> 27
        x = (x * M2) & M64
        x ^= x >> 31
        return x
    raw = bytes(raw)
    c = mix(len(raw))
    for g in range((len(raw) + 7) // 8):
        w = 0
        for i, byte in enumerate(raw[8 * g:8 * g + 8]):
            w |= byte << (8 * i)
        c = (c + mix((w + (g + 1) * K) & M64)) & M64
    return c


def test_header_states_the_constants_as_numbers():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dswx_hip.h')).read()
    for name, v in (('DSWX_CHECKSUM_K', K), ('DSWX_CHECKSUM_M1', M1), ('DSWX_CHECKSUM_M2', M2)):
        assert f'#define {name} 0x{v:016X}ULL' in text
    assert K & 1 and M1 & 1 and M2 & 1
    assert '#define DSWX_ABI_VERSION 7' in text and _capi.DSWX_ABI_VERSION == 7


BIG_SIZES = (4095, 4096, 4097, 65536 + 3, 1 << 20)


def test_numpy_statement_against_a_scalar_loop():
    rng = np.random.default_rng(7001)
    pool = rng.integers(0, 256, size=(1 << 20) + 64, dtype=np.uint8)
    assert checksum(b'') == scalar_checksum(b'') == 0                   # mix(0)
    n_cases = 0
    for nbytes in list(range(0, 81)) + list(BIG_SIZES):
        offsets = (0,) + tuple(range(1, 16, 2)) if nbytes <= 80 or nbytes == 65536 + 3 else (0, 1, 7)
        for off in offsets:
            raw = pool[off:off + nbytes]
            want = scalar_checksum(raw.tobytes())
            assert checksum(raw) == want, (nbytes, off)
            assert checksum(raw.tobytes()) == want and checksum(memoryview(raw.tobytes())) == want
            for dt in (np.uint16, np.int32, np.float64):               # the same bytes as 2-, 4-, 8-byte elements, at this address
                if nbytes % np.dtype(dt).itemsize == 0:
                    assert checksum(raw.view(dt)) == want, (nbytes, off, dt)
                    n_cases += 1
            n_cases += 1
    assert n_cases > 1400
    # an array is taken in C order whatever its shape and strides
    a = rng.integers(-32768, 32768, size=(37, 53)).astype(np.int16)
    assert checksum(a) == scalar_checksum(a.tobytes())
    assert checksum(a.T) == scalar_checksum(np.ascontiguousarray(a.T).tobytes())
    assert checksum(a[::2, 1::3]) == scalar_checksum(a[::2, 1::3].tobytes())
    t = rng.integers(0, 256, size=(5, 9, 11), dtype=np.uint8)
    assert checksum_tiles(t).tolist() == [scalar_checksum(t[k].tobytes()) for k in range(5)]
    # many tiles at a time: every tile length around a word and two, every element size, a view that is not contiguous
    for nbytes in list(range(1, 26)) + [136, 4097]:
        for dt in (np.uint8, np.int16, np.uint32, np.float64):
            if nbytes % np.dtype(dt).itemsize == 0:
                t = rng.integers(0, 256, size=(7, nbytes + 8), dtype=np.uint8).view(dt)[:, :nbytes // np.dtype(dt).itemsize]
                assert checksum_tiles(t).tolist() == [scalar_checksum(t[k].tobytes()) for k in range(7)], (nbytes, dt)
    assert checksum_tiles(np.zeros((0, 4), dtype=np.uint8)).shape == (0,)
    assert checksum_tiles(np.zeros((3, 0), dtype=np.uint8)).tolist() == [0, 0, 0]


def test_library_scalar_statement_against_the_numpy_statement():
    """dswx_checksum_host loads and runs without a GPU."""
    lib = _capi.load_library()
    rng = np.random.default_rng(7002)
    pool = rng.integers(0, 256, size=(1 << 20) + 64, dtype=np.uint8)
    for nbytes in list(range(0, 81)) + list(BIG_SIZES):
        for off in (0,) + tuple(range(1, 16, 2)):
            raw = pool[off:off + nbytes]
            v = ctypes.c_uint64(123)
            assert lib.dswx_checksum_host(ctypes.c_void_p(raw.ctypes.data), nbytes, ctypes.byref(v)) == 0
            assert v.value == checksum(raw), (nbytes, off)
    for dt in (np.uint8, np.int16, np.float32, np.int64):
        a = rng.integers(0, 200, size=(31, 17)).astype(dt)
        assert _capi.checksum_host(a) == checksum(a) == scalar_checksum(a.tobytes())
    assert _capi.checksum_host(b'') == 0 and _capi.checksum_host(np.zeros(0, np.uint16)) == 0
    assert _capi.checksum_host(b'abc') == checksum(b'abc')


def test_any_single_bit_flip_changes_the_value():
    """mix is a bijection, so a change confined to one 8-byte word ALWAYS shows: every bit of a 203-byte buffer, then random
    bits of random buffers of every element size."""
    rng = np.random.default_rng(7003)
    base = rng.integers(0, 256, size=203, dtype=np.uint8)
    c0 = checksum(base)
    seen = {c0}
    for bit in range(203 * 8):
        b = base.copy()
        b[bit >> 3] ^= 1 << (bit & 7)
        c = checksum(b)
        assert c != c0, bit
        seen.add(c)
    assert len(seen) == 203 * 8 + 1
    n = 0
    for case in range(10000):
        eb = (1, 2, 4, 8)[case & 3]
        a = rng.integers(0, 256, size=eb * int(rng.integers(1, 40)), dtype=np.uint8)
        if case % 7 == 0:
            a[:] = (0, 255)[case & 1]                                   # constant planes are what real layers often are
        bit = int(rng.integers(0, a.size * 8))
        b = a.copy()
        b[bit >> 3] ^= 1 << (bit & 7)
        assert checksum(a.view(f'u{eb}')) != checksum(b.view(f'u{eb}')), case
        n += 1
    assert n >= 10000


def test_swaps_shifts_and_row_swaps_change_the_value():
    rng = np.random.default_rng(7004)
    n = 0
    for case in range(10000):
        dt = (np.uint8, np.uint16, np.uint32, np.uint64)[case & 3]
        # few distinct values, as in a classified layer: equal elements are common, cancellation would be easy
        a = rng.integers(0, int(rng.integers(2, 6)), size=int(rng.integers(2, 120))).astype(dt)
        c0 = checksum(a)
        i, j = (int(v) for v in rng.integers(0, a.size, size=2))
        if a[i] != a[j]:
            b = a.copy()
            b[i], b[j] = a[j], a[i]
            assert checksum(b) != c0, ('swap', case)
            n += 1
        if (a != a[0]).any():
            assert checksum(np.roll(a, 1)) != c0, ('shift 1', case)
            n += 1
    assert n >= 10000
    n = 0
    for case in range(2500):                                            # shifts by 1024 need longer buffers
        dt = (np.uint8, np.uint16, np.uint32, np.uint64)[case & 3]
        a = rng.integers(0, 3, size=int(rng.integers(1025, 3000))).astype(dt)
        c0 = checksum(a)
        for k in (1, 1024):
            b = np.roll(a, k)
            if not np.array_equal(a, b):
                assert checksum(b) != c0, ('shift', k, case)
                n += 1
        h = int(rng.integers(2, 12))
        p = rng.integers(0, 3, size=(h, int(rng.integers(1, 300)))).astype(dt)
        r0, r1 = (int(v) for v in rng.integers(0, h, size=2))
        if not np.array_equal(p[r0], p[r1]):
            q = p.copy()
            q[[r0, r1]] = p[[r1, r0]]
            assert checksum(q) != checksum(p), ('rows', case)
            n += 1
    assert n >= 5000
    # a period-aligned plane: rows of exactly 1024 bytes that differ, swapped; and a transposed square
    p = rng.integers(0, 256, size=(8, 1024), dtype=np.uint8)
    q = p.copy()
    q[[2, 5]] = p[[5, 2]]
    assert checksum(q) != checksum(p)
    s = rng.integers(0, 4, size=(64, 64), dtype=np.uint8)
    assert not np.array_equal(s, s.T) and checksum(s.T) != checksum(s)


def test_the_construction_that_defeats_a_linear_checksum_is_detected():
    """sum of w_g * odd(g) misses a swap of two words 128 apart that differ in their top bytes only: (w_g - w_h) is a
    multiple of 2^56 and odd(g) - odd(h) = -256.  The position key inside mix does not."""
    def linear(words):
        return sum(int(w) * (2 * g + 1) for g, w in enumerate(words)) & M64
    rng = np.random.default_rng(7005)
    n = 0
    for case in range(2000):
        m = int(rng.integers(130, 400))
        w = rng.integers(0, 1 << 63, size=m, dtype=np.uint64)
        g = int(rng.integers(0, m - 128))
        low = int(w[g]) & ((1 << 56) - 1)
        tops = rng.choice(256, size=2, replace=False)
        w[g] = (int(tops[0]) << 56) | low
        w[g + 128] = (int(tops[1]) << 56) | low
        v = w.copy()
        v[g], v[g + 128] = w[g + 128], w[g]
        assert not np.array_equal(v, w)
        assert linear(v) == linear(w)                                   # the construction does defeat the linear form
        assert checksum(v.astype('<u8')) != checksum(w.astype('<u8')), case
        assert _capi.checksum_host(v.astype('<u8')) != _capi.checksum_host(w.astype('<u8'))
        n += 1
    assert n == 2000


def test_length_and_padding_are_part_of_the_value():
    """Trailing zero bytes are told apart from a shorter buffer (the zero padding of the last word is not the data)."""
    seen = set()
    for n in range(0, 64):
        seen.add(checksum(bytes(n)))
    assert len(seen) == 64
    a = np.arange(1, 20, dtype=np.uint8)
    assert checksum(a) != checksum(np.concatenate([a, np.zeros(1, np.uint8)]))


def test_error_paths_that_need_no_device():
    lib = _capi.load_library()
    vp = ctypes.c_void_p
    plane, out = vp(0x10000), vp(0x20000)          # never dereferenced: every call below fails before the device is touched

    def dev(ctx=None, plane=plane, eb=2, n_tiles=3, n=100, stride=0, out=out):
        return lib.dswx_checksum_device(ctx, plane, eb, n_tiles, n, stride, out, None)
    assert dev() == _capi.ERR_ARG and b'ctx' in lib.dswx_last_error()                       # null context, arguments fine
    for eb in (0, 3, 5, 16, -1):
        assert dev(eb=eb) == _capi.ERR_ARG and b'elem_bytes' in lib.dswx_last_error()
    assert dev(n_tiles=-1) == _capi.ERR_ARG and b'negative' in lib.dswx_last_error()
    assert dev(n=-1) == _capi.ERR_ARG and b'negative' in lib.dswx_last_error()
    assert dev(stride=-5) == _capi.ERR_ARG and b'negative' in lib.dswx_last_error()
    assert dev(n=100, stride=99) == _capi.ERR_ARG and b'stride' in lib.dswx_last_error()
    assert dev(plane=None) == _capi.ERR_ARG and dev(out=None) == _capi.ERR_ARG and b'NULL' in lib.dswx_last_error()
    assert dev(n_tiles=1 << 40) == _capi.ERR_ARG and dev(n=1 << 50) == _capi.ERR_ARG       # sizes whose products would overflow
    for eb in (2, 4, 8):
        for off in range(1, eb):
            assert dev(plane=vp(0x10000 + off), eb=eb) == _capi.ERR_ALIGN, (eb, off)
        assert dev(plane=vp(0x10000 + eb), eb=eb) == _capi.ERR_ARG                          # aligned: on to the context check
    assert dev(plane=vp(0x10001), eb=1) == _capi.ERR_ARG                                   # bytes sit anywhere
    for off in (1, 2, 4):
        assert dev(out=vp(0x20000 + off)) == _capi.ERR_ALIGN and b'out' in lib.dswx_last_error()
    # dswx_batch_checksum
    buf = (ctypes.c_uint64 * 4)()
    assert lib.dswx_batch_checksum(None, 1, 0, 1, buf, None) == _capi.ERR_ARG and b'batch is NULL' in lib.dswx_last_error()
    # dswx_checksum_host
    v = ctypes.c_uint64()
    assert lib.dswx_checksum_host(None, 8, ctypes.byref(v)) == _capi.ERR_ARG
    assert lib.dswx_checksum_host(buf, 8, None) == _capi.ERR_ARG and b'NULL' in lib.dswx_last_error()
    assert lib.dswx_checksum_host(None, 0, ctypes.byref(v)) == 0 and v.value == 0           # an empty buffer needs no pointer
    with pytest.raises(_capi.DswxError):
        _capi._check(dev())
