"""The per-pixel composite of include/dswx_hip.h ("stack") without a GPU: the rule as a per-pixel Python loop written here,
pinned to the numpy statement (proteus_amd/stack.py) and to the library's scalar statement (dswx_stack_host) over every byte
value, every n_cats, tile counts and sizes either side of the kernel's units, strides with countable padding and odd
addresses; 65535 tiles whose packed counts must not carry; every refusal that needs no device; the header; the struct
mirrors; the WTR specs written out by hand; the C example."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from proteus_amd import _capi
from proteus_amd.stack import MAX_CATS, MAX_TILES, NONE, NO_SHARE, Spec, stack_tiles, wtr_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT8, SENT16 = 0xEE, 0xEEEE
KEYS = ('count', 'last', 'last_index', 'share')


# ---- the rule, written out again: one pixel at a time -----------------------------------------------------------------
def scalar_stack(tiles, n_cats, cat_of_byte, fill):
    """Python lists per output for a stack [T, N], by the words of the header."""
    T, N = tiles.shape
    count = [[0] * N for _ in range(n_cats)]
    last, last_index, share = [fill] * N, [65535] * N, [255] * N
    rows = tiles.tolist()
    cat = [int(c) for c in cat_of_byte]
    for i in range(N):
        for t in range(T):
            c = cat[rows[t][i]]
            if c < n_cats:
                count[c][i] += 1
                last[i], last_index[i] = rows[t][i], t
        n_obs = sum(count[k][i] for k in range(n_cats))
        if n_obs:
            share[i] = (100 * count[0][i]) // n_obs
    return {'count': np.array(count, dtype=np.uint16).reshape(n_cats, N), 'last': np.array(last, dtype=np.uint8),
            'last_index': np.array(last_index, dtype=np.uint16), 'share': np.array(share, dtype=np.uint8)}


def same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:4])


def random_spec(rng, n_cats, fill=None):
    # categories 0 .. 5: 4 and 5 are never observations, and for n_cats < 4 some of 1 .. 3 are not either
    return Spec(n_cats, rng.integers(0, 6, size=256).astype(np.uint8), rng.integers(0, 256) if fill is None else fill)


def test_numpy_statement_against_the_per_pixel_loop():
    rng = np.random.default_rng(9100)
    for n_cats in range(1, MAX_CATS + 1):
        for T, N in ((0, 5), (1, 7), (3, 1), (9, 40), (20, 33), (4, 0)):
            spec = random_spec(rng, n_cats)
            tiles = rng.integers(0, 256, size=(T, N), dtype=np.uint8)
            same(stack_tiles(tiles, spec), scalar_stack(tiles, n_cats, spec.cat_of_byte, spec.fill), (n_cats, T, N))
    # a few byte values only: long histories of one pixel, gaps of non-observations at either end
    spec = Spec(2, [1, 0, 0] + [9] * 253, 77)
    tiles = rng.choice(np.array([0, 1, 2, 253, 255], dtype=np.uint8), size=(31, 50))
    tiles[:5, :10] = 253
    tiles[-6:, 5:20] = 255
    tiles[:, 49] = 253
    want = scalar_stack(tiles, 2, spec.cat_of_byte, 77)
    same(stack_tiles(tiles, spec), want, 'few values')
    assert want['last'][49] == 77 and want['last_index'][49] == NONE == 65535 and want['share'][49] == NO_SHARE == 255
    # the shape of a tile is kept
    shaped = stack_tiles(tiles.reshape(31, 5, 10), spec)
    assert shaped['count'].shape == (2, 5, 10) and shaped['last'].shape == (5, 10)
    assert np.array_equal(shaped['share'].reshape(-1), want['share'])


def run_host(tiles, n_elems, stride, spec, stack_off=0, out_off=0, want=KEYS, n_tiles=None):
    """dswx_stack_host on a buffer [n_tiles][stride] whose first n_elems bytes per tile are `tiles`, placed `stack_off`
    bytes into an aligned allocation; the outputs `out_off` bytes into theirs, every output byte a sentinel beforehand.
    Returns (rc, outputs, raw output buffers)."""
    lib = _capi.load_library()
    T = len(tiles) if n_tiles is None else n_tiles
    raw = np.zeros(max(T * stride, 1) + 64, dtype=np.uint8)
    base = (-raw.ctypes.data) % 16 + stack_off
    bufs, out, res = {}, _capi.StackOut(), {}
    for k in KEYS:
        eb = 2 if k in ('count', 'last_index') else 1
        planes = spec.n_cats if k == 'count' else 1
        b = np.full(planes * n_elems * eb + 64, SENT8, dtype=np.uint8)
        start = (-b.ctypes.data) % 16 + out_off
        bufs[k] = (b, start, eb, planes)
        if k not in want:
            continue
        if k == 'count':
            for c in range(planes):
                out.count[c] = b.ctypes.data + start + c * n_elems * eb
        else:
            setattr(out, k, b.ctypes.data + start)
    return lib, raw, base, bufs, out


def host_planes(bufs, n_elems, want=KEYS):
    res = {}
    for k in want:
        b, start, eb, planes = bufs[k]
        a = b[start:start + planes * n_elems * eb].copy().view(np.uint16 if eb == 2 else np.uint8)
        res[k] = a.reshape(planes, n_elems) if k == 'count' else a
    return res


def untouched_outside(bufs, n_elems, want=KEYS):
    for k, (b, start, eb, planes) in bufs.items():
        used = planes * n_elems * eb if k in want else 0
        assert np.all(b[:start] == SENT8) and np.all(b[start + used:] == SENT8), k
        if k not in want:
            assert np.all(b == SENT8), k


@pytest.mark.parametrize('n_cats', [1, 2, 3, 4])
def test_host_entry_over_tile_counts_sizes_strides_and_addresses(n_cats):
    """n_tiles in {0, 1, 2, 255, 256, 257} x n_elems in {0, 1, 15, 16, 17}; every byte value in the stack; the stride equal to
    the tile and above it, the padding full of a byte that IS an observation of category 0; the stack and the outputs at
    even and odd addresses."""
    rng = np.random.default_rng(9200 + n_cats)
    for T in (0, 1, 2, 255, 256, 257):
        for n in (0, 1, 15, 16, 17):
            spec = random_spec(rng, n_cats)
            pad = 0xA5
            spec.cat_of_byte[pad] = 0                                                  # the padding would be counted
            tiles = rng.integers(0, 256, size=(T, n), dtype=np.uint8)
            if T * n >= 256:
                tiles.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)               # every byte value
            want = stack_tiles(tiles, spec)
            for stride, stack_off, out_off in ((n, 0, 0), (n + 3, 1, 1), (n + 16, 0, 3), (n, 7, 2)):
                lib, raw, base, bufs, out = run_host(tiles, n, stride, spec, stack_off, out_off)
                raw[:] = pad
                for t in range(T):
                    raw[base + t * stride:base + t * stride + n] = tiles[t]
                rc = lib.dswx_stack_host(raw.ctypes.data + base, ctypes.byref(_capi.StackSpec.of(spec)), T, n,
                                         0 if stride == n else stride, ctypes.byref(out))
                assert rc == 0, lib.dswx_last_error()
                same(host_planes(bufs, n), want, (n_cats, T, n, stride, stack_off, out_off))
                untouched_outside(bufs, n)
    same(_capi.stack_host(tiles, spec), want, 'the Python wrapper')


def test_tables_in_which_every_byte_is_and_no_byte_is_an_observation():
    rng = np.random.default_rng(9300)
    tiles = rng.integers(0, 256, size=(6, 300), dtype=np.uint8)
    tiles[2] = np.arange(300) % 256
    for n_cats in range(1, MAX_CATS + 1):
        every = Spec(n_cats, np.arange(256) % n_cats, 3)
        got = _capi.stack_host(tiles, every)
        same(got, stack_tiles(tiles, every), ('every', n_cats))
        assert np.all(got['count'].sum(axis=0) == 6) and np.all(got['last_index'] == 5) and np.array_equal(got['last'], tiles[5])
        none = Spec(n_cats, np.full(256, n_cats), 3)
        got = _capi.stack_host(tiles, none)
        same(got, stack_tiles(tiles, none), ('none', n_cats))
        assert not got['count'].any() and np.all(got['last'] == 3) and np.all(got['last_index'] == NONE) and np.all(got['share'] == NO_SHARE)
        top = Spec(n_cats, np.full(256, 255), 0)                                           # 255 is never a category
        assert not _capi.stack_host(tiles, top)['count'].any()


def test_subsets_of_outputs_on_the_host():
    rng = np.random.default_rng(9400)
    spec = random_spec(rng, 3)
    tiles = rng.integers(0, 256, size=(5, 37), dtype=np.uint8)
    want = stack_tiles(tiles, spec)
    for k in KEYS:
        lib, raw, base, bufs, out = run_host(tiles, 37, 37, spec, want=(k,))
        raw[base:base + tiles.size] = tiles.reshape(-1)
        assert lib.dswx_stack_host(raw.ctypes.data + base, ctypes.byref(_capi.StackSpec.of(spec)), 5, 37, 0, ctypes.byref(out)) == 0
        same(host_planes(bufs, 37, (k,)), {k: want[k]}, k)
        untouched_outside(bufs, 37, (k,))
        same(_capi.stack_host(tiles, spec, want=(k,)), {k: want[k]}, k)


def test_65535_tiles_do_not_carry_between_the_packed_counts_and_65536_are_refused():
    """65535 tiles x 16 pixels, pixels alternating between "always category 0" and "always category 1": counts of 65535 beside
    counts of 0, last_index 65534, share in {0, 100}."""
    T = MAX_TILES
    assert T == 65535
    spec = Spec(2, [1, 0] + [255] * 254, 9)
    tiles = np.zeros((T, 16), dtype=np.uint8)
    tiles[:, 1::2] = 1
    got = _capi.stack_host(tiles, spec)
    same(got, stack_tiles(tiles, spec), '65535 tiles')
    assert np.all(got['count'][1, 0::2] == 65535) and np.all(got['count'][0, 0::2] == 0)
    assert np.all(got['count'][0, 1::2] == 65535) and np.all(got['count'][1, 1::2] == 0)
    assert np.all(got['last_index'] == 65534) and np.array_equal(got['last'], tiles[0])
    assert np.all(got['share'][0::2] == 0) and np.all(got['share'][1::2] == 100)
    # all four fields at once: category k in pixel k, so every field reaches 65535 next to three zeros
    spec4 = Spec(4, [0, 1, 2, 3] + [255] * 252, 9)
    tiles4 = np.tile(np.arange(16, dtype=np.uint8) % 4, (T, 1))
    got = _capi.stack_host(tiles4, spec4)
    same(got, stack_tiles(tiles4, spec4), '65535 tiles, 4 categories')
    for k in range(4):
        assert np.all(got['count'][k, k::4] == 65535) and got['count'][k].sum() == 4 * 65535
    # one more tile
    lib = _capi.load_library()
    big = np.zeros((T + 1, 1), dtype=np.uint8)
    with pytest.raises(_capi.DswxError, match='65535') as e:
        _capi.stack_host(big, spec)
    assert e.value.code == _capi.ERR_ARG and b'n_tiles' in lib.dswx_last_error()
    with pytest.raises(ValueError):
        stack_tiles(big, spec)


def test_refusals_that_need_no_device():
    lib = _capi.load_library()
    vp = ctypes.c_void_p
    good = Spec(2, [1, 0] + [255] * 254, 255)
    n = 8
    tiles = np.zeros((3, n), dtype=np.uint8)
    planes = {k: np.full(2 * n if k == 'count' else n, SENT16 if k in ('count', 'last_index') else SENT8,
                         dtype=np.uint16 if k in ('count', 'last_index') else np.uint8) for k in KEYS}

    def outs(**kw):
        o = _capi.StackOut.of(count=[planes['count'].ctypes.data, planes['count'].ctypes.data + 2 * n],
                              last=planes['last'].ctypes.data, last_index=planes['last_index'].ctypes.data,
                              share=planes['share'].ctypes.data)
        for k, v in kw.items():
            if k.startswith('count'):
                o.count[int(k[5:])] = v
            else:
                setattr(o, k, v)
        return o

    def spec_c(n_cats=2, fill=255):
        s = _capi.StackSpec.of(good)
        s.n_cats, s.fill = n_cats, fill
        return s

    def host(stack=tiles.ctypes.data, spec=None, n_tiles=3, n_elems=n, stride=0, out=None, null_spec=False, null_out=False):
        spec = spec_c() if spec is None else spec
        out = outs() if out is None else out
        return lib.dswx_stack_host(stack, None if null_spec else ctypes.byref(spec), n_tiles, n_elems, stride,
                                   None if null_out else ctypes.byref(out))

    def dev(stack=0x10000, spec=None, n_tiles=3, n_elems=n, stride=0, out=None, null_spec=False, null_out=False, ctx=None):
        spec = spec_c() if spec is None else spec
        out = outs() if out is None else out                   # host addresses, never dereferenced: every call fails first
        return lib.dswx_stack_device(ctx, vp(stack) if stack else None, None if null_spec else ctypes.byref(spec), n_tiles,
                                     n_elems, stride, None if null_out else ctypes.byref(out), None)

    def refused(rc, code, text):
        assert rc == code and text in lib.dswx_last_error(), (rc, lib.dswx_last_error())

    for call in (host, dev):
        refused(call(null_spec=True), _capi.ERR_ARG, b'spec is NULL')
        refused(call(null_out=True), _capi.ERR_ARG, b'out is NULL')
        for n_cats in (-1, 0, 5, 100):
            refused(call(spec=spec_c(n_cats=n_cats)), _capi.ERR_ARG, b'n_cats')
        for fill in (-1, 256, 1 << 20):
            refused(call(spec=spec_c(fill=fill)), _capi.ERR_ARG, b'fill')
        for kw in ({'n_tiles': -1}, {'n_elems': -1}, {'stride': -5}):
            refused(call(**kw), _capi.ERR_ARG, b'negative')
        refused(call(stride=n - 1), _capi.ERR_ARG, b'stride')
        for T in (65536, 1 << 20, 1 << 40):
            refused(call(n_tiles=T), _capi.ERR_ARG, b'n_tiles')
            assert b'65535' in lib.dswx_last_error()
        refused(call(n_elems=1 << 50, n_tiles=1), _capi.ERR_ARG, b'too large')
        refused(call(n_elems=1 << 40, n_tiles=65535), _capi.ERR_ARG, b'too large')
        refused(call(stack=0), _capi.ERR_ARG, b'stack is NULL')
        for k in (2, 3):                                       # n_cats is 2
            refused(call(out=outs(**{f'count{k}': planes['count'].ctypes.data})), _capi.ERR_ARG, f'count[{k}]'.encode())
        refused(call(out=_capi.StackOut()), _capi.ERR_ARG, b'every output is NULL')
    # the device entry: alignment of the uint16 outputs; then, with everything in order, the context
    for k, name in ((0, b'count[0]'), (1, b'count[1]')):
        refused(dev(out=outs(**{f'count{k}': planes['count'].ctypes.data + 1})), _capi.ERR_ALIGN, name)
    refused(dev(out=outs(last_index=planes['last_index'].ctypes.data + 1)), _capi.ERR_ALIGN, b'last_index')
    refused(dev(out=outs(last=planes['last'].ctypes.data + 1, share=planes['share'].ctypes.data + 3)), _capi.ERR_ARG, b'ctx')
    refused(dev(stack=0x10001), _capi.ERR_ARG, b'ctx')                                   # the stack takes any address
    refused(dev(), _capi.ERR_ARG, b'ctx')
    refused(dev(stride=n), _capi.ERR_ARG, b'ctx')
    refused(dev(stride=n + 1, n_tiles=65535), _capi.ERR_ARG, b'ctx')
    refused(dev(stack=0, n_tiles=0), _capi.ERR_ARG, b'ctx')                              # nothing to read: no stack needed
    refused(dev(stack=0, n_elems=0), _capi.ERR_ARG, b'ctx')
    refused(dev(out=outs(count0=None, count1=None, last=None, last_index=None)), _capi.ERR_ARG, b'ctx')   # share alone
    refused(lib.dswx_batch_stack(None, 14, ctypes.byref(spec_c()), 0, 1, ctypes.byref(outs()), None), _capi.ERR_ARG, b'batch is NULL')
    # a refused call wrote nothing
    for k in KEYS:
        assert np.all(planes[k] == (SENT16 if k in ('count', 'last_index') else SENT8)), k
    # and the same arguments, accepted: legal corners of the host entry
    assert host() == 0 and np.all(planes['share'] == 0) and np.all(planes['count'][n:] == 3)
    assert host(stack=None, n_tiles=0) == 0 and np.all(planes['share'] == NO_SHARE) and np.all(planes['last_index'] == NONE)
    planes['last'][:] = SENT8
    assert host(stack=None, n_elems=0) == 0 and np.all(planes['last'] == SENT8)          # n_elems == 0 writes nothing
    # the Python side refuses what the library would
    for bad in (lambda: Spec(0, np.zeros(256)), lambda: Spec(5, np.zeros(256)), lambda: Spec(2, np.zeros(255)),
                lambda: Spec(2, np.zeros(256), fill=256), lambda: stack_tiles(np.zeros((2, 2), dtype=np.int16), good),
                lambda: _capi.stack_host(np.zeros((2, 2), dtype=np.uint16), good),
                lambda: _capi.stack_host(tiles, good, want=('median',)), lambda: _capi.stack_host(tiles, good, want=())):
        with pytest.raises(ValueError):
            bad()


def test_stack_and_mosaic_host_entries_under_asan_and_ubsan_in_a_program_of_their_own():
    """tests/native/stack_host_san.cpp with proteus_amd/csrc/dswx_stack.hip and dswx_mosaic.hip compiled into it, host code under
    ASan + UBSan: 0, 1 and 9 tiles of 0, 15, 16 and 33 elements, and three tiles of 3 x 5 and 1 x 1 hanging over every side of a
    7 x 20 canvas (INT32_MIN and INT32_MAX among the placements), on heap blocks of exactly the bytes the entries may touch, at
    odd addresses.  A child process; nothing is loaded into this interpreter."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('needs hipcc')
    out_dir = os.path.join(ROOT, 'tests', 'native', '_build')
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, 'stack_host_san')
    csrc = os.path.join(ROOT, 'proteus_amd', 'csrc')
    cmd = [hipcc, '--offload-arch=gfx950', '-std=c++17', '-g', '-O1', '-ffp-contract=off', '-Wall', '-Wno-unused-function',
           '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
           '-I', os.path.join(ROOT, 'include'), '-I', csrc, os.path.join(ROOT, 'tests', 'native', 'stack_host_san.cpp'),
           os.path.join(csrc, 'dswx_stack.hip'), os.path.join(csrc, 'dswx_mosaic.hip'), '-o', exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if res.returncode != 0 and 'libclang_rt.asan' in res.stderr:     # (only the runtime: an error in the sources must fail)
        pytest.skip(f'sanitizer runtime missing: {res.stderr[-300:]}')
    assert res.returncode == 0, res.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-4000:])
    assert 'ERROR: AddressSanitizer' not in res.stderr and 'runtime error' not in res.stderr and 'LeakSanitizer' not in res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out['failures'] == 0 and out['cases'] == 143


def test_header_says_has_stack_and_abi_7():
    text = open(os.path.join(ROOT, 'include', 'dswx_hip.h')).read()
    assert '#define DSWX_HAS_STACK 1' in text
    assert '#define DSWX_ABI_VERSION 7' in text and _capi.DSWX_ABI_VERSION == 7 and _capi.load_library().dswx_abi_version() == 7
    for name, v in (('DSWX_STACK_MAX_CATS', 4), ('DSWX_STACK_MAX_TILES', 65535), ('DSWX_STACK_NONE', 65535), ('DSWX_STACK_NO_SHARE', 255)):
        assert f'#define {name} {v}' in text
    assert (_capi.HAS_STACK, _capi.STACK_MAX_CATS, _capi.STACK_MAX_TILES, _capi.STACK_NONE, _capi.STACK_NO_SHARE) == (1, 4, 65535, 65535, 255)
    assert (MAX_CATS, MAX_TILES, NONE, NO_SHARE) == (4, 65535, 65535, 255)
    assert text.index('---- crosstab:') < text.index('---- stack:') < text.index('---- device plumbing')
    for name in ('dswx_stack_device', 'dswx_batch_stack', 'dswx_stack_host'):
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(_capi.load_library(), name)
    assert 'MUST NOT OVERLAP' in text and 'NOT CHECKED' in text


def test_struct_mirrors_match_offsetof_as_gcc_sees_the_header(tmp_path):
    assert ctypes.sizeof(_capi.StackSpec) == 264
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    mirrors = {'dswx_stack_spec_t': _capi.StackSpec, 'dswx_stack_out_t': _capi.StackOut}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dswx_hip.h"', 'int main(void) {']
    for st, cls in mirrors.items():
        for n, _ in cls._fields_:
            lines.append(f'  printf("{st}.{n} %zu\\n", offsetof({st}, {n}));')
        lines.append(f'  printf("{st}.sizeof %zu\\n", sizeof({st}));')
    lines += ['  return 0;', '}']
    src = tmp_path / 'off.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'off'
    subprocess.run(['gcc', '-std=c11', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got['dswx_stack_spec_t.sizeof']) == 264
    for st, cls in mirrors.items():
        assert int(got[f'{st}.sizeof']) == ctypes.sizeof(cls), st
        for n, _ in cls._fields_:
            assert int(got[f'{st}.{n}']) == getattr(cls, n).offset, (st, n)
    o = _capi.StackOut.of(count=[16, 32], last=48, last_index=None, share=64)
    assert list(o.count) == [16, 32, None, None] and (o.last, o.last_index, o.share) == (48, None, 64)
    s = _capi.StackSpec.of(Spec(3, np.arange(256) % 7, 9))
    assert (s.n_cats, s.fill) == (3, 9) and list(s.cat_of_byte) == [b % 7 for b in range(256)]


def test_wtr_specs_written_out_by_hand():
    """Category 0 = water, 1 = clear and not water, 255 = not an observation.  Bytes 0 .. 5, then 6 .. 251 and 252 .. 255."""
    by_hand = {(True, True): [1, 0, 0, 255, 255, 255], (True, False): [1, 0, 1, 255, 255, 255],
               (False, True): [1, 0, 0, 0, 0, 255], (False, False): [1, 0, 0, 1, 1, 255]}
    for (collapsed, partial), head in by_hand.items():
        s = wtr_spec(collapsed=collapsed, partial_is_water=partial)
        assert (s.n_cats, s.fill) == (2, 255)
        assert s.cat_of_byte.dtype == np.uint8 and s.cat_of_byte.tolist() == head + [255] * 250, (collapsed, partial)
    assert wtr_spec().cat_of_byte.tolist() == wtr_spec(True, True, 255).cat_of_byte.tolist()
    assert wtr_spec(fill=0).fill == 0
    # one pixel's history in the saved form: not water, cloud, open water, partial, snow, fill
    history = np.array([0, 253, 1, 2, 252, 255], dtype=np.uint8).reshape(6, 1)
    got = stack_tiles(history, wtr_spec())
    assert (got['count'][0, 0], got['count'][1, 0], got['last'][0], got['last_index'][0], got['share'][0]) == (2, 1, 2, 3, 66)
    got = stack_tiles(history, wtr_spec(partial_is_water=False))
    assert (got['count'][0, 0], got['count'][1, 0], got['last'][0], got['last_index'][0], got['share'][0]) == (1, 2, 2, 3, 33)


def test_stack_example_compiles_against_the_header(tmp_path):
    """examples/batch_stack.c is C (gcc -std=c11 -Wall -Wextra -Werror) and links against the library; without a device the
    program stops at dswx_ctx_create."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_stack')
    lib_dir = os.path.dirname(_capi.library_path())
    _capi.load_library()
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_stack.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}',
                    '-o', exe], check=True)
    if _capi.device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and 'dswx_ctx_create' in r.stderr and 'no CPU fallback' in r.stderr
