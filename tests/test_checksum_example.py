"""examples/batch_checksums.c: the checksum entries of ABI v7 from plain C.  Built with gcc against include/dswx_hip.h
everywhere; run where there is a GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from proteus_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_checksums')
    lib_dir = os.path.dirname(_capi.library_path())
    _capi.load_library()                      # builds the library when missing or stale
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_checksums.c'), '-L', lib_dir, '-ldswx_hip',
                    f'-Wl,-rpath,{lib_dir}', '-o', exe], check=True)
    return exe


def test_checksum_example_compiles_against_the_header(tmp_path):
    """The header's new declarations are C (gcc -std=c11 -Wall -Wextra -Werror) and the library links from C; without a
    device the program stops at dswx_ctx_create."""
    exe = _build(tmp_path)
    if _capi.device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and 'dswx_ctx_create' in r.stderr and 'no CPU fallback' in r.stderr


@pytest.mark.gpu
def test_checksum_example_runs_and_agrees_with_the_oracle(tmp_path):
    """The program's own comparison (exit status 0), and the checksums it prints against the numpy statement applied to
    the oracle's layers of the same synthetic tiles."""
    from oracle import c_oracle
    from proteus_amd.checksum import checksum
    from proteus_amd.synth import synth_tile
    exe = _build(tmp_path)
    n_tiles, size = 3, 301
    r = subprocess.run([exe, str(n_tiles), str(size)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert 'diag: device and host checksums agree' in r.stdout
    got = {(m.group(1), int(m.group(2))): int(m.group(3), 16)
           for m in re.finditer(r'^checksum (\w+) (\d+) ([0-9a-f]{16})$', r.stdout, re.M)}
    layers = ('diag', 'wtr1', 'wtr2', 'wtr', 'bwtr', 'conf', 'cloud')
    assert len(got) == n_tiles * len(layers)
    p = _capi.default_params()
    for t in range(n_tiles):
        s = synth_tile(t, size, size, seed=20251010)
        exp = c_oracle.classify(p, s['bands'], s['fmask'], layers=layers)
        for name in layers:
            assert got[(name, t)] == checksum(np.ascontiguousarray(exp[name])), (name, t)
