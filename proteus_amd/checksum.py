"""The per-tile checksum of include/dswx_hip.h ("checksums", ABI v7) stated in numpy.

For the n b bytes of one tile in memory order, split into m = ceil(n b / 8) little-endian 64-bit words w_0 .. w_(m-1)
(the last one zero-padded):

    C = mix(n b) + sum_g mix(w_g + (g + 1) K)        (mod 2^64)

with K odd and mix the splitmix64 finaliser.  This module is an INDEPENDENT statement of that definition -- vectorised
uint64 arithmetic, which wraps silently -- and calls neither dswx_checksum_host nor the device: the tests pin the three to
each other, and a host that holds the array a resident tile should equal computes the expected value here.
"""
import numpy as np

K = np.uint64(0x9E3779B97F4A7C15)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)
_CHUNK_WORDS = 1 << 20          # words per step: bounds the temporaries to a few times 8 MiB


def _mix(x):
    """splitmix64 finaliser on a uint64 array, in place."""
    x ^= x >> np.uint64(30)
    x *= M1
    x ^= x >> np.uint64(27)
    x *= M2
    x ^= x >> np.uint64(31)
    return x


def checksum(data):
    """The checksum of one tile: `data` is bytes-like or an array (taken in C order, whatever its dtype and address)."""
    if isinstance(data, (bytes, bytearray, memoryview)):
        b = np.frombuffer(data, dtype=np.uint8)
    else:
        b = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    n = b.size
    total = _mix(np.array([n], dtype=np.uint64))[0]
    with np.errstate(over='ignore'):
        for g0 in range(0, (n + 7) // 8, _CHUNK_WORDS):
            piece = b[g0 * 8:(g0 + _CHUNK_WORDS) * 8]
            if piece.size % 8 or piece.ctypes.data % 8:
                padded = np.zeros(-(-piece.size // 8) * 8, dtype=np.uint8)      # the last word zero-padded; word 0 at element 0
                padded[:piece.size] = piece
                piece = padded
            w = piece.view('<u8').astype(np.uint64)                             # (a copy: mixed in place below)
            w += np.arange(g0 + 1, g0 + 1 + w.size, dtype=np.uint64) * K
            total += np.add.reduce(_mix(w), dtype=np.uint64)
    return int(total)


def checksum_tiles(array):
    """uint64 [n_tiles]: the checksum of every tile array[t] of an array [n_tiles, ...].  Tiles of up to _CHUNK_WORDS words
    are taken many at a time -- the words of a tile along axis 1, the same arithmetic as `checksum` -- so that a plane of
    tens of thousands of small tiles costs a few numpy calls and not a Python loop."""
    a = np.ascontiguousarray(array)
    n_tiles = len(a)
    nb = a[0].nbytes if n_tiles else 0
    m = (nb + 7) // 8
    if n_tiles == 0 or m == 0 or m > _CHUNK_WORDS:
        return np.array([checksum(a[t]) for t in range(n_tiles)], dtype=np.uint64)
    b = a.reshape(n_tiles, -1).view(np.uint8)
    out = np.full(n_tiles, _mix(np.array([nb], dtype=np.uint64))[0], dtype=np.uint64)
    keys = np.arange(1, m + 1, dtype=np.uint64) * K
    step = max(1, _CHUNK_WORDS // m)
    for t0 in range(0, n_tiles, step):
        piece = b[t0:t0 + step]
        padded = np.zeros((len(piece), m * 8), dtype=np.uint8)                  # the last word of every tile zero-padded
        padded[:, :nb] = piece
        w = padded.view('<u8').astype(np.uint64)
        w += keys
        out[t0:t0 + step] += np.add.reduce(_mix(w), axis=1, dtype=np.uint64)
    return out
