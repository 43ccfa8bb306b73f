"""numpy twin of the device's normal generator (fvgp_amd/csrc/sample.hip, include/fvgp_hip.h "sampling").

z(seed, stream, i, j) is a pure function: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
SC 2011; the Random123 constants) on the counter (i, j, lo32(stream), hi32(stream)) with the key (lo32(seed), hi32(seed)); with its
output words w0..w3

    u1 = (((w0 | w1 << 32) >> 11) + 0.5) 2^-53,   u2 the same from w2, w3,   z = sqrt(-2 ln u1) cos(2 pi u2)

i is the point (row) index, j the sample index.  Everything is vectorised over i and j (they broadcast against each other).
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or integers) of 32-bit words that broadcast against each other, key: two 32-bit integers;
    returns the four output words as uint64 arrays holding 32-bit values"""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & MASK for c in counter])
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                     # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def uniforms(seed, stream, i, j):
    """(u1, u2) in (0, 1]: 53 bits each, centred in their cell"""
    seed, stream = int(seed), int(stream)
    w0, w1, w2, w3 = philox4x32_10((i, j, stream & 0xFFFFFFFF, (stream >> 32) & 0xFFFFFFFF), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    s11 = np.uint64(11)
    u1 = (((w0 | (w1 << S32)) >> s11).astype(np.float64) + 0.5) * 2.0 ** -53
    u2 = (((w2 | (w3 << S32)) >> s11).astype(np.float64) + 0.5) * 2.0 ** -53
    return u1, u2


def normal(seed, stream, i, j):
    """z(seed, stream, i, j) as float64; i and j integers or integer arrays below 2^32 that broadcast against each other"""
    u1, u2 = uniforms(seed, stream, i, j)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def normal_block(seed, stream, row0, col0, rows, cols):
    """the rows x cols block Z[r][c] = z(seed, stream, row0 + r, col0 + c)"""
    return normal(seed, stream, (row0 + np.arange(rows, dtype=np.uint64))[:, None], (col0 + np.arange(cols, dtype=np.uint64))[None, :])
