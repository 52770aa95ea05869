"""Philox4x32-10 in plain numpy, and the project's counter layouts on top of it.

The round function is Random123's (Salmon et al., SC'11): vectorised over
counters, with the 32 x 32 -> 64 bit products taken in uint64.  It is held to
the three Random123 known-answer vectors by tests/test_philox_cpu.py, and the
device streams (csrc/interaction.hip noise_uniform_k, csrc/gt_layer.hip
gt_lin_fwd_k) are held to it bit for bit by tests/test_gpu_rng.py.

Layouts (include/scgib.h at scgib_noise_uniform): key = the two halves of the
seed; off_lo / off_hi the two halves of the per-launch offset;
  gate of row r        = word 0 of counter (r, 16, off_lo, off_hi)
  feature quad c, row r = the four words of (r, c, off_lo, off_hi), c = 0..15
  dropout row r        = the four words of (r_lo, tag ^ r_hi, off_lo, off_hi)
and a word x becomes the uniform (x >> 8) * 2^-24.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57  # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85  # key bumps (golden ratio, sqrt(3) - 1)
GATE_WORD1 = 16                  # counter word 1 of the gate draw
FEAT_QUADS = 16                  # 64 channels = 16 blocks of four words
DROP_TAG = 0x47544C31            # counter word 1 of the dropout draws
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr [..., 4], key [..., 2] (broadcastable; any integers < 2^32) ->
    uint32 [..., 4]: ten rounds, the key bumped between rounds."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    shape = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(ctr[..., i], shape) for i in range(4))
    k0, k1 = (np.broadcast_to(key[..., i], shape) for i in range(2))
    for _ in range(10):
        p0 = np.uint64(M0) * c0  # < 2^64: both factors < 2^32
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = ((p1 >> _S32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK)
        k0 = (k0 + np.uint64(W0)) & _MASK
        k1 = (k1 + np.uint64(W1)) & _MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def u01(x):
    """uint32 -> float32 uniform in [0, 1): the top 24 bits, exact in fp32."""
    return (np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def _halves(v):
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v & 0xFFFFFFFF, v >> 32


def gate_counters(off, rows):
    """uint64 [n, 4]: the gate's counter of every row."""
    rows = np.asarray(rows, dtype=np.uint64)
    lo, hi = _halves(off)
    c = np.empty(rows.shape + (4,), np.uint64)
    c[..., 0], c[..., 1], c[..., 2], c[..., 3] = rows & _MASK, GATE_WORD1, lo, hi
    return c


def feat_counters(off, rows):
    """uint64 [n, 16, 4]: the counter of every (row, channel quad)."""
    rows = np.asarray(rows, dtype=np.uint64)
    lo, hi = _halves(off)
    c = np.empty(rows.shape + (FEAT_QUADS, 4), np.uint64)
    c[..., 0] = (rows & _MASK)[..., None]
    c[..., 1] = np.arange(FEAT_QUADS, dtype=np.uint64)
    c[..., 2], c[..., 3] = lo, hi
    return c


def dropout_counters(off, rows):
    """uint64 [n, 4]: the dropout counter of every row."""
    rows = np.asarray(rows, dtype=np.uint64)
    lo, hi = _halves(off)
    c = np.empty(rows.shape + (4,), np.uint64)
    c[..., 0], c[..., 1] = rows & _MASK, np.uint64(DROP_TAG) ^ (rows >> _S32)
    c[..., 2], c[..., 3] = lo, hi
    return c


def noise_gate(seed, off, rows):
    """float32 [n]: u_gate of the given rows."""
    return u01(philox4x32_10(gate_counters(off, rows), _halves(seed))[..., 0])


def noise_feat(seed, off, rows):
    """float32 [n, 64]: u_feat of the given rows (quad c -> channels 4c..4c+3)."""
    rows = np.asarray(rows)
    return u01(philox4x32_10(feat_counters(off, rows), _halves(seed))).reshape(rows.shape + (64,))


def dropout_keep(seed, off, rows):
    """bool [n, 128]: column c is kept iff bit c % 32 of word c / 32 is set,
    the block's words in x, y, z, w order."""
    rows = np.asarray(rows)
    words = philox4x32_10(dropout_counters(off, rows), _halves(seed))  # [n, 4]
    bits = (words[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.astype(bool).reshape(rows.shape + (128,))
