"""The device draw stream (pvcnn_amd/csrc/philox.h, include/pvcnn_hip.h "Device draws") restated in numpy integers.

A Philox4x32-10 stream: the key is the two halves of seed[0], counter word 2 the low 32 bits of seed[1], counter word 3 names the use
(COUNTERS), counter words 0 and 1 are the use's own (the point and the sample, mostly).  Everything here is exact: integer arithmetic,
and conversions that are one exact product of an integer below 2^32 (2^24 in fp32) with a power of two."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
# counter word 3: who draws with it
COUNTERS = {'pick': 0, 'jitter': 1, 'flip_shift': 2, 'box': 3, 'aug_cloud': 16, 'aug_jitter': 20, 'aug_keep': 21}
AUG_CLOUD_WORDS = 4                  # aug_cloud .. aug_cloud + 3


def philox4x32_10(counter, key):
    """counter: four integers or integer arrays (broadcast), key: two integers -> uint32 array (..., 4)."""
    c = [np.asarray(x, dtype=np.uint64) for x in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    mask = np.uint64(MASK)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def draw_stream(seed):
    """seed: two int64 words -> ((key0, key1), stream)."""
    s0, s1 = int(seed[0]) & 0xFFFFFFFFFFFFFFFF, int(seed[1]) & 0xFFFFFFFFFFFFFFFF
    return (s0 & MASK, s0 >> 32), s1 & MASK


def draw_words(seed, a, b, ctr):
    key, stream = draw_stream(seed)
    return philox4x32_10((a, b, stream, ctr), key)


def draw_index(seed, p, b, n):
    """The uniform pick of [0, n): the high half of word x times n."""
    return ((draw_words(seed, p, b, COUNTERS['pick'])[..., 0].astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def sort_words(seed, b, n):
    """The sort words of the selection without replacement: key << 32 | i for i in [0, n)."""
    i = np.arange(n, dtype=np.uint64)
    return (draw_words(seed, i, b, COUNTERS['pick'])[..., 0].astype(np.uint64) << np.uint64(32)) | i


def select_distinct(seed, b, n, count):
    """`count` distinct of n in random order: the low halves of the `count` smallest sort words."""
    return (np.sort(sort_words(seed, b, n))[:count] & np.uint64(MASK)).astype(np.int64)


def mask_select(seed, b, k, m):
    """Positions into a cloud's k foreground candidates (k >= 1) that mask_select's device mode picks for its m outputs."""
    order = select_distinct(seed, b, k, k)
    if k >= m:
        return order[:m]
    rep = m // k
    entry = np.concatenate([np.repeat(np.arange(k), rep), order[:m - rep * k]])
    s = np.arange(m, dtype=np.uint64)
    keys = (draw_words(seed, s, b, COUNTERS['jitter'])[..., 0].astype(np.uint64) << np.uint64(32)) | s
    return entry[np.argsort(keys)]


def flip_bit(seed, b):
    return (draw_words(seed, 0, b, COUNTERS['flip_shift'])[..., 0] >> np.uint32(31)).astype(np.int64)


def unit_f32(r):
    """fp32 in [0, 1): (r >> 8) * 2^-24."""
    return (np.asarray(r, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def open_f64(r):
    """fp64 in (0, 1): (r + 0.5) * 2^-32."""
    return (np.asarray(r, dtype=np.uint32).astype(np.float64) + 0.5) * 2.0 ** -32


def unit_f64(r):
    """fp64 in [0, 1): r * 2^-32."""
    return np.asarray(r, dtype=np.uint32).astype(np.float64) * 2.0 ** -32
