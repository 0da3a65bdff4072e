"""NumPy statement of the texture noise rule (wct_tf_amd/csrc/noise_rule.h; include/wct_hip.h, wct_texture_noise): integers only,
so the GPU, a host program and this file agree bit for bit.  All arithmetic is mod 2^32.

    fmix(h):  h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16        (murmur3's finaliser)
    key = fmix(seed ^ (sample * 0x9E3779B9))
    n   = (y * W + x) * 3 + ch                                  the byte's index in its [H][W][3] image
    raw = fmix(fmix(n ^ key) + key) >> 24                       one uniform byte
    smooth: out = (sum_dy sum_dx w[dy] w[dx] raw(sym(y + dy, H), sym(x + dx, W), ch) + 32768) >> 16,  w = 27 202 27,
            sym(-1, n) = 0, sym(n, n) = n - 1                   (scipy's mode='reflect' = NumPy's 'symmetric')

noise / noise_batch are vectorised; noise_loop is the same rule byte by byte in Python integers."""
import numpy as np

M32 = 0xFFFFFFFF
GOLDEN = 0x9E3779B9
TAPS = (27, 202, 27)


def fmix(h):
    """murmur3's finaliser on a uint32 array (wraps mod 2^32)"""
    h = np.asarray(h, np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def key(seed, sample):
    return fmix(np.uint32(((int(sample) & M32) * GOLDEN & M32) ^ (int(seed) & M32)))


def raw(h, w, seed, sample):
    """the raw bytes of one image, uint8 [h][w][3]"""
    k = key(seed, sample)
    n = np.arange(h * w * 3, dtype=np.uint32)
    return (fmix(fmix(n ^ k) + k) >> np.uint32(24)).astype(np.uint8).reshape(h, w, 3)


def smooth(img):
    """the 3-tap 27 202 27 filter along y and x of any uint8 [H][W][C] image, edges symmetric, rounded to nearest"""
    a = np.asarray(img)
    assert a.dtype == np.uint8 and a.ndim == 3
    p = np.pad(a.astype(np.int64), ((1, 1), (1, 1), (0, 0)), mode='symmetric')
    h, w = a.shape[:2]
    acc = np.zeros(a.shape, np.int64)
    for dy in range(3):
        for dx in range(3):
            acc += TAPS[dy] * TAPS[dx] * p[dy:dy + h, dx:dx + w]
    return ((acc + 32768) >> 16).astype(np.uint8)


def noise(h, w, seed, sample=0, smooth_on=False):
    r = raw(h, w, seed, sample)
    return smooth(r) if smooth_on else r


def noise_batch(h, w, b, seed, first_sample=0, smooth_on=False):
    """uint8 [b][h][w][3]: image i is sample first_sample + i"""
    return np.stack([noise(h, w, seed, first_sample + i, smooth_on) for i in range(b)])


# ---- the same rule, one byte at a time, in Python integers ------------------------------------------------------------------
def _fmix_int(h):
    h ^= h >> 16
    h = h * 0x85EBCA6B & M32
    h ^= h >> 13
    h = h * 0xC2B2AE35 & M32
    return h ^ (h >> 16)


def _sym(i, n):
    return 0 if i < 0 else (n - 1 if i >= n else i)


def noise_loop(h, w, seed, sample=0, smooth_on=False):
    k = _fmix_int((seed & M32) ^ ((sample & M32) * GOLDEN & M32))

    def raw_at(y, x, ch):
        n = (y * w + x) * 3 + ch
        return _fmix_int((_fmix_int(n ^ k) + k) & M32) >> 24

    out = np.empty((h, w, 3), np.uint8)
    for y in range(h):
        for x in range(w):
            for ch in range(3):
                if not smooth_on:
                    out[y, x, ch] = raw_at(y, x, ch)
                    continue
                acc = 0
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        acc += TAPS[dy + 1] * TAPS[dx + 1] * raw_at(_sym(y + dy, h), _sym(x + dx, w), ch)
                out[y, x, ch] = (acc + 32768) >> 16
    return out
