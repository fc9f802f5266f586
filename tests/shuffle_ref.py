"""CPU restatement of the device point shuffle (csrc/shuffle.hip), written from the specification alone — NumPy uint64
arithmetic masked to 32 bits, nothing imported from the package.

  vn_permute_points: out[i] = points[index[i]]; an index outside [0, n) gives a NaN point (four quiet NaNs, 0x7FC00000)
  vn_shuffle_points: out[i] = points[p(i)], p a keyed bijection of [0, n): a six-round Feistel network over 2h bits,
                     walked until it lands inside the range (cycle walking)

    k = max(2, bit_length(n - 1));   h = (k + 1) // 2;   mask = 2^h - 1
    fmix32(x): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16        (uint32, wrapping)
    F(x):  L = x >> h;  R = x & mask;  for r in 0..5:  (L, R) = (R, L ^ (fmix32(R ^ keys[r]) & mask));  (L << h) | R
    p(i):  x = F(i);  while x >= n: x = F(x)"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
NAN_WORD = np.int32(0x7FC00000)


def half_bits(n):
    k = max(2, int(n - 1).bit_length())
    return (k + 1) // 2


def fmix32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & M32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & M32
    x ^= x >> np.uint64(16)
    return x


def feistel(x, keys, h):
    h = np.uint64(h)
    mask = (np.uint64(1) << h) - np.uint64(1)
    x = np.asarray(x, dtype=np.uint64)
    L, R = x >> h, x & mask
    for r in range(6):
        L, R = R, L ^ (fmix32(R ^ (np.uint64(int(keys[r])) & M32)) & mask)
    return (L << h) | R


def permutation(n, keys, steps=None):
    """p (n,) int64.  steps: an optional list that receives the longest walk of any element"""
    n = int(n)
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    h = half_bits(n)
    x = feistel(np.arange(n, dtype=np.uint64), keys, h)
    walked = 1
    while True:
        out = np.nonzero(x >= np.uint64(n))[0]
        if out.size == 0:
            break
        x[out] = feistel(x[out], keys, h)
        walked += 1
    if steps is not None:
        steps.append(walked)
    return x.astype(np.int64)


def shuffle_points(cloud, keys):
    """(n,4) float32 -> rows p(i), moved as bits"""
    cloud = np.ascontiguousarray(cloud, dtype=np.float32)
    return cloud.view(np.int32)[permutation(cloud.shape[0], keys)].view(np.float32)


def permute_points(cloud, index):
    """(n,4) float32, index (n,) any integer type -> rows index[i] moved as bits; an index outside [0, n) -> a NaN point"""
    cloud = np.ascontiguousarray(cloud, dtype=np.float32)
    n = cloud.shape[0]
    index = np.asarray(index, dtype=np.int64)
    ok = (index >= 0) & (index < n)
    out = np.full((index.shape[0], 4), NAN_WORD, dtype=np.int32)
    out[ok] = cloud.view(np.int32)[index[ok]]
    return out.view(np.float32)
