"""Host restatement of the device noise generator (include/e2eft.h, "Latent noise on the device"), written from that definition and vectorised
with numpy.  TEST INFRASTRUCTURE ONLY.

  philox4x32_10(counter [...,4] uint32, key [...,2] uint32) -> [...,4] uint32
  uniforms / normals(seed, draw, slot, n)                    -> float64 [n], element e = logical NCHW linear index
  pyramid(seed, draw, shape, sizes, discount)                -> float64 torch tensor [B,C,H,W]: base + sum discount^i * bilinear_up(level_i), / unbiased std
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k0 = np.asarray(key)[..., 0].astype(np.uint64)
    k1 = np.asarray(key)[..., 1].astype(np.uint64)
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(W0)) & np.uint64(MASK)
            k1 = (k1 + np.uint64(W1)) & np.uint64(MASK)
        p0 = np.uint64(M0) * c[0]          # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & np.uint64(MASK), (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & np.uint64(MASK)]
    return np.stack(c, axis=-1).astype(np.uint32)


def words(seed, draw, slot, n):
    """the uint32 word of elements 0..n-1"""
    e = np.arange(n, dtype=np.uint64)
    q = e >> np.uint64(2)
    ctr = np.stack([q & np.uint64(MASK), q >> np.uint64(32), np.full(n, slot, np.uint64), np.full(n, draw, np.uint64)], axis=-1)
    key = np.array([seed & MASK, (seed >> 32) & MASK], dtype=np.uint64)
    out = philox4x32_10(ctr, np.broadcast_to(key, (n, 2)))
    return out, e


def uniforms(seed, draw, slot, n):
    """[n, 4] float64: the four uniforms of every element's counter (row e holds the words of quad e >> 2)"""
    out, _ = words(seed, draw, slot, n)
    return ((out >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def normals(seed, draw, slot, n):
    u = uniforms(seed, draw, slot, n)
    e = np.arange(n)
    pair = (e & 2)                       # 0: words (0,1); 2: words (2,3)
    ua = u[e, pair]
    ub = u[e, pair + 1]
    r = np.sqrt(-2.0 * np.log(ua))
    th = 2.0 * np.pi * ub
    return np.where(e & 1, r * np.sin(th), r * np.cos(th))


def normal_grid(seed, draw, slot, shape):
    import torch
    n = int(np.prod(shape))
    return torch.from_numpy(normals(seed, draw, slot, n).reshape(shape))


def pyramid(seed, draw, shape, sizes, discount=0.9):
    """float64 [B,C,H,W] of e2eft_pyramid_noise for explicit level sizes [(rows, cols), ...]"""
    import torch
    B, C, H, W = shape
    total = normal_grid(seed, draw, 0, shape)
    for i, (r, c) in enumerate(sizes):
        lvl = normal_grid(seed, draw, 1 + i, (B, C, r, c))
        total = total + torch.nn.functional.interpolate(lvl, size=(H, W), mode="bilinear", align_corners=False) * discount ** i
    return total / total.std()
