"""numpy restatement of the reference's Hypersim preprocessing (Marigold/script/dataset_preprocess/hypersim/preprocess_hypersim.py:83-138 over
hypersim_util.py:9-69) — what csrc/hypersimprep.hip computes, step by step, with the percentile as an explicit order statistic + numpy's lerp and the
two casts the reference leaves to the platform written out.  TEST INFRASTRUCTURE: the fixture tests/golden/hypersim_prep_golden.pt
holds the reference's own outputs; tests/test_hypersim_prep_cpu.py checks that this file reproduces them exactly."""
import numpy as np

FOCAL = 886.81                      # preprocess_hypersim.py:19
RECORD_FIELDS = ("invalid_ratio", "rgb_mean", "rgb_std", "rgb_min", "rgb_max", "depth_mean", "depth_std", "depth_min", "depth_max",
                 "zero_ids", "nan_brightness", "n_valid", "percentile", "scale")


def percentile90(x):
    """np.percentile(x, 90) of a 1-D float64 array, n >= 1: method "linear" = virtual index (n - 1) * 0.9, the order statistics on both sides, numpy's
    two-branch lerp.  Asserts that this IS np.percentile."""
    n = x.size
    if np.isnan(x).any():
        p = np.float64(np.nan)
    else:
        v = np.float64(n - 1) * np.float64(0.9)
        k = int(np.floor(v))
        g = v - np.float64(k)
        k2 = min(k + 1, n - 1)
        s = np.partition(x, sorted({k, k2}))
        a, b = s[k], s[k2]
        diff = b - a
        p = b - diff * (1 - g) if g >= 0.5 else a + diff * g
    want = np.percentile(x, 90)
    assert (np.isnan(p) and np.isnan(want)) or p == want, (p, want)
    return np.float64(p)


def tone_scale(color64, valid):
    """hypersim_util.py:19-44 -> (scale, percentile, nan flag)"""
    if np.count_nonzero(valid) == 0:
        return np.float64(1.0), np.float64(np.nan), False
    brightness = 0.3 * color64[:, :, 0] + 0.59 * color64[:, :, 1] + 0.11 * color64[:, :, 2]
    bv = brightness[valid]
    p = percentile90(bv)
    if p < 0.0001:
        return np.float64(0.0), p, bool(np.isnan(bv).any())
    with np.errstate(all="ignore"):
        return np.power(0.8, 1.0 / (1.0 / 2.2)) / p, p, bool(np.isnan(bv).any())


def tone_map(color64, scale):
    """hypersim_util.py:46-47 -> float64 [H,W,3] in [0,1] (NaN where scale * rgb is NaN)"""
    with np.errstate(all="ignore"):
        return np.clip(np.power(np.maximum(scale * color64, 0), 1.0 / 2.2), 0, 1)


def cast_u8(out255):
    """(x * 255).astype(np.uint8) for x in [0,1]; a NaN -> 0 (the platform decides in numpy; the kernel defines 0)"""
    with np.errstate(all="ignore"):
        return np.where(np.isnan(out255), 0.0, out255).astype(np.int64).astype(np.uint8)


def cast_u16(v):
    """float64 -> uint16 as the kernel defines it, which is what the reference's x86-64 host is observed to do: the low 16 bits of the truncated integer
    while it fits int32; NaN and anything beyond the int32 range -> 0"""
    with np.errstate(all="ignore"):
        ok = (v > -2147483649.0) & (v < 2147483648.0)
        t = np.where(ok, v, 0.0).astype(np.int64)
    return (t & 0xFFFF).astype(np.uint16)


def planar_depth_mm(distance64, valid, focal=FOCAL):
    """hypersim_util.py:52-69 + preprocess_hypersim.py:98-119 -> float64 millimetres before the cast"""
    H, W = distance64.shape
    x = (np.arange(W, dtype=np.float64) - 0.5 * W + 0.5).astype(np.float32)[None, :]
    y = (np.arange(H, dtype=np.float64) - 0.5 * H + 0.5).astype(np.float32)[:, None]
    z = np.float32(focal)
    norm = np.sqrt((x * x + y * y) + z * z)                 # float32 throughout (np.linalg.norm of a float32 array)
    assert norm.dtype == np.float32
    with np.errstate(all="ignore"):
        depth = distance64 / norm.astype(np.float64) * focal
        depth[~valid] = 0
        return depth * 1000.0


def preprocess(color, distance, ids, focal=FOCAL):
    """one frame: color [H,W,3], distance [H,W] (float16 / float32 / float64), ids [H,W] integer -> dict(rgb_u8, u16, depth_f32, out255, record)"""
    color64, distance64 = np.asarray(color).astype(np.float64), np.asarray(distance).astype(np.float64)      # :83-88
    ids = np.asarray(ids)
    valid = ids != -1
    scale, p, nan = tone_scale(color64, valid)
    with np.errstate(all="ignore"):
        out255 = tone_map(color64, scale) * 255
    rgb_u8 = cast_u8(out255)
    u16 = cast_u16(planar_depth_mm(distance64, valid, focal))
    restored = u16 / 1000.0                                                                                    # :132
    n = valid.size
    rec = {"invalid_ratio": (n - valid.sum()) / n, "rgb_mean": np.mean(rgb_u8), "rgb_std": np.std(rgb_u8), "rgb_min": float(np.min(rgb_u8)),
           "rgb_max": float(np.max(rgb_u8)), "depth_mean": np.mean(restored), "depth_std": np.std(restored), "depth_min": np.min(restored),
           "depth_max": np.max(restored), "zero_ids": float((ids == 0).sum()), "nan_brightness": float(nan), "n_valid": float(valid.sum()),
           "percentile": float(p), "scale": float(scale)}
    return {"rgb_u8": rgb_u8, "u16": u16, "depth_f32": (u16 / 1000).astype(np.float32), "out255": out255, "record": {k: float(v) for k, v in rec.items()}}


def record_row(rec):
    return np.array([rec[k] for k in RECORD_FIELDS] + [0.0, 0.0], dtype=np.float64)


# ---- the full-size frame of the fixture: rebuilt from small stored palettes by integer index arithmetic and gathers only (no random stream) ----------
def full_frame_index(H, W):
    i, j = np.arange(H, dtype=np.int64)[:, None], np.arange(W, dtype=np.int64)[None, :]
    return i, j, (i * 131 + j * 31 + (i * j) % 97) % 4096


def full_frame(color_palette, distance_palette, H=768, W=1024):
    """-> color [H,W,3], distance [H,W] in the palettes' dtype, ids int32 [H,W]: 4096 distinct colours (heavy ties), about 4 % invalid pixels"""
    i, j, idx = full_frame_index(H, W)
    ids = np.where((i * j + 3 * i + 5 * j) % 23 == 0, -1, 1 + idx % 50).astype(np.int32)
    return np.ascontiguousarray(color_palette[idx]), np.ascontiguousarray(distance_palette[(idx * 7 + 3) % distance_palette.shape[0]]), ids


# ---- shared checks (tests/test_hypersim_prep_cpu.py, tests/test_hypersim_prep_gpu.py) ------------------------------------------------------------------
EXACT_FIELDS = ("invalid_ratio", "rgb_mean", "rgb_min", "rgb_max", "depth_min", "depth_max")      # ratios of exact integers, extrema
CLOSE_FIELDS = ("rgb_std", "depth_mean", "depth_std")                                               # 1e-10 relative: another summation order
REL = 1e-10


def check_record(got, want, what=""):
    """got: a record row (sequence in RECORD_FIELDS order) or dict; want: dict with at least the reference's nine columns"""
    if not isinstance(got, dict):
        got = dict(zip(RECORD_FIELDS, (float(v) for v in got)))
    for k in EXACT_FIELDS:
        assert got[k] == want[k], "%s %s: %r != %r" % (what, k, got[k], want[k])
    for k in CLOSE_FIELDS:
        assert abs(got[k] - want[k]) <= REL * abs(want[k]), "%s %s: %r vs %r" % (what, k, got[k], want[k])
    for k in ("zero_ids", "nan_brightness", "n_valid", "percentile", "scale"):
        if k in want:
            assert got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])), "%s %s: %r != %r" % (what, k, got[k], want[k])


def check_u8(got, ref, what="", margin=1e-9):
    """exact uint8 equality; a mismatch is reported with the float64 `out * 255` at that element and excused only within `margin` of an integer"""
    bad = np.argwhere(got != ref["rgb_u8"])
    for idx in bad[:20]:
        x = ref["out255"][tuple(idx)]
        print("%s: uint8 mismatch at %s: got %d, reference %d, float64 out * 255 = %r" % (what, tuple(idx), got[tuple(idx)], ref["rgb_u8"][tuple(idx)], x))
    for idx in bad:
        x = ref["out255"][tuple(idx)]
        assert abs(x - np.rint(x)) <= margin and abs(int(got[tuple(idx)]) - int(ref["rgb_u8"][tuple(idx)])) == 1, "%s: uint8 differs at %s away from an integer boundary (%r)" % (what, tuple(idx), x)
    return len(bad)
