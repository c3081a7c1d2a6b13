"""Latent noise drawn on the device (csrc/noise.hip): `--noise_type gaussian | pyramid` of training/train.py:483-491 and the `noise=` settings of
marigold_pipeline.py:420-431, written straight into the noise channels of the UNet input.

The generator is counter-based (Philox4x32-10 on the logical NCHW index, include/e2eft.h): a value is a pure function of (seed, draw, slot, element), so
nothing is synchronised with the host, the result does not depend on memory layout or launch geometry, and a host restatement reproduces it
(tests/noise_ref.py).  Bit parity with torch's own RNG streams is not a goal — torch's CPU and device generators already disagree with each other.

Capture: `draw` is a host counter.  `randn_into` / `pyramid_noise_into` pass it to the kernels by value, so a replayed hipGraph would repeat the noise it was
captured with — they stay on the eager paths.  `randn_at` is the capture-safe Gaussian draw (`e2eft_randn_fill_at`): the kernel reads `draw` from a one-element
int64 device tensor that belongs to the graph, and the caller sets it with `set_draw(tensor, gen)` — `fill_(gen.next_draw())`, one launch with the value as a
kernel argument, no host-to-device copy, no synchronisation — before each replay.  The host counter stays the single source of truth: eager and captured calls on
one generator interleave and see the sequence they see without capture.  `DrawAt(seed, draw_dev)` is the generator-shaped handle for code that takes a
`generator=`: `randn_into` on it is `randn_at` (training.CapturedTrainStep).  "pyramid" by value is not captured: its level sizes are fresh host draws of Python's `random`
per call, as in the reference, so its launch arguments differ from call to call.

The level sizes never index memory, though: every level value is a pure function of (seed, draw, slot, element), and only the level TABLE differs between calls.
`pyramid_noise_at` / `geowizard_pyramid_noise_at` (`e2eft_pyramid_noise_at`, `e2eft_pyramid_noise_weighted_at`) read the draw and the table from 22 int64 device
words, and `set_pyramid_table(table_dev, gen, sizes, rows, cols)` fills them before a replay — the caller draws `sizes` on the host where the eager loop draws
them, so Python's `random` / numpy's stream end where they end without capture.  `randint_into(dst_int64, high, gen, repeat)` is the counter-based
`torch.randint(0, high, (n,)).repeat(repeat)` (the diffusion objective's timesteps), by value or — on a `DrawAt` — read on the device.  A captured micro-step
may make several draws (timesteps, then noise): a `DrawAt` carries one device word per draw site, named by what reads it, and — when the noise is a pyramid — the
table; every draw reads the value `gen.next_draw()` would have returned at that point of the eager order (training.CapturedTrainStepAt).

The GeoWizard trainer has a multi-resolution noise of its own (GeoWizard/geowizard/training/train_depth_normal.py:286-296): level sizes shrunk from the original size by
numpy's global stream, every level weighted per sample by `timesteps / 1000`.  `geowizard_pyramid_level_sizes` / `geowizard_pyramid_noise_into` are that function
(`e2eft_pyramid_noise_weighted`; the timesteps are read on the device); the trainers call it `noise_type="geowizard_pyramid"`.
"""
import random

import numpy as np

from . import ops


class DeviceNoise:
    """seed + a host-side `draw` counter that advances once per call (`next_draw`) and never reads the device.  Two generators with the same seed that
    have made the same number of calls produce the same noise."""

    def __init__(self, seed=0, draw=0):
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.draw = int(draw) & 0xFFFFFFFF

    def next_draw(self):
        d = self.draw
        self.draw = (d + 1) & 0xFFFFFFFF
        return d


class DrawAt(DeviceNoise):
    """a DeviceNoise whose draws are read ON THE DEVICE: `randn_into` with it is `randn_at(dst, seed, draw_dev)`.  What a captured graph is handed in place of the
    caller's generator (training.CapturedTrainStep); the caller's generator stays the source of truth and feeds the words through `set_draw` /
    `set_pyramid_table`.

    One device word PER DRAW SITE of a micro-step, each named by what reads it — no cursor, no order to keep, and a draw that is executed again (a recomputed
    segment) reads the same word again:
      draw_dev      one-element int64: the Gaussian draw (`randn_into`)
      randint_dev   one-element int64: the integer draw (`randint_into`: the diffusion objective's timesteps); None when the micro-step makes none
      table         the 22-word level table of the pyramid draw (`pyramid_noise_into` / `geowizard_pyramid_noise_into`; its word 0 is that draw's `draw`,
                    `set_pyramid_table`), with table_hw the latent (rows, cols) it is filled for; None when the micro-step draws no pyramid
    A micro-step therefore makes at most one draw of each kind."""

    def __init__(self, seed, draw_dev, table=None, table_hw=None, randint_dev=None):
        super().__init__(seed)
        self.draw_dev, self.randint_dev = draw_dev, randint_dev
        self.table, self.table_hw = table, (None if table_hw is None else (int(table_hw[0]), int(table_hw[1])))

    def next_draw(self):
        raise RuntimeError("noise.DrawAt holds no host counter: only the Gaussian draw (randn_into) can read its draw on the device")

    def randint_word(self):
        if self.randint_dev is None:
            raise RuntimeError("noise.DrawAt: this handle carries no word for an integer draw (DrawAt(seed, draw_dev, randint_dev=...))")
        return self.randint_dev

    def table_for(self, rows, cols):
        if self.table is None:
            raise RuntimeError("noise.DrawAt: this handle carries no pyramid table (DrawAt(seed, draw_dev, table, (rows, cols)))")
        if self.table_hw != (int(rows), int(cols)):
            raise ValueError("noise.DrawAt: the pyramid table is filled for %s latents, the destination is %s" % (self.table_hw, (int(rows), int(cols))))
        return self.table


def pyramid_level_sizes(rows, cols, rng=random):
    """the (rows, cols) of every level grid `pipeline.pyramid_noise_like` (training/util/noise.py:8-18) would draw for a [.., rows, cols] latent: one
    `rng.random()` per level in the reference's order (level 0 included, where shrink ** 0 = 1), the shrink cumulative, stopping after the first level
    with a dimension of 1 — so `seed_all` gives the reference's sizes and leaves Python's `random` where the reference leaves it."""
    sizes = []
    for level in range(10):
        shrink = (rng.random() * 2 + 2) ** level
        rows, cols = max(1, int(rows / shrink)), max(1, int(cols / shrink))
        sizes.append((rows, cols))
        if rows == 1 or cols == 1:
            break
    return sizes


def randn_into(dst_nhwc_slice, gen):
    """standard normals into an NHWC view [B,H,W,C] (e.g. `xin[..., 4:]`); advances `gen.draw` (a `DrawAt` reads its draw on the device instead)"""
    if isinstance(gen, DrawAt):
        return randn_at(dst_nhwc_slice, gen.seed, gen.draw_dev)
    return ops.randn_fill_(dst_nhwc_slice, gen.seed, gen.next_draw(), slot=0)


def set_draw(draw_dev, gen):
    """advance `gen.draw` and put the value drawn into the one-element int64 device tensor a captured `randn_at` reads (one fill launch, nothing is copied or read)"""
    return draw_dev.fill_(gen.next_draw())


def randn_at(dst_nhwc_slice, seed, draw_dev):
    """`randn_into` with the draw read on the device from `draw_dev` (see `set_draw`): the same bits for the same value, safe inside a hipGraph capture"""
    return ops.randn_fill_at_(dst_nhwc_slice, seed, draw_dev, slot=0)


def randint_into(dst_int64, high, gen, repeat=1):
    """`torch.randint(0, high, (n,)).repeat(repeat)` from the device generator into a contiguous int64 tensor of n * repeat elements (`e2eft_randint_fill`: the raw
    word of every element, t = (word * high) >> 32); advances `gen.draw` once (a `DrawAt` reads its next draw word on the device instead)"""
    if isinstance(gen, DrawAt):
        return ops.randint_fill_at_(dst_int64, high, gen.seed, gen.randint_word(), slot=0, repeat=repeat)
    return ops.randint_fill_(dst_int64, high, gen.seed, gen.next_draw(), slot=0, repeat=repeat)


def set_pyramid_table(table_dev, gen, sizes, rows, cols):
    """advance `gen.draw` and put the value drawn, with the level `sizes` of a rows x cols latent, into the 22-word int64 device table a captured
    `pyramid_noise_at` / `geowizard_pyramid_noise_at` reads (one one-thread launch with the values as kernel arguments, nothing is copied or read)"""
    return ops.pyramid_table_set_(table_dev, gen.next_draw(), sizes, rows, cols)


def pyramid_noise_at(dst_nhwc_slice, seed, table_dev, discount=0.9):
    """`pyramid_noise_into` with the draw and the level sizes read on the device from `table_dev` (see `set_pyramid_table`): the same bits for the same values,
    safe inside a hipGraph capture"""
    return ops.pyramid_noise_at_(dst_nhwc_slice, seed, table_dev, discount)


def geowizard_pyramid_noise_at(dst_nhwc_slice, seed, table_dev, timesteps, discount=0.9):
    """`geowizard_pyramid_noise_into` with the draw and the level sizes read on the device from `table_dev`"""
    return ops.pyramid_noise_weighted_at_(dst_nhwc_slice, seed, table_dev, timesteps, discount, 1000.0)


def _table_of(gen, dst_nhwc_slice, sizes):
    if sizes is not None:
        raise ValueError("a noise.DrawAt reads its level sizes from its device table: explicit `sizes` go through set_pyramid_table")
    _, H, W, _ = dst_nhwc_slice.shape
    return gen.table_for(H, W)


def pyramid_noise_into(dst_nhwc_slice, gen, discount=0.9, sizes=None):
    """multi-resolution noise of unit std into an NHWC view [B,H,W,C]; `sizes` defaults to `pyramid_level_sizes(H, W)` (Python's `random`, as the
    reference); advances `gen.draw`.  A `DrawAt` reads draw and sizes from its device table instead (`pyramid_noise_at`) and draws nothing on the host."""
    if isinstance(gen, DrawAt):
        return pyramid_noise_at(dst_nhwc_slice, gen.seed, _table_of(gen, dst_nhwc_slice, sizes), discount)
    _, H, W, _ = dst_nhwc_slice.shape
    if sizes is None:
        sizes = pyramid_level_sizes(H, W)
    return ops.pyramid_noise_(dst_nhwc_slice, gen.seed, gen.next_draw(), sizes, discount)


def geowizard_pyramid_level_sizes(rows, cols, rng=np.random, scale=1.5):
    """the (rows, cols) of every level grid the GeoWizard trainer's `pyramid_noise_like` (GeoWizard/geowizard/training/train_depth_normal.py:286-296) draws for a
    [.., rows, cols] latent: one `rng.random()` per level in the reference's order (level 0 included, where r ** 0 = 1), `r = rng.random() * scale + scale`, every
    level shrunk from the ORIGINAL size — `max(1, int(rows / r ** i))`, not cumulative as `pyramid_level_sizes` — stopping after the first level with a dimension
    of 1, at most 10 levels.  rng defaults to numpy's global stream (`np.random`), the reference's: `np.random.seed(s)` gives the reference's sizes and leaves the
    stream where the reference leaves it."""
    sizes = []
    for level in range(10):
        r = rng.random() * scale + scale
        lr, lc = max(1, int(rows / (r ** level))), max(1, int(cols / (r ** level)))
        sizes.append((lr, lc))
        if lr == 1 or lc == 1:
            break
    return sizes


def geowizard_pyramid_noise_into(dst_nhwc_slice, gen, timesteps, discount=0.9, sizes=None):
    """the GeoWizard trainer's timestep-weighted multi-resolution noise (train_depth_normal.py:286-296, called at :658-659) of unit std into an NHWC view [B,H,W,C]:
    level i of sample b weighted by timesteps[b] / 1000 * discount^i (the literal 1000 of :294).  timesteps: int64 device tensor [B], read on the device; `sizes`
    defaults to `geowizard_pyramid_level_sizes(H, W)` (numpy's global stream, as the reference); advances `gen.draw` once.  By value it is not captured, for
    `pyramid_noise_into`'s reason: the sizes are fresh host draws per call.  A `DrawAt` reads draw and sizes from its device table (`geowizard_pyramid_noise_at`)."""
    if isinstance(gen, DrawAt):
        return geowizard_pyramid_noise_at(dst_nhwc_slice, gen.seed, _table_of(gen, dst_nhwc_slice, sizes), timesteps, discount)
    _, H, W, _ = dst_nhwc_slice.shape
    if sizes is None:
        sizes = geowizard_pyramid_level_sizes(H, W)
    return ops.pyramid_noise_weighted_(dst_nhwc_slice, gen.seed, gen.next_draw(), sizes, timesteps, discount, 1000.0)


def noise_into(kind, dst_nhwc_slice, gen):
    if kind == "gaussian":
        return randn_into(dst_nhwc_slice, gen)
    if kind == "pyramid":
        return pyramid_noise_into(dst_nhwc_slice, gen)
    raise ValueError("Unknown noise type %s" % kind)
