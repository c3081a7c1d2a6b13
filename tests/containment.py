"""Memory containment harness: does an op write only its output and read only its input?

guarded()               an operand as an interior view of a larger allocation whose every other byte is a known fill;
assert_bands_intact()   after the op, every byte of that allocation outside the allowed write set still is the fill;
poisoned_allocations()  inside it torch.empty / empty_like / new_empty / empty_strided return tensors whose bytes are the fill, so a workspace slab, a pad column or a
                        split that no workgroup wrote holds the fill and not whatever the caching allocator recycled;
check_two_fills()       the protocol: run the op once per fill; outputs finite and right, the bands of every guarded buffer intact, the two runs equal bit for bit.

The two fills: 0xFF bytes are a NaN in f16, bf16, fp32 and fp64 (-1 in int32 / int64, 255 in uint8) — a read outside the input or of unwritten scratch turns the
output NaN even where it is multiplied by a zero weight or a masked probability; 0x00 bytes are zero everywhere — the same read is then harmless, so the two runs
differ.  A stray write shows under either fill unless it writes the fill's own value, hence both are checked."""
import contextlib

import torch

FILLS = (0xFF, 0x00)
GUARD_ROWS_BEFORE = 3
GUARD_ROWS_AFTER = 256        # one full row tile of the largest kernel: an overrun of a whole ragged tile still lands in this allocation
GUARD_COLS_AFTER = 64
_EMPTY = torch.empty         # the unpatched allocator, for the byte views of the harness itself


def _fill_bytes(t, fill):
    flat = _EMPTY(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())
    flat.fill_(fill)


def guarded(shape, dtype, device, fill, data=None, col0=None, rows_before=GUARD_ROWS_BEFORE, rows_after=GUARD_ROWS_AFTER, cols_after=GUARD_COLS_AFTER, ld_unit=None):
    """-> (buffer, view).  buffer: one flat allocation of `dtype` whose bytes are all `fill`; view: an as_strided view of it of the logical `shape` [..., C], row-major
    with unit inner stride, every leading dimension dense over ONE row stride ld (pixel-dense NHWC, batch-dense [B, N, C]): column offset col0 (default: one 16-byte
    unit), ld >= col0 + C + cols_after and a multiple of the 16-byte unit, rows_before guard rows in front and rows_after behind.  With the default col0 the view's
    base pointer is 16-byte aligned; col0 = unit + 1 puts it one element off.  ld_unit: ld a multiple of this many elements instead (a multiple of the 16-byte unit
    itself: kernels whose vector epilogue asks for rows of whole 32 bytes).  data: written into the logical region (an input); otherwise the region keeps the fill."""
    shape = tuple(int(s) for s in shape)
    assert len(shape) >= 1 and all(s > 0 for s in shape), shape
    es = _EMPTY(0, dtype=dtype).element_size()
    unit = max(16 // es, 1)
    col0 = unit if col0 is None else col0
    C = shape[-1]
    rows = 1
    for s in shape[:-1]:
        rows *= s
    ld_unit = unit if ld_unit is None else ld_unit
    assert ld_unit % unit == 0, (ld_unit, unit)
    ld = -(-(col0 + C + cols_after) // ld_unit) * ld_unit
    total = (rows_before + rows + rows_after) * ld
    buffer = torch.zeros(total, dtype=dtype, device=device)
    _fill_bytes(buffer, fill)
    strides, s = [1], ld
    for n in reversed(shape[:-1]):
        strides.insert(0, s)
        s *= n
    view = buffer.as_strided(shape, strides, rows_before * ld + col0)
    assert col0 % unit != 0 or view.data_ptr() % 16 == 0
    buffer._guard = dict(fill=fill, ld=ld, rows=rows, cols=C, offset=rows_before * ld + col0)
    if data is not None:
        view.copy_(data.to(dtype))
    return buffer, view


def grid(buffer):
    """the rows x ld grid of a guarded buffer as a tensor: grid[r, j] is the element j columns right of the view's row r (columns >= C are the pad up to the next row)"""
    g = buffer._guard
    return buffer.as_strided((g["rows"], g["ld"]), (g["ld"], 1), g["offset"])


def allowed_mask(buffer):
    """an all-False boolean mask over grid(buffer), to be filled in with documented pad writes"""
    g = buffer._guard
    return torch.zeros(g["rows"], g["ld"], dtype=torch.bool)


def assert_bands_intact(buffer, view, allowed=None, what=""):
    """Every byte of `buffer` outside the view's logical extent (and outside `allowed`, a boolean mask over the view's rows x ld grid) still equals the fill."""
    g = buffer._guard
    es = buffer.element_size()
    assert view.storage_offset() == g["offset"] and view.shape[-1] == g["cols"] and view.numel() == g["rows"] * g["cols"], "not the view guarded() returned"
    ld, rows, cols, offset = g["ld"], g["rows"], g["cols"], g["offset"]
    dirty = (_EMPTY(0, dtype=torch.uint8, device=buffer.device).set_(buffer.untyped_storage()) != g["fill"]).view(-1, es).any(dim=1)
    writable = torch.zeros(rows, ld, dtype=torch.bool)
    writable[:, :cols] = True
    if allowed is not None:
        assert tuple(allowed.shape) == (rows, ld) and allowed.dtype == torch.bool, (allowed.shape, allowed.dtype)
        writable |= allowed.cpu()
    mask = torch.zeros(buffer.numel(), dtype=torch.bool)
    mask[offset:offset + rows * ld] = writable.view(-1)
    bad = dirty.cpu() & ~mask
    if bad.any():
        idx = bad.nonzero().view(-1)
        rel = int(idx[0]) - offset
        raise AssertionError("%s: %d element(s) outside the allowed write set no longer hold the fill 0x%02X; first at (row %d, column %d) relative to the view "
                             "(view: %d rows x %d columns, ld %d)" % (what or "guard bands", idx.numel(), g["fill"], rel // ld, rel % ld, rows, cols, ld))


def _on_gpu(device):
    return device.type == "cuda"


@contextlib.contextmanager
def poisoned_allocations(fill, device_filter=_on_gpu):
    """Inside: torch.empty, torch.empty_like, Tensor.new_empty and torch.empty_strided return tensors whose bytes are all `fill` on the devices device_filter(device)
    accepts (default: device tensors only, CPU tensors are left alone).  The originals are restored on the way out."""
    saved = dict(empty=torch.empty, empty_like=torch.empty_like, empty_strided=torch.empty_strided, new_empty=torch.Tensor.new_empty)

    def wrap(fn):
        def poisoned(*args, **kwargs):
            t = fn(*args, **kwargs)
            if isinstance(t, torch.Tensor) and t.untyped_storage().nbytes() > 0 and device_filter(t.device):
                _fill_bytes(t, fill)
            return t
        return poisoned

    try:
        torch.empty, torch.empty_like, torch.empty_strided = wrap(saved["empty"]), wrap(saved["empty_like"]), wrap(saved["empty_strided"])
        torch.Tensor.new_empty = wrap(saved["new_empty"])
        yield
    finally:
        torch.empty, torch.empty_like, torch.empty_strided = saved["empty"], saved["empty_like"], saved["empty_strided"]
        torch.Tensor.new_empty = saved["new_empty"]


def check_two_fills(run, check=None, device_filter=_on_gpu, what=""):
    """run(fill) -> (outputs, guards): outputs {name: tensor}; guards a list of (buffer, view) or (buffer, view, allowed) of EVERY guarded operand, inputs included.
    run builds its operands with guarded(..., fill) and makes the call; it runs under poisoned_allocations(fill).  Asserted, per fill: every output finite, check(name,
    tensor) (the comparison with the reference), every guard's bands intact; then across the fills: torch.equal for every output — the two runs have identical
    layout and addresses.
    -> the outputs of the first fill."""
    results = {}
    for fill in FILLS:
        with poisoned_allocations(fill, device_filter):
            outputs, guards = run(fill)
        tag = "%s fill 0x%02X" % (what, fill)
        for i, g in enumerate(guards):
            assert_bands_intact(g[0], g[1], g[2] if len(g) > 2 else None, what="%s: guarded operand %d" % (tag, i))
        for name, t in outputs.items():
            if t.is_floating_point():
                bad = ~torch.isfinite(t)
                assert not bad.any(), "%s: output %s has %d non-finite entries, first at %s" % (tag, name, int(bad.sum()), tuple(bad.nonzero()[0].tolist()))
            if check is not None:
                check(name, t)
        results[fill] = {name: t.detach().clone() for name, t in outputs.items()}
    a, b = results[FILLS[0]], results[FILLS[1]]
    signed = {torch.uint16: torch.int16, torch.uint32: torch.int32, torch.uint64: torch.int64}      # (comparisons of the wide unsigned types are not implemented everywhere)
    for name in a:
        ta, tb = (t.view(signed[t.dtype]) if t.dtype in signed else t for t in (a[name], b[name]))
        if not torch.equal(ta, tb):
            ne = ta != tb
            raise AssertionError("%s: output %s depends on the fill: %d of %d entries differ between the 0xFF and the 0x00 run, first at %s"
                                 % (what, name, int(ne.sum()), ne.numel(), tuple(ne.nonzero()[0].tolist())))
    return a
