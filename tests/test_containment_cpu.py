"""tests/containment.py on plain torch functions (no GPU): the harness passes on a correct fake op and FAILS on four fake ops that carry the defects
tests/test_containment_gpu.py exists to find — the proof that those tests can fail.  The fake ops are torch on CPU tensors; the allocation patch is told to poison
CPU tensors too (device_filter)."""
import pytest
import torch

from containment import FILLS, allowed_mask, assert_bands_intact, check_two_fills, grid, guarded, poisoned_allocations

M, K, N = 7, 12, 5
ANY = lambda device: True


def _data(seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)


def _ld(t):
    return t.stride(0)


def _flat(t, extra_rows=0, extra_cols=0):
    """what a kernel sees: the raw memory behind a row view, as a [rows + extra_rows, cols + extra_cols] window of row stride ld starting at the view's base"""
    return t.as_strided((t.shape[0] + extra_rows, t.shape[1] + extra_cols), (_ld(t), 1), t.storage_offset())


def op_good(a, w, out):
    ws = torch.empty(2, M, N)                 # two split-K partials, both written
    ws[0] = a[:, :K // 2] @ w[:, :K // 2].t()
    ws[1] = a[:, K // 2:] @ w[:, K // 2:].t()
    out.copy_(ws.sum(0))


def op_writes_pad(a, w, out):
    op_good(a, w, out)
    _flat(out, extra_cols=1)[2, N] = 1.0      # one element between C and ld


def op_writes_row_past_m(a, w, out):
    op_good(a, w, out)
    _flat(out, extra_rows=1)[M] = 1.0         # the row a ragged last tile would touch


def op_reads_neighbour(a, w, out):
    op_good(a, w, out)
    out += 0.0 * _flat(a, extra_cols=1)[:, K:K + 1]      # "masked" by a zero weight: invisible next to finite data


def op_sums_unwritten_scratch(a, w, out):
    ws = torch.empty(3, M, N)                 # three slabs allocated, two written
    ws[0] = a[:, :K // 2] @ w[:, :K // 2].t()
    ws[1] = a[:, K // 2:] @ w[:, K // 2:].t()
    out.copy_(ws.sum(0))


def _case(op):
    a, w = _data()
    ref = a.double() @ w.double().t()

    def run(fill):
        ab, av = guarded((M, K), torch.float32, "cpu", fill, data=a)
        ob, ov = guarded((M, N), torch.float32, "cpu", fill)
        op(av, w, ov)
        return dict(out=ov), [(ab, av), (ob, ov)]

    def check(name, t):
        assert (t.double() - ref).abs().max() <= 1e-5 * ref.abs().max()

    check_two_fills(run, check, device_filter=ANY, what=op.__name__)


def test_passes_on_a_correct_op():
    _case(op_good)


@pytest.mark.parametrize("op,message", [(op_writes_pad, r"first at \(row 2, column %d\)" % N), (op_writes_row_past_m, r"first at \(row %d, column 0\)" % M),
                                        (op_reads_neighbour, "non-finite"), (op_sums_unwritten_scratch, "non-finite")])
def test_fails_on_a_broken_op(op, message):
    with pytest.raises(AssertionError, match=message):
        _case(op)


def test_unwritten_scratch_is_invisible_without_the_patch_and_fill_dependent_with_it():
    """the zero fill alone passes the broken op (what a fresh process usually hands out): only the pair of fills, or the NaN fill, sees it"""
    a, w = _data()
    outs = {}
    for fill in FILLS:
        out = torch.zeros(M, N)
        with poisoned_allocations(fill, ANY):
            op_sums_unwritten_scratch(a, w, out)
        outs[fill] = out
    assert torch.isfinite(outs[0x00]).all() and not torch.isfinite(outs[0xFF]).any()


def test_fill_dependence_alone_is_reported():
    """an op that leaks an unwritten INTEGER workspace into its output is finite under both fills; bit-equality between the fills catches it"""
    def run(fill):
        ob, ov = guarded((M, N), torch.float32, "cpu", fill)
        ov.copy_(torch.ones(M, N) + torch.empty(M, N, dtype=torch.int32).float() * 0.125)
        return dict(out=ov), [(ob, ov)]
    with pytest.raises(AssertionError, match="depends on the fill"):
        check_two_fills(run, device_filter=ANY)


def test_allowed_mask_admits_documented_pad_writes_only():
    for fill in FILLS:
        ob, ov = guarded((M, N), torch.float32, "cpu", fill)
        ov.fill_(1.0)
        grid(ob)[:, N:8] = 0.0                # zeros up to the 16-byte round-up: visible under 0xFF, the fill's own value under 0x00
        allowed = allowed_mask(ob)
        allowed[:, N:8] = True
        assert_bands_intact(ob, ov, allowed)
        if fill == 0xFF:
            with pytest.raises(AssertionError, match=r"%d element\(s\).*first at \(row 0, column %d\)" % (M * (8 - N), N)):
                assert_bands_intact(ob, ov)
        grid(ob)[3, 8] = 2.0
        with pytest.raises(AssertionError, match=r"first at \(row 3, column 8\)"):
            assert_bands_intact(ob, ov, allowed)
        ob2, ov2 = guarded((M, N), torch.float32, "cpu", fill)
        ob2[ov2.storage_offset() - 1] = 5.0   # the element in front of the view
        with pytest.raises(AssertionError, match=r"first at \(row -1, column %d\)" % (ob2._guard["ld"] - 1)):
            assert_bands_intact(ob2, ov2)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64])
def test_ff_bytes_are_nan_in_every_float_type(dtype):
    with poisoned_allocations(0xFF, ANY):
        for t in (torch.empty(5, 3, dtype=dtype), torch.empty_like(torch.zeros(4, dtype=dtype)), torch.zeros(2, dtype=dtype).new_empty(6),
                  torch.empty_strided((3, 2), (4, 1), dtype=dtype)):
            assert torch.isnan(t).all()
    with poisoned_allocations(0x00, ANY):
        assert (torch.empty(5, 3, dtype=dtype) == 0).all()
    buf, view = guarded((3, 5), dtype, "cpu", 0xFF)
    assert torch.isnan(buf).all() and torch.isnan(view).all()


def test_ff_bytes_in_integer_types_and_patch_scope():
    saved = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)
    with pytest.raises(ZeroDivisionError):
        with poisoned_allocations(0xFF, ANY):
            assert (torch.empty(4, dtype=torch.int32) == -1).all() and (torch.empty(4, dtype=torch.int64) == -1).all() and (torch.empty(4, dtype=torch.uint8) == 255).all()
            1 / 0
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == saved      # restored on an exception too
    import containment

    def refuse(t, fill):
        raise AssertionError("a CPU tensor was poisoned under the default device filter")

    real, containment._fill_bytes = containment._fill_bytes, refuse      # the default filter leaves CPU tensors alone: the fill routine is never reached
    try:
        with poisoned_allocations(0xFF):
            t = torch.zeros(8)
            made = (torch.empty(16), torch.empty_like(t), t.new_empty(4), torch.empty_strided((2, 2), (2, 1)))
        assert all(m.device.type == "cpu" for m in made) and (t == 0).all()
        with pytest.raises(AssertionError, match="was poisoned"):
            with poisoned_allocations(0xFF, ANY):
                torch.empty(16)
    finally:
        containment._fill_bytes = real


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.uint8])
@pytest.mark.parametrize("shape", [(5, 7), (2, 3, 4, 24), (2, 9, 128), (1, 13)])
def test_guarded_geometry(dtype, shape):
    es = torch.empty(0, dtype=dtype).element_size()
    unit = 16 // es
    data = (torch.arange(torch.Size(shape).numel()).view(shape) % 100).to(dtype)
    buf, view = guarded(shape, dtype, "cpu", 0xFF, data=data)
    g = buf._guard
    C = shape[-1]
    assert view.shape == shape and view.stride(-1) == 1 and torch.equal(view, data)
    assert g["ld"] % unit == 0 and g["ld"] >= unit + C + 64 and view.storage_offset() % g["ld"] == unit
    assert view.data_ptr() % 16 == 0
    assert view.storage_offset() // g["ld"] >= 3 and buf.numel() // g["ld"] - view.storage_offset() // g["ld"] - g["rows"] >= 256
    # dense over one row stride: flattening the leading dimensions is a view
    assert torch.equal(view.as_strided((g["rows"], C), (g["ld"], 1), view.storage_offset()), data.view(-1, C))
    for i in range(len(shape) - 2, -1, -1):
        exp = g["ld"] if i == len(shape) - 2 else view.stride(i + 1) * shape[i + 1]
        assert view.stride(i) == exp
    assert_bands_intact(buf, view)
    off1 = guarded(shape, dtype, "cpu", 0x00, col0=unit + 1)[1]
    assert off1.data_ptr() % 16 == es % 16
