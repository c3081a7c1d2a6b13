"""Depth-to-normal translation (D2NT) without a GPU: the numpy restatement tests/d2nt_ref.py reproduces the reference's translator as recorded in
tests/golden/d2nt_golden.pt (and as re-run live from the reference's own files when they are present), the 16-bit PNG writer makes the file the
training loader reads, VirtualKITTI2(normals="d2nt") needs no normals folder, and e2eft_depth_to_normals rejects bad arguments before launching."""
import ctypes
import os
import struct
import sys
import zlib

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import d2nt_ref  # noqa: E402
import make_d2nt_golden as mk  # noqa: E402

GOLD = torch.load(os.path.join(HERE, "golden", "d2nt_golden.pt"), weights_only=False)


def _host_power_is_recorded_power():
    """numpy's float32 power is SIMD-dispatched: the fixture's bits are reproducible only where np.power gives the recorded values"""
    pp = GOLD["power_probe"]
    return np.array_equal(np.power(np.e, -pp["x"].numpy()), pp["p"].numpy())


def test_fixture_is_small_and_covers_ties_and_margins():
    assert os.path.getsize(os.path.join(HERE, "golden", "d2nt_golden.pt")) < 1 << 20
    assert GOLD["sha256"] == mk.REF_SHA256
    shapes = [tuple(c["depth_cm"].shape) for c in GOLD["cases"]]
    assert (2, 2) in shapes and len({c["K"] for c in GOLD["cases"]}) == 2
    ch = torch.cat([c["choice"].flatten() for c in GOLD["cases"]])
    assert all(int((ch == k).sum()) > 0 for k in range(5))           # every direction chosen (flat regions tie to index 0)
    assert sum(int((c["margin"] < 1e-5).sum()) for c in GOLD["cases"]) > 0      # snapping ratios within round-off of e are present
    assert any(int(c["depth_cm"].numpy().max()) == 65535 for c in GOLD["cases"])        # sky


@pytest.mark.parametrize("i", range(len(mk.CASES)))
def test_restatement_equals_fixture(i):
    c = GOLD["cases"][i]
    cm = c["depth_cm"].numpy()
    seed, H, W, K, sky = mk.CASES[i]
    assert np.array_equal(cm, d2nt_ref.vkitti_like_depth_cm(np.random.default_rng(seed), H, W, sky=sky))
    r3 = d2nt_ref.depth_to_normals(d2nt_ref.cm_to_metres(cm), K, True)
    r2 = d2nt_ref.depth_to_normals(d2nt_ref.cm_to_metres(cm), K, False)
    assert np.array_equal(r3["choice"], c["choice"].numpy())            # fp32 Laplacian + argmin: no powf involved
    if _host_power_is_recorded_power():
        assert np.array_equal(r3["normal"], c["normal_v3"].numpy()) and np.array_equal(r2["normal"], c["normal_v2"].numpy())
        for v, r in (("v2", r2), ("v3", r3)):
            assert np.array_equal(r["u16"], c["u16_" + v].numpy()) and np.array_equal(r["u8"], c["u8_" + v].numpy())
        assert np.array_equal(r3["margin"].astype(np.float32), c["margin"].numpy())
    else:       # another SIMD path: powf differs by 1 ulp on some inputs; the normals move by < 1e-9
        assert np.abs(r3["normal"] - c["normal_v3"].numpy()).max() < 1e-6
    assert np.array_equal(c["u8_v3"].numpy(), c["u16_v3"].numpy() >> 8)


def test_reference_rerun_live():
    if not mk.reference_available():
        pytest.skip("reference tree not present: the recorded fixture is the pin")
    g = mk.make()
    assert g["sha256"] == GOLD["sha256"]
    for a, b in zip(g["cases"], GOLD["cases"]):
        for k in ("depth_cm", "normal_v2", "normal_v3", "choice", "u16_v2", "u16_v3", "margin"):
            assert np.array_equal(a[k].numpy(), b[k].numpy()), k


def test_correctly_rounded_power_close_to_numpy():
    x = GOLD["power_probe"]["x"].numpy()
    a, b = np.power(np.e, -x), d2nt_ref.correctly_rounded_power(np.e, -x)
    assert np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32)).max() <= 1


def _parse_png16(path):
    blob = open(path, "rb").read()
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, ihdr = 8, b"", None
    while pos < len(blob):
        n, tag = struct.unpack(">I4s", blob[pos:pos + 8])
        body = blob[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", blob[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        if tag == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    W, H, depth, ctype = ihdr[:4]
    assert (depth, ctype) == (16, 2)
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(H, 1 + W * 6)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].copy().view(">u2").reshape(H, W, 3).astype(np.uint16)


def test_png16_writer_roundtrip(tmp_path):
    from PIL import Image
    from diffusion_e2e_ft_amd import data
    rng = np.random.default_rng(3)
    u16 = rng.integers(0, 65536, (37, 53, 3)).astype(np.uint16)
    u16[0, :4] = [[0, 0, 0], [65535, 65535, 65535], [255, 256, 257], [32767, 32768, 511]]
    p = str(tmp_path / "n.png")
    data.write_png16(p, u16)
    assert np.array_equal(_parse_png16(p), u16)
    with Image.open(p) as im:
        assert np.array_equal(np.array(im.convert("RGB")), (u16 >> 8).astype(np.uint8))
        assert np.array_equal(data.pil_decoder(p, "normal"), (u16 >> 8).astype(np.uint8))


def test_vkitti_d2nt_mode_needs_no_normals_folder(tmp_path):
    import shutil
    import dataset_fixture as dfx
    from diffusion_e2e_ft_amd import data
    vroot = dfx.make_vkitti_tree(str(tmp_path), n=2, H=40, W=70)
    files = data.VirtualKITTI2(vroot, transform=True)
    a = files[1]
    assert files.normals == "files" and sorted(a) == ["depth", "normal_u8", "rgb_u8"]
    shutil.rmtree(os.path.join(vroot, "vkitti_DAG_normals"))
    syn = data.VirtualKITTI2(vroot, transform=True, normals="d2nt")
    assert syn.pairs == files.pairs and len(syn) == 2
    b = syn[1]
    assert sorted(b) == ["depth", "rgb_u8"]
    assert np.array_equal(a["rgb_u8"], b["rgb_u8"]) and np.array_equal(a["depth"], b["depth"]) and a["depth"].dtype == b["depth"].dtype == np.float32
    with pytest.raises(FileNotFoundError):
        files[0]                                                # the default still reads the normal files
    with pytest.raises(ValueError):
        data.VirtualKITTI2(vroot, normals="cv2")


def test_generator_walk_matches_reference_lists(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "scripts"))
    try:
        import gen_vkitti_normals as gen
    finally:
        sys.path.pop(0)
    assert gen.CONDITIONS == ["15-deg-left", "15-deg-right", "30-deg-left", "30-deg-right", "clone", "morning", "fog", "rain", "sunset", "overcast"]
    import dataset_fixture as dfx
    vroot = dfx.make_vkitti_tree(str(tmp_path), n=3, H=8, W=9)
    pr = gen.find_pairs(vroot)
    assert [os.path.basename(n) for _, n in pr] == ["normal_00000.png", "normal_00001.png", "normal_00002.png"]
    from diffusion_e2e_ft_amd import data
    assert [n for _, n in pr] == [p[2] for p in data.VirtualKITTI2(vroot).pairs]


def test_entry_point_rejects_bad_arguments():
    from diffusion_e2e_ft_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    d = _lib.D2ntDesc()
    d.batch, d.height, d.width, d.refine, d.out_format, d.depth_scale = 1, 1, 8, 1, _lib.D2NT_F32, 1.0
    assert lib.e2eft_depth_to_normals(ctypes.byref(d), p, p, p, None) == 1 and b"height and width >= 2" in lib.e2eft_last_error()
    d.height, d.width = 8, 1
    assert lib.e2eft_depth_to_normals(ctypes.byref(d), p, p, p, None) == 1
    d.width = 8
    assert lib.e2eft_depth_to_normals(ctypes.byref(d), None, p, p, None) == 1 and b"null" in lib.e2eft_last_error()
    assert lib.e2eft_depth_to_normals(None, p, p, p, None) == 1
    d.out_format = 3
    assert lib.e2eft_depth_to_normals(ctypes.byref(d), p, p, p, None) == 1 and b"out_format" in lib.e2eft_last_error()
    d.out_format, d.refine = _lib.D2NT_U8, 2
    assert lib.e2eft_depth_to_normals(ctypes.byref(d), p, p, p, None) == 1 and b"refine" in lib.e2eft_last_error()
    assert ctypes.sizeof(_lib.D2ntDesc) == 6 * 4
