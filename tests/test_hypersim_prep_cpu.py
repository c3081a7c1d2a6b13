"""Hypersim preprocessing without a GPU: the numpy restatement tests/hypersim_prep_ref.py reproduces the reference's script as recorded in
tests/golden/hypersim_prep_golden.pt exactly (uint8 image, uint16 depth; the record within 1e-10) and as re-run live from the reference's own files
when they are present; e2eft_hypersim_preprocess rejects bad arguments before it launches; Hypersim(source="raw") finds the released layout and the
default still reads processed/; the generator script's core writes a tree that Hypersim(source="processed") reads back."""
import csv
import ctypes
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import hypersim_prep_ref as hpr  # noqa: E402
import hypersim_raw_fixture as rawfx  # noqa: E402
import make_hypersim_prep_golden as mk  # noqa: E402

GOLD_PATH = os.path.join(HERE, "golden", "hypersim_prep_golden.pt")
GOLD = torch.load(GOLD_PATH, weights_only=False)
NCASES = 14


def _script():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "scripts"))
    try:
        import preprocess_hypersim as script
    finally:
        sys.path.pop(0)
    return script


def test_fixture_is_small_and_covers_the_edge_cases():
    assert os.path.getsize(GOLD_PATH) <= os.path.getsize(os.path.join(HERE, "golden", "d2nt_golden.pt"))
    assert GOLD["sha256"] == mk.REF_SHA256 and len(GOLD["cases"]) == NCASES == len(mk.build_cases())
    shapes = [tuple(c["ids"].shape) for c in GOLD["cases"]]
    assert (1, 1) in shapes and (2, 2) in shapes and (37, 53) in shapes
    nvalid = [int((c["ids"] != -1).sum()) for c in GOLD["cases"]]
    assert 0 in nvalid and 1 in nvalid and any((n - 1) % 10 == 0 and n > 1 for n in nvalid)
    assert {c["color"].dtype for c in GOLD["cases"]} == {torch.float16, torch.float32} == {c["distance"].dtype for c in GOLD["cases"]}
    assert any(bool((c["color"] < 0).any()) for c in GOLD["cases"])
    weights = [np.float64(n - 1) * 0.9 % 1.0 for n in nvalid if n > 0]
    assert any(w == 0 for w in weights) and any(w >= 0.5 for w in weights) and any(0 < w < 0.5 for w in weights)
    nan_valid = [c for c in GOLD["cases"] if bool((torch.isnan(c["distance"].float()) & (c["ids"] != -1)).any())]
    far = [c for c in GOLD["cases"] if bool(((c["distance"].float() > 65.535 * 1.5) & (c["ids"] != -1)).any())]
    assert nan_valid and far
    mm = [c for c in GOLD["cases"] if bool((c["distance"].float().abs() > 2.2e6).any())]      # millimetres beyond int32: this host casts them to 0
    assert mm and all(int(c["u16"][c["distance"].float().abs() > 2.2e6].abs().max()) == 0 for c in mm)
    for c in nan_valid:                                  # the NaN distance became 0, as the kernel defines it
        m = (torch.isnan(c["distance"].float()) & (c["ids"] != -1))
        assert int(c["u16"][m].abs().max()) == 0
    assert all(c["min_gap"] > GOLD["margin"] for c in GOLD["cases"]) and GOLD["full"]["min_gap"] > GOLD["margin"] == 1e-9
    scales = [hpr.preprocess(c["color"].numpy(), c["distance"].numpy(), c["ids"].numpy())["record"]["scale"] for c in GOLD["cases"]]
    assert 0.0 in scales and 1.0 in scales


@pytest.mark.parametrize("i", range(NCASES))
def test_restatement_equals_fixture(i):
    c = GOLD["cases"][i]
    name, color, distance, ids = mk.build_cases()[i]
    assert name == c["name"] and np.array_equal(color, c["color"].numpy(), equal_nan=True) and np.array_equal(distance, c["distance"].numpy(), equal_nan=True)
    r = hpr.preprocess(c["color"].numpy(), c["distance"].numpy(), c["ids"].numpy())
    assert np.array_equal(r["rgb_u8"], c["rgb_u8"].numpy()), name
    assert np.array_equal(r["u16"], c["u16"].numpy().astype(np.uint16)), name
    assert np.array_equal(r["depth_f32"], c["depth_f32"].numpy()) and r["depth_f32"].dtype == np.float32
    hpr.check_record(r["record"], c["record"], name)


def _full_inputs():
    f = GOLD["full"]
    return hpr.full_frame(f["color_palette"].numpy(), f["distance_palette"].numpy())


def test_restatement_equals_the_whole_script_on_a_full_frame():
    f = GOLD["full"]
    color, distance, ids = _full_inputs()
    assert color.shape == (768, 1024, 3) and color.dtype == np.float16 and 0.02 < (ids == -1).mean() < 0.1
    r = hpr.preprocess(color, distance, ids)
    dig = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    assert dig(r["rgb_u8"]) == f["rgb_sha256"] and dig(r["u16"]) == f["u16_sha256"] and dig(r["depth_f32"]) == f["depth_f32_sha256"]
    row = f["csv_row"]
    hpr.check_record(r["record"], {k: float(row[k]) for k in hpr.RECORD_FIELDS[:9]}, "csv row")
    # the generator script formats that row as pandas did
    script = _script()
    columns = [k for k in row if k and k not in script.STAT_COLUMNS]
    mine = dict(zip([""] + columns + list(script.STAT_COLUMNS), script.meta_row(int(row[""]), row, columns, hpr.record_row(r["record"]))))
    assert list(mine) == list(row)
    for k in row:
        if k in hpr.CLOSE_FIELDS:
            assert abs(float(mine[k]) - float(row[k])) <= hpr.REL * abs(float(row[k])), k
        else:
            assert mine[k] == row[k], (k, mine[k], row[k])
    assert f["filename_list"] == "%s %s" % script.frame_names(row)


def test_reference_rerun_live():
    if not mk.reference_available():
        pytest.skip("reference tree not present: the recorded fixture is the pin")
    g = mk.make(full=True)
    assert g["sha256"] == GOLD["sha256"]
    for a, b in zip(g["cases"], GOLD["cases"]):
        for k in ("rgb_u8", "u16", "depth_f32"):
            assert np.array_equal(a[k].numpy(), b[k].numpy()), (a["name"], k)
        assert a["record"] == b["record"]
    for k in ("rgb_sha256", "u16_sha256", "csv_row", "filename_list"):
        assert g["full"][k] == GOLD["full"][k], k


def test_entry_point_rejects_bad_arguments():
    from diffusion_e2e_ft_amd import _lib, ops
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    ok = dict(batch=2, height=5, width=7, color_dtype=_lib.F16, distance_dtype=_lib.F32, depth_format=_lib.HYPERSIM_DEPTH_U16, focal=886.81,
              scale_numerator=ops.hypersim_scale_numerator())

    def desc(**kw):
        d = _lib.HypersimDesc()
        for k, v in dict(ok, **kw).items():
            setattr(d, k, v)
        return d

    assert ctypes.sizeof(_lib.HypersimDesc) == 6 * 4 + 2 * 8
    need = lib.e2eft_hypersim_preprocess_workspace_bytes(ctypes.byref(desc()))
    assert 0 < need < 1 << 16
    call = lambda d, *a: lib.e2eft_hypersim_preprocess(ctypes.byref(d) if d is not None else None, *a)
    for kw, msg in ((dict(batch=0), b"shape"), (dict(height=-1), b"shape"), (dict(width=0), b"shape"), (dict(batch=65536), b"65535"), (dict(height=1 << 16, width=1 << 15), b"2^31"),
                    (dict(color_dtype=_lib.BF16), b"color_dtype"), (dict(distance_dtype=3), b"distance_dtype"), (dict(depth_format=2), b"depth_format"),
                    (dict(focal=0.0), b"focal"), (dict(focal=float("nan")), b"focal"), (dict(scale_numerator=-1.0), b"scale_numerator")):
        d = desc(**kw)
        assert lib.e2eft_hypersim_preprocess_workspace_bytes(ctypes.byref(d)) == 0
        assert call(d, p, p, p, p, p, p, p, need, None) == 1 and msg in lib.e2eft_last_error(), (kw, lib.e2eft_last_error())
    assert lib.e2eft_hypersim_preprocess_workspace_bytes(None) == 0
    assert call(None, p, p, p, p, p, p, p, need, None) == 1
    for k in range(7):
        args = [p] * 7
        args[k] = None
        assert call(desc(), *args, need, None) == 1 and b"null" in lib.e2eft_last_error(), k
    assert call(desc(), p, p, p, p, p, p, p, need - 1, None) == 2 and b"workspace" in lib.e2eft_last_error()
    odd = ctypes.c_void_p(p.value + 8)
    assert call(desc(), p, p, p, p, p, p, odd, need, None) == 1 and b"aligned" in lib.e2eft_last_error()
    assert call(desc(), ctypes.c_void_p(p.value + 2), p, p, p, p, p, p, need, None) == 1 and b"aligned" in lib.e2eft_last_error()
    assert abs(ok["scale_numerator"] - 0.8 ** 2.2) < 1e-15
    with pytest.raises(ValueError, match="depth_format"):
        ops.hypersim_preprocess(torch.zeros(1, 2, 2, 3), torch.zeros(1, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int32), depth_format="mm")
    with pytest.raises(TypeError, match="int32"):
        ops.hypersim_preprocess(torch.zeros(1, 2, 2, 3), torch.zeros(1, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int64))
    with pytest.raises(TypeError, match="color"):
        ops.hypersim_preprocess(torch.zeros(1, 2, 2, 3, dtype=torch.float64), torch.zeros(1, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="color"):
        ops.hypersim_preprocess(torch.zeros(1, 2, 2, 4), torch.zeros(1, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int32))


def test_hypersim_source_argument(tmp_path, monkeypatch):
    import dataset_fixture as dfx
    from diffusion_e2e_ft_amd import data
    # the default: the processed/ tree, exactly as before
    root_dir, split_path = dfx.make_hypersim_tree(str(tmp_path), n=2, H=24, W=32)
    ds = data.Hypersim(root_dir, split_path=split_path)
    assert ds.source == "processed" and ds.decoder is data.pil_decoder and len(ds) == 2
    assert all(sorted(p) == ["depth_path", "normal_path", "rgb_path"] for p in ds.pairs)
    s = ds[1]
    assert sorted(s) == ["depth", "normal_u8", "rgb_u8"] and s["depth"].dtype == np.float32 and s["rgb_u8"].shape == (24, 32, 3)
    assert data.Hypersim(root_dir, split_path=split_path, source="processed").pairs == ds.pairs
    for bad in ("hdf5", "RAW", None, ""):
        with pytest.raises(ValueError, match="source"):
            data.Hypersim(root_dir, split_path=split_path, source=bad)
    # raw: file discovery as the preprocessing script's, the same row filter
    raw, split, kept = rawfx.make_raw_tree(str(tmp_path), n=3, H=12, W=16)
    with pytest.raises(FileNotFoundError, match="metadata_images_split_scene_v1.csv"):      # without split_path: the release's split file, not a processed CSV
        data.Hypersim(raw, source="raw")
    rd = data.Hypersim(raw, split_path=split, source="raw", decoder=rawfx.npy_decoder)
    assert rd.source == "raw" and len(rd) == 3 and rd.transform == (480, 640) and rd.name == "hypersim"
    for pr, (row, color, distance, ids, normal) in zip(rd.pairs, kept):
        img = os.path.join(raw, row["scene_name"], "images")
        fr, cam = "frame.%04d" % int(row["frame_id"]), row["camera_name"]
        assert pr == {"color_path": os.path.join(img, "scene_%s_final_hdf5" % cam, fr + ".color.hdf5"),
                      "distance_path": os.path.join(img, "scene_%s_geometry_hdf5" % cam, fr + ".depth_meters.hdf5"),
                      "entity_path": os.path.join(img, "scene_%s_geometry_hdf5" % cam, fr + ".render_entity_id.hdf5"),
                      "normal_path": os.path.join(img, "scene_%s_geometry_preview" % cam, fr + ".normal_cam.png")}
    for k, (row, color, distance, ids, normal) in enumerate(kept):
        s = rd[k]
        assert sorted(s) == ["color", "distance", "entity_id", "normal_u8"]
        assert np.array_equal(s["color"], color) and s["color"].dtype == np.float16 and np.array_equal(s["distance"], distance) and s["distance"].dtype == distance.dtype
        assert np.array_equal(s["entity_id"], ids) and s["entity_id"].dtype == np.int32 and np.array_equal(s["normal_u8"], normal)
    # the default raw decoder reads HDF5 through h5py, imported on first use: without it the error names the package
    monkeypatch.setitem(sys.modules, "h5py", None)
    default = data.Hypersim(raw, split_path=split, source="raw")
    assert default.decoder is data.raw_decoder and len(default) == 3
    with pytest.raises(ImportError, match="h5py"):
        default[0]
    with pytest.raises(ImportError, match="needs the h5py package"):
        data.read_hdf5(rd.pairs[0]["color_path"])


def test_script_core_writes_the_tree_the_loader_reads(tmp_path):
    from diffusion_e2e_ft_amd import data
    script = _script()
    raw, split, kept = rawfx.make_raw_tree(str(tmp_path), n=3, H=12, W=16)
    columns, by_split = script.read_split(split)
    assert columns == rawfx.COLUMNS and [len(by_split[s]) for s in script.SPLITS] == [4, 1, 0]       # (the row without a normal map is still preprocessed)
    frames = {(r["scene_name"], r["camera_name"], r["frame_id"]): (c, d, i) for r, c, d, i, _ in kept}

    def load(row):
        pr = data.Hypersim.raw_paths(raw, row["scene_name"], row["camera_name"], row["frame_id"])
        return tuple(rawfx.npy_decoder(pr[k], kind) for k, kind in (("color_path", "color"), ("distance_path", "distance"), ("entity_path", "entity_id")))

    def host(color, dist, ids):
        rs = [hpr.preprocess(color[b], dist[b], ids[b]) for b in range(len(ids))]
        return np.stack([r["rgb_u8"] for r in rs]), np.stack([r["u16"] for r in rs]), np.stack([hpr.record_row(r["record"]) for r in rs])

    processed = os.path.join(str(tmp_path), "processed")
    assert script.write_split(os.path.join(processed, "train"), "train", by_split["train"], columns, load, batch=3, preprocess=host) == 4
    rawfx.copy_normals(raw, processed, kept)
    meta = os.path.join(processed, "train", "filename_meta_train.csv")
    with open(meta, newline="") as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0]) == [""] + rawfx.COLUMNS + list(script.STAT_COLUMNS) and [r[""] for r in rows] == ["0", "1", "2", "5"]
    with open(os.path.join(processed, "train", "filename_list_train.txt")) as f:
        assert f.read().split("\n") == ["%s %s" % (r["rgb_path"], r["depth_path"]) for r in rows]
    assert rows[0]["rgb_path"] == os.path.join("ai_001_002", "rgb_cam_00_fr0000.png") and rows[1]["depth_path"] == os.path.join("ai_002_002", "depth_plane_cam_01_fr0005.png")
    ds = data.Hypersim(processed, split_path=meta)
    assert len(ds) == 3                                   # the frame without a normal map is skipped by the loader, as always
    for k, (row, color, distance, ids, normal) in enumerate(kept):
        want = hpr.preprocess(color, distance, ids)
        s = ds[k]
        assert np.array_equal(s["rgb_u8"], want["rgb_u8"]) and np.array_equal(s["depth"], want["depth_f32"]) and np.array_equal(s["normal_u8"], normal)
        assert float(rows[k]["invalid_ratio"]) == want["record"]["invalid_ratio"] and float(rows[k]["depth_max"]) == want["record"]["depth_max"]
    # the reference's assertion on ids equal to 0 surfaces with the frame's name
    ids0 = kept[1][3].copy()
    ids0[0, 0] = 0
    bad = lambda row: (kept[1][1], kept[1][2], ids0)
    with pytest.raises(ValueError, match="ai_002_002 cam_01 frame 5.*render_entity_id == 0"):
        script.write_split(os.path.join(str(tmp_path), "p2", "train"), "train", by_split["train"][1:2], columns, bad, preprocess=host)
