"""Write Hypersim's processed/ tree on the GPU: what Marigold/script/dataset_preprocess/hypersim/preprocess_hypersim.py writes with OpenCV, h5py, pandas and
float64 numpy per frame — processed/{train,val,test}/<scene>/rgb_<cam>_fr<id>.png (8-bit tone-mapped RGB) and depth_plane_<cam>_fr<id>.png (16-bit
millimetres of planar depth), filename_list_{split}.txt and filename_meta_{split}.csv with the reference's columns — through
e2eft_hypersim_preprocess (csrc/hypersimprep.hip).  PNGs are written with Pillow; HDF5 is read through data.read_hdf5 (needs h5py, imported there).
The reference's `assert (entity_id_map != 0).all()` is kept: a frame with an id equal to 0 stops the run with its name.

usage: python scripts/preprocess_hypersim.py [--split_csv data/hypersim/metadata_images_split_scene_v1.csv] [--dataset_dir data/hypersim/raw_data]
                                              [--output_dir data/hypersim/processed] [--batch 8]
`write_split` is the core (rows + a frame loader in -> files out): tests drive it with arrays instead of HDF5 files."""
import argparse
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

SPLITS = ("train", "val", "test")
STAT_COLUMNS = ("rgb_path", "rgb_mean", "rgb_std", "rgb_min", "rgb_max", "depth_path", "depth_mean", "depth_std", "depth_min", "depth_max", "invalid_ratio")
# where each statistic sits in the kernel's record (ops.HYPERSIM_RECORD_FIELDS)
RECORD_INDEX = {"invalid_ratio": 0, "rgb_mean": 1, "rgb_std": 2, "rgb_min": 3, "rgb_max": 4, "depth_mean": 5, "depth_std": 6, "depth_min": 7, "depth_max": 8}


def read_split(split_csv):
    """-> (columns, {split: [(index, row dict)]}): the rows with included_in_public_release, by split_partition_name, with their line index in the file
    (the unnamed first column pandas writes, preprocess_hypersim.py:39-47)"""
    by_split = {s: [] for s in SPLITS}
    with open(split_csv, newline="") as f:
        rd = csv.DictReader(f)
        columns = list(rd.fieldnames)
        for k, row in enumerate(rd):
            if str(row["included_in_public_release"]).strip().lower() in ("true", "1") and row["split_partition_name"] in by_split:
                by_split[row["split_partition_name"]].append((k, row))
    return columns, by_split


def frame_names(row):
    """preprocess_hypersim.py:107-121 -> (rgb path, depth path) relative to the split's directory"""
    cam, fr = row["camera_name"], int(row["frame_id"])
    return os.path.join(row["scene_name"], "rgb_%s_fr%04d.png" % (cam, fr)), os.path.join(row["scene_name"], "depth_plane_%s_fr%04d.png" % (cam, fr))


def meta_row(index, row, columns, record):
    """one line of filename_meta_{split}.csv as pandas' to_csv writes it: index, the split file's columns, then STAT_COLUMNS (floats by repr)"""
    rgb_rel, depth_rel = frame_names(row)
    stats = {k: repr(float(record[i])) for k, i in RECORD_INDEX.items()}
    stats.update(rgb_path=rgb_rel, depth_path=depth_rel)
    return [str(index)] + [row[c] for c in columns] + [stats[c] for c in STAT_COLUMNS]


def device_preprocess(device="cuda"):
    """-> preprocess(color [B,H,W,3], distance [B,H,W], ids int32 [B,H,W]) -> (rgb uint8, depth uint16, record float64 [B,16]) numpy, through the kernels"""
    import torch
    from diffusion_e2e_ft_amd import ops

    def run(color, dist, ids):
        out = ops.hypersim_preprocess(torch.from_numpy(color).to(device), torch.from_numpy(dist).to(device), torch.from_numpy(ids).to(device), depth_format="u16")
        return tuple(t.cpu().numpy() for t in out)

    return run


def write_split(split_dir, split, rows, columns, load_frame, batch=8, preprocess=None):
    """rows: [(index, row dict)] of one split; load_frame(row) -> (color [H,W,3], distance [H,W] float16 / float32, entity_id [H,W] integer) numpy arrays;
    preprocess: device_preprocess() unless given (the same contract on the host: tests).  Writes the split's PNGs, filename_list_{split}.txt and
    filename_meta_{split}.csv under split_dir; returns the number of frames."""
    from PIL import Image
    if preprocess is None:
        preprocess = device_preprocess()
    os.makedirs(split_dir, exist_ok=True)
    lines, metas = [], []
    for b0 in range(0, len(rows), batch):
        chunk = rows[b0:b0 + batch]
        frames = [load_frame(r) for _, r in chunk]
        # frames of one batch share a size and a dtype (Hypersim's all do); a frame that differs starts a batch of its own
        groups = []
        for k, fr in enumerate(frames):
            sig = (fr[0].shape, fr[0].dtype, fr[1].dtype)
            if groups and groups[-1][0] == sig:
                groups[-1][1].append(k)
            else:
                groups.append((sig, [k]))
        for _, ks in groups:
            rgb, u16, rec = preprocess(np.stack([np.ascontiguousarray(frames[k][0]) for k in ks]), np.stack([np.ascontiguousarray(frames[k][1]) for k in ks]),
                                       np.stack([np.ascontiguousarray(frames[k][2], dtype=np.int32) for k in ks]))
            for j, k in enumerate(ks):
                index, row = chunk[k]
                if rec[j, 9] != 0:
                    raise ValueError("%s %s frame %s: %d pixels with render_entity_id == 0 (the reference's tone_map asserts there is none)"
                                     % (row["scene_name"], row["camera_name"], row["frame_id"], int(rec[j, 9])))
                rgb_rel, depth_rel = frame_names(row)
                os.makedirs(os.path.join(split_dir, row["scene_name"]), exist_ok=True)
                Image.fromarray(rgb[j]).save(os.path.join(split_dir, rgb_rel))
                Image.fromarray(u16[j]).save(os.path.join(split_dir, depth_rel))
                lines.append("%s %s" % (rgb_rel, depth_rel))
                metas.append(meta_row(index, row, columns, rec[j]))
    with open(os.path.join(split_dir, "filename_list_%s.txt" % split), "w") as f:
        f.write("\n".join(lines))
    with open(os.path.join(split_dir, "filename_meta_%s.csv" % split), "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow([""] + list(columns) + list(STAT_COLUMNS))
        w.writerows(metas)
    return len(lines)


def hdf5_loader(dataset_dir):
    from diffusion_e2e_ft_amd import data

    def load(row):
        pr = data.Hypersim.raw_paths(dataset_dir, row["scene_name"], row["camera_name"], row["frame_id"])
        return data.read_hdf5(pr["color_path"]), data.read_hdf5(pr["distance_path"]), data.read_hdf5(pr["entity_path"])

    return load


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--split_csv", default="data/hypersim/metadata_images_split_scene_v1.csv")
    ap.add_argument("--dataset_dir", default="data/hypersim/raw_data")
    ap.add_argument("--output_dir", default="data/hypersim/processed")
    ap.add_argument("--batch", type=int, default=8)
    args = ap.parse_args(argv)
    columns, by_split = read_split(args.split_csv)
    total = 0
    for split in SPLITS:
        total += write_split(os.path.join(args.output_dir, split), split, by_split[split], columns, hdf5_loader(args.dataset_dir), batch=args.batch)
        print("%s: %d frames" % (split, len(by_split[split])))
    print("Preprocess finished")
    return total


if __name__ == "__main__":
    main()
