#!/usr/bin/env python
"""The 3DMatch train / val tables from a download, on the device: what the reference's dataloader/3DMatch_preprocess.py makes offline
with open3d and cv2.

    python examples/preprocess_3dmatch.py --root /data/3dmatch/fragments --split train

reads `<root>/scene_list_<split>.txt`, `<root>/<scene>/seq*/*.ply` and the `.pose.npy` next to every fragment, and writes
`3DMatch_<split>_0.030_points.pkl`, `_overlap.pkl` and `_keypts.pkl` under --save (default `<root>/3dmatch_train_val`, where
`deepsir_amd.data.ThreeDMatchTrain(root, engine)` and the reference's loader look for them).  Existing files are reloaded."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", required=True)
    ap.add_argument("--save", default=None)
    ap.add_argument("--split", default="train", choices=("train", "val"))
    ap.add_argument("--downsample", type=float, default=0.03)
    ap.add_argument("--overlap-thres", type=float, default=0.30)
    ap.add_argument("--max-jobs-bytes", type=int, default=1 << 28)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.data import preprocess_3dmatch
    from deepsir_amd.engine import Engine
    eng = Engine(NetConfig(), a.device)
    t0 = time.time()
    points, overlap, keypts = preprocess_3dmatch(a.root, a.save or os.path.join(a.root, "3dmatch_train_val"), a.split, eng, a.downsample,
                                                 a.overlap_thres, a.max_jobs_bytes)
    print(f"{len(points)} fragments, {len(overlap)} pairs above {a.overlap_thres} ({sum(len(v) for v in keypts.values())} key-point pairs) "
          f"in {time.time() - t0:.1f} s")
    eng.close()


if __name__ == "__main__":
    main()
