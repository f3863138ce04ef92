"""Dataset front ends of the registration path: the on-disk formats of the reference's TEST splits -> the pair dicts
`harness.inference_align` consumes (the callers immediately in front of the path).

  reference                                              here
  threeDMatch_loader.read_trajectory (:15-37)            read_trajectory
  o3d.io.read_point_cloud (:165-166)                     read_ply_xyz  (vertex x, y, z of ascii / binary PLY)
  ThreeDMatch.prepare_test / get_data test branch        ThreeDMatchTest
      (:118-175): gt.log pairs, cloud_bin_{i}.ply,
      voxel_down_sample(0.03)
  KITTIPair.prepare_kitti_test (:98-131)                 KittiOdometryTest.pairs
  KITTIPair.get_data (:299-346): velodyne .bin,          KittiOdometryTest.__getitem__
      process_point_cloud crop, pose_refine (ICP,
      cached as icp_opti_pose/<drive>_<t0>_<t1>.npy),
      voxel_down_sample(voxel_size)

File parsing is host IO in numpy.  Every per-point step runs on the device through the engine: crop + voxel average
(csrc/preprocess.hip, `Engine.voxel_downsample`), the point-to-point ICP of pose_refine (csrc/icp.hip,
`Engine.icp_refine`), resampling to a fixed size (`Engine.resample`).  The voxel output order is this engine's own
(ascending voxel index; open3d's hash order is not reproducible without open3d, see include/dsir.h), which is
immaterial to the network: its input is a point SET that the resampler permutes anyway.

The train / val branches (bottom of this file): `ThreeDMatchTrain` (pickled fragments + overlap table,
threeDMatch_loader.py:39-115, :139-159), `KittiOdometryTrain` (prepare_kitti, kitti_loader.py:80-96, :299-346, :384-406) and
`TrainBatches`, which turns either into device-resident training batches: host parsing, then voxel grid -> augmentation
(`Engine.augment`, csrc/augment.hip; the rule is deepsir_amd/augment.py) -> ground-truth matches (`Engine.radius_matches`), all
on the device.  `OxfordTrain` / `OxfordTest` (oxford_loader.py): the train split has one scan per sample and no pose - the pair is the
scan cropped twice by random half-spaces (`Engine.halfspace_crop`, csrc/crop.hip; the rule is deepsir_amd/crop.py) under the identity."""
from __future__ import annotations

import glob
import logging
import os
import pickle
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

_logger = logging.getLogger(__name__)

# the reference's split files (dataloader/split/test_3dmatch.txt, test_kitti.txt): the standard public test splits
THREEDMATCH_TEST_SCENES = (
    "7-scenes-redkitchen", "sun3d-home_at-home_at_scan1_2013_jan_1", "sun3d-home_md-home_md_scan9_2012_sep_30",
    "sun3d-hotel_uc-scan3", "sun3d-hotel_umd-maryland_hotel1", "sun3d-hotel_umd-maryland_hotel3",
    "sun3d-mit_76_studyroom-76-1studyroom2", "sun3d-mit_lab_hj-lab_hj_tea_nov_2_2012_scan1_erika")
KITTI_TEST_SEQUENCES = (8, 9, 10)

# SemanticKITTI `learning_map` (raw label -> training class 0..19, 0 = unlabeled): the public SemanticKITTI API table the
# reference reads from dataloader/semantic-kitti.yaml (kitti_loader.py:358-362)
SEMANTIC_KITTI_LEARNING_MAP = {0: 0, 1: 0, 10: 1, 11: 2, 13: 5, 15: 3, 16: 5, 18: 4, 20: 5, 30: 6, 31: 7, 32: 8, 40: 9, 44: 10,
                               48: 11, 49: 12, 50: 13, 51: 14, 52: 0, 60: 9, 70: 15, 71: 16, 72: 17, 80: 18, 81: 19, 99: 0,
                               252: 1, 253: 7, 254: 6, 255: 8, 256: 5, 257: 5, 258: 4, 259: 5}

# velodyne -> camera-0 calibration the reference hard-codes (kitti_loader.py:148-159)
_VELO2CAM = np.array([[7.533745e-03, -9.999714e-01, -6.166020e-04, -4.069766e-03],
                      [1.480249e-02, 7.280733e-04, -9.998902e-01, -7.631618e-02],
                      [9.998621e-01, 7.523790e-03, 1.480755e-02, -2.717806e-01],
                      [0.0, 0.0, 0.0, 1.0]])


def read_trajectory(path: str, dim: int = 4) -> List[Tuple[Tuple[int, ...], np.ndarray]]:
    """`gt.log` of a 3DMatch evaluation folder: records of one metadata line (ints: i, j, n_fragments) and `dim` matrix
    rows -> [(metadata, pose [dim, dim] float64)]."""
    out = []
    with open(path, "r") as f:
        lines = [ln for ln in f.read().splitlines() if ln.strip()]
    if len(lines) % (dim + 1) != 0:
        raise ValueError(f"{path}: {len(lines)} non-empty lines are not a whole number of {dim + 1}-line records")
    for r in range(0, len(lines), dim + 1):
        meta = tuple(int(x) for x in lines[r].split())
        mat = np.array([[float(x) for x in lines[r + 1 + i].split()] for i in range(dim)], dtype=np.float64)
        if mat.shape != (dim, dim):
            raise ValueError(f"{path}: record {r // (dim + 1)} is not a {dim}x{dim} matrix")
        out.append((meta, mat))
    return out


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def read_ply_xyz(path: str) -> np.ndarray:
    """Vertex positions of a PLY file (ascii, binary_little_endian or binary_big_endian; any extra scalar vertex
    properties such as normals / colours are skipped) -> [n, 3] float32."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, n_vertex, props, in_vertex, seen_vertex = None, 0, [], False, False
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: unterminated PLY header")
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] == "comment" or tok[0] == "obj_info":
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                if tok[1] == "vertex":
                    if seen_vertex:
                        raise ValueError(f"{path}: two vertex elements")
                    n_vertex, in_vertex, seen_vertex = int(tok[2]), True, True
                else:
                    if not seen_vertex:
                        raise ValueError(f"{path}: element '{tok[1]}' precedes the vertices (unsupported)")
                    in_vertex = False
            elif tok[0] == "property" and in_vertex:
                if tok[1] == "list":
                    raise ValueError(f"{path}: list property on vertices (unsupported)")
                if tok[1] not in _PLY_TYPES:
                    raise ValueError(f"{path}: unknown property type {tok[1]}")
                props.append((tok[2], _PLY_TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        names = [p[0] for p in props]
        if not all(k in names for k in ("x", "y", "z")):
            raise ValueError(f"{path}: vertices without x, y, z")
        if fmt == "ascii":
            cols = [names.index(k) for k in ("x", "y", "z")]
            rows = np.loadtxt(f, dtype=np.float64, max_rows=n_vertex, ndmin=2) if n_vertex else np.zeros((0, len(names)))
            if rows.shape[0] != n_vertex:
                raise ValueError(f"{path}: {rows.shape[0]} of {n_vertex} vertices present")
            return np.ascontiguousarray(rows[:, cols], dtype=np.float32)
        if fmt not in ("binary_little_endian", "binary_big_endian"):
            raise ValueError(f"{path}: unknown PLY format {fmt}")
        order = "<" if fmt == "binary_little_endian" else ">"
        dt = np.dtype([(n, order + t) for n, t in props])
        raw = f.read(n_vertex * dt.itemsize)
        if len(raw) != n_vertex * dt.itemsize:
            raise ValueError(f"{path}: truncated vertex data")
        v = np.frombuffer(raw, dtype=dt, count=n_vertex)
        return np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float32)


def read_velodyne(path: str) -> np.ndarray:
    """KITTI velodyne scan: float32 records (x, y, z, reflectance) -> [n, 4]."""
    a = np.fromfile(path, dtype=np.float32)
    if a.size % 4 != 0:
        raise ValueError(f"{path}: {a.size} floats are not a whole number of (x, y, z, reflectance) records")
    return a.reshape(-1, 4)


def read_semantic_labels(path: str, n: Optional[int] = None) -> np.ndarray:
    """SemanticKITTI `.label` file: one uint32 per point, semantic label in the lower 16 bits (instance id above), mapped
    through `learning_map` -> [n] uint8 training classes (kitti_loader.py:368-377)."""
    raw = np.fromfile(path, dtype=np.uint32) & 0xFFFF
    if n is not None and raw.size != n:
        raise ValueError(f"{path}: {raw.size} labels for {n} points")
    lut = np.zeros(65536, dtype=np.int32) - 1
    for k, v in SEMANTIC_KITTI_LEARNING_MAP.items():
        lut[k] = v
    out = lut[raw]
    if (out < 0).any():
        raise KeyError(f"{path}: label {int(raw[out < 0][0])} is not in the SemanticKITTI learning map")
    return out.astype(np.uint8)


def _to_device(engine, a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(engine.device)


def _voxelize(engine, clouds: Sequence[np.ndarray], voxel_size: float, crop=None) -> List[torch.Tensor]:
    """crop + voxel average of a ragged list on the device -> list of [n_i, C] CUDA tensors."""
    dev = [_to_device(engine, c) for c in clouds]
    vox, counts = engine.voxel_downsample(dev, voxel_size, crop)
    n = counts.cpu().tolist()
    return [vox[i, :n[i]].contiguous() for i in range(len(clouds))]


def as_batch(item: Dict[str, object]) -> Dict[str, object]:
    """One dataset sample -> the batch-of-one dict of the reference's collate (data_base.py:196-219), points staying on
    the device: what `harness.inference_align` / `evaluate_align` take as an element of `pairs`."""
    out = {"points_src": item["points_src"][None].contiguous(), "points_ref": item["points_ref"][None].contiguous(),
           "transform_gt": np.asarray(item["transform_gt"], dtype=np.float32)[None], "others": [item["others"]]}
    for k in ("labels_src", "labels_ref"):
        if k in item:
            out[k] = item[k][None].contiguous()
    return out


class ThreeDMatchTest:
    """The 3DMatch test split as the reference walks it (threeDMatch_loader.py:118-175): for every record (i, j, T_gt) of
    `<root>/test/<scene>-evaluation/gt.log`, ref = `<scene>/cloud_bin_i.ply`, src = `<scene>/cloud_bin_j.ply`, both
    voxel-averaged at 0.03 m.  `num_points`: resample to a fixed size (what the collate needs for batches > 1;
    seeded, Resampler semantics); None keeps the ragged sizes."""

    def __init__(self, root: str, engine, scenes: Sequence[str] = THREEDMATCH_TEST_SCENES, voxel_size: float = 0.03,
                 num_points: Optional[int] = None, seed: int = 0):
        self.test_path = os.path.join(root, "test")
        if not os.path.isdir(self.test_path):
            raise FileNotFoundError(f"Invalid path: {self.test_path}")
        self.engine, self.voxel_size, self.num_points, self.seed = engine, float(voxel_size), num_points, int(seed)
        self.files: List[Tuple[str, int, int, np.ndarray]] = []
        for s in scenes:
            traj = os.path.join(self.test_path, s + "-evaluation", "gt.log")
            if not os.path.exists(traj):
                raise FileNotFoundError(traj)
            for meta, pose in read_trajectory(traj):
                self.files.append((s, meta[0], meta[1], pose))

    def __len__(self):
        return len(self.files)

    def __getitem__(self, index: int) -> Dict[str, object]:
        s, i, j, T_gt = self.files[index]
        ref = read_ply_xyz(os.path.join(self.test_path, s, f"cloud_bin_{i}.ply"))
        src = read_ply_xyz(os.path.join(self.test_path, s, f"cloud_bin_{j}.ply"))
        if self.num_points:
            pts, _ = self.engine.preprocess([_to_device(self.engine, src), _to_device(self.engine, ref)], self.voxel_size,
                                            int(self.num_points), seed=self.seed + index)
            vs, vr = pts[0], pts[1]
        else:
            vs, vr = _voxelize(self.engine, [src, ref], self.voxel_size)
        return {"points_src": vs, "points_ref": vr, "transform_gt": T_gt[:3, :].astype(np.float32),
                "others": {"seq": s, "id_ref": i, "id_src": j}}


class KittiOdometryTest:
    """KITTI odometry test pairs as the reference builds them (kitti_loader.py:98-131, :241-346): within a sequence,
    from the current scan the first one more than 10 m away (looking at most 100 scans ahead, minus one - the
    3DFeatNet convention), then continue after it; pair (8, 15, 58) dropped.  A sample = both scans cropped
    (3 m < r <= 60 m, -3 m <= z <= 10 m) and voxel-averaged at `voxel_size` with the reflectance as 4th channel, and
    the ground-truth pose: odometry poses through the velodyne calibration, refined by point-to-point ICP (0.2 m,
    <= 200 iterations, on 0.05 m voxels) and cached as `<root>/icp_opti_pose_dsir/<drive>_<t0>_<t1>.npy`; the
    reference's own cache `<root>/icp_opti_pose/` is read when present and never written.

    Sizes: `num_points` None = what the reference's test split does (SemanticKITTIPair.__getitem__ with fixed=True,
    apply_augment_V2, data_base.py:271-283): the cloud with fewer voxels is tiled (FixedResampler) to the size of the
    other; an int = seeded random resample of both to that size (Resampler).  `with_labels`: the SemanticKITTI class of
    every point rides through the voxel average as a 5th channel and is truncated to an integer afterwards, exactly the
    reference's treatment (kitti_loader.py:324-341, :401-402): `labels_src` / `labels_ref` [n] int32."""

    MIN_DIST = 10.0

    def __init__(self, root: str, engine, sequences: Sequence[int] = KITTI_TEST_SEQUENCES, voxel_size: float = 0.3,
                 feat_len: int = 4, num_points: Optional[int] = None, seed: int = 0, refine_pose: bool = True,
                 with_labels: bool = False):
        self.root_path = os.path.join(root, "dataset")
        if not os.path.isdir(self.root_path):
            raise FileNotFoundError(f"Invalid path: {self.root_path}")
        self.icp_path = os.path.join(root, "icp_opti_pose")
        self.engine, self.voxel_size, self.feat_len = engine, float(voxel_size), int(feat_len)
        self.num_points, self.seed, self.refine_pose = num_points, int(seed), bool(refine_pose)
        self.with_labels = bool(with_labels)
        self._poses: Dict[int, np.ndarray] = {}
        self.files: List[Tuple[int, int, int]] = []
        for drive in sequences:
            self.files.extend(self.pairs(int(drive)))
        if (8, 15, 58) in self.files:
            self.files.remove((8, 15, 58))

    # ---- index
    def scan_ids(self, drive: int) -> List[int]:
        names = glob.glob(os.path.join(self.root_path, "sequences", "%02d" % drive, "velodyne", "*.bin"))
        if not names:
            raise FileNotFoundError(f"Make sure that the path {self.root_path} has drive id: {drive}")
        return sorted(int(os.path.basename(n)[:-4]) for n in names)

    def poses(self, drive: int) -> np.ndarray:
        """[frames, 4, 4] camera-0 poses T_w_cam0 of `poses/<drive>.txt`."""
        if drive not in self._poses:
            a = np.atleast_2d(np.genfromtxt(os.path.join(self.root_path, "poses", "%02d.txt" % drive)))
            T = np.tile(np.eye(4), (a.shape[0], 1, 1))
            T[:, :3, :] = a.reshape(-1, 3, 4)
            self._poses[drive] = T
        return self._poses[drive]

    def pairs(self, drive: int) -> List[Tuple[int, int, int]]:
        inames = set(self.scan_ids(drive))
        pos = self.poses(drive)[:, :3, 3]
        out = []
        curr = min(inames)
        while curr in inames:
            d2 = ((pos[curr:curr + 100] - pos[curr]) ** 2).sum(-1)
            far = np.where(d2 > self.MIN_DIST ** 2)[0]
            if len(far) == 0:
                curr += 1
                continue
            nxt = int(far[0]) + curr - 1
            if nxt in inames:
                out.append((drive, curr, nxt))
                curr = nxt + 1
            # else: the reference loops on the same `curr` forever; a missing scan inside a sequence does not occur
            else:
                curr += 1
        return out

    def __len__(self):
        return len(self.files)

    # ---- ground truth
    def odometry_pose(self, drive: int, t0: int, t1: int) -> np.ndarray:
        """Scan t0 -> scan t1 from the provided poses (kitti_loader.py:257-259): [4, 4] float64."""
        p = self.poses(drive)
        M = (_VELO2CAM.T @ p[t0].T @ np.linalg.inv(p[t1].T) @ np.linalg.inv(_VELO2CAM.T)).T
        return M

    def gt_pose(self, drive: int, t0: int, t1: int, xyz0: np.ndarray, xyz1: np.ndarray) -> np.ndarray:
        key = "%d_%d_%d" % (drive, t0, t1)
        # The reference's own cache (open3d ICP) is READ when present, never written: this engine's refinement is not
        # pinned against open3d (voxel order, termination bookkeeping), so its poses go to a directory of their own and
        # neither side's ground truth silently becomes the other's.
        ref_fn = os.path.join(self.icp_path, key + ".npy")
        if os.path.exists(ref_fn):
            return np.load(ref_fn)
        fn = os.path.join(self.icp_path + "_dsir", key + ".npy")
        if os.path.exists(fn):
            return np.load(fn)
        M = self.odometry_pose(drive, t0, t1)
        if not self.refine_pose:
            return M
        # as the reference: scan 0 is moved by M first, ICP starts from the identity and its result T' is applied on the
        # RIGHT (M2 = M @ T', kitti_loader.py:264-271)
        v0, v1 = _voxelize(self.engine, [xyz0[:, :3], xyz1[:, :3]], 0.05)
        Md = torch.from_numpy(M.astype(np.float32)).to(self.engine.device)
        v0 = (v0 @ Md[:3, :3].T + Md[:3, 3]).contiguous()
        eye = torch.eye(4, device=self.engine.device)[None, :3, :].contiguous()
        T, _ = self.engine.icp_refine(v0[None].contiguous(), v1[None].contiguous(), eye, 0.2, max_iter=200, search="auto")
        Tp = np.eye(4)
        Tp[:3, :] = T[0].double().cpu().numpy()
        M2 = M @ Tp
        os.makedirs(os.path.dirname(fn), exist_ok=True)
        np.save(fn, M2)
        return M2

    # ---- samples
    def __getitem__(self, index: int) -> Dict[str, object]:
        drive, t0, t1 = self.files[index]
        seq = os.path.join(self.root_path, "sequences", "%02d" % drive, "velodyne")
        xyz0 = read_velodyne(os.path.join(seq, "%06d.bin" % t0))
        xyz1 = read_velodyne(os.path.join(seq, "%06d.bin" % t1))
        crop = (3.0, 60.0, -3.0, 10.0)

        def crop_host(c):   # process_point_cloud (data_base.py:299-312), for the pose refinement's input
            r2 = (c[:, :3].astype(np.float64) ** 2).sum(1)
            return c[(r2 <= crop[1] ** 2) & (r2 > crop[0] ** 2) & (c[:, 2] >= crop[2]) & (c[:, 2] <= crop[3])]
        T_gt = self.gt_pose(drive, t0, t1, crop_host(xyz0), crop_host(xyz1))
        C = max(3, min(self.feat_len, 4))
        raw = [xyz0, xyz1]
        if self.with_labels:
            lab = os.path.join(self.root_path, "sequences", "%02d" % drive, "labels")
            raw = [np.concatenate([c, read_semantic_labels(os.path.join(lab, "%06d.label" % t), len(c))[:, None].astype(np.float32)], 1)
                   for c, t in ((xyz0, t0), (xyz1, t1))]          # [x, y, z, reflectance, class]
        else:
            raw = [c[:, :C] for c in raw]
        vox, counts = self.engine.voxel_downsample([_to_device(self.engine, c) for c in raw], self.voxel_size, crop)
        if self.num_points:
            pts = self.engine.resample(vox, counts, int(self.num_points), self.seed + index, "random")
        else:
            pts = self.engine.resample(vox, counts, int(counts.max().item()), 0, "fixed")
        out = {"points_src": pts[0, :, :C].contiguous(), "points_ref": pts[1, :, :C].contiguous(),
               "transform_gt": T_gt[:3, :].astype(np.float32), "others": {"seq": drive, "id_src": t0, "id_ref": t1}}
        if self.with_labels:
            out["labels_src"] = pts[0, :, 4].to(torch.int32)       # astype(np.int32): truncation of the voxel mean
            out["labels_ref"] = pts[1, :, 4].to(torch.int32)
        return out


# ================================================================================================== train / val splits
KITTI_TRAIN_SEQUENCES = (0, 1, 2, 3, 4, 5)       # the reference's dataloader/split/train_kitti.txt, val_kitti.txt
KITTI_VAL_SEQUENCES = (6, 7)


class ThreeDMatchTrain:
    """The 3DMatch train / val split as the reference reads it (threeDMatch_loader.py:39-115, :139-159): fragments from
    `<root>/3dmatch_train_val/3DMatch_{split}_0.030_points.pkl` ({id: [n, 3]}), pairs "src@ref" of `..._overlap.pkl` whose
    overlap exceeds 0.3 in the file's order, ground truth the identity (the fragments are stored in a common frame);
    `num_val` > 0 truncates the val split.  Augmentation switches per split as :54-69: val keeps the rotation and drops
    jitter and scale."""

    def __init__(self, root: str, engine, split: str = "train", num_points: int = 18000, num_val: int = -1, voxel_size: float = 0.03,
                 overlap_thres: float = 0.3, positive_pair_radius_multiplier: float = 3.0, reference_gt: bool = False):
        from .augment import AugmentConfig
        if split not in ("train", "val"):
            raise ValueError("ThreeDMatchTrain: split is 'train' or 'val' (the test split is ThreeDMatchTest)")
        self.root_path = os.path.join(root, "3dmatch_train_val")
        pts_fn = os.path.join(self.root_path, f"3DMatch_{split}_0.030_points.pkl")
        ovl_fn = os.path.join(self.root_path, f"3DMatch_{split}_0.030_overlap.pkl")
        for fn in (pts_fn, ovl_fn):
            if not os.path.exists(fn):
                raise FileNotFoundError(fn)
        with open(pts_fn, "rb") as f:
            self.points = pickle.load(f)
        with open(ovl_fn, "rb") as f:
            overlap = pickle.load(f)
        self.engine, self.split, self.voxel_size, self.crop = engine, split, float(voxel_size), None
        self.files = self.select_pairs(overlap, overlap_thres)
        if num_val > 0 and split == "val":
            self.files = self.files[:num_val]
        train = split == "train"
        self.feat_len, self.label_col = 3, None
        self.match_radius = self.voxel_size * float(positive_pair_radius_multiplier)
        self.augment_cfg = AugmentConfig(variant="v1", num_points=int(num_points), random_rotation=True, rotation_range=90.0,
                                         random_jitter=train, jitter_scale=0.005, random_scale=train, min_scale=0.8, max_scale=1.2,
                                         reference_gt=reference_gt)

    @staticmethod
    def select_pairs(overlap: Dict[str, float], thres: float = 0.3) -> List[Tuple[str, str]]:
        """prepare_files (:110-115)."""
        return [tuple(k.split("@")) for k, v in overlap.items() if v > thres]

    def __len__(self):
        return len(self.files)

    def raw(self, index: int):
        """Host part of get_data (:141-159): (src [n, 3], ref [n, 3] float32, pose [4, 4], others)."""
        src_id, ref_id = self.files[index]
        others = {"seq": src_id.split("/")[0], "id_ref": int(ref_id.split("_")[-1]), "id_src": int(src_id.split("_")[-1])}
        return (np.asarray(self.points[src_id], np.float32)[:, :3], np.asarray(self.points[ref_id], np.float32)[:, :3], np.identity(4),
                others)


class KittiOdometryTrain(KittiOdometryTest):
    """KITTI odometry / SemanticKITTI train and val pairs (kitti_loader.py:16-96, :299-346, :384-406).  train: `prepare_kitti`,
    every scan paired with the one MIN_TIME_DIFF = 2 later (time differences range(2, MAX_TIME_DIFF = 3); for drive 1 the
    reference would shorten the range, which its own condition never does with these constants - kept as written).  val: the
    >= 10 m selection of the test split (`KittiOdometryTest.pairs`) on the val sequences.  A sample is both scans cropped and
    voxel-averaged as in the test branch, columns [x, y, z, reflectance, class]; ground truth from the same ICP-refined cache.
    Augmentation (apply_augment_V2): train rotates and jitters, val does neither; neither scales; both permute."""

    MIN_TIME_DIFF, MAX_TIME_DIFF = 2, 3

    def __init__(self, root: str, engine, split: str = "train", sequences: Optional[Sequence[int]] = None, voxel_size: float = 0.3,
                 feat_len: int = 4, num_points: int = 18000, num_val: int = -1, refine_pose: bool = True, with_labels: bool = True,
                 positive_pair_radius_multiplier: float = 3.0, rot_mag: float = 45.0, trans_mag: float = 2.0, xy_rot_scale: float = 0.1):
        from .augment import AugmentConfig
        if split not in ("train", "val"):
            raise ValueError("KittiOdometryTrain: split is 'train' or 'val' (the test split is KittiOdometryTest)")
        if sequences is None:
            sequences = KITTI_TRAIN_SEQUENCES if split == "train" else KITTI_VAL_SEQUENCES
        self.split = split
        if split == "train":
            super().__init__(root, engine, (), voxel_size, feat_len, num_points, 0, refine_pose, with_labels)
            for drive in sequences:
                self.files.extend(self.train_pairs(int(drive), self.scan_ids(int(drive))))
        else:
            super().__init__(root, engine, sequences, voxel_size, feat_len, num_points, 0, refine_pose, with_labels)
            if num_val > 0:
                self.files = self.files[:num_val]
        train = split == "train"
        self.crop = (3.0, 60.0, -3.0, 10.0)
        self.label_col = 4 if self.with_labels else None
        self.match_radius = self.voxel_size * float(positive_pair_radius_multiplier)
        self.augment_cfg = AugmentConfig(variant="v2", num_points=int(num_points), random_rotation=train, random_jitter=train,
                                         random_scale=False, rot_mag=rot_mag, trans_mag=trans_mag, xy_rot_scale=xy_rot_scale)

    @classmethod
    def train_pairs(cls, drive: int, inames: Sequence[int]) -> List[Tuple[int, int, int]]:
        """prepare_kitti (:80-96) for one drive."""
        if drive == 1 and (cls.MAX_TIME_DIFF - 1) > cls.MIN_TIME_DIFF:
            max_time_diff = cls.MAX_TIME_DIFF - 1
        else:
            max_time_diff = cls.MAX_TIME_DIFF
        have, out = set(inames), []
        for start in inames:
            for diff in range(cls.MIN_TIME_DIFF, max_time_diff):
                if start + diff in have:
                    out.append((drive, start, start + diff))
        return out

    def raw(self, index: int):
        """Host part of get_data (:299-346): both scans as [n, 4 | 5] float32 (uncropped: the crop runs with the voxel grid on the
        device), the refined pose [4, 4], others."""
        drive, t0, t1 = self.files[index]
        seq = os.path.join(self.root_path, "sequences", "%02d" % drive)
        scans = [read_velodyne(os.path.join(seq, "velodyne", "%06d.bin" % t)) for t in (t0, t1)]
        c = self.crop

        def crop_host(a):
            r2 = (a[:, :3].astype(np.float64) ** 2).sum(1)
            return a[(r2 <= c[1] ** 2) & (r2 > c[0] ** 2) & (a[:, 2] >= c[2]) & (a[:, 2] <= c[3])]
        M = self.gt_pose(drive, t0, t1, crop_host(scans[0]), crop_host(scans[1]))
        if self.with_labels:
            scans = [np.concatenate([a, read_semantic_labels(os.path.join(seq, "labels", "%06d.label" % t), len(a))[:, None].astype(np.float32)], 1)
                     for a, t in zip(scans, (t0, t1))]
        return scans[0], scans[1], M, {"seq": drive, "id_src": t0, "id_ref": t1}


OXFORD_CROP = (0.0, 50.0, -3.0, 20.0)            # process_point_cloud(r_min, r_max, z_min, z_max) of oxford_loader.py:168-169


def read_oxford_train_list(path: str) -> List[Dict[str, object]]:
    """`train_relative.txt` (oxford_loader.py:62-86): lines `file | positives | non-negatives` -> [{'file', 'pos_list', 'nonneg_list'}];
    a line that does not have three fields is skipped with a log message, as in the reference."""
    out = []
    with open(path, "r") as f:
        for i, line in enumerate(f.readlines()):
            parts = line.split("|")
            if len(parts) != 3:
                _logger.info("Invalid line %d: %s", i, parts)
                continue
            out.append({"file": parts[0].strip(), "pos_list": [int(x) for x in parts[1].split()],
                        "nonneg_list": [int(x) for x in parts[2].split()]})
    return out


class OxfordTrain:
    """The Oxford train split (oxford_loader.py:16-86, :137-153): every line of `<root>/train_np_nofilter/train_relative.txt` is one
    sample, ONE scan `[n, 7]` = [x y z nx ny nz curvature] of which the first `feat_len` columns are kept.  There is no second scan and
    no pose: the pair is the scan cropped twice by random half-spaces keeping `p_crop` of its rows (`self_pair_crop`, which
    `TrainBatches` runs on the device per batch), ground truth the identity, and the augmentation supplies the motion
    (apply_augment_V2 with rotation, jitter and scale 0.8 to 1.2 on, :33-41).  Range crop and voxel grid as :168-175."""

    TRAIN_DIR = "train_np_nofilter"

    def __init__(self, root: str, engine, num_points: int, p_crop: float = 0.6, voxel_size: float = 0.3, feat_len: int = 3,
                 positive_pair_radius_multiplier: float = 3.0, rot_mag: float = 45.0, trans_mag: float = 2.0, xy_rot_scale: float = 0.1,
                 reference_gt: bool = False):
        from .augment import AugmentConfig
        self.root_path = os.path.join(root, self.TRAIN_DIR)
        fn = os.path.join(self.root_path, "train_relative.txt")
        if not os.path.exists(fn):
            raise FileNotFoundError(fn)
        if not (0.0 < float(p_crop) <= 1.0):
            raise ValueError("OxfordTrain: p_crop is a share of the scan, in (0, 1]")
        self.engine, self.split, self.voxel_size, self.crop = engine, "train", float(voxel_size), OXFORD_CROP
        self.files = read_oxford_train_list(fn)
        self.feat_len, self.label_col = max(3, min(int(feat_len), 7)), None
        self.self_pair_crop = float(p_crop)
        self.match_radius = self.voxel_size * float(positive_pair_radius_multiplier)
        self.augment_cfg = AugmentConfig(variant="v2", num_points=int(num_points), random_rotation=True, random_jitter=True,
                                         random_scale=True, min_scale=0.8, max_scale=1.2, rot_mag=rot_mag, trans_mag=trans_mag,
                                         xy_rot_scale=xy_rot_scale, reference_gt=reference_gt)

    def __len__(self):
        return len(self.files)

    def raw(self, index: int) -> np.ndarray:
        """The one scan of a sample, [n, feat_len] float32 (:142-144)."""
        a = np.load(os.path.join(self.root_path, self.files[index]["file"]))
        return np.ascontiguousarray(a[:, :self.feat_len], dtype=np.float32)

    def others(self, index: int) -> Dict[str, object]:
        name = self.files[index]["file"]
        return {"seq": None, "id_src": name, "id_ref": name}


class OxfordTest:
    """The Oxford val / test split (oxford_loader.py:88-94, :155-183): `<root>/test_models_20k_np_nofilter/groundtruths.pkl` is a list
    of dicts with `anc_idx`, `pos_idx`, `t` and `q` = [qw qx qy qz]; src = `<pos_idx>.npy`, ref = `<anc_idx>.npy`, the pose
    `se3.xyzquat2mat`.  No half-space crop; the range crop and voxel grid of the train split; augmentation off and no permutation
    (apply_augment_V2 with fixed=True: the cloud with fewer voxels is tiled to the size of the other, in voxel order), or
    `num_points` rows of each.  `num_val` > 0 truncates the val split.  Yields the dicts `harness.inference_align` takes; with
    `num_points` it is also a dataset `TrainBatches` accepts (`raw`, the validation batches of the training loop)."""

    TEST_DIR = "test_models_20k_np_nofilter"

    def __init__(self, root: str, engine, split: str = "test", num_val: int = -1, voxel_size: float = 0.3, feat_len: int = 3,
                 num_points: Optional[int] = None, positive_pair_radius_multiplier: float = 3.0):
        from .augment import AugmentConfig
        if split not in ("val", "test"):
            raise ValueError("OxfordTest: split is 'val' or 'test' (the train split is OxfordTrain)")
        self.root_path = os.path.join(root, self.TEST_DIR)
        fn = os.path.join(self.root_path, "groundtruths.pkl")
        if not os.path.exists(fn):
            raise FileNotFoundError(fn)
        with open(fn, "rb") as f:
            self.files = list(pickle.load(f))
        if num_val > 0 and split == "val":
            self.files = self.files[:num_val]
        self.engine, self.split, self.voxel_size, self.crop = engine, split, float(voxel_size), OXFORD_CROP
        self.feat_len, self.num_points, self.label_col = max(3, min(int(feat_len), 7)), num_points, None
        self.match_radius = self.voxel_size * float(positive_pair_radius_multiplier)
        self.augment_cfg = AugmentConfig(variant="v2", num_points=int(num_points or 0), random_rotation=False, random_jitter=False,
                                         random_scale=False, permute=False)

    def __len__(self):
        return len(self.files)

    def pose(self, index: int) -> np.ndarray:
        """[4, 4] float64: ref = R src + t (:163-166)."""
        from .se3 import xyzquat2mat
        rec = self.files[index]
        return xyzquat2mat(np.concatenate([np.asarray(rec["t"], np.float64).reshape(3), np.asarray(rec["q"], np.float64).reshape(4)]))

    def raw(self, index: int):
        """Host part of get_data (:155-166): (src [n, feat_len], ref [n', feat_len] float32, pose [4, 4], others)."""
        rec = self.files[index]
        pos, anc = int(rec["pos_idx"]), int(rec["anc_idx"])
        src, ref = (np.ascontiguousarray(np.load(os.path.join(self.root_path, "%d.npy" % i))[:, :self.feat_len], dtype=np.float32)
                    for i in (pos, anc))
        return src, ref, self.pose(index), {"seq": None, "id_src": pos, "id_ref": anc}

    def __getitem__(self, index: int) -> Dict[str, object]:
        src, ref, pose, others = self.raw(index)
        raw = [src, ref]
        vox, counts = self.engine.voxel_downsample([_to_device(self.engine, c) for c in raw], self.voxel_size, self.crop)
        k = int(self.num_points) if self.num_points else int(counts.max().item())
        pts = self.engine.resample(vox, counts, max(k, 1), 0, "fixed")
        return {"points_src": pts[0].contiguous(), "points_ref": pts[1].contiguous(), "transform_gt": pose[:3, :].astype(np.float32),
                "others": others}


class TrainBatches:
    """Device-resident training batches of a train / val dataset above: an iterable with `set_epoch(e)`.

    Per batch: host parsing of the samples not seen before; then on the device the voxel grid (`Engine.voxel_downsample`, every
    new cloud of the batch in ONE ragged call; the voxelised clouds are cached per dataset index, at most `cache_size` samples like
    the reference's cache, so later epochs skip parsing and voxelising), `Engine.augment`, and for `pipeline='align'` the
    reference's `get_matches` on the augmented clouds: `Engine.radius_matches` + `as_reference_matches` with the dataset's radius
    voxel_size * positive_pair_radius_multiplier, or - `match_radius` given - just that radius in the dict, from which
    `Network.train_step` forms the same targets without a list.

    Yields the reference's collate dict (data_base.py:196-219): points_src / points_ref [B, N, feat_len] fp32 and transform_gt
    [B, 3, 4] fp32 on the device, labels_src / labels_ref [B, N] int64 when the dataset has labels, matches (list of B int64
    arrays [n', 2]) or match_radius, others (list of B dicts), plus `invalid` [2, B] int32 (`Engine.augment`).

    A dataset that declares `self_pair_crop = p_keep` (`OxfordTrain`) has ONE scan per sample: the cache then holds the raw scan on
    the device, once per index, and every batch crops it twice by random half-spaces (`Engine.halfspace_crop`, sides src and ref
    keyed by (seed, epoch, index)) in front of the same voxel grid, augmentation and matches; the pose is the identity.

    Every random number comes from (seed, epoch, dataset index): a sample is the same bytes whatever batch it lands in, and the
    epoch's order is a permutation drawn from the same counter RNG (`augment.epoch_order`)."""

    def __init__(self, dataset, batch_size: int, seed: int, shuffle: bool = True, pipeline: str = "align",
                 match_radius: Optional[float] = None, drop_last: bool = True, cache_size: int = 8000):
        self.dataset, self.engine = dataset, dataset.engine
        self.batch_size, self.seed, self.shuffle, self.pipeline = int(batch_size), int(seed), bool(shuffle), pipeline
        self.match_radius, self.drop_last, self.cache_size = match_radius, bool(drop_last), int(cache_size)
        self.epoch = 0
        self.cache: Dict[int, tuple] = {}

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def order(self) -> np.ndarray:
        from .augment import epoch_order
        return epoch_order(self.seed, self.epoch, len(self.dataset), self.shuffle)

    def __iter__(self):
        order = self.order()
        for b in range(len(self)):
            yield self.batch(order[b * self.batch_size:(b + 1) * self.batch_size].tolist())

    def voxels(self, indices: Sequence[int]) -> List[tuple]:
        """(voxels_src [n, C], voxels_ref [n', C] on the device, pose [4, 4], others) of every index, from the cache where present."""
        ds = self.dataset
        new = [i for i in dict.fromkeys(indices) if i not in self.cache]
        fresh = {}
        if new:
            raws = [ds.raw(i) for i in new]
            clouds = [_to_device(self.engine, c) for r in raws for c in r[:2]]
            vox, counts = self.engine.voxel_downsample(clouds, ds.voxel_size, ds.crop)
            n = counts.cpu().tolist()
            for j, i in enumerate(new):
                fresh[i] = (vox[2 * j, :n[2 * j]].clone(), vox[2 * j + 1, :n[2 * j + 1]].clone(), raws[j][2], raws[j][3])
                if len(self.cache) < self.cache_size:
                    self.cache[i] = fresh[i]
        return [self.cache[i] if i in self.cache else fresh[i] for i in indices]

    def assemble(self, items: Sequence[tuple]):
        """Cached ragged clouds -> (voxels [2, B, cap, C], counts [2, B] i32, poses [B, 4, 4]): copies only."""
        B = len(items)
        cap = max(1, max(int(t.shape[0]) for it in items for t in it[:2]))
        vox = torch.zeros((2, B, cap, items[0][0].shape[1]), dtype=torch.float32, device=self.engine.device)
        counts = np.zeros((2, B), np.int32)
        for b, it in enumerate(items):
            for s in (0, 1):
                counts[s, b] = it[s].shape[0]
                vox[s, b, :counts[s, b]] = it[s]
        return vox, torch.from_numpy(counts).to(self.engine.device), np.stack([it[2] for it in items])

    def finish(self, vox, counts, poses, indices, others) -> Dict[str, object]:
        """Voxel tensors -> the finished dict, all on the device."""
        ds = self.dataset
        src, ref, gt, invalid = self.engine.augment(vox[0], counts[0], vox[1], counts[1], poses, ds.augment_cfg, self.seed, self.epoch,
                                                    indices)
        F = int(ds.feat_len)
        out = {"points_src": src[:, :, :F].contiguous() if src.shape[2] != F else src,
               "points_ref": ref[:, :, :F].contiguous() if ref.shape[2] != F else ref, "transform_gt": gt, "others": list(others),
               "invalid": invalid}
        if ds.label_col is not None:
            out["labels_src"] = src[:, :, ds.label_col].to(torch.int64)       # truncation of the voxel mean, then .long()
            out["labels_ref"] = ref[:, :, ds.label_col].to(torch.int64)
        if self.pipeline == "align":
            if self.match_radius is not None:
                out["match_radius"] = float(self.match_radius)
            else:
                from .train import as_reference_matches
                off, cols = self.engine.radius_matches(out["points_src"], out["points_ref"], gt, ds.match_radius)
                out["matches"] = as_reference_matches(off, cols, src.shape[0], src.shape[1])
        return out

    def scans(self, indices: Sequence[int]) -> List[tuple]:
        """self_pair_crop datasets: (scan [n, C] on the device, others) of every index, from the cache where present."""
        ds, fresh = self.dataset, {}
        for i in dict.fromkeys(indices):
            if i not in self.cache:
                fresh[i] = (_to_device(self.engine, ds.raw(i)), ds.others(i))
                if len(self.cache) < self.cache_size:
                    self.cache[i] = fresh[i]
        return [self.cache[i] if i in self.cache else fresh[i] for i in indices]

    def self_pairs(self, indices: Sequence[int]):
        """One scan per sample -> (voxels [2, B, cap, C], counts [2, B] i32, identity poses, others): both half-space crops of every scan
        in ONE call (clouds 0..B-1 the src side, B..2B-1 the ref side), then the ragged voxel grid over the 2 B crops."""
        from .augment import SIDE_REF, SIDE_SRC
        ds, B = self.dataset, len(indices)
        items = self.scans(indices)
        n = [int(it[0].shape[0]) for it in items]
        cap = max(1, max(n))
        raw = torch.zeros((2 * B, cap, items[0][0].shape[1]), dtype=torch.float32, device=self.engine.device)
        for b, it in enumerate(items):
            raw[b, :n[b]] = it[0]
            raw[B + b, :n[b]] = it[0]
        counts = torch.from_numpy(np.asarray(n + n, np.int32)).to(self.engine.device)
        out, kept, _ = self.engine.halfspace_crop(raw, counts, ds.self_pair_crop, self.seed, self.epoch, list(indices) + list(indices),
                                                  [SIDE_SRC] * B + [SIDE_REF] * B)
        m = kept.cpu().tolist()
        vox, vcounts = self.engine.voxel_downsample([out[c, :m[c]] for c in range(2 * B)], ds.voxel_size, ds.crop)
        capv = max(1, int(vcounts.max().item()))
        vox = vox[:, :capv].contiguous().view(2, B, capv, vox.shape[2])
        return vox, vcounts.view(2, B), np.tile(np.identity(4), (B, 1, 1)), [it[1] for it in items]

    def batch(self, indices: Sequence[int]) -> Dict[str, object]:
        if getattr(self.dataset, "self_pair_crop", None) is not None:
            vox, counts, poses, others = self.self_pairs(indices)
            return self.finish(vox, counts, poses, indices, others)
        items = self.voxels(indices)
        vox, counts, poses = self.assemble(items)
        return self.finish(vox, counts, poses, indices, [it[3] for it in items])


# ================================================================================================== 3DMatch train tables
def list_3dmatch_fragments(root: str, split: str) -> Dict[str, List[str]]:
    """The fragments of a 3DMatch download as the reference's preprocessing lists them (dataloader/3DMatch_preprocess.py:32-47):
    scenes in the order of `<root>/scene_list_{split}.txt`, their `seq*` folders sorted, the `*.ply` of a sequence sorted by the
    integer after the last '_' -> {scene: [ids]}, an id being `scene/seq/name` (no extension)."""
    from .overlap import fragment_sort_key
    with open(os.path.join(root, f"scene_list_{split}.txt")) as f:
        scenes = [ln.strip() for ln in f.read().splitlines() if ln.strip()]
    out: Dict[str, List[str]] = {}
    for scene in scenes:
        out[scene] = []
        for seq in sorted(os.listdir(os.path.join(root, scene))):
            if not seq.startswith("seq"):
                continue
            names = [fn.split(".")[0] for fn in os.listdir(os.path.join(root, scene, seq)) if fn.endswith("ply")]
            out[scene] += sorted([f"{scene}/{seq}/{n}" for n in names], key=fragment_sort_key)
    return out


class _EngineSearch:
    """The `overlap.Search` of an engine: one cell index per fragment list (a scene), kept between the count and the fill pass; job
    lists are cut so that no call's job table and neighbour lists exceed `max_jobs_bytes`."""

    def __init__(self, engine, max_jobs_bytes: int):
        self.engine, self.max_jobs_bytes = engine, int(max_jobs_bytes)
        self._frags, self._index = None, None

    def chunks(self, jobs: np.ndarray, sizes: np.ndarray, fill: bool) -> List[Tuple[int, int]]:
        cost = 16 + (4 * sizes[jobs[:, 0]] if fill else np.zeros(len(jobs), np.int64))
        out, start, used = [], 0, 0
        for k, c in enumerate(cost.tolist()):
            if k > start and used + c > self.max_jobs_bytes:
                out.append((start, k))
                start, used = k, 0
            used += c
        if len(jobs) > start:
            out.append((start, len(jobs)))
        return out

    def __call__(self, fragments: List[np.ndarray], jobs: np.ndarray, radius: float, fill: bool):
        if self._frags is not fragments:
            sizes = np.array([len(f) for f in fragments], np.int64)
            host = np.concatenate([np.asarray(f, np.float32).reshape(-1, 3) for f in fragments])
            ok = np.isfinite(host).all(1)
            bounds = np.concatenate([host[ok].min(0), host[ok].max(0)]) if ok.any() else np.zeros(6, np.float32)
            self._index = self.engine.nn_index(_to_device(self.engine, host), np.concatenate([[0], np.cumsum(sizes)]), radius, bounds)
            self._frags, self._sizes = fragments, sizes
        jobs = np.asarray(jobs, np.int32).reshape(-1, 2)
        counts, lists = [], []
        for a, b in self.chunks(jobs, self._sizes, fill):
            c, flat = self._index.search(jobs[a:b], fill=fill)
            counts.append(c.cpu().numpy())
            if fill:
                rows, flat = self._index.rows(jobs[a:b]), flat.cpu().numpy()
                lists += [flat[rows[k]:rows[k + 1]] for k in range(b - a)]
        return (np.concatenate(counts) if counts else np.zeros(0, np.int32)), (lists if fill else None)


def preprocess_3dmatch(root: str, savepath: str, split: str, engine, downsample: float = 0.03, overlap_thres: float = 0.30,
                       max_jobs_bytes: int = 1 << 28, batch: int = 16):
    """dataloader/3DMatch_preprocess.py on the device: writes `3DMatch_{split}_{downsample:.3f}_points.pkl` ({id: float64 [n, 3]}:
    every fragment read with `read_ply_xyz`, thinned by `Engine.voxel_downsample` - the engine's voxel rule -, then moved by
    `<id>.pose.npy` in float64 on the host), `_overlap.pkl` ({"src@ref": ratio}) and `_keypts.pkl` ({"src@ref": int32 [m, 2]}) under
    `savepath`, the last two for the pairs i < j of a scene whose share of src points with a ref point closer than `downsample`
    (`Engine.nn_index` on the float32 cast: csrc/overlap.hip) exceeds `overlap_thres`.  Existing files are reloaded, not recomputed.
    `ThreeDMatchTrain(root_of(savepath), engine)` and the reference's loader read what it wrote when `savepath` is
    `<root>/3dmatch_train_val`.  -> (points, overlap, keypts)."""
    from .overlap import write_3dmatch_tables

    def load_points(ids: List[str]) -> Dict[str, np.ndarray]:
        pts: Dict[str, np.ndarray] = {}
        for s in range(0, len(ids), batch):
            part = ids[s:s + batch]
            vox = _voxelize(engine, [read_ply_xyz(os.path.join(root, i + ".ply")) for i in part], float(downsample))
            for i, v in zip(part, vox):
                M = np.load(os.path.join(root, i + ".pose.npy")).astype(np.float64)
                pts[i] = v[:, :3].cpu().numpy().astype(np.float64) @ M[:3, :3].T + M[:3, 3]
        return pts

    return write_3dmatch_tables(savepath, split, float(downsample), list_3dmatch_fragments(root, split), load_points,
                                _EngineSearch(engine, max_jobs_bytes), overlap_thres)
