"""Evaluation harness: the caller contract of the reference's
``test.py::inference_align`` (test.py:358-457) around the accelerated model.

Same iteration order, ``opt = (num_reg_iter, True)``, the last transform
duplicated as the "pose_optimized" entry (pose_optimization is the identity in
the reference, test.py:209-216), and one stats row ``[succ, rte, rre, time, seq]``
per pair (test.py:432-441).  Differences, both deliberate:

* pairs are taken ``batch`` at a time (the reference hard-codes batch 1,
  test.py:56) — the per-pair time is the batch time divided by its size;
* pairs shard across ranks (``deepsir_amd.dist``), results are gathered once.
"""
from __future__ import annotations

import time
from typing import Callable, Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from .dist import gather_results, shard_range, shard_sizes
from .metrics import THRESHOLDS, rte_rre


@torch.no_grad()
def inference_align(pairs: Sequence[Dict[str, np.ndarray]], model, num_reg_iter: int = 5, dataset_type: str = "3DMatch",
                    batch: int = 1, device: Optional[torch.device] = None, dist=None, pose_opt: Optional[str] = None,
                    voxel_size: float = 0.3, in_flight: int = 1, safeguard_wsum: Optional[float] = None,
                    ransac_hypotheses: int = 80000, ransac_seed: int = 0, icp_search: str = "auto", icp_kernel: str = "l2",
                    icp_kernel_scale: Optional[float] = None, ndt_resolution: Optional[float] = None):
    """pairs: sequence of dicts with ``points_src/points_ref [1,N,C]``, ``transform_gt [1,3,4]`` and optionally the
    pyramid tensors and ``others`` (as the reference's collate, data_base.py:196-219).
    ``in_flight`` > 1: the reference's one-pair-per-call loop fed AHEAD - the pairs go one by one to a
    ``deepsir_amd.serve.PairServer`` that keeps that many requests outstanding (same results bit for bit; the per-pair
    time is then the shard's wall time divided by its size).
    ``pose_opt='icp'`` / ``'icp_plane'``: ICP on the raw clouds from the last pose, point-to-point / point-to-plane;
    ``icp_search`` is ``Engine.icp_refine``'s ``search`` ("auto": the cell index on large clouds; the poses are the same bytes),
    ``icp_kernel`` / ``icp_kernel_scale`` its robust ``kernel`` and ``kernel_scale`` (open3d's ``robust_kernel``; "l2": none).
    ``pose_opt='ndt'``: NDT registration on the raw clouds from the last pose (``Engine.ndt_refine``: no search, no normals);
    ``ndt_resolution`` is its cell edge, by default 4 x ``voxel_size`` - a choice (a cell of a voxel grid then holds tens of
    points), not a tuned value.
    ``pose_opt='ransac'``: DGR's safeguard (network/DGR.py:249-306) over the last iteration's correspondences, see below;
    ``pose_opt='consensus'``: the same correspondences through ``consensus_correspondence`` instead of the seeded sampling;
    ``pose_opt='fgr'``: through ``fgr_correspondence`` (fast global registration; ``ransac_seed`` keys its tuple draws);
    ``safeguard_wsum``: only pairs whose summed sigmoid inlier weight is below it take the RANSAC pose (DGR.py:273-304).
    Returns (pred_transforms_all [n_pairs, n_iter+1, 3, 4], stats [n_pairs, 5]) gathered over ranks."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    rte_t, rre_t = THRESHOLDS[dataset_type]
    world = dist.get_world_size() if dist is not None and dist.is_initialized() else 1
    rank = dist.get_rank() if world > 1 else 0
    mine = list(shard_range(len(pairs), rank, world))
    preds: List[np.ndarray] = []
    stats = np.zeros((len(mine), 5))
    opt = (num_reg_iter, True)
    if in_flight > 1:
        if pose_opt is not None:
            raise ValueError("in_flight > 1 serves the registration alone (pose_opt must be None)")
        if any(k.endswith("_neigh_idx") for i in mine for k in pairs[i]):
            # the served path builds the KNN pyramid on the device; a loader's own pyramid (whose tie rule may differ) is honoured by
            # the one-pair-per-call path only - say so instead of silently diverging from in_flight=1
            raise ValueError("in_flight > 1 recomputes the KNN pyramid on the device: pairs that carry their own pyramid tensors "
                             "must be evaluated with in_flight=1 (or have the pyramid keys removed)")
        keys = ("points_src", "points_ref", "transform_gt")
        datas = [_stack([{k: v for k, v in pairs[i].items() if k in keys}], [0], device) for i in mine]
        n_max = max([max(d["points_src"].shape[1], d["points_ref"].shape[1]) for d in datas], default=1024)
        srv = model.serve(max_points=n_max, max_in_flight=in_flight, n_iter=num_reg_iter, want_aux=False)
        torch.cuda.synchronize(device)
        t0 = time.time()
        res = srv.run_closed_loop(((d["points_src"].float(), d["points_ref"].float()) for d in datas), in_flight)
        torch.cuda.synchronize(device)
        dt = (time.time() - t0) / max(len(mine), 1)
        srv.close()
        for row, (i, d, r) in enumerate(zip(mine, datas, res)):
            T = r["transforms"].cpu().numpy()
            preds.append(np.concatenate([T, T[-1:]], 0)[None])            # pose_optimization == identity (test.py:215-216)
            stats[row, :3] = rte_rre(T[-1], d["transform_gt"].cpu().numpy()[0], rte_t, rre_t)
            stats[row, 3] = dt
            others = pairs[i].get("others")
            stats[row, 4] = _seq_id(others[0]["seq"]) if others else -1
        mine_batches = range(0)
    else:
        mine_batches = range(0, len(mine), batch)
    for b0 in mine_batches:
        ids = mine[b0:b0 + batch]
        data = _stack(pairs, ids, device)
        torch.cuda.synchronize(device)
        t0 = time.time()
        transforms, endpoints = model(data, opt)
        torch.cuda.synchronize(device)
        dt = (time.time() - t0) / len(ids)
        if pose_opt == "icp":
            # pose_optimization with use_icp (test.py:241-258; off in the reference): point-to-point ICP on the raw clouds,
            # correspondence radius 2 x voxel size (test.py:219), open3d's default criteria
            T_opt, _ = _aux_engine(model, data).icp_refine(data["points_src"].float(), data["points_ref"].float(),
                                                transforms[-1].contiguous(), 2.0 * voxel_size, search=icp_search,
                                                kernel=icp_kernel, kernel_scale=icp_kernel_scale)
            transforms.append(T_opt)
        elif pose_opt == "icp_plane":
            # the same refinement with the point-to-plane estimator (open3d's TransformationEstimationPointToPlane; include/dsir.h,
            # dsir_icp_refine_ex), same radius; the normals are those of use_ppf rows where the data has them, else estimated from
            # the reference cloud's level-0 neighbour lists
            T_opt, _ = _aux_engine(model, data).icp_refine(data["points_src"].float(), data["points_ref"].float(),
                                                           transforms[-1].contiguous(), 2.0 * voxel_size, estimator="plane",
                                                           search=icp_search, kernel=icp_kernel, kernel_scale=icp_kernel_scale)
            transforms.append(T_opt)
        elif pose_opt == "ndt":
            # the correspondence-free refinement (csrc/ndt.hip): one Gaussian per cell of the reference cloud, cell edge 4 x voxel size
            T_opt, _ = _aux_engine(model, data).ndt_refine(data["points_src"].float(), data["points_ref"].float(), transforms[-1].contiguous(),
                                                           float(ndt_resolution) if ndt_resolution is not None else 4.0 * voxel_size)
            transforms.append(T_opt)
        elif pose_opt == "tune":
            # pose_optimization with use_tune (test.py:218-239; off in the reference): Adam fine-tune of the 6-D-rotation
            # pose on the last iteration's correspondences, weights = sigmoid of its inlier logits, distances in units
            # of 2 x voxel size (test.py:219, :238)
            T_opt, _ = _aux_engine(model, data).pose_finetune(endpoints["pt_src"].float(), endpoints["pt_ref_new"].float(),
                                                   transforms[-1].contiguous(), weights=endpoints["perm_matrices"][-1],
                                                   weights_are_logits=True, quantization_size=2.0 * voxel_size)
            transforms.append(T_opt)
        elif pose_opt in ("ransac", "consensus", "fgr"):
            # DGR.safeguard_registration (network/DGR.py:249-306): RANSAC over the last iteration's correspondences (row i of pt_src
            # with row i of pt_ref_new), threshold 2 x voxel size, DGR's 80 000 hypotheses by default; with safeguard_wsum only the
            # pairs whose inlier network assigned less total weight than that take it, the others keep the network's pose
            xs, xr = endpoints["pt_src"].float().contiguous(), endpoints["pt_ref_new"].float().contiguous()
            m = xs.shape[1]
            corr = torch.arange(m, dtype=torch.int32, device=xs.device)[None, :, None].expand(xs.shape[0], m, 2).contiguous()
            T_net = transforms[-1].contiguous()
            # 'consensus' (csrc/consensus.hip) takes neither keyword: no sampling, no seed; for 'fgr' (csrc/fgr.hip) the seed keys its tuples
            T_opt = _pose_from_corr(_aux_engine(model, data), pose_opt, xs, xr, corr, None, 2.0 * voxel_size, T_init=T_net,
                                    hypotheses=ransac_hypotheses, seed=ransac_seed)
            if safeguard_wsum is not None:
                wsum = torch.sigmoid(endpoints["perm_matrices"][-1].float()).reshape(xs.shape[0], -1).sum(1)
                T_opt = torch.where((wsum < safeguard_wsum)[:, None, None], T_opt, T_net)
            transforms.append(T_opt)
        elif pose_opt is None:
            transforms.append(transforms[-1].detach())        # pose_optimization == identity (test.py:215-216, :406-408)
        else:
            raise ValueError("pose_opt must be None, 'icp', 'icp_plane', 'ndt', 'tune', 'ransac', 'consensus' or 'fgr'")
        T = torch.stack(transforms, dim=1).cpu().numpy()      # [B, n_iter+1, 3, 4]
        preds.append(T)
        gt = data["transform_gt"].cpu().numpy()
        for j, i in enumerate(ids):
            row = b0 + j
            stats[row, :3] = rte_rre(T[j, -1], gt[j], rte_t, rre_t)
            stats[row, 3] = dt
            others = pairs[i].get("others")
            stats[row, 4] = _seq_id(others[0]["seq"]) if others else -1
    pred = np.concatenate(preds, 0) if preds else np.zeros((0, num_reg_iter + 1, 3, 4), np.float32)
    if world > 1:
        sizes = shard_sizes(len(pairs), world)
        pred = gather_results(torch.from_numpy(pred).to(device), dist, sizes).cpu().numpy()
        stats = gather_results(torch.from_numpy(stats).to(device), dist, sizes).cpu().numpy()
    return pred, stats


def _aux_engine(model, data):
    """The plain engine behind the drop-in model for the operators next to the path (ICP, fine-tune): ``forward`` may have run on
    the model's server or pool instead."""
    n = max(int(data["points_src"].shape[1]), int(data["points_ref"].shape[1]))
    return model._ensure_engine(n, int(data["points_src"].shape[0]))


def summarize(stats: np.ndarray) -> Dict[str, float]:
    """Aggregate as the reference's print_stats: recall, mean RTE/RRE over successes, mean time."""
    ok = stats[:, 0] > 0
    return {
        "recall": float(ok.mean()) if len(stats) else 0.0,
        "rte_mean": float(stats[ok, 1].mean()) if ok.any() else float("nan"),
        "rre_mean": float(stats[ok, 2].mean()) if ok.any() else float("nan"),
        "time_mean": float(stats[:, 3].mean()) if len(stats) else 0.0,
        "pairs_per_sec": float(1.0 / stats[:, 3].mean()) if len(stats) and stats[:, 3].mean() > 0 else 0.0,
    }


@torch.no_grad()
def evaluate_align(pred_transforms: np.ndarray, pairs: Sequence[Dict[str, np.ndarray]], engine, dataset_type: str = "3DMatch",
                   batch: int = 64, device: Optional[torch.device] = None):
    """Counterpart of the reference's ``test.py::evaluate_align`` (test.py:308-355): per registration
    iteration, the metrics of ``compute_metrics`` (common/metrics_util.py:27-85) on the first 1024 points of
    each cloud (test.py:331-332), computed on device by ``dsir_eval_metrics``.

    pred_transforms [n_pairs, n_iter(+1), 3, 4]; pairs as for ``inference_align``; ``engine`` a
    ``deepsir_amd.engine.Engine``.  Returns (metrics_for_iter: list of dicts of arrays, summary of the last iteration)."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    rte_t, rre_t = THRESHOLDS[dataset_type]
    pred = torch.from_numpy(np.ascontiguousarray(pred_transforms, dtype=np.float32)).to(device)
    if pred.dim() == 3:
        pred = pred[:, None]
    n_it = pred.shape[1]
    acc = [dict((k, []) for k in engine.METRIC_NAMES) for _ in range(n_it)]
    for b0 in range(0, len(pairs), batch):
        ids = range(b0, min(len(pairs), b0 + batch))
        def head(k):   # numpy (reference collate) or device tensors (deepsir_amd.data)
            return torch.cat([torch.as_tensor(pairs[i][k][:, :1024]).to(device) for i in ids], 0).float().contiguous()
        src, ref = head("points_src"), head("points_ref")
        gt = torch.cat([torch.as_tensor(pairs[i]["transform_gt"]).to(device) for i in ids], 0).float()
        for it in range(n_it):
            m = engine.eval_metrics(pred[b0:b0 + len(ids), it], gt, src, ref, rte_t, rre_t)
            for k, v in m.items():
                acc[it][k].append(v.cpu().numpy())
    metrics_for_iter = [{k: np.concatenate(v) for k, v in a.items()} for a in acc]
    return metrics_for_iter, summarize_metrics(metrics_for_iter[-1])


def summarize_metrics(metrics: Dict[str, np.ndarray]) -> Dict[str, float]:
    """Mean over instances with the reference's naming (common/metrics_util.py:88-101):
    ``*mse`` -> ``*rmse``; ``err_*`` -> ``_mean`` and ``_rmse``; everything else -> mean."""
    out = {}
    for k, v in metrics.items():
        if k.endswith("mse"):
            out[k[:-3] + "rmse"] = float(np.sqrt(np.mean(v)))
        elif k.startswith("err"):
            out[k + "_mean"] = float(np.mean(v))
            out[k + "_rmse"] = float(np.sqrt(np.mean(v ** 2)))
        else:
            out[k] = float(np.mean(v))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# 'feat' / 'label' pipelines (reference test.py:460-567): the caller side of Network.forward = forward_pair
class SemanticMetric:
    """Running semantic-segmentation statistics of the reference's ``SemanticLoss`` (network/loss.py:854-992):
    label 0 ('unlabeled') is ignored, label l > 0 is class l-1; per-class IoU = TP / (GT + P - TP) (0 for an absent
    class), mean IoU over all ``num_classes``, overall accuracy, and the inverse-frequency weighted cross entropy
    (class weights 1 / (freq + 0.02) from the SemanticKITTI point counts, loss.py:905-911)."""

    NUM_PER_CLASS = np.array([55437630, 320797, 541736, 2578735, 3274484, 552662, 184064, 78858, 240942562, 17294618,
                              170599734, 6369672, 230413074, 101130274, 476491114, 9833174, 129609852, 4506626, 1168181],
                             dtype=np.float64)

    def __init__(self, num_classes: int = 19):
        self.num_classes = num_classes
        w = self.NUM_PER_CLASS / self.NUM_PER_CLASS.sum()
        self.class_weights = (1.0 / (w + 0.02)).astype(np.float32)
        self.reset()

    def reset(self):
        self.gt = np.zeros(self.num_classes, np.int64)
        self.pos = np.zeros(self.num_classes, np.int64)
        self.tp = np.zeros(self.num_classes, np.int64)
        self.correct = 0
        self.seen = 0

    def add(self, logits: torch.Tensor, labels: torch.Tensor):
        """logits [B, num_classes, N], labels [B, N] (0 = ignored).  Returns (weighted CE loss, accuracy) of this
        batch (loss.py:929-958) and accumulates the confusion counts (:960-971)."""
        lg = logits.transpose(1, 2).reshape(-1, self.num_classes).float()
        lb = labels.reshape(-1).long()
        valid = lb != 0
        lg, lb = lg[valid], lb[valid] - 1
        if lb.numel() == 0:
            return float("nan"), float("nan")
        w = torch.from_numpy(self.class_weights).to(lg.device)
        loss = torch.nn.functional.cross_entropy(lg, lb, weight=w, reduction="mean")
        pred = lg.max(dim=1)[1]
        acc = (pred == lb).sum().float() / float(lb.shape[0])
        conf = torch.bincount(lb * self.num_classes + pred, minlength=self.num_classes ** 2)
        conf = conf.reshape(self.num_classes, self.num_classes).cpu().numpy()
        self.gt += conf.sum(1)
        self.pos += conf.sum(0)
        self.tp += np.diagonal(conf)
        self.correct += int((pred == lb).sum())
        self.seen += int(lb.numel())
        return float(loss), float(acc)

    def result(self):
        """(mean IoU, per-class IoU list, mean accuracy); resets like the reference (loss.py:973-987)."""
        denom = (self.gt + self.pos - self.tp).astype(np.float64)
        iou = np.where(denom != 0, self.tp / np.where(denom != 0, denom, 1.0), 0.0)
        out = float(iou.sum() / self.num_classes), [float(x) for x in iou], self.correct / float(max(self.seen, 1))
        self.reset()
        return out


def _stack(pairs, ids, device):
    """Batch the array entries of the pair dicts `ids` on the device: numpy (the reference's collate output) or torch
    tensors (deepsir_amd.data: already resident), each with a leading batch dimension of 1."""
    out = {}
    for k, v in pairs[ids[0]].items():
        if k == "others":
            continue
        if isinstance(v, np.ndarray):
            out[k] = torch.from_numpy(np.concatenate([pairs[i][k] for i in ids], 0)).to(device)
        elif isinstance(v, torch.Tensor):
            out[k] = torch.cat([pairs[i][k].to(device) for i in ids], 0)
    return out


_SEQ_IDS: Dict[str, int] = {}


def _seq_id(seq) -> float:
    """The sequence column of the stats table (test.py:439) is numeric; scene NAMES (3DMatch) get a running index."""
    try:
        return float(seq)
    except (TypeError, ValueError):
        return float(_SEQ_IDS.setdefault(str(seq), len(_SEQ_IDS)))


def _pair_batches(pairs, batch, device):
    for b0 in range(0, len(pairs), batch):
        ids = list(range(b0, min(b0 + batch, len(pairs))))
        yield ids, _stack(pairs, ids, device)


@torch.no_grad()
def inference_feat(pairs: Sequence[Dict[str, np.ndarray]], model, batch: int = 1, device: Optional[torch.device] = None):
    """test.py::inference_feat (:460-505): key points + saliency per cloud.  Returns a list (one entry per pair) of
    {'pt_src' [M,3], 'score_src' [M], 'feat_src' [M,64], ... same for ref} as numpy, and the total model time."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    out, total = [], 0.0
    for ids, data in _pair_batches(pairs, batch, device):
        torch.cuda.synchronize(device)
        t0 = time.time()
        _, ep = model(data)
        torch.cuda.synchronize(device)
        total += time.time() - t0
        for j in range(len(ids)):
            rec = {}
            for s in ("src", "ref"):
                rec[f"pt_{s}"] = ep[f"pt_{s}"][j].t().cpu().numpy()
                rec[f"feat_{s}"] = ep[f"feat_{s}"][j].t().cpu().numpy()
                rec[f"score_{s}"] = ep[f"score_{s}"][j].cpu().numpy()
            out.append(rec)
    return out, total


# pose name -> (Engine method, the harness keywords it takes; the harness's fgr_iterations is the method's `iterations`)
_POSES = {"ransac": ("ransac_correspondence", ("ransac_n", "edge_sim", "hypotheses", "refine_iters", "seed")),
          "consensus": ("consensus_correspondence", ("seeds", "members", "refine_iters")),
          "fgr": ("fgr_correspondence", ("tuple_test", "tuple_scale", "max_tuples", "fgr_iterations", "refine_iters", "seed"))}


def _pose_from_corr(eng, pose, xs, xr, corr, counts, max_dist, T_init=None, **opts):
    """The pose stage of ``register_feat`` / ``register_fpfh`` / ``inference_align``: 'ransac' (seeded sampling), 'consensus' (spatial
    compatibility) or 'fgr' (tuple pre-filter and graduated Gauss-Newton).  Of ``opts`` the estimator takes the keywords it knows."""
    if pose not in _POSES:
        raise ValueError("pose must be 'ransac', 'consensus' or 'fgr'")
    method, names = _POSES[pose]
    kw = {("iterations" if k == "fgr_iterations" else k): v for k, v in opts.items() if k in names}
    return getattr(eng, method)(xs, xr, corr, max_dist, counts=counts, T_init=T_init, **kw)[0]


@torch.no_grad()
def register_feat(pairs: Sequence[Dict[str, np.ndarray]], model, voxel_size: float = 0.3, hypotheses: int = 8192, mutual: bool = True,
                  num_reg: int = 1, dataset_type: str = "3DMatch", batch: int = 1, device: Optional[torch.device] = None,
                  ransac_n: int = 3, edge_sim: float = 0.9, refine_iters: int = 2, seed: int = 0, pose: str = "ransac",
                  seeds: int = 64, members: int = 32, match_k: int = 1, match_ratio: float = 0.0, fgr_iterations: int = 64,
                  tuple_scale: float = 0.95, max_tuples: int = 1000, tuple_test: bool = True):
    """The 'feat' pipeline as a registration (what the reference reaches through open3d's
    registration_ransac_based_on_feature_matching, network/DGR.py:7-24, test.py:259-263): forward_pair -> key points and
    descriptors -> (mutual) nearest-neighbour correspondences -> RANSAC pose (threshold 2 x voxel size), all on the device.
    ``pose='consensus'``: the pose from ``consensus_correspondence`` (``seeds``, ``members``; no sampling, no seed) instead.
    ``pose='fgr'``: the pose from ``fgr_correspondence`` (``fgr_iterations``, ``tuple_scale``, ``max_tuples``, ``tuple_test``; ``seed``
    keys its tuple draws) instead.
    ``match_k`` > 1: the k nearest descriptors of every src point as candidates (M = J x match_k rows for the pose stage);
    ``match_ratio`` in (0, 1): Lowe's ratio test on the 1-NN set (``Engine.feature_correspondences``).
    Returns (pred_transforms [n_pairs, num_reg, 3, 4] - the one pose repeated ``num_reg`` times, so that the result has
    ``inference_align``'s layout and ``evaluate_align`` works on it -, stats [n_pairs, 5] rows ``[succ, rte, rre, time, seq]``)."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    rte_t, rre_t = THRESHOLDS[dataset_type]
    preds, stats = [], np.zeros((len(pairs), 5))
    for ids, data in _pair_batches(pairs, batch, device):
        torch.cuda.synchronize(device)
        t0 = time.time()
        _, ep = model(data)
        eng = _aux_engine(model, data)
        xs, xr = ep["pt_src"].permute(0, 2, 1).contiguous(), ep["pt_ref"].permute(0, 2, 1).contiguous()
        corr, counts = eng.feature_correspondences(ep["feat_src"].permute(0, 2, 1).contiguous(), ep["feat_ref"].permute(0, 2, 1).contiguous(),
                                                   mutual=mutual, k=match_k, ratio=match_ratio)
        T = _pose_from_corr(eng, pose, xs, xr, corr, counts, 2.0 * voxel_size, ransac_n=ransac_n, edge_sim=edge_sim, hypotheses=hypotheses,
                            refine_iters=refine_iters, seed=seed, seeds=seeds, members=members, fgr_iterations=fgr_iterations,
                            tuple_scale=tuple_scale, max_tuples=max_tuples, tuple_test=tuple_test)
        torch.cuda.synchronize(device)
        dt = (time.time() - t0) / len(ids)
        T = T.cpu().numpy()
        preds.append(np.repeat(T[:, None], num_reg, 1))
        gt = data["transform_gt"].cpu().numpy() if "transform_gt" in data else None
        for j, i in enumerate(ids):
            if gt is not None:
                stats[i, :3] = rte_rre(T[j], gt[j], rte_t, rre_t)
            stats[i, 3] = dt
            others = pairs[i].get("others")
            stats[i, 4] = _seq_id(others[0]["seq"]) if others else -1
    pred = np.concatenate(preds, 0) if preds else np.zeros((0, num_reg, 3, 4), np.float32)
    return pred, stats


def csr_of_cloud(csr, b: int, n: int, bounds=None):
    """Cloud b's rows of a batch CSR (offsets [B n + 1], cloud-local cols) as a CSR of its own: (offsets [n + 1] from 0, cols).
    ``bounds``: offsets[::n] on the host, when the caller has read them once for all clouds."""
    off, cols = csr
    lo, hi = (int(off[b * n]), int(off[(b + 1) * n])) if bounds is None else (int(bounds[b]), int(bounds[b + 1]))
    return (off[b * n:(b + 1) * n + 1] - lo).contiguous(), cols[lo:hi].contiguous()


def _fpfh_side(engine, pts, viewpoints, radius, search="brute", max_nn=0, normal_radius=None, normal_max_nn=0):
    """One side of a batch for ``register_fpfh``: pts [B, N, C] -> (desc [B, N, 64], flags [B, N], normals [B, N, 3])."""
    def normals_of(neigh_multi=None, csr=None):
        if all(v == viewpoints[0] for v in viewpoints):
            return engine.estimate_normals(pts, neigh_multi, viewpoints[0], csr=csr)[0]
        # one viewpoint per call; clouds are independent bit for bit, so per-cloud calls change nothing
        B, n = pts.shape[:2]
        if csr is None:
            return torch.cat([engine.estimate_normals(pts[b:b + 1], neigh_multi[b:b + 1], viewpoints[b])[0] for b in range(B)], 0)
        bounds = csr[0][::n].cpu().numpy()                          # one read for all clouds
        return torch.cat([engine.estimate_normals(pts[b:b + 1], viewpoint=viewpoints[b], csr=csr_of_cloud(csr, b, n, bounds))[0]
                          for b in range(B)], 0)

    neigh = None
    if normal_radius is None or radius is None:
        _, neigh, _, _ = engine.knn_pyramid(pts)
    if normal_radius is None:
        normals = normals_of(neigh_multi=neigh)
    else:
        normals = normals_of(csr=engine.radius_neighbors(pts, float(normal_radius), int(normal_max_nn)))
    if radius is None:
        desc, flags = engine.fpfh(pts, normals, neigh_multi=neigh)
    elif search == "grid":
        desc, flags = engine.fpfh(pts, normals, csr=engine.radius_neighbors(pts, float(radius), int(max_nn)))
    else:
        eye = torch.eye(3, 4, device=pts.device).repeat(pts.shape[0], 1, 1).contiguous()
        desc, flags = engine.fpfh(pts, normals, csr=engine.radius_matches(pts, pts, eye, float(radius)))
    return desc, flags, normals


def _register_one_pair(engine, xs, xr, ds, dr, j, sel, pose, max_dist, match_kw, pose_kw):
    """Pair j of a batch matched and solved alone (a batch of ONE pair) on the rows ``sel`` = (idx_src, idx_ref), int32 device
    tensors of original point indices, or None for all rows -> (T [1, 3, 4], corr [count, 2] int32 numpy in ORIGINAL point indices,
    (idx_src, idx_ref) as numpy)."""
    if sel is None:
        sel = [torch.arange(x.shape[1], dtype=torch.int32, device=x.device) for x in (xs, xr)]
        px, pr, qs, qr = xs[j:j + 1].contiguous(), xr[j:j + 1].contiguous(), ds[j:j + 1].contiguous(), dr[j:j + 1].contiguous()
    else:
        rows_s, rows_r = sel[0].long(), sel[1].long()
        px, pr = xs[j, rows_s][None].contiguous(), xr[j, rows_r][None].contiguous()
        qs, qr = ds[j, rows_s][None].contiguous(), dr[j, rows_r][None].contiguous()
    corr, counts = engine.feature_correspondences(qs, qr, **match_kw)
    T = _pose_from_corr(engine, pose, px, pr, corr, counts, max_dist, **pose_kw)
    cc = corr[0, :int(counts[0])].long()
    orig = torch.stack([sel[0][cc[:, 0]], sel[1][cc[:, 1]]], 1).to(torch.int32).cpu().numpy().reshape(-1, 2)
    return T, orig, (sel[0].cpu().numpy(), sel[1].cpu().numpy())


def _register_on_keypoints(engine, xs, xr, ds, dr, iss_kw, min_keypoints, pose, max_dist, match_kw, pose_kw):
    """The matching and pose stages of ``register_fpfh(keypoints="iss")`` for one batch: xs / xr [B, N, C] points, ds / dr [B, N, 64]
    descriptors of every point.  One ``iss_keypoints`` call per side, then per pair the gather of the keypoint rows (all rows where
    either side has fewer than ``min_keypoints``) and one-pair calls of ``feature_correspondences`` and the pose stage.
    -> (T [B, 3, 4], per pair corr [count, 2] int32 numpy in ORIGINAL point indices, per pair (idx_src, idx_ref, fell_back))."""
    sides = []
    for x in (xs, xr):
        index, counts, _, _ = engine.iss_keypoints(x, **iss_kw)
        sides.append((index, counts.cpu().numpy()))
    Ts, corrs, kpts = [], [], []
    for j in range(xs.shape[0]):
        ks, kr = int(sides[0][1][j]), int(sides[1][1][j])
        fell_back = ks < min_keypoints or kr < min_keypoints
        sel = None if fell_back else [sides[0][0][j, :ks], sides[1][0][j, :kr]]
        T, corr, idx = _register_one_pair(engine, xs, xr, ds, dr, j, sel, pose, max_dist, match_kw, pose_kw)
        Ts.append(T)
        corrs.append(corr)
        kpts.append(idx + (bool(fell_back),))
    return torch.cat(Ts, 0), corrs, kpts


def _register_on_fps(engine, xs, xr, ds, dr, num_keypoints, min_keypoints, pose, max_dist, match_kw, pose_kw):
    """The matching and pose stages of ``register_fpfh(keypoints="fps")`` for one batch (arguments and result as
    ``_register_on_keypoints``).  One ``farthest_point_sample`` call per side on the whole batch; the pairs that got exactly
    ``num_keypoints`` rows on both sides are gathered to [F, num_keypoints, .] and go through ONE ``feature_correspondences`` call and
    ONE pose call.  A pair with fewer than ``min_keypoints`` sampled rows on a side, or of clouds smaller than ``num_keypoints``,
    falls back to all of its points; a pair in between (non-finite rows left fewer than ``num_keypoints`` candidates) keeps its
    shorter lists.  Both go through the one-pair path."""
    B, k = xs.shape[0], int(num_keypoints)
    if min(xs.shape[1], xr.shape[1]) < k:
        index, cs, cr = None, np.zeros(B, np.int64), np.zeros(B, np.int64)            # every pair of this batch falls back
    else:
        sides = [engine.farthest_point_sample(x, k) for x in (xs, xr)]
        index, cs, cr = (sides[0][0], sides[1][0]), sides[0][1].cpu().numpy(), sides[1][1].cpu().numpy()
    fell_back = (cs < min_keypoints) | (cr < min_keypoints)
    full = [j for j in range(B) if not fell_back[j] and cs[j] == k and cr[j] == k]
    Ts, corrs, kpts = [None] * B, [None] * B, [None] * B
    if full:
        at = torch.tensor(full, dtype=torch.long, device=xs.device)
        rows_s, rows_r = index[0][at].long(), index[1][at].long()
        pick = torch.arange(len(full), device=xs.device)[:, None]
        px, pr = xs[at][pick, rows_s].contiguous(), xr[at][pick, rows_r].contiguous()
        qs, qr = ds[at][pick, rows_s].contiguous(), dr[at][pick, rows_r].contiguous()
        corr, counts = engine.feature_correspondences(qs, qr, **match_kw)
        T = _pose_from_corr(engine, pose, px, pr, corr, counts, max_dist, **pose_kw)
        orig = torch.stack([torch.gather(rows_s, 1, corr[:, :, 0].long().clamp_(0, k - 1)),
                            torch.gather(rows_r, 1, corr[:, :, 1].long().clamp_(0, k - 1))], 2).to(torch.int32).cpu().numpy()
        cn, idx_s, idx_r = counts.cpu().numpy(), index[0][at].cpu().numpy(), index[1][at].cpu().numpy()
        for f, j in enumerate(full):
            Ts[j], corrs[j], kpts[j] = T[f:f + 1], orig[f, :cn[f]].reshape(-1, 2), (idx_s[f], idx_r[f], False)
    for j in range(B):
        if Ts[j] is None:
            sel = None if fell_back[j] else [index[0][j, :int(cs[j])], index[1][j, :int(cr[j])]]
            Ts[j], corrs[j], idx = _register_one_pair(engine, xs, xr, ds, dr, j, sel, pose, max_dist, match_kw, pose_kw)
            kpts[j] = idx + (bool(fell_back[j]),)
    return torch.cat(Ts, 0), corrs, kpts


@torch.no_grad()
def register_fpfh(pairs: Sequence[Dict[str, np.ndarray]], engine, voxel_size: float = 0.3, radius: Optional[float] = None,
                  hypotheses: int = 8192, mutual: bool = True, num_reg: int = 1, dataset_type: str = "3DMatch", batch: int = 1,
                  device: Optional[torch.device] = None, ransac_n: int = 3, edge_sim: float = 0.9, refine_iters: int = 2, seed: int = 0,
                  want_corr: bool = False, pose: str = "ransac", seeds: int = 64, members: int = 32, match_k: int = 1,
                  match_ratio: float = 0.0, search: str = "brute", max_nn: int = 0, normal_radius: Optional[float] = None,
                  normal_max_nn: int = 0, fgr_iterations: int = 64, tuple_scale: float = 0.95, max_tuples: int = 1000,
                  tuple_test: bool = True, keypoints: Optional[str] = None, salient_radius: Optional[float] = None,
                  non_max_radius: Optional[float] = None, gamma_21: float = 0.975, gamma_32: float = 0.975, min_neighbors: int = 5,
                  min_keypoints: int = 32, want_keypoints: bool = False, num_keypoints: int = 1024, ground: Optional[dict] = None):
    """The weight-independent baseline of ``register_feat``: FPFH + feature-matching RANSAC (open3d compute_fpfh_feature ->
    registration_ransac_based_on_feature_matching; parity unpinned, the rules are the engine's own), all on the device.  Per batch
    and side: ``knn_pyramid`` -> ``estimate_normals`` on its level-0 lists (towards the pair's optional ``viewpoint_src`` /
    ``viewpoint_ref`` entry, 3 floats; default the origin) -> ``fpfh`` over those 16-NN lists, or with ``radius`` set over the CSR of
    ``radius_matches(x, x, identity, radius)`` -> ``feature_correspondences(mutual)`` -> ``ransac_correspondence`` (threshold
    2 x voxel size), or with ``pose='consensus'`` -> ``consensus_correspondence`` (``seeds``, ``members``), or with ``pose='fgr'`` ->
    ``fgr_correspondence`` (``fgr_iterations``, ``tuple_scale``, ``max_tuples``, ``tuple_test``).  Returns what ``register_feat`` returns - (pred_transforms [n_pairs, num_reg, 3, 4], stats [n_pairs, 5] rows
    ``[succ, rte, rre, time, seq]``) - so ``evaluate_align`` and ``Engine.icp_refine`` take it the same way; with ``want_corr`` a
    third value, per pair the (corr [count, 2], flags_src [J], flags_ref [K]) numpy arrays.  ``match_k`` / ``match_ratio``: k candidate
    matches per src point (M = J x match_k) or Lowe's ratio test, as in ``register_feat``.

    ``search``: where the ``radius`` neighbourhoods come from - ``"brute"`` (the default: ``radius_matches``, J x K distance tests)
    or ``"grid"`` (``radius_neighbors`` over the cell index; with ``max_nn`` = 0 the same CSR bytes, so the same poses).  ``max_nn``
    > 0 keeps the max_nn nearest of a neighbourhood (grid only).  ``normal_radius`` (with ``normal_max_nn``) takes the normals from
    radius neighbourhoods over the cell index instead of the 16-NN lists: open3d's recipe is ``normal_radius = 2 voxel,
    normal_max_nn = 30, radius = 5 voxel, max_nn = 100, search = "grid"``.  With ``normal_radius`` and ``radius`` both set and
    ``search="grid"`` no pyramid is built, so clouds under 1024 points work, up to what the FPFH, correspondence and pose entries take.

    ``keypoints="iss"``: match and solve on ISS keypoints only (``Engine.iss_keypoints``, csrc/iss.hip; ``salient_radius`` default
    6 x voxel size, ``non_max_radius`` default 4 x voxel size - open3d's multiples of the resolution with the voxel size standing in
    for it -, ``gamma_21``, ``gamma_32``, ``min_neighbors``).  Normals and descriptors are still computed on every point (SPFH needs
    the neighbours); then, per pair, the keypoint rows of points and descriptors are gathered and ``feature_correspondences`` and the
    pose stage run on them as a batch of ONE pair (the counts are ragged), so a pair's result does not depend on ``batch``.  A pair
    with fewer than ``min_keypoints`` keypoints on either side uses all of its points (the same one-pair calls).  ``corr`` under
    ``want_corr`` holds original point indices.  ``want_keypoints`` appends one more value: per pair (idx_src, idx_ref, fell_back),
    the original indices matched on (all points after a fall-back; with ``keypoints=None`` every pair is (all, all, False)).
    ``keypoints="fps"``: match and solve on ``num_keypoints`` farthest-point samples per cloud (``Engine.farthest_point_sample``,
    csrc/fps.hip; no radius, no index, no normals, and the same count for every cloud).  Descriptors are still computed on every
    point; the sampled rows of the whole batch are gathered to [B, num_keypoints, .] and ``feature_correspondences`` and the pose
    stage run ONCE per batch on them (under ``pose="ransac"`` / ``"fgr"`` a pair's draws are keyed by its position in that call, as on
    the ``keypoints=None`` path).  A pair whose clouds hold fewer than ``num_keypoints`` points, or with fewer than ``min_keypoints``
    sampled rows on a side, uses all of its points through the one-pair calls; ``corr`` and ``want_keypoints`` as above, the
    indices in selection order.
    ``keypoints=None`` (the default) is the path above, unchanged.
    ``ground``: a dict of ``remove_ground`` arguments (``distance_threshold`` and what else it takes): ``points_src`` and
    ``points_ref`` of every pair lose their ground plane before anything else, so the result is that of the call on pairs holding
    the clouds ``remove_ground`` returns (the sizes become ragged: use ``batch=1``).  None (the default): nothing is removed.

    ``engine`` is a ``deepsir_amd.engine.Engine`` THE CALLER PREPARED: the descriptor itself needs no weights, but the pyramid and
    the other existing entries this calls refuse a context whose weights are not loaded (``Call::kWeights``, csrc/engine_ctx.h), so
    load a state dict first - any, e.g. ``weights.generate_state_dict(cfg, 0)``; its values are never read here.  Its max_points /
    max_pairs must cover the clouds and ``batch``; unless both radii are set with ``search="grid"`` (no pyramid, above), the clouds
    must be ones the pyramid takes (>= 1024 points with the default ratios)."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    if search not in ("brute", "grid"):
        raise ValueError(f"register_fpfh: search must be 'brute' or 'grid', got {search!r}")
    if max_nn < 0 or normal_max_nn < 0:
        raise ValueError("register_fpfh: max_nn and normal_max_nn must be 0 (no cap) or positive")
    if max_nn > 0 and (radius is None or search != "grid"):
        raise ValueError("register_fpfh: max_nn needs radius and search='grid' (the brute-force lists have no cap)")
    if normal_max_nn > 0 and normal_radius is None:
        raise ValueError("register_fpfh: normal_max_nn needs normal_radius")
    if keypoints not in (None, "iss", "fps"):
        raise ValueError(f"register_fpfh: keypoints must be None, 'iss' or 'fps', got {keypoints!r}")
    if min_keypoints < 1:
        raise ValueError("register_fpfh: min_keypoints >= 1 expected")
    if keypoints == "fps" and (int(num_keypoints) != num_keypoints or num_keypoints < 1):
        raise ValueError(f"register_fpfh: num_keypoints must be a positive integer, got {num_keypoints}")
    if ground is not None and len(pairs):
        sides = {k: _without_ground([p[k][0] for p in pairs], engine, ground, "register_fpfh") for k in ("points_src", "points_ref")}
        pairs = [dict(p, points_src=sides["points_src"][i][None], points_ref=sides["points_ref"][i][None]) for i, p in enumerate(pairs)]
    nbr = (search, int(max_nn), normal_radius, int(normal_max_nn))
    rte_t, rre_t = THRESHOLDS[dataset_type]
    preds, corrs, kpts, stats = [], [], [], np.zeros((len(pairs), 5))
    iss_kw = dict(salient_radius=float(6.0 * voxel_size if salient_radius is None else salient_radius),
                  non_max_radius=float(4.0 * voxel_size if non_max_radius is None else non_max_radius),
                  gamma_21=gamma_21, gamma_32=gamma_32, min_neighbors=min_neighbors)
    pose_kw = dict(ransac_n=ransac_n, edge_sim=edge_sim, hypotheses=hypotheses, refine_iters=refine_iters, seed=seed, seeds=seeds,
                   members=members, fgr_iterations=fgr_iterations, tuple_scale=tuple_scale, max_tuples=max_tuples, tuple_test=tuple_test)

    def view(i, side):
        v = pairs[i].get("viewpoint_" + side)
        return (0.0, 0.0, 0.0) if v is None else tuple(float(x) for x in np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v).reshape(-1)[:3])

    for ids, data in _pair_batches(pairs, batch, device):
        torch.cuda.synchronize(device)
        t0 = time.time()
        xs, xr = data["points_src"].float().contiguous(), data["points_ref"].float().contiguous()
        ds, fs, _ = _fpfh_side(engine, xs, [view(i, "src") for i in ids], radius, *nbr)
        dr, fr, _ = _fpfh_side(engine, xr, [view(i, "ref") for i in ids], radius, *nbr)
        if keypoints is None:
            corr, counts = engine.feature_correspondences(ds, dr, mutual=mutual, k=match_k, ratio=match_ratio)
            T = _pose_from_corr(engine, pose, xs, xr, corr, counts, 2.0 * voxel_size, **pose_kw)
            pair_corr = None
        else:
            how = (_register_on_keypoints, iss_kw) if keypoints == "iss" else (_register_on_fps, int(num_keypoints))
            T, pair_corr, pair_kpts = how[0](engine, xs, xr, ds, dr, how[1], int(min_keypoints), pose, 2.0 * voxel_size,
                                             dict(mutual=mutual, k=match_k, ratio=match_ratio), pose_kw)
            kpts += pair_kpts
        torch.cuda.synchronize(device)
        dt = (time.time() - t0) / len(ids)
        T = T.cpu().numpy()
        preds.append(np.repeat(T[:, None], num_reg, 1))
        gt = data["transform_gt"].cpu().numpy() if "transform_gt" in data else None
        if want_keypoints and keypoints is None:
            kpts += [(np.arange(xs.shape[1], dtype=np.int32), np.arange(xr.shape[1], dtype=np.int32), False) for _ in ids]
        if want_corr and pair_corr is not None:
            corrs += [(pair_corr[j], fs[j].cpu().numpy(), fr[j].cpu().numpy()) for j in range(len(ids))]
        elif want_corr:
            cn, cc = counts.cpu().numpy(), corr.cpu().numpy()
            corrs += [(cc[j, :cn[j]], fs[j].cpu().numpy(), fr[j].cpu().numpy()) for j in range(len(ids))]
        for j, i in enumerate(ids):
            if gt is not None:
                stats[i, :3] = rte_rre(T[j], gt[j], rte_t, rre_t)
            stats[i, 3] = dt
            others = pairs[i].get("others")
            stats[i, 4] = _seq_id(others[0]["seq"]) if others else -1
    pred = np.concatenate(preds, 0) if preds else np.zeros((0, num_reg, 3, 4), np.float32)
    return (pred, stats) + ((corrs,) if want_corr else ()) + ((kpts,) if want_keypoints else ())


@torch.no_grad()
def inference_label(pairs: Sequence[Dict[str, np.ndarray]], model, batch: int = 1, device: Optional[torch.device] = None):
    """test.py::inference_label (:508-567): semantic head over every pair; ``labels_src`` / ``labels_ref`` [1,N]
    (0 = unlabeled) give accuracy / IoU.  Returns (per-pair predicted labels (1-based like the reference's export),
    {'mean_iou', 'iou', 'mean_acc', 'loss'}, total model time)."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    metric = SemanticMetric(model.cfg.num_classes)
    preds, losses, total = [], [], 0.0
    for ids, data in _pair_batches(pairs, batch, device):
        torch.cuda.synchronize(device)
        t0 = time.time()
        _, ep = model(data)
        torch.cuda.synchronize(device)
        total += time.time() - t0
        if "labels_src" in data:
            l_s, _ = metric.add(ep["logits_src"], data["labels_src"])
            l_r, _ = metric.add(ep["logits_ref"], data["labels_ref"])
            losses.append(l_s + l_r)
        for j in range(len(ids)):
            preds.append({s: (torch.argmax(ep[f"logits_{s}"][j], dim=0) + 1).cpu().numpy() for s in ("src", "ref")})
    mean_iou, iou, mean_acc = metric.result()
    return preds, {"mean_iou": mean_iou, "iou": iou, "mean_acc": mean_acc,
                   "loss": float(np.nanmean(losses)) if losses else float("nan")}, total


# ----------------------------------------------------------------------------------------------------------------------
# scene registration: pairwise poses -> edge information matrices -> pose graph (include/dsir.h, dsir_information_matrix and
# dsir_pose_graph_optimize; the host rules are deepsir_amd/pose_graph.py)
OVERLAP_MIN = 0.3          # open3d's reconstruction rule: an edge needs info[5,5] / min(n_s, n_t) of at least this


def _scene_pairs(fragments, pairs):
    n = len(fragments)
    return [(int(s), int(t)) for s, t in pairs] if pairs is not None else [(i, j) for i in range(n) for j in range(i + 1, n)]


def _scene_table(fragments, pairs, register, **kw):
    """The candidate-edge table of a scene from a pairwise registration: rows (s, t, T [3,4], uncertain), t = s + 1 certain."""
    as_np = lambda f: f.cpu().numpy() if isinstance(f, torch.Tensor) else np.asarray(f)
    st = _scene_pairs(fragments, pairs)
    data = [{"points_src": as_np(fragments[s])[None].astype(np.float32), "points_ref": as_np(fragments[t])[None].astype(np.float32)} for s, t in st]
    pred = register(data, **kw)[0]
    return [(s, t, np.asarray(pred[k, -1], np.float64), t != s + 1) for k, (s, t) in enumerate(st)]


def scene_edges_fpfh(fragments, engine, pairs=None, **kw):
    """Candidate edges of a scene through ``register_fpfh`` (its keyword arguments pass through): all pairs s < t, or ``pairs``.
    -> list of (s, t, T [3,4] with p_t = T p_s, uncertain); edges t = s + 1 are certain (odometry), the rest uncertain."""
    return _scene_table(fragments, pairs, lambda d, **k: register_fpfh(d, engine, **k), **kw)


def scene_edges_feat(fragments, model, pairs=None, **kw):
    """``scene_edges_fpfh`` through ``register_feat`` and a 'feat' model."""
    return _scene_table(fragments, pairs, lambda d, **k: register_feat(d, model, **k), **kw)


def _chain_poses(N, edges, reference_node):
    """Node poses implied by a spanning tree of the edges from the reference node (certain edges first): X_s = X_t T."""
    inv = lambda A: np.hstack([A[:, :3].T, (-A[:, :3].T @ A[:, 3])[:, None]])
    mul = lambda A, B: np.hstack([A[:, :3] @ B[:, :3], (A[:, :3] @ B[:, 3] + A[:, 3])[:, None]])
    X = {int(reference_node): np.eye(3, 4)}
    order = sorted(edges, key=lambda e: bool(e[3]))
    for _ in range(N):
        for s, t, T, _u in order:
            if t in X and s not in X:
                X[s] = mul(X[t], T)
            elif s in X and t not in X:
                X[t] = mul(X[s], inv(T))
    if len(X) != N:
        raise ValueError("register_scene: the kept edges do not connect the scene (disconnected)")
    return np.stack([X[i] for i in range(N)])


def pad_clouds(clouds):
    """Clouds [n_i, stride] of unequal sizes (tensors on one device, or numpy) as one batch for the entries that take per-pair
    counts (``Engine.icp_refine(counts_src=, counts_ref=)``, ...): -> (tensor [P, cap, stride] float32, counts [P] int32), cap the
    largest n_i (at least 1).  The padding rows are NaN on purpose: the engine never reads them, and a kernel that did would show."""
    cl = [c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c, np.float32)) for c in clouds]
    if not cl or any(c.dim() != 2 or c.shape[1] != cl[0].shape[1] for c in cl):
        raise ValueError("pad_clouds: expected at least one cloud, all [n_i, stride] with the same stride")
    out = torch.full((len(cl), max(1, max(c.shape[0] for c in cl)), cl[0].shape[1]), float("nan"), dtype=torch.float32, device=cl[0].device)
    for i, c in enumerate(cl):
        out[i, :c.shape[0]] = c
    return out, torch.tensor([c.shape[0] for c in cl], dtype=torch.int32, device=cl[0].device)


@torch.no_grad()
def remove_planes(clouds, engine, distance_threshold: float, keep: str = "rest", batch: Optional[int] = None, **segment_kw):
    """Split clouds by ``Engine.segment_plane`` (csrc/plane.hip): clouds [n_i, C >= 3] of any sizes (numpy or tensors) ->
    (kept: per cloud the rows no plane took (``keep="rest"``) or the rows of the planes (``keep="planes"``), in input order, all
    columns; planes [P, max_planes, 4]; num_planes [P]; removed [P] float64: the share of each cloud's rows that was dropped).
    ``pad_clouds``, then one ``segment_plane`` call per ``batch`` clouds (default: all, at most the engine's max_pairs), cloud i
    drawing with id i (``cloud_ids`` in ``segment_kw`` overrides it), so a cloud's split does not depend on ``batch``; the split
    itself is torch boolean indexing per cloud.  ``segment_kw``: hypotheses, max_planes, min_inliers, axis, max_angle_deg,
    refine_iters, seed."""
    if keep not in ("rest", "planes"):
        raise ValueError(f"remove_planes: keep must be 'rest' or 'planes', got {keep!r}")
    dev = engine.device
    cl = [(c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c, np.float32))).to(dev).float().contiguous() for c in clouds]
    P = len(cl)
    if P < 1:
        raise ValueError("remove_planes: at least one cloud expected")
    per = int(batch or min(P, engine.max_pairs))
    if per < 1:
        raise ValueError("remove_planes: batch must be at least 1")
    kw = dict(segment_kw)
    ids = kw.pop("cloud_ids", None)
    ids = list(range(P)) if ids is None else [int(i) for i in (ids.cpu().tolist() if isinstance(ids, torch.Tensor) else ids)]
    if len(ids) != P:
        raise ValueError(f"remove_planes: cloud_ids must hold one id per cloud ({P})")
    kept, planes, nums, removed = [], [], [], np.zeros(P)
    for b0 in range(0, P, per):
        part = cl[b0:b0 + per]
        pad, counts = pad_clouds(part)
        labels, num, pl = engine.segment_plane(pad, distance_threshold, counts=counts, cloud_ids=ids[b0:b0 + per], **kw)[:3]
        for i, c in enumerate(part):
            taken = labels[i, :c.shape[0]] >= 0
            kept.append(c[taken if keep == "planes" else ~taken])
            removed[b0 + i] = 1.0 - kept[-1].shape[0] / max(c.shape[0], 1)
        planes.append(pl)
        nums.append(num)
    return kept, torch.cat(planes, 0), torch.cat(nums, 0), removed


def remove_ground(clouds, engine, distance_threshold: float, axis=(0.0, 0.0, 1.0), max_angle_deg: float = 15.0, **kw):
    """``remove_planes`` with ``max_planes=1`` and the angle constraint: the dominant plane whose normal lies within ``max_angle_deg``
    of ``axis`` (the road of a lidar scan, the floor of a fragment) is dropped (or, with ``keep="planes"``, kept alone)."""
    if kw.get("max_planes", 1) != 1:
        raise ValueError("remove_ground: one plane only (max_planes=1); use remove_planes for more")
    return remove_planes(clouds, engine, distance_threshold, axis=axis, max_angle_deg=max_angle_deg, **dict(kw, max_planes=1))


def _without_ground(clouds, engine, ground, who):
    """the ``ground=`` option of register_fpfh / icp_multiscale / ndt_multiscale: a dict of ``remove_ground`` arguments"""
    if not isinstance(ground, dict) or "distance_threshold" not in ground:
        raise ValueError(f"{who}: ground must be a dict of remove_ground arguments with a 'distance_threshold'")
    kw = dict(ground)
    return remove_ground(clouds, engine, kw.pop("distance_threshold"), **kw)[0]


def _per_scale(value, n, name):
    """None, a scalar or a sequence of n entries -> a list of n entries"""
    if value is None or isinstance(value, (int, float)):
        return [value] * n
    if len(value) != n:
        raise ValueError(f"icp_multiscale: {name} must have one entry per scale ({n}), got {len(value)}")
    return list(value)


@torch.no_grad()
def icp_multiscale(src_clouds, ref_clouds, T_init, voxel_sizes, max_iters, radii=None, estimator: str = "point",
                   kernel: str = "l2", kernel_scales=None, search: str = "auto", batch: Optional[int] = None, *, engine,
                   ground: Optional[dict] = None):
    """open3d's ``multi_scale_icp`` for lists of clouds of any sizes: coarse to fine, every scale one ``Engine.icp_refine`` from the
    previous scale's pose.  src_clouds / ref_clouds: P clouds [n_i, >=3] each (numpy or tensors), T_init [P,3,4] with p_ref = T p_src;
    voxel_sizes, max_iters: one entry per scale, in the order they run (coarse first); radii: the correspondence radius per scale
    (None, or a None entry: 2 x that scale's voxel size); kernel_scales: the robust kernel's scale per scale (a scalar: the same at
    every scale).  ``engine`` (keyword): the ``Engine`` that runs it; ``batch``: pairs per engine call (default: all of them, at most
    the engine's max_pairs).
    Per scale, and per batch of pairs: ``voxel_downsample`` of both sides (a voxel size of None or 0: the clouds as given),
    ``pad_clouds`` with the counts, for ``estimator="plane"`` the normals of the downsampled reference from
    ``radius_neighbors(radius = 2 x voxel, max_nn = 30)`` and ``estimate_normals(csr=)`` cloud by cloud (this needs a non-zero voxel
    size at that scale, or rows that carry the normals in columns 3..5), then ``icp_refine``.  No kernel of its own: exactly these
    engine calls, so the result is theirs byte for byte.  ``ground``: a dict of ``remove_ground`` arguments (``distance_threshold``
    and what else it takes); both sides lose their ground plane before anything else, so the result is that of the call on the
    clouds ``remove_ground`` returns.  None (the default): nothing is removed.
    -> (T [P,3,4] float32 tensor of the last scale, stats: one [P,4|5] float64 tensor per scale)."""
    S = len(voxel_sizes)
    if S < 1 or len(max_iters) != S:
        raise ValueError("icp_multiscale: voxel_sizes and max_iters need one entry per scale, at least one")
    radii, kernel_scales = _per_scale(radii, S, "radii"), _per_scale(kernel_scales, S, "kernel_scales")
    dev = engine.device
    as_dev = lambda c: (c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c, np.float32))).to(dev).float().contiguous()
    srcs, refs = [as_dev(c) for c in src_clouds], [as_dev(c) for c in ref_clouds]
    P = len(srcs)
    if P < 1 or len(refs) != P:
        raise ValueError("icp_multiscale: as many reference clouds as source clouds, at least one pair")
    if ground is not None:
        srcs, refs = _without_ground(srcs, engine, ground, "icp_multiscale"), _without_ground(refs, engine, ground, "icp_multiscale")
    T = as_dev(np.asarray(T_init.detach().cpu() if isinstance(T_init, torch.Tensor) else T_init, np.float32)[:, :3]).clone()
    if tuple(T.shape) != (P, 3, 4):
        raise ValueError(f"icp_multiscale: T_init must be [{P}, 3, 4]")
    per = int(batch or min(P, engine.max_pairs))
    if per < 1:
        raise ValueError("icp_multiscale: batch must be at least 1")

    def down(clouds, voxel):
        if not voxel:
            return clouds
        vox, counts = engine.voxel_downsample(clouds, float(voxel))
        engine.sync()
        n = counts.cpu().tolist()
        return [vox[i, :n[i]].contiguous() for i in range(len(clouds))]

    stats = []
    for voxel, iters, radius, kscale in zip(voxel_sizes, max_iters, radii, kernel_scales):
        if radius is None:
            if not voxel:
                raise ValueError("icp_multiscale: a scale without a voxel size needs its radius given")
            radius = 2.0 * float(voxel)
        st_scale = []
        for b0 in range(0, P, per):
            ids = range(b0, min(P, b0 + per))
            s_list, r_list = down([srcs[i] for i in ids], voxel), down([refs[i] for i in ids], voxel)
            src, n_s = pad_clouds(s_list)
            ref, n_t = pad_clouds(r_list)
            nrm = None
            if estimator == "plane" and ref.shape[2] < 6:
                if not voxel:
                    raise ValueError("icp_multiscale: estimator='plane' at a scale without a voxel size needs rows that carry the "
                                     "normals in columns 3..5")
                nrm = pad_clouds([engine.estimate_normals(c[None], csr=engine.radius_neighbors(c[None], 2.0 * float(voxel), max_nn=30))[0][0]
                                  for c in r_list])[0]
            Tb, st = engine.icp_refine(src, ref, T[b0:b0 + len(ids)].contiguous(), float(radius), max_iter=int(iters), estimator=estimator,
                                       normals_ref=nrm, search=search, counts_src=n_s, counts_ref=n_t, kernel=kernel, kernel_scale=kscale)
            T[b0:b0 + len(ids)] = Tb
            st_scale.append(st)
        stats.append(torch.cat(st_scale, 0))
    return T, stats


@torch.no_grad()
def ndt_multiscale(src_clouds, ref_clouds, T_init, resolutions, max_iters, neighbors: int = 7, step_tol: float = 1e-4,
                   outlier_ratio: float = 0.55, batch: Optional[int] = None, *, engine, ground: Optional[dict] = None):
    """NDT coarse to fine for lists of clouds of any sizes: every scale one ``Engine.ndt_refine`` on the clouds as given, from the
    previous scale's pose.  src_clouds / ref_clouds: P clouds [n_i, >=3] each (numpy or tensors), T_init [P,3,4] with p_ref = T p_src;
    resolutions, max_iters: one entry per scale, in the order they run (coarse first).  ``engine`` (keyword): the ``Engine`` that
    runs it; ``batch``: pairs per engine call (default: all of them, at most the engine's max_pairs).  No kernel of its own:
    ``pad_clouds`` with the counts and these engine calls, so the result is theirs byte for byte.
    ``ground``: a dict of ``remove_ground`` arguments; both sides lose their ground plane before anything else (None: nothing removed).
    -> (T [P,3,4] float32 tensor of the last scale, stats: one [P,5] float32 tensor per scale)."""
    S = len(resolutions)
    if S < 1 or len(max_iters) != S:
        raise ValueError("ndt_multiscale: resolutions and max_iters need one entry per scale, at least one")
    dev = engine.device
    as_dev = lambda c: (c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c, np.float32))).to(dev).float().contiguous()
    srcs, refs = [as_dev(c) for c in src_clouds], [as_dev(c) for c in ref_clouds]
    P = len(srcs)
    if P < 1 or len(refs) != P:
        raise ValueError("ndt_multiscale: as many reference clouds as source clouds, at least one pair")
    if ground is not None:
        srcs, refs = _without_ground(srcs, engine, ground, "ndt_multiscale"), _without_ground(refs, engine, ground, "ndt_multiscale")
    T = as_dev(np.asarray(T_init.detach().cpu() if isinstance(T_init, torch.Tensor) else T_init, np.float32)[:, :3]).clone()
    if tuple(T.shape) != (P, 3, 4):
        raise ValueError(f"ndt_multiscale: T_init must be [{P}, 3, 4]")
    per = int(batch or min(P, engine.max_pairs))
    if per < 1:
        raise ValueError("ndt_multiscale: batch must be at least 1")
    padded = []
    for b0 in range(0, P, per):
        ids = range(b0, min(P, b0 + per))
        padded.append((b0, len(ids), pad_clouds([srcs[i] for i in ids]), pad_clouds([refs[i] for i in ids])))
    stats = []
    for res, iters in zip(resolutions, max_iters):
        st_scale = []
        for b0, n, (src, n_s), (ref, n_t) in padded:
            Tb, st = engine.ndt_refine(src, ref, T[b0:b0 + n].contiguous(), float(res), neighbors=neighbors, max_iter=int(iters),
                                       step_tol=step_tol, outlier_ratio=outlier_ratio, counts_src=n_s, counts_ref=n_t)
            T[b0:b0 + n] = Tb
            st_scale.append(st)
        stats.append(torch.cat(st_scale, 0))
    return T, stats


def scene_batches(sizes, batch: int):
    """The ICP calls of ``register_scene``: ``sizes`` = (n_s, n_t) per edge -> lists of edge numbers, ``batch`` at a time in the order
    of a stable sort by n_s + n_t, so that a call's capacity stays close to its pairs' sizes.  Every edge is in exactly one list."""
    if batch < 1:
        raise ValueError("register_scene: batch must be at least 1")
    order = sorted(range(len(sizes)), key=lambda k: int(sizes[k][0]) + int(sizes[k][1]))       # sorted() is stable
    return [order[b0:b0 + batch] for b0 in range(0, len(order), batch)]


@torch.no_grad()
def register_scene(fragments, engine, edges, voxel_size: float = 0.05, max_corr_dist: Optional[float] = None, icp_max_iter: int = 30,
                   estimator: str = "point", search: str = "auto", preference: float = 1.0, overlap_min: float = OVERLAP_MIN,
                   max_iter: int = 100, reference_node: int = 0, batch: int = 1, icp_kernel: str = "l2",
                   icp_kernel_scale: Optional[float] = None):
    """A scene from its pairwise registrations.  fragments: clouds [n_i, >=3] (numpy or tensors, any sizes the engine takes);
    edges: rows (s, t, T_init [3,4] with p_t = T p_s, uncertain) from any pairwise path (``scene_edges_fpfh``, ...).  Per edge
    ``icp_refine`` (radius ``max_corr_dist``, default 2 x voxel size) then ``information_matrix``; an edge with
    info[5,5] / min(n_s, n_t) < ``overlap_min`` is dropped ("overlap"); ``pose_graph_optimize`` on the rest with
    mu = ``line_process_weight(..., preference)`` from the chained poses; uncertain edges with l < 0.25 are dropped ("line") and the
    graph is optimised again from the first result.  ``batch``: edges per ICP call (at most the engine's max_pairs), whatever their
    sizes: each call pads its clouds (``pad_clouds``) and passes the sizes as counts, and by the contract of those entries
    (include/dsir.h, dsir_icp_refine_ex3) the result is the same, byte for byte, for every ``batch``.  ``estimator="plane"`` on rows
    without normals estimates each fragment's normals once (``engine.icp_normals``).  ``icp_kernel`` / ``icp_kernel_scale``:
    ``icp_refine``'s robust ``kernel`` and ``kernel_scale`` for the edge poses; the information matrices do not see them.
    -> {"X": [N,3,4] f64 node poses (fragment -> scene, reference node the identity), "edges": one dict per input edge
    {s, t, T (refined), info, count, uncertain, line, dropped: None | "overlap" | "line"}, "stats": [stats of both optimisations]}."""
    from . import pose_graph as PG
    r = float(2.0 * voxel_size if max_corr_dist is None else max_corr_dist)
    dev = engine.device
    frs = [(f if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f, np.float32))).to(dev).float().contiguous() for f in fragments]
    N = len(frs)
    rows = [{"s": int(s), "t": int(t), "T": None, "info": None, "count": 0, "uncertain": bool(u), "line": 1.0, "dropped": None} for s, t, _, u in edges]
    normals = {}                                                       # estimator "plane" on rows without normals: once per fragment
    if estimator == "plane" and any(f.shape[1] < 6 for f in frs):
        normals = {t: engine.icp_normals(frs[t][None])[0] for t in sorted({r_["t"] for r_ in rows})}
    sizes = [(frs[r_["s"]].shape[0], frs[r_["t"]].shape[0]) for r_ in rows]
    for kb in scene_batches(sizes, batch):
        src, n_s = pad_clouds([frs[rows[k]["s"]] for k in kb])
        ref, n_t = pad_clouds([frs[rows[k]["t"]] for k in kb])
        nrm = pad_clouds([normals[rows[k]["t"]] for k in kb])[0] if normals else None
        T0 = torch.from_numpy(np.stack([np.asarray(edges[k][2], np.float32)[:3] for k in kb])).to(dev).contiguous()
        T, _ = engine.icp_refine(src, ref, T0, r, max_iter=icp_max_iter, estimator=estimator, normals_ref=nrm, search=search,
                                 counts_src=n_s, counts_ref=n_t, kernel=icp_kernel, kernel_scale=icp_kernel_scale)
        info, count = engine.information_matrix(src, ref, T, r, search=search, counts_src=n_s, counts_ref=n_t)
        T, info, count = T.cpu().numpy().astype(np.float64), info.cpu().numpy(), count.cpu().numpy()
        for j, k in enumerate(kb):
            rows[k].update(T=T[j], info=info[j], count=int(count[j]))
            if info[j, 5, 5] / max(1, min(sizes[k])) < overlap_min:
                rows[k]["dropped"] = "overlap"

    def graph(keep, X0):
        return PG.PoseGraph(X0, np.array([(rows[k]["s"], rows[k]["t"]) for k in keep], np.int32).reshape(-1, 2),
                            np.array([rows[k]["T"] for k in keep]).reshape(-1, 3, 4), np.array([rows[k]["info"] for k in keep]).reshape(-1, 6, 6),
                            np.array([rows[k]["uncertain"] for k in keep], np.uint8),
                            PG.line_process_weight([rows[k]["info"] for k in keep], [rows[k]["uncertain"] for k in keep], r, preference),
                            reference_node)

    keep = [k for k in range(len(rows)) if rows[k]["dropped"] is None]
    X0 = _chain_poses(N, [(rows[k]["s"], rows[k]["t"], rows[k]["T"], rows[k]["uncertain"]) for k in keep], reference_node)
    (X, line, st1), = engine.pose_graph_optimize([graph(keep, X0)], max_iter=max_iter)
    for k, l in zip(keep, line):
        rows[k]["line"] = float(l)
        if rows[k]["uncertain"] and l < PG.PRUNE_LINE:
            rows[k]["dropped"] = "line"
    keep = [k for k in keep if rows[k]["dropped"] is None]
    _chain_poses(N, [(rows[k]["s"], rows[k]["t"], rows[k]["T"], rows[k]["uncertain"]) for k in keep], reference_node)   # still connected
    (X, line, st2), = engine.pose_graph_optimize([graph(keep, X)], max_iter=max_iter)
    for k, l in zip(keep, line):
        rows[k]["line"] = float(l)
    return {"X": X, "edges": rows, "stats": [st1, st2]}


def implied_pose(X, s: int, t: int) -> np.ndarray:
    """The pair pose the node poses imply, p_t = T p_s: T = X_t^-1 X_s [3,4]."""
    Rt = X[t][:, :3].T
    return np.hstack([Rt @ X[s][:, :3], (Rt @ (X[s][:, 3] - X[t][:, 3]))[:, None]])


def summarize_scene(result, gt: Optional[Dict[tuple, np.ndarray]] = None, dataset_type: str = "3DMatch", gt_info: Optional[Dict[tuple, np.ndarray]] = None):
    """Counts of a ``register_scene`` result and, with ``gt`` {(s, t): T_gt [3,4]}, the pairwise recall (RTE / RRE thresholds) of the
    refined pair poses and of the poses the optimised nodes imply; with ``gt_info`` {(s, t): info as read from gt.info} also under
    ``metrics.info_rmse``."""
    from .metrics import info_rmse
    rows = result["edges"]
    out = {"edges": len(rows), "dropped_overlap": sum(r["dropped"] == "overlap" for r in rows),
           "dropped_line": sum(r["dropped"] == "line" for r in rows), "status": [int(s[3]) for s in result["stats"]]}
    if gt:
        rte_t, rre_t = THRESHOLDS[dataset_type]
        inv = lambda A: np.hstack([A[:3, :3].T, (-A[:3, :3].T @ A[:3, 3])[:, None]])
        raw, opt, raw_i, opt_i = [], [], [], []
        for r in rows:                                        # a ground-truth record may be keyed (s, t) or, as gt.log is, (t, s)
            key, flip = ((r["s"], r["t"]), False) if (r["s"], r["t"]) in gt else ((r["t"], r["s"]), True)
            if key not in gt:
                continue
            T_raw, T_opt = r["T"], implied_pose(result["X"], r["s"], r["t"])
            if flip:
                T_raw, T_opt = inv(T_raw), inv(T_opt)
            T_gt = np.asarray(gt[key], np.float64)[:3]
            raw.append(rte_rre(T_raw, T_gt, rte_t, rre_t)[0])
            opt.append(rte_rre(T_opt, T_gt, rte_t, rre_t)[0])
            if gt_info and key in gt_info:
                raw_i.append(info_rmse(T_raw, T_gt, gt_info[key])[1])
                opt_i.append(info_rmse(T_opt, T_gt, gt_info[key])[1])
        out.update(pairs=len(raw), recall_raw=float(np.mean(raw)) if raw else 0.0, recall_optimized=float(np.mean(opt)) if opt else 0.0)
        if raw_i:
            out.update(pairs_info=len(raw_i), recall_raw_info=float(np.mean(raw_i)), recall_optimized_info=float(np.mean(opt_i)))
    return out
