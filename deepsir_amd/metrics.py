"""Registration criteria of the evaluation harness (reference
common/metrics_util.py:13-24 ``rte_rre``; thresholds test.py:49-54; test.py names none for Oxford, which gets
the defaults of arguments.py:116-119 that the reference's training loop validates with)."""
import numpy as np

THRESHOLDS = {"3DMatch": (0.3, 15.0), "KITTI": (0.6, 5.0), "Oxford": (0.6, 5.0)}   # (RTE m, RRE deg)


def rte_rre(T_pred, T_gt, rte_thresh, rre_thresh, eps=1e-16):
    """-> array [success, rte (m), rre (deg)]; ``None`` prediction counts as a failure."""
    if T_pred is None:
        return np.array([0, np.inf, np.inf])
    T_pred, T_gt = np.asarray(T_pred), np.asarray(T_gt)
    rte = np.linalg.norm(T_pred[:3, 3] - T_gt[:3, 3])
    c = (np.trace(T_pred[:3, :3].T @ T_gt[:3, :3]) - 1) / 2
    rre = np.arccos(np.clip(c, -1 + eps, 1 - eps)) * 180 / np.pi
    return np.array([rte < rte_thresh and rre < rre_thresh, rte, rre])


INFO_RMSE_THRESHOLD = 0.2   # metres: the 3DMatch benchmark accepts a pair whose estimated correspondence RMSE is at most this


def info_rmse(T_pred, T_gt, info, threshold: float = INFO_RMSE_THRESHOLD):
    """The 3DMatch benchmark's registration criterion, on the host: with E = T_gt^-1 T_pred and
    er = [translation of E; vector part of the unit quaternion (w >= 0) of E's rotation],
    p = er^T info er / info[0, 0] estimates the mean squared distance of the pair's ground-truth correspondences under T_pred.
    ``info`` [6,6] is taken as read from the scene's ``gt.info`` (``read_trajectory(path, dim=6)``), whose own order is
    [translation; rotation]: it is NOT the order of ``Engine.information_matrix``, and nothing here converts between the two.
    -> (p, success: p <= threshold^2)."""
    T_pred, T_gt, info = np.asarray(T_pred, np.float64), np.asarray(T_gt, np.float64), np.asarray(info, np.float64)
    R = T_gt[:3, :3].T @ T_pred[:3, :3]
    t = T_gt[:3, :3].T @ (T_pred[:3, 3] - T_gt[:3, 3])
    # unit quaternion of R, the branch with the largest component (Shepperd), then the sign with w >= 0
    d = np.array([np.trace(R), R[0, 0], R[1, 1], R[2, 2]])
    k = int(np.argmax(d))
    if k == 0:
        q = np.array([1.0 + d[0], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    else:
        i, j, l = k - 1, k % 3, (k + 1) % 3
        q = np.zeros(4)
        q[0] = R[l, j] - R[j, l]
        q[1 + i] = 1.0 + R[i, i] - R[j, j] - R[l, l]
        q[1 + j] = R[j, i] + R[i, j]
        q[1 + l] = R[l, i] + R[i, l]
    q = q / np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    er = np.concatenate([t, q[1:]])
    p = float(er @ info @ er / info[0, 0])
    return p, bool(p <= threshold * threshold)
