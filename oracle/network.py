"""Oracle: PyTorch-CPU fp32 restatement of the registration network
(TEST INFRASTRUCTURE ONLY — see oracle/__init__.py).

Functional (no nn.Module); parameters are looked up by the reference's
state-dict key names.  Layout follows the reference (channel-major
``[B,C,N(,k)]``) so that the oracle and the imported reference execute the
same ATen kernels on the same shapes and agree to rounding.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from deepsir_amd.arch import LABEL_WEIGHTS, NetConfig, level_sizes

_EPS = 1e-16  # reference network/model.py:18


def _gather_nbr(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """[B,C,N], [B,M,k] -> [B,C,M,k]   (reference network/tools.py:197-209)."""
    B, C, _ = x.shape
    M, k = idx.shape[1], idx.shape[2]
    flat = idx.reshape(B, 1, M * k).expand(B, C, M * k)
    return torch.gather(x, 2, flat).reshape(B, C, M, k)


def _gather_pts(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """[B,C,N], [B,M] -> [B,C,M]   (reference network/tools.py:211-221)."""
    return torch.gather(x, 2, idx[:, None, :].expand(-1, x.shape[1], -1))


class OracleNet:
    def __init__(self, cfg: NetConfig, state_dict: Dict[str, "np.ndarray | torch.Tensor"], dtype: torch.dtype = torch.float32):
        """dtype: of every floating tensor (parameters, running statistics, constants); torch.float64 makes the same function
        an fp64 reference for error bounds (inputs are then handed over in fp64 too)."""
        self.cfg = cfg
        self.dtype = dtype
        self.p: Dict[str, torch.Tensor] = {}
        for k, v in state_dict.items():
            t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.array(v))
            t = t.detach().clone()
            self.p[k] = t.to(dtype) if t.is_floating_point() else t
        self.label_weights = torch.tensor(LABEL_WEIGHTS, dtype=dtype)

    # ------------------------------------------------------------------ layers
    def mlp2d(self, prefix: str, x: torch.Tensor, act: bool = True) -> torch.Tensor:
        """Conv2d 1x1 + GroupNorm(4 if C<64 else 8) + LeakyReLU(0.2)
        (reference network/RandLANet.py:58-107)."""
        w = self.p[prefix + ".conv.weight"]
        y = F.conv2d(x, w, self.p[prefix + ".conv.bias"])
        groups = 8 if w.shape[0] >= 64 else 4
        y = F.group_norm(y, groups, self.p[prefix + ".norm.weight"], self.p[prefix + ".norm.bias"], 1e-5)
        return F.leaky_relu(y, 0.2) if act else y

    def mlp1d(self, prefix: str, x: torch.Tensor, n_layers: int) -> torch.Tensor:
        """Conv1d + BatchNorm1d(eval) + LeakyReLU(0.2), last layer bare
        (reference network/RandLANet.py:34-55)."""
        pos = 0
        for i in range(n_layers):
            x = F.conv1d(x, self.p[f"{prefix}.{pos}.weight"], self.p[f"{prefix}.{pos}.bias"])
            pos += 1
            if i < n_layers - 1:
                x = F.batch_norm(x, self.p[f"{prefix}.{pos}.running_mean"], self.p[f"{prefix}.{pos}.running_var"],
                                 self.p[f"{prefix}.{pos}.weight"], self.p[f"{prefix}.{pos}.bias"], False, 0.1, 1e-5)
                x = F.leaky_relu(x, 0.2)
                pos += 2
        return x

    def att_pooling(self, prefix: str, f: torch.Tensor) -> torch.Tensor:
        """softmax_k(W f) * f summed over k, then MLP2D (RandLANet.py:148-157)."""
        a = F.softmax(F.conv2d(f, self.p[prefix + ".fc.weight"]), dim=3)
        return self.mlp2d(prefix + ".mlp", torch.sum(f * a, dim=3, keepdim=True))

    @staticmethod
    def rel_pos_encoding(xyz: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        """[|pj-pi|, pj-pi, pi, pj] -> [B,10,n,k]  (RandLANet.py:197-212)."""
        pj = _gather_nbr(xyz, idx)
        pi = xyz.unsqueeze(-1).expand_as(pj)
        rel = pj - pi
        dis = torch.sqrt(torch.sum(rel * rel, dim=1, keepdim=True))
        return torch.cat([dis, rel, pi, pj], dim=1)

    def res_block(self, prefix: str, feat: torch.Tensor, xyz: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        """Dilated residual block with the two-stage local feature aggregation
        (RandLANet.py:173-195, :225-230).  feat [B,C,n,1]."""
        f = self.mlp2d(prefix + ".mlp1", feat)
        enc = self.mlp2d(prefix + ".lfa.mlp1", self.rel_pos_encoding(xyz, idx))
        cat = torch.cat([_gather_nbr(f.squeeze(-1), idx), enc], dim=1)
        agg = self.att_pooling(prefix + ".lfa.att_pooling_1", cat)
        enc = self.mlp2d(prefix + ".lfa.mlp2", enc)
        cat = torch.cat([_gather_nbr(agg.squeeze(-1), idx), enc], dim=1)
        agg = self.att_pooling(prefix + ".lfa.att_pooling_2", cat)
        main = self.mlp2d(prefix + ".mlp2", agg, act=False)
        skip = self.mlp2d(prefix + ".mlp_skip", feat, act=False)
        return F.leaky_relu(main + skip, 0.2)

    # ------------------------------------------------------------------ RandLA
    def randla(self, prefix: str, features: torch.Tensor, xyz_multi: torch.Tensor, neigh_idx: torch.Tensor,
               sub_idx: torch.Tensor, interp_idx: torch.Tensor, taps: Optional[dict] = None):
        """RandLA.forward (RandLANet.py:311-372).
        features [B,N,Cin]; xyz_multi [B,sum n_l,3]; neigh_idx [B,sum n_l,k];
        sub_idx [B,sum n_{l+1},k]; interp_idx [B,sum n_l,1]
        -> feat [B,64,N], xyz [B,3,N], logits [B,ncls,N]."""
        L = len(self.cfg.d_out)
        N = features.shape[1]
        n = level_sizes(N, self.cfg.sub_sampling_ratio)            # n_0..n_L
        off = np.concatenate([[0], np.cumsum(n[:L])])               # level offsets   (:287-299)
        soff = np.concatenate([[0], np.cumsum(n[1:L + 1])])         # sub_idx offsets (:301-309)
        xyz = xyz_multi.permute(0, 2, 1).contiguous()
        x = self.mlp2d(prefix + ".mlp_pre", features.permute(0, 2, 1).contiguous().unsqueeze(3))
        skips: List[torch.Tensor] = []
        for l in range(L):
            a, b = int(off[l]), int(off[l + 1])
            enc = self.res_block(f"{prefix}.dilated_res_blocks.{l}", x, xyz[:, :, a:b], neigh_idx[:, a:b])
            # "random sampling" = max over the K neighbours of the first n/4 points (:374-391)
            pool = sub_idx[:, int(soff[l]):int(soff[l + 1])]
            x = _gather_nbr(enc.squeeze(3), pool).max(dim=3, keepdim=True)[0]
            if l == 0:
                skips.append(enc)
            skips.append(x)
            if taps is not None:
                taps[f"enc{l}"] = enc.squeeze(3)
        x = self.mlp2d(prefix + ".mlp_mid", skips[-1])
        for j in range(L):
            a, b = int(off[L - j - 1]), int(off[L - j])
            up = _gather_pts(x.squeeze(3), interp_idx[:, a:b, 0]).unsqueeze(3)   # nearest interpolation (:393-408)
            x = self.mlp2d(f"{prefix}.decoder_blocks.{j}", torch.cat([skips[-j - 2], up], dim=1))
        feat = F.conv2d(x, self.p[prefix + ".mlp_out.weight"]).squeeze(3)
        logits = self.mlp1d(prefix + ".fc_label", feat, 3)           # dropout is identity in eval (:366)
        return feat, xyz[:, :, :N], logits

    # ------------------------------------------------------------------ score
    def score(self, feat: torch.Tensor, xyz: torch.Tensor, prob: torch.Tensor, label: torch.Tensor,
              neigh_idx: torch.Tensor) -> torch.Tensor:
        """score_fun (model.py:701-757).  feat [B,C,N], xyz [B,3,N],
        prob/label [B,1,N], neigh_idx [B,N,k] -> [B,N]."""
        B, _, N = feat.shape
        idx = neigh_idx[:, :, :16]
        fmax = feat.reshape(B, -1).max(dim=1, keepdim=True)[0]
        fn = feat / (fmax.view(B, 1, 1) + _EPS)
        saliency = F.softplus(fn - _gather_nbr(fn, idx).mean(dim=3))
        rel = _gather_nbr(xyz, idx) - xyz.unsqueeze(-1)
        density = (torch.norm(rel, dim=1, keepdim=True).mean(dim=-1) < 2.0).to(feat.dtype)
        chan = fn / (fn.max(dim=1, keepdim=True)[0] + _EPS)
        ls = self.label_weights[label.reshape(-1).long()].view(B, 1, N)
        ls = ls / (ls.max(dim=-1, keepdim=True)[0] + _EPS)
        pr = prob / (prob.max(dim=-1, keepdim=True)[0] + _EPS)
        ls = ls * torch.gt(pr, 0.2)
        return (saliency * density * chan * ls).max(dim=1)[0]

    def forward_pair(self, data: Dict[str, torch.Tensor]):
        """forward_pair with compute_score and return_flag (model.py:609-648);
        num_sub <= 0 => no top-k sub-selection (:138,682)."""
        out = []
        for k in ("points_src", "points_ref"):
            feat, xyz, logits = self.randla("feat_extractor", data[k], data[k + "_xyz"], data[k + "_neigh_idx"],
                                            data[k + "_sub_idx"], data[k + "_interp_idx"])
            prob, label = torch.max(logits, dim=1, keepdim=True)
            N = xyz.shape[2]
            s = self.score(feat, xyz, prob, label, data[k + "_neigh_idx"][:, :N])
            out += [feat, xyz, label, s]
        return tuple(out)

    @torch.no_grad()
    def forward_endpoints(self, data: Dict[str, torch.Tensor], pipeline: str, num_sub: int = -1) -> Dict[str, torch.Tensor]:
        """Network.forward of the 'feat' / 'label' pipelines = forward_pair without return_flag
        (model.py:173-179, :609-666) incl. feat_score's top-num_sub selection (:682-697).
        torch.topk's order among equal scores is unspecified; the rule here (and in select.hip) is
        descending score, equal scores (+0 == -0) in ascending index, a NaN of either sign before every number and
        NaNs among themselves in ascending index (torch's stable descending sort)."""
        ep: Dict[str, torch.Tensor] = {}
        sides = {}
        for s, k in (("src", "points_src"), ("ref", "points_ref")):
            feat, xyz, logits = self.randla("feat_extractor", data[k], data[k + "_xyz"], data[k + "_neigh_idx"],
                                            data[k + "_sub_idx"], data[k + "_interp_idx"])
            ep[f"logits_{s}"] = logits
            score = label = index = None
            if pipeline != "label":
                prob, label = torch.max(logits, dim=1, keepdim=True)
                N = xyz.shape[2]
                score = self.score(feat, xyz, prob, label, data[k + "_neigh_idx"][:, :N])
                if num_sub > 0:
                    index = torch.sort(score + 0.0, dim=-1, descending=True, stable=True)[1][:, :num_sub]
                    score = torch.gather(score, 1, index)
                    xyz, feat, label = _gather_pts(xyz, index), _gather_pts(feat, index), _gather_pts(label, index)
            sides[s] = (feat, xyz, label, score, index)
        for s in ("src", "ref"):
            feat, xyz, label, score, index = sides[s]
            if pipeline != "label":
                feat = self.aggregate(xyz, feat, score)
                ep[f"score_{s}"] = score
                ep[f"label_{s}"] = label
                if index is not None:
                    ep[f"index_{s}"] = index
            ep[f"pt_{s}"] = xyz
            ep[f"feat_{s}"] = F.normalize(feat, p=2, dim=1)
        return ep

    # ------------------------------------------------------------------ per-iteration stages
    def aggregate(self, xyz: torch.Tensor, feat0: torch.Tensor, score: torch.Tensor) -> torch.Tensor:
        """One cloud's half of ``aggregation`` (model.py:209-235):
        normalize(mlp_proj(mlp_feat(f) + mlp_att([xyz; score])))."""
        g = torch.cat((xyz, score[:, None, :]), dim=1)
        d = self.mlp1d("mlp_feat", feat0, 3) + self.mlp1d("mlp_att", g, 5)
        return F.normalize(self.mlp1d("mlp_proj", d, 1), p=2, dim=1)

    @staticmethod
    def nn_match(desc_src: torch.Tensor, desc_ref: torch.Tensor, stride: int = 6000) -> torch.Tensor:
        """arg-min over ref of (-2 a.b + |a|^2) + |b|^2 in fp32, row-chunked
        (matchnet.py:96-113, model.py:558-569) -> int64 [B,J]."""
        sb = torch.sum(desc_ref ** 2, dim=1)[:, None, :]
        out = []
        for a in range(0, desc_src.shape[2], stride):
            s = desc_src[:, :, a:a + stride]
            d = -2 * torch.matmul(s.permute(0, 2, 1).contiguous(), desc_ref)
            d += torch.sum(s ** 2, dim=1)[:, :, None]
            d += sb
            out.append(d.min(dim=2)[1])
        return torch.cat(out, dim=1)

    @staticmethod
    def nn_gap(desc_src: torch.Tensor, desc_ref: torch.Tensor, chunk: int = 2048):
        """fp64 top-2 distances per src row (test aid: how close to a tie a row is)."""
        a = desc_src.double().permute(0, 2, 1)
        b = desc_ref.double()
        sb = (b * b).sum(1)[:, None, :]
        best, second, idx = [], [], []
        for s in range(0, a.shape[1], chunk):
            x = a[:, s:s + chunk]
            d = -2 * (x @ b) + (x * x).sum(2)[:, :, None] + sb
            v, i = torch.topk(d, 2, dim=2, largest=False)
            best.append(v[..., 0]); second.append(v[..., 1]); idx.append(i[..., 0])
        return torch.cat(best, 1), torch.cat(second, 1), torch.cat(idx, 1)

    @staticmethod
    def kabsch(src: torch.Tensor, tgt: torch.Tensor, w: torch.Tensor) -> Tuple[torch.Tensor, bool]:
        """Weighted Kabsch (compute_rigid_transform_2, model.py:22-66):
        moments in the inputs' precision (fp32 as the reference's), fp64 SVD, R = V U^T with V[:,2] flipped when
        det < 0, R cast back to the inputs' precision before t = -R c_s + c_t.  SVD failure -> identity + flag."""
        wn = w / (torch.sum(torch.abs(w), dim=1, keepdim=True) + _EPS)
        cs = torch.sum(src * wn, dim=1)
        ct = torch.sum(tgt * wn, dim=1)
        H = (src - cs[:, None, :]).transpose(-2, -1).contiguous() @ ((tgt - ct[:, None, :]) * wn)
        try:
            if not torch.isfinite(H).all():
                raise RuntimeError("non-finite covariance")
            U, S, Vh = torch.linalg.svd(H.double())
            V = Vh.transpose(-1, -2)
            Rp = V @ U.transpose(-1, -2)
            Vn = V.clone()
            Vn[:, :, 2] *= -1
            Rn = Vn @ U.transpose(-1, -2)
            R = torch.where(torch.det(Rp)[:, None, None] > 0, Rp, Rn).to(src.dtype)
            t = -R @ cs[:, :, None] + ct[:, :, None]
            return torch.cat((R, t), dim=2), False
        except Exception:
            return torch.eye(3, 4, dtype=src.dtype)[None].repeat(len(src), 1, 1), True

    # ------------------------------------------------------------------ SE(3) (common/math/se3_torch.py:28-77)
    @staticmethod
    def se3_apply(T: torch.Tensor, p: torch.Tensor) -> torch.Tensor:
        return p @ T[..., :3, :3].transpose(-1, -2) + T[..., :3, 3][..., None, :]

    @staticmethod
    def se3_compose(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        Ra, ta, Rb, tb = a[..., :3, :3], a[..., :3, 3], b[..., :3, :3], b[..., :3, 3]
        return torch.cat([Ra @ Rb, Ra @ tb[..., None] + ta[..., None]], dim=-1)

    # ------------------------------------------------------------------ driver
    @torch.no_grad()
    def register(self, data: Dict[str, torch.Tensor], num_reg_iter: int = 5,
                 forced_idx: Optional[Sequence[torch.Tensor]] = None, taps: Optional[dict] = None):
        """forward_align_4 (model.py:520-607).  ``forced_idx`` teacher-forces
        the arg-min correspondences per iteration (test aid)."""
        f_s, x_s, lab_s, sc_s, f_r, x_r, lab_r, sc_r = self.forward_pair(data)
        ep = {"pt_src": x_s.permute(0, 2, 1).contiguous(), "pt_ref": x_r.permute(0, 2, 1).contiguous(),
              "perm_matrices": [], "pred_pairs": [], "invalid_gradient": False}
        if taps is not None:
            taps.update(feat_src=f_s, feat_ref=f_r, score_src=sc_s, score_ref=sc_r, desc_src=[], desc_ref=[])
        transforms: List[torch.Tensor] = []
        xyz = x_s
        for it in range(num_reg_iter):
            d_s = self.aggregate(xyz, f_s, sc_s)
            d_r = self.aggregate(x_r, f_r, sc_r)
            idx = self.nn_match(d_s, d_r) if forced_idx is None else forced_idx[it].long()
            ref_new = _gather_pts(x_r, idx)
            cat = torch.cat((xyz, ref_new), dim=1).permute(0, 2, 1).contiguous()
            _, _, logit = self.randla("inlier_model", cat, data["points_src_xyz"], data["points_src_neigh_idx"],
                                      data["points_src_sub_idx"], data["points_src_interp_idx"])
            logit = logit.squeeze(1)
            w = logit.sigmoid()[:, :, None]
            p_s = xyz.permute(0, 2, 1).contiguous()
            p_r = ref_new.permute(0, 2, 1).contiguous()
            T, bad = self.kabsch(p_s, p_r, w)
            xyz = self.se3_apply(T, p_s).permute(0, 2, 1).contiguous()
            transforms.append(T if it == 0 else self.se3_compose(T, transforms[-1]))
            ep["perm_matrices"].append(logit)
            ep["invalid_gradient"] = ep["invalid_gradient"] or bad
            J = idx.shape[1]
            ar = torch.arange(J, dtype=torch.int32)[None, :, None].expand(idx.shape[0], J, 1)
            ep["pred_pairs"].append(torch.cat([ar, idx.int()[:, :, None]], dim=2))
            ep["pt_ref_new"] = p_r
            if taps is not None:
                taps["desc_src"].append(d_s); taps["desc_ref"].append(d_r)
        return transforms, ep


def to_torch(data: Dict[str, np.ndarray], dtype: Optional[torch.dtype] = None) -> Dict[str, torch.Tensor]:
    """Index arrays -> int64; floating arrays -> ``dtype`` (None: as they are)."""
    out = {}
    for k, v in data.items():
        t = torch.from_numpy(np.ascontiguousarray(v))
        if t.dtype in (torch.int32, torch.int64):
            t = t.long()
        elif dtype is not None and t.is_floating_point():
            t = t.to(dtype)
        out[k] = t
    return out
