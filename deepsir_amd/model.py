"""Drop-in for the reference's ``network.model.Network`` (align, feat and label pipelines: inference, and the optimisation
step of each through ``Network.train_step``).

Keeps the reference's host API verbatim (reference network/model.py:119-195,
:297-298, :520-607; test.py:609-614):

    net = Network(args); net.load_state_dict(torch.load(p)['state_dict'])
    net.to(device); net.eval()
    transforms, endpoints = net(data, (num_reg_iter, clip_weight))

but everything inside ``forward`` runs in libdsir.so (hand-written HIP for
gfx950) through the C ABI of include/dsir.h.  The module holds the
checkpoint tensors as buffers under the reference's key names so that
``state_dict()`` / ``load_state_dict()`` round-trip a reference checkpoint.
There is no CPU path: calling it without the built library or without a GPU
raises.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from collections.abc import Sequence

from .arch import NetConfig, network_specs
from . import graph_replay_safe
from .engine import Engine, EngineError, EnginePool

_PYR_KEYS = ("xyz", "neigh_idx", "sub_idx", "interp_idx")


class _Node(nn.Module):
    """Name-space node of the checkpoint tree (no computation)."""


def _attach(root: nn.Module, dotted: str, tensor: torch.Tensor, trainable: bool, requires_grad: bool):
    """Trainable tensors are ``nn.Parameter``s under the reference's names and in its registration order, so that
    ``optim.Adam(my_model.parameters(), lr)`` (reference train.py:323) constructs and ``named_parameters()`` reads as the
    reference's; BatchNorm running statistics stay buffers."""
    parts = dotted.split(".")
    m = root
    for p in parts[:-1]:
        if p not in m._modules:
            m.add_module(p, _Node())
        m = m._modules[p]
    if trainable:
        m.register_parameter(parts[-1], nn.Parameter(tensor, requires_grad=requires_grad))
    else:
        m.register_buffer(parts[-1], tensor)


def _requires_grad(pipeline: str, name: str) -> bool:
    """freeze_model / freeze_model_2 (reference model.py:196-207): 'label' trains the extractor; 'feat' freezes it; 'align'
    also freezes the aggregation layers and trains the inlier model alone."""
    top = name.split(".", 1)[0]
    if pipeline == "label":
        return True
    if pipeline == "feat":
        return top != "feat_extractor"
    return top == "inlier_model"


class _LazyPredPairs(Sequence):
    """``endpoints['pred_pairs']``: per iteration an int32 CPU tensor [B, J, 2] of (src row, matched ref row) as the reference
    builds it (model.py:603-606).  The device-to-host copy - a device synchronisation - is deferred until an element is READ:
    a caller that only wants the poses never waits for it."""

    def __init__(self, idx_dev: torch.Tensor):
        self._idx, self._items = idx_dev, None          # [n_iter, B, J] int32 on the device

    def _materialise(self):
        if self._items is None:
            idx = self._idx.cpu()
            n, B, J = idx.shape
            ar = torch.arange(J, dtype=torch.int32)[None, :, None].expand(B, J, 1)
            self._items = [torch.cat([ar, idx[i][:, :, None]], dim=2) for i in range(n)]
            self._idx = None
        return self._items

    def __len__(self):
        return len(self._items) if self._items is not None else int(self._idx.shape[0])

    def __getitem__(self, i):
        return self._materialise()[i]


class _LazyFlag:
    """``endpoints['invalid_gradient']`` (model.py:61-64): truth value read from the device only when asked for."""

    def __init__(self, invalid_dev: torch.Tensor):
        self._t, self._v = invalid_dev, None

    def __bool__(self):
        if self._v is None:
            self._v = bool((self._t & 1).any().item())   # bit 0 = SVD failure
            self._t = None
        return self._v

    def __eq__(self, other):
        return bool(self) == other

    def __repr__(self):
        return repr(bool(self))


class _TrainState:
    """The training state of one ``Network``, shared by the training-mode forward and ``train_step``: the pipeline's trainers
    (deepsir_amd/train.py), whose flat device buffers ARE the module's parameters and BatchNorm running statistics.
    ``main`` receives gradients and holds the Adam moments and step count; ``frozen`` only move their running statistics."""

    def __init__(self, dev: torch.device, main, frozen: tuple, names: List[str], params: List[nn.Parameter]):
        self.dev, self.main, self.frozen = dev, main, frozen
        self.names, self.params = names, params          # what receives gradients, in ``main``'s order
        self.engine: Optional[Engine] = None             # the training forward's own engine (Network._train_engine)
        self.stepper = self.stepper_key = None           # AlignTrainStep of train_step(frozen_mode='eval'): fixed batch geometry


class Network(nn.Module):
    POOL_MIN_PAIRS = 64
    """Batches of that many pairs and more run on an ``EnginePool`` (two HIP streams): same bits, higher throughput."""
    SERVE_MAX_PAIRS = 8
    """Batches of up to that many pairs (the reference evaluates ONE, test.py:56) go through a ``PairServer``: the launch
    sequence replayed from a captured hipGraph on one of two engines in turn, no host synchronisation in ``forward`` - the
    results are ordered on torch's current stream, consecutive calls overlap until the caller reads a result."""

    def __init__(self, args):
        super().__init__()
        self.cfg = NetConfig.from_args(args)
        self.pipeline = self.cfg.pipeline
        if self.pipeline not in ("align", "feat", "label"):
            raise AssertionError("pipeline must be 'align', 'feat' or 'label' (reference model.py:131)")
        if self.pipeline == "align" and self.cfg.num_sub > 0:
            # the reference's inlier model runs on the FULL src pyramid (model.py:575): it cannot follow a top-k selection
            raise NotImplementedError("num_sub > 0 with pipeline='align' is not runnable in the reference either")
        self.num_sub, self.num_knn, self.d_out = self.cfg.num_sub, self.cfg.num_knn, self.cfg.out_feat_dim
        self.clip_weight_thresh = getattr(args, "clip_weight_thresh", 0.0)
        # use_ppf (RandLANet.py:251-254, :324-332): inference and the training-mode forward in all three pipelines.  Two fields the reference lacks: clouds
        # without normals (3DMatch, KITTI rows) get them from the engine's own rule (deepsir_amd/ppf.py) when asked to.
        self.ppf_estimate_normals = bool(getattr(args, "ppf_estimate_normals", False))
        self.ppf_viewpoint = tuple(float(x) for x in getattr(args, "ppf_viewpoint", (0.0, 0.0, 0.0)))
        # the engines read rows of exactly xyz + normal under use_ppf (_ppf_rows); no state-dict shape depends on feat_len there
        self._engine_cfg = dataclasses.replace(self.cfg, feat_len=6) if self.cfg.use_ppf else self.cfg
        for spec in network_specs(self.cfg):
            dtype = torch.int64 if spec.kind == "bn_count" else torch.float32
            trainable = spec.kind not in ("bn_mean", "bn_var", "bn_count")
            _attach(self, spec.name, torch.zeros(spec.shape, dtype=dtype), trainable, _requires_grad(self.pipeline, spec.name))
        self._engine: Optional[Engine] = None
        self._pool: Optional[EnginePool] = None
        self._dirty = True
        self._pool_dirty = True
        self._max_points = 0
        self._max_pairs = 0
        self._pool_points = 0
        self._pool_pairs = 0
        self._seen_version = -1
        self._server = None
        self._server_dirty = True
        # the loss modules the reference's training loop calls (model.py:173-195; train.py:409, :421, :426): call contract restated
        # over the HIP loss operators (deepsir_amd/autograd.py)
        from .autograd import DetDesLoss, ScanAlignmentLoss, SemanticLoss
        if self.pipeline == "align":
            self.loss_align_fun = ScanAlignmentLoss(self, args)
        elif self.pipeline == "feat":
            self.loss_feat_fun = DetDesLoss(self, args)
        else:
            self.loss_label_fun = SemanticLoss(self, args)
        self._tstate: Optional[_TrainState] = None    # built by the first training call (_training_state)
        self.dropout_masks = None         # test aid: {'fe_src', 'fe_ref', 'inlier'} keep flags instead of random Dropout draws

    # ---- checkpoint plumbing
    def load_state_dict(self, state_dict, strict: bool = True):
        r = super().load_state_dict(state_dict, strict=strict)
        self._dirty = self._pool_dirty = self._server_dirty = True
        self._tstate = None           # Adam moments and step count start again; rebuilt over the new weights by the next training call
        return r

    def _device_index(self) -> int:
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise EngineError("Network is on the CPU: this engine has no CPU path; call .to('cuda') / .cuda() first")
        return dev.index or 0

    def _check_weights_touched(self):
        """An optimiser (or any in-place write) that changed a parameter bumps its version counter: the engines reload."""
        v = sum(p._version for p in self.parameters()) + sum(b._version for b in self.buffers())
        if v != self._seen_version:
            self._dirty = self._pool_dirty = self._server_dirty = True
            self._seen_version = v

    def _ensure_pool(self, n_points: int, pairs: int) -> EnginePool:
        dev = self._device_index()
        self._check_weights_touched()
        if self._pool is None or n_points > self._pool_points or pairs > self._pool_pairs:
            if self._pool is not None:
                self._pool.close()
            self._pool_points = max(self._pool_points, n_points, 1024)
            self._pool_pairs = max(self._pool_pairs, pairs)
            self._pool = EnginePool(self._engine_cfg, dev, self._pool_points, self._pool_pairs, streams=2)
            self._pool_dirty = True
        if self._pool_dirty:
            self._pool.load_state_dict({k: v for k, v in self.state_dict().items()})
            self._pool_dirty = False
        return self._pool

    def _ensure_server(self, n_points: int, n_iter: int):
        from .serve import PairServer
        dev = self._device_index()
        self._check_weights_touched()
        srv = getattr(self, "_server", None)
        if srv is None or n_points > srv.max_points or srv.n_iter != n_iter:
            if srv is not None:
                srv.close()
            self._server = srv = PairServer(self._engine_cfg, {k: v for k, v in self.state_dict().items()}, dev, max(n_points, 1024),
                                            2 * self.SERVE_MAX_PAIRS, 2, n_iter, True)
            self._server_dirty = False
        if self._server_dirty:       # new weights (load_state_dict, an optimiser step): reloaded into the running engines
            srv.load_state_dict({k: v for k, v in self.state_dict().items()})
            self._server_dirty = False
        return srv

    def serve(self, max_points: int = 5000, max_in_flight: int = 8, engines: Optional[int] = None, n_iter: Optional[int] = None, want_aux: bool = True):
        """A ``deepsir_amd.serve.PairServer`` on this network's weights: K single-pair registrations in flight
        (the reference's batch-1 evaluation mode, test.py:56, fed ahead)."""
        from .serve import PairServer
        return PairServer(self._engine_cfg, {k: v for k, v in self.state_dict().items()}, self._device_index(), max_points, max_in_flight,
                          engines, self.cfg.num_reg_iter if n_iter is None else n_iter, want_aux)

    def _ensure_engine(self, n_points: int, pairs: int) -> Engine:
        dev = self._device_index()
        self._check_weights_touched()
        if self._engine is None or n_points > self._max_points or pairs > self._max_pairs:
            if self._engine is not None:
                self._engine.close()
            self._max_points = max(self._max_points, n_points, 1024)
            self._max_pairs = max(self._max_pairs, pairs)
            self._engine = Engine(self._engine_cfg, dev, self._max_points, self._max_pairs)
            self._dirty = True
        if self._dirty:
            self._engine.load_state_dict({k: v for k, v in self.state_dict().items()})
            self._dirty = False
        return self._engine

    # ---- forward = forward_pair for 'feat' / 'label' (model.py:173-179, :609-666)
    def _forward_pair(self, eng: Engine, src, ref, pyr):
        out = eng.forward_pair(src.float(), ref.float(), self.cfg.num_sub, pyramids=pyr)
        endpoints = {}
        for side in ("src", "ref"):
            o = out[side]
            endpoints[f"pt_{side}"] = o["xyz"].permute(0, 2, 1).contiguous()          # [B, 3, M]
            endpoints[f"feat_{side}"] = o["feat"].permute(0, 2, 1).contiguous()       # [B, C, M]
            endpoints[f"logits_{side}"] = o["logits"].permute(0, 2, 1).contiguous()   # [B, num_class, N]
            if self.pipeline != "label":
                endpoints[f"score_{side}"] = o["score"]                               # [B, M]
        return None, endpoints

    # ---- forward in TRAINING mode (train.py:379 my_model.train(); :401): outputs with a grad_fn that leads into the parameters
    def _training_state(self, dev: torch.device) -> _TrainState:
        """The pipeline's trainers (deepsir_amd/train.py) over THIS module's tensors: from the first training call on a trainable
        ``nn.Parameter`` (and every BatchNorm running statistic) is a view of its trainer's flat device buffer, so what
        ``optimizer.step()`` or ``train_step`` writes is what the next training forward computes with - no copies either way."""
        from . import train as T
        st = self._tstate
        named = dict(self.named_parameters())
        named.update(dict(self.named_buffers()))
        if st is not None:
            k0, v0 = next(iter(st.main.params.items()))
            if st.dev == dev and named[k0].data_ptr() == v0.data_ptr():
                return st
        sd = self.state_dict()
        extractor = lambda: T.RandlaTrainer(self.cfg, sd, "feat_extractor", self.cfg.feat_len, self.cfg.num_classes, dev)
        if self.pipeline == "align":
            main, frozen = T.RandlaTrainer(self.cfg, sd, "inlier_model", 6, 1, dev), (extractor(), T.AggregationTrainer(self.cfg, sd, dev))
        elif self.pipeline == "label":
            main, frozen = extractor(), ()
        else:
            main, frozen = T.AggregationTrainer(self.cfg, sd, dev), (extractor(),)
        with torch.no_grad():
            for tr in (main,) + frozen:
                for k, v in list(tr.params.items()) + list(tr.buffers.items()):
                    named[k].data = v.view(named[k].shape)
        names = [k for k in main.params if named[k].requires_grad]
        self._tstate = st = _TrainState(dev, main, frozen, names, [named[k] for k in names])
        return st

    def _no_ppf_train_step(self):
        """``train_step`` alone still refuses a use_ppf network: its callers hand it raw loader rows, and the normals hand-over of
        ``_ppf_rows`` is not wired into it.  The trainers and the training-mode forward do train under use_ppf."""
        if self.cfg.use_ppf:
            raise NotImplementedError("train_step with use_ppf=True is not built: train a use_ppf network through the training-mode forward "
                                      "(net.train(); net(data, opt); loss.backward(); optimizer.step()) or the trainers of deepsir_amd.train")

    def _train_engine(self, st: _TrainState, n_points: int, pairs: int) -> Engine:
        """The weight-free operators of the training forward (score, arg-min, Kabsch, loss)."""
        eng = st.engine
        have = (eng.max_points, eng.max_pairs) if eng is not None else (1024, 1)
        if eng is None or n_points > have[0] or pairs > have[1]:
            # an outgrown engine is not closed: the endpoints of an earlier forward may still hold it for their loss (_AlignLoss);
            # Engine.__del__ frees it once the last of them is gone
            st.engine = eng = Engine(self._engine_cfg, st.dev.index or 0, max(n_points, have[0]), max(pairs, have[1]))
            eng.load_state_dict({k: v for k, v in self.state_dict().items()})
        return eng

    def _pyramids(self, eng: Engine, data, src, ref) -> dict:
        batch = {"points_src": src, "points_ref": ref}
        for s_, pts in (("src", src), ("ref", ref)):
            if all(f"points_{s_}_{k}" in data for k in _PYR_KEYS):
                pyr = [data[f"points_{s_}_xyz"].float()] + [data[f"points_{s_}_{k}"].to(torch.int32) for k in _PYR_KEYS[1:]]
            else:
                pyr = eng.knn_pyramid(pts)
            batch[f"{s_}_xyz"], batch[f"{s_}_neigh"], batch[f"{s_}_sub"], batch[f"{s_}_interp"] = [t.contiguous() for t in pyr]
        return batch

    def _draw_masks(self, shapes: Dict[str, tuple], dev) -> Optional[dict]:
        """Dropout(0.5) keep flags of one training forward (RandLANet.py:363-367): drawn from torch's global generator like
        nn.Dropout's, unless the test aid ``self.dropout_masks`` supplies them."""
        from . import train as T
        if self.dropout_masks is not None:
            return self.dropout_masks
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
        return {k: T.dropout_keep_masks(seed + 7919 * i, shp, dev) for i, (k, shp) in enumerate(shapes.items())}

    @staticmethod
    def _seeded_masks(seed: Optional[int], B: int, J: int, K: int, dev, n_iter: Optional[int] = None) -> Optional[dict]:
        """Keep flags of one ``train_step`` with ``dropout_seed`` (None: dropout off): the frozen extractor's from 3 seed + 1 (src) and
        3 seed + 2 (ref); with ``n_iter`` the inlier model's from the seed itself, as the frozen_mode='eval' variant draws them."""
        from . import train as T
        if seed is None:
            return None
        masks = {"fe_src": T.dropout_keep_masks(3 * int(seed) + 1, (B, J, 64), dev), "fe_ref": T.dropout_keep_masks(3 * int(seed) + 2, (B, K, 64), dev)}
        if n_iter is not None:
            masks["inlier"] = T.dropout_keep_masks(int(seed), (n_iter, B, J, 64), dev)
        return masks

    def _forward_train(self, data: Dict[str, torch.Tensor], opt=None):
        from . import se3
        from . import train as T
        from .autograd import run_taped
        src, ref = data["points_src"].float().contiguous(), data["points_ref"].float().contiguous()
        if not src.is_cuda:
            raise EngineError("Network is on the CPU: this engine has no CPU path; call .to('cuda') / .cuda() first")
        dev = src.device
        B, J, _ = src.shape
        K = ref.shape[1]
        st = self._training_state(dev)
        eng = self._train_engine(st, max(J, K), B)
        if self.cfg.use_ppf:
            # rows of xyz + normal for the point-pair-feature layer (RandLANet.py:325-326); normals that have to be estimated come from
            # the training engine itself (weight-free operators), and the pyramid built for them is handed on
            have = all(f"points_{s}_{k}" in data for s in ("src", "ref") for k in _PYR_KEYS)
            src, ref, pyr = self._ppf_rows(src, ref, {f"points_{s}_{k}": data[f"points_{s}_{k}"] for s in ("src", "ref") for k in _PYR_KEYS} if have else None, eng)
            if pyr is not None:
                data = {**data, **pyr}
        main, frozen, params, names = st.main, st.frozen, st.params, st.names
        batch = self._pyramids(eng, data, src, ref)
        self._dirty = self._pool_dirty = self._server_dirty = True      # running statistics move now, the weights at optimizer.step()

        # every backward starts with zero_grad (the flat gradient buffer and the scatter plans) and returns its OWN tape's
        # gradient, which autograd adds into param.grad: two training forwards alive before their backwards (or one backward of
        # loss_A + loss_B) give gA + gB, as torch's autograd does.  The forward needs no plan (only the backward scatters).
        def taped(outputs, backward):
            """``run_taped``'s pair for the main trainer: ``backward(grads)`` walks this forward's tapes back into ``main.grads``."""
            def back(grads):
                main.zero_grad()
                backward(grads)
                g = main.flat_g.clone()       # ONE copy: autograd may keep what it is handed, the trainer's buffer is zeroed by the next backward
                out = []
                for k, p in zip(names, params):
                    v = main.grads[k]
                    off = v.data_ptr() - main.flat_g.data_ptr()
                    out.append(g[off // 4: off // 4 + v.numel()].view(p.shape))
                return out
            return outputs, back

        if self.pipeline == "align":
            n_iter = int(opt[0]) if opt is not None else self.cfg.num_reg_iter
            fe, ag = frozen
            masks = self._draw_masks({"fe_src": (B, J, 64), "fe_ref": (B, K, 64), "inlier": (n_iter, B, J, 64)}, dev)
            box = {}

            def run():
                fw = T.forward_align_train(eng, main, fe, ag, batch, n_iter, masks)
                box["fw"] = fw
                return taped((fw["logits"],), lambda grads: T.inlier_backwards(main, fw["tapes"], grads[0], fw["shared"]))

            (logits,) = run_taped(params, run, 1)
            fw = box["fw"]
            transforms, cum = [], None
            for it in range(n_iter):                                   # se3_torch.concatenate(R_t, transforms[-1]), model.py:595
                cum = fw["T"][it] if cum is None else se3.concatenate(fw["T"][it], cum)
                transforms.append(cum.detach())
            invalid = fw["invalid"][0]
            for f_ in fw["invalid"][1:]:
                invalid = invalid | f_
            endpoints = {"pt_src": src[:, :, :3].contiguous(), "pt_ref": ref[:, :, :3].contiguous(),
                         "perm_matrices": [logits[i] for i in range(n_iter)], "pred_pairs": _LazyPredPairs(fw["idx"]),
                         "invalid_gradient": _LazyFlag(invalid), "pt_ref_new": fw["pt_ref_new"],
                         "_train": {"engine": eng, "idx": fw["idx"], "logits": logits}}
            return transforms, endpoints

        if self.pipeline == "label":
            masks = self._draw_masks({"fe_src": (B, J, 64), "fe_ref": (B, K, 64)}, dev)
            box = {}

            def run():
                outs, tapes = [], []
                for s_ in ("src", "ref"):
                    lg, tape = main.forward(batch[f"points_{s_}"], batch[f"{s_}_xyz"], batch[f"{s_}_neigh"], batch[f"{s_}_sub"], batch[f"{s_}_interp"],
                                            masks.get(f"fe_{s_}"))
                    outs.append(lg); tapes.append(tape)
                box["tapes"] = tapes

                def backward(grads):
                    for tape, g, lg in zip(tapes, grads, outs):
                        if g is not None:
                            main.backward(tape, g.reshape(-1, lg.shape[-1]).contiguous())
                return taped(tuple(outs), backward)

            lg_s, lg_r = run_taped(params, run, 2)
            endpoints = {}
            for s_, lg, tape, pts in (("src", lg_s, box["tapes"][0], src), ("ref", lg_r, box["tapes"][1], ref)):
                endpoints[f"pt_{s_}"] = pts[:, :, :3].permute(0, 2, 1).contiguous()
                endpoints[f"feat_{s_}"] = torch.nn.functional.normalize(tape.misc["feat"].detach(), dim=2).permute(0, 2, 1).contiguous()
                endpoints[f"logits_{s_}"] = lg.permute(0, 2, 1)
            return None, endpoints

        # feat: the frozen extractor in training mode picks the key points, the aggregation layers are taped
        if self.cfg.num_sub <= 0:
            raise EngineError("pipeline='feat' trains on the top-num_sub key points: set args.num_sub > 0")
        masks = self._draw_masks({"fe_src": (B, J, 64), "fe_ref": (B, K, 64)}, dev)
        inp = T.feat_pipeline_inputs_train(eng, frozen[0], batch, self.cfg.num_sub, masks)

        def run():
            d_s, tape_s = main.forward(inp["xyz_src"], inp["feat_src"], inp["score_src"])
            d_r, tape_r = main.forward(inp["xyz_ref"], inp["feat_ref"], inp["score_ref"])

            def backward(grads):
                for tape, g in ((tape_s, grads[0]), (tape_r, grads[1])):
                    if g is not None:
                        main.backward(tape, g)
            return taped((d_s, d_r), backward)

        d_s, d_r = run_taped(params, run, 2)
        endpoints = {}
        for s_, d in (("src", d_s), ("ref", d_r)):
            endpoints[f"pt_{s_}"] = inp[f"xyz_{s_}"].permute(0, 2, 1).contiguous()
            endpoints[f"feat_{s_}"] = d.permute(0, 2, 1)
            endpoints[f"score_{s_}"] = inp[f"score_{s_}"]
        return None, endpoints

    # ---- forward = forward_align_4 for 'align'
    def forward(self, data: Dict[str, torch.Tensor], opt=None):
        """Evaluation mode (or under ``torch.no_grad()``): the inference engine.  Training mode with gradients enabled - the state the
        reference's loop calls it in (train.py:379, :401) - the training forward on the device, outputs carrying a grad_fn."""
        if self.training and torch.is_grad_enabled():
            return self._forward_train(data, opt)
        with torch.no_grad():
            return self._forward_eval(data, opt)

    def _forward_eval(self, data: Dict[str, torch.Tensor], opt=None):
        src, ref = data["points_src"], data["points_ref"]
        B, J, _ = src.shape
        K = ref.shape[1]
        have = all(f"points_{s}_{k}" in data for s in ("src", "ref") for k in _PYR_KEYS)
        pyr = {f"points_{s}_{k}": data[f"points_{s}_{k}"] for s in ("src", "ref") for k in _PYR_KEYS} if have else None
        if self.cfg.use_ppf:
            src, ref, pyr = self._ppf_rows(src, ref, pyr)
        if self.pipeline != "align":
            return self._forward_pair(self._ensure_engine(max(J, K), B), src, ref, pyr)
        num_reg_iter, _clip_weight = opt  # clip_weight is ignored by the reference too (model.py:581-582)
        # the served path replays captured hipGraphs: only where replay is known to be right in this process (deepsir_amd/__init__.py);
        # a caller that had touched the GPU before importing the package keeps the eager engine below - same bits, host-synchronised
        if B <= self.SERVE_MAX_PAIRS and pyr is None and src.is_cuda and graph_replay_safe():
            out = self._ensure_server(max(J, K), int(num_reg_iter)).submit_batch(src.float(), ref.float()).result(wait="stream")
            return self._align_outputs(out, src, ref, int(num_reg_iter))
        # large batches: two engines on two HIP streams (EnginePool) - same bits, the throughput configuration of bench.py
        eng = self._ensure_pool(max(J, K), B) if B >= self.POOL_MIN_PAIRS else self._ensure_engine(max(J, K), B)
        if pyr is not None and isinstance(eng, EnginePool):
            pyr = {k: (v if v.dtype != torch.int64 else v.to(torch.int32)) for k, v in pyr.items()}
        out = eng.register(src.float(), ref.float(), int(num_reg_iter), pyramids=pyr)
        return self._align_outputs(out, src, ref, int(num_reg_iter))

    def _ppf_rows(self, src, ref, pyr, eng: Optional[Engine] = None):
        """use_ppf: rows of xyz + normal for the engine (RandLANet.py:325-326).  Clouds that carry them pass through (columns
        beyond 6 are not read by the reference either); clouds that do not get normals from ``Engine.estimate_normals`` on the
        pyramid the registration needs anyway - handed on, not built twice - when ``args.ppf_estimate_normals`` says so; else the
        reference's assertion.  eng: the engine to estimate with (the training forward hands its own; default: the inference engine)."""
        if src.shape[2] >= 6 and ref.shape[2] >= 6:
            return src[:, :, :6].float().contiguous(), ref[:, :, :6].float().contiguous(), pyr
        if not self.ppf_estimate_normals:
            raise AssertionError("feature dimension error")       # RandLANet.py:325
        if eng is None:
            eng = self._ensure_engine(max(src.shape[1], ref.shape[1]), src.shape[0])
        out, rows = {}, []
        for s_, pts in (("src", src), ("ref", ref)):
            pts = pts.float().contiguous()
            if pyr is not None:
                py = [pyr[f"points_{s_}_xyz"].float().contiguous()] + [eng.narrow(pyr[f"points_{s_}_{k}"]) for k in _PYR_KEYS[1:]]
            else:
                py = list(eng.knn_pyramid(pts))
            normals, _ = eng.estimate_normals(pts, py[1].reshape(pts.shape[0], -1, 16), self.ppf_viewpoint)
            rows.append(torch.cat([pts[:, :, :3], normals], dim=2).contiguous())
            for k, t in zip(_PYR_KEYS, py):
                out[f"points_{s_}_{k}"] = t
        return rows[0], rows[1], out

    @staticmethod
    def _align_outputs(out, src, ref, num_reg_iter: int):
        transforms: List[torch.Tensor] = [out["transforms"][:, i].contiguous() for i in range(num_reg_iter)]
        endpoints = {
            "pt_src": src[:, :, :3].contiguous(),
            "pt_ref": ref[:, :, :3].contiguous(),
            "perm_matrices": [out["logits"][i] for i in range(num_reg_iter)],
            "pred_pairs": _LazyPredPairs(out["idx"]),          # CPU tensors like the reference's, copied when first read
            "invalid_gradient": _LazyFlag(out["invalid"]),     # model.py:61-64; read from the device when tested
            "pt_ref_new": out["pt_ref_new"],
        }
        return transforms, endpoints

    # ---- one optimisation step of the pipeline: train.py:396-448 without autograd (deepsir_amd/train.py)
    def train_step(self, data: Dict[str, torch.Tensor], opt=None, lr: float = 1e-3, dropout_seed: Optional[int] = None,
                   thres_radius: float = 0.1, det_loss_weight: float = 1.0, loss_kwargs: Optional[dict] = None, dist=None,
                   frozen_mode: str = "train", match_radius: Optional[float] = None, wt_pose_loss: Optional[float] = None) -> dict:
        """What the reference's loop does per batch - ``my_model(train_data, opt)``, ``loss_*_fun``, ``loss.backward()``,
        ``optimizer.step()`` (train.py:396-448) - for this network's pipeline, on the device:
          align: trains ``inlier_model`` (the only sub-network ScanAlignmentLoss reaches; data: transform_gt [B,3,4] and,
                 for the confidence term, ``matches`` = per pair an int [n',2] array as the reference's data loader gives, or a
                 ``train.MatchKeys``; without a list, ``match_radius`` - the argument or data['match_radius'] - gives the same
                 targets from the geometry: (j, idx[j]) is a match iff |T_gt src_j - ref_idx[j]| < radius.  The targets are
                 made on the device, ``deepsir_amd.train.inlier_targets``).
                 wt_pose_loss: the weight of the loss's pose-error term (loss.py:830-842); None reads ``args.wt_pose_loss`` (0 = off).
                 frozen_mode 'train' (default): the whole network in training mode as ``my_model.train()`` leaves it - the
                 frozen sub-networks' BatchNorm on batch statistics, their running statistics moving, Dropout on
                 (``train_step_align_full``); 'eval': the frozen half from ONE inference pass of the engine (faster; the
                 correspondences are those of the evaluation-mode network);
          label: trains ``feat_extractor`` through SemanticLoss (data: labels_src / labels_ref [B,N] in 0..19);
          feat:  trains ``mlp_feat`` / ``mlp_att`` / ``mlp_proj`` through DetDesLoss (data: transform_gt; needs num_sub > 0); frozen_mode
                 as for align: 'train' runs the frozen extractor in training mode, 'eval' takes the key points from the engine.
        The step updates this module's own tensors - they are views of the trainers' device buffers (``_training_state``), shared with
        the training-mode forward - so ``state_dict()`` is the trained checkpoint and the next ``forward`` serves it.  Adam state lives
        in that state's main trainer; ``load_state_dict`` resets it.  Returns the step's dict (loss ...)."""
        from . import train as T
        self._no_ppf_train_step()
        src, ref = data["points_src"].float(), data["points_ref"].float()
        B, J, _ = src.shape
        K = ref.shape[1]
        dev = src.device
        eng = self._ensure_engine(max(J, K), B)
        st = self._training_state(dev)
        tr = st.main
        batch = self._pyramids(eng, data, src, ref)
        # the confidence term's 0/1 targets, on the device (deepsir_amd/train.py::inlier_targets): from the caller's match list - its
        # keys are built ONCE per step, not per iteration -, else from the radius and the geometry, else no term
        targets = None
        if wt_pose_loss is None:
            wt_pose_loss = (loss_kwargs or {}).get("wt_pose_loss", getattr(getattr(self, "loss_align_fun", None), "wt_pose_loss", 0.0))
        wt_pose = float(wt_pose_loss)
        if loss_kwargs and "wt_pose_loss" in loss_kwargs:
            loss_kwargs = {k: v for k, v in loss_kwargs.items() if k != "wt_pose_loss"}
        if self.pipeline == "align":
            radius = data.get("match_radius", match_radius)
            if "matches" in data:
                m = data["matches"]
                tr.ops.begin()
                targets = {"matches": m if isinstance(m, T.MatchKeys) else tr.ops.match_keys(m, J)}
            elif radius is not None:
                targets = {"match_radius": float(radius), "src": src, "ref": ref, "transform_gt": data["transform_gt"].to(dev)}
        if self.pipeline == "align" and frozen_mode == "train":
            n_iter = int(opt[0]) if opt is not None else self.cfg.num_reg_iter
            fe, ag = st.frozen
            fn = None
            if targets is not None:
                fn = lambda idx: T.inlier_targets(tr.ops, idx, J, **targets)
            out = T.train_step_align_full(eng, tr, fe, ag, batch, data["transform_gt"].float().to(dev), n_iter, fn, lr,
                                          self._seeded_masks(dropout_seed, B, J, K, dev, n_iter), loss_kwargs, dist=dist, wt_pose_loss=wt_pose)
            out["loss"] = out["losses"]["total"]
        elif self.pipeline == "align":
            n_iter = int(opt[0]) if opt is not None else self.cfg.num_reg_iter
            res = eng.register(src, ref, n_iter)
            labels = None if targets is None else T.inlier_targets(tr.ops, res["idx"], J, **targets)
            key = (id(eng), B, J, K, n_iter, wt_pose)
            if st.stepper_key != key:                                           # hipGraph-replayed halves, fixed batch geometry and loss weight
                st.stepper, st.stepper_key = T.AlignTrainStep(eng, tr, B, J, K, n_iter, wt_pose_loss=wt_pose), key
            out = st.stepper.step(batch, res, data["transform_gt"].float().to(dev), labels, lr, dropout_seed, loss_kwargs, dist=dist)
            out["loss"] = out["losses"]["total"]
        elif self.pipeline == "label":
            out = T.train_step_label(tr, batch, data["labels_src"].to(torch.int32).to(dev), data["labels_ref"].to(torch.int32).to(dev), lr,
                                     dropout_seed, dist=dist)
        else:
            if self.cfg.num_sub <= 0:
                raise EngineError("pipeline='feat' trains on the top-num_sub key points: set args.num_sub > 0")
            if frozen_mode == "train":      # the frozen extractor in training mode, as my_model.train() leaves it
                inp = T.feat_pipeline_inputs_train(eng, st.frozen[0], batch, self.cfg.num_sub, self._seeded_masks(dropout_seed, B, J, K, dev))
            else:
                inp = T.feat_pipeline_inputs(eng, batch, self.cfg.num_sub)
            out = T.train_step_feat(tr, inp, data["transform_gt"].float().to(dev), thres_radius, det_loss_weight, lr, dist=dist)
        # on skipped steps too: the parameters are then unchanged, but the BatchNorm running statistics moved in the forward pass
        # whatever optimizer.step() did afterwards (train.py:401 runs before :437-446).  The kernels wrote the shared buffers
        # directly, which bumps no version counter (_check_weights_touched): the inference engines are told here.
        self._dirty = self._pool_dirty = self._server_dirty = True
        return out

    # ---- the optimiser's checkpoint entry (CheckPointManager saves optimizer.state_dict(), common/torch_utils.py:62-67)
    def _param_order(self) -> List[str]:
        """``my_model.parameters()`` order = the state-dict order without the buffers (train.py:323 hands it to Adam)."""
        return [sp.name for sp in network_specs(self.cfg) if sp.kind not in ("bn_mean", "bn_var", "bn_count")]

    def optimizer_state_dict(self, lr: float = 1e-3) -> dict:
        """What ``torch.optim.Adam(my_model.parameters(), lr).state_dict()`` would hold after the steps taken through
        ``train_step``: state entries (by parameter index) for the tensors that received gradients, one param group."""
        order = self._param_order()
        tr = self._tstate.main if self._tstate is not None else None
        named = tr.adam_state() if tr is not None and tr.step_count > 0 else {}
        state = {i: named[k] for i, k in enumerate(order) if k in named}
        group = {"lr": lr, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0, "amsgrad": False, "maximize": False, "foreach": None,
                 "capturable": False, "differentiable": False, "fused": None, "params": list(range(len(order)))}
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, sd: dict) -> None:
        """Resume the device optimiser from a reference checkpoint's 'optimizer' entry (call after ``prepare_training``, or after the
        first ``train_step`` built the training state)."""
        if self._tstate is None:
            raise EngineError("no trainer yet: call prepare_training() or train_step first")
        order = self._param_order()
        self._tstate.main.load_adam_state({order[int(i)]: st for i, st in sd["state"].items()})

    def prepare_training(self) -> None:
        """Builds the training state from the current weights (train_step and the training forward do it lazily)."""
        self._training_state(torch.device("cuda", self._device_index()))
