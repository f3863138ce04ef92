"""The scope of one C-ABI call (csrc/engine_ctx.h, Call): what a call leaves on the context - an exhausted arena's flag, a launcher's
refusal, the GroupNorm statistics' cursor, the walker's programs and staging set - ends with the call.  A call that failed must not
change what the next one returns, and the walker's two pinned staging sets must serve consecutive calls with the same bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, M = 1024, 64


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def _engine(sd=None, feat_len=3):
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    eng = Engine(NetConfig(feat_len=feat_len), 0, max_points=N, max_pairs=1)
    if sd is not None:
        eng.load_state_dict(sd)
    return eng


@pytest.fixture(scope="module")
def weights():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.weights import generate_state_dict
    return generate_state_dict(NetConfig(feat_len=3), 0)


@pytest.fixture(scope="module")
def clouds():
    from deepsir_amd.synth import make_batch
    b = make_batch(N, [900], 3)
    return torch.from_numpy(b["points_src"]).cuda().contiguous(), torch.from_numpy(b["points_ref"]).cuda().contiguous()


def _pose_inputs():
    g = torch.Generator().manual_seed(5)
    src = torch.randn(1, M, 3, generator=g).cuda()
    ref = (src + 0.01 * torch.randn(1, M, 3, generator=g).cuda() + 0.1).contiguous()
    w = torch.rand(1, M, generator=g).cuda()
    T = torch.eye(4)[:3].reshape(1, 3, 4).contiguous().cuda()
    return src, ref, w, T


def _kabsch(eng):
    src, ref, w, _ = _pose_inputs()
    return eng.kabsch(src, ref, w)


def _finetune(eng):
    src, ref, w, T = _pose_inputs()
    return eng.pose_finetune(src, ref, T, weights=w, max_iter=20)


def _metrics(eng):
    src, ref, _, T = _pose_inputs()
    m = eng.eval_metrics(T, T, src, ref, 0.3, 15.0)
    return tuple(m[k] for k in eng.METRIC_NAMES)


def _narrow(eng):
    return (eng.narrow(torch.arange(M, dtype=torch.int64).cuda() * 7 - 3),)


def _fail_fpfh(eng):
    """dsir_fpfh on 2 000 000 points: 272 MB of scratch against an arena of about 100 MB - refused before any launch, so the
    pointers only have to be non-null."""
    some = torch.zeros(64, device="cuda")
    p = some.data_ptr()
    rc = eng.lib.dsir_fpfh(eng.h, p, 6, None, p, 0, None, None, 1, 2_000_000, p, 64, None)
    err = eng.lib.dsir_last_error(eng.h).decode()
    assert rc != 0, "dsir_fpfh accepted 2 000 000 points on a 1024-point context"
    assert "workspace too small" in err, err


@pytest.mark.parametrize("op", [_kabsch, _finetune, _metrics, _narrow], ids=["kabsch", "pose_finetune", "eval_metrics", "narrow_i64"])
def test_a_failed_call_does_not_poison_the_next(op):
    """An entry that takes nothing from the arena, called right after a call that exhausted it: returns 0 (the wrappers raise on
    anything else) with the bytes of the same call on a fresh context.  Before the call scope, these four entries ended in the
    overflow check without a reset of their own and failed with "workspace exhausted" (profiles/engine_call_scope.md)."""
    fresh = _engine()
    want = [t.clone() for t in op(fresh)]
    fresh.close()
    eng = _engine()
    _fail_fpfh(eng)
    got = op(eng)
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert _same_bytes(g, w), f"output {i} differs"
    eng.close()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_a_refused_batch_does_not_change_the_next_registration(weights, clouds, graph):
    """dsir_score refused by the batch check (n beyond max_points), then a registration at (1, 1024, 3): the bytes of the same
    registration on a fresh context."""
    from deepsir_amd.engine import EngineError
    src, ref = clouds
    keys = ("transforms", "idx", "logits", "pt_ref_new", "invalid")

    def register(eng):
        eng.enable_graph(graph)
        out = eng.register(src, ref, 5)
        torch.cuda.synchronize()
        return {k: out[k].clone() for k in keys}

    fresh = _engine(weights)
    want = register(fresh)
    fresh.close()
    eng = _engine(weights)
    n = 2 * N
    with pytest.raises(EngineError, match="batch exceeds max_pairs/max_points"):
        eng.score(torch.zeros(1, n, 64).cuda(), torch.zeros(1, n, eng.cfg.num_classes).cuda(), torch.zeros(1, n, 3).cuda(),
                  torch.zeros(1, n, 16, dtype=torch.int32).cuda())
    got = register(eng)
    for k in keys:
        assert _same_bytes(got[k], want[k]), f"{k} differs"
    eng.close()


def test_consecutive_walker_calls_under_the_scope(weights, clouds):
    """Three eager dsir_randla_forward calls with the walker on take the two pinned staging sets in turn, the third one after
    waiting on the first one's event: all three give the bytes of the separate launches."""
    eng = _engine(weights)
    pts = torch.cat(clouds, 0)
    xyz, neigh, sub, interp = eng.knn_pyramid(pts)
    eng.enable_walk(False)
    f0, l0 = eng.randla_forward("feat_extractor", pts, xyz, neigh, sub, interp)
    eng.enable_walk(True)
    for rep in range(3):
        f1, l1 = eng.randla_forward("feat_extractor", pts, xyz, neigh, sub, interp)
        assert _same_bytes(f0, f1) and _same_bytes(l0, l1), rep
    eng.close()
