"""Fused global-norm gradient clipping (``_FusedBase.set_grad_clip``: grad_norm_mt_kernel + the
clip coefficient inside the multi-tensor update) against ``torch.nn.utils.clip_grad_norm_`` +
``torch.optim``.

Parameter sets as in test_ce_optim.py::test_fused_optimizer_matches_torch: the small one (1024-
element chunks, several blocks, odd sizes) and the big one (> 2M parameters: 4096-element chunks,
the vectorised full-chunk path plus scalar tails)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = [(6, 1, 5, 5), (6,), (16, 6, 5, 5), (16,), (120, 400), (120,), (84, 120), (84,), (10, 84), (10,), (5000,)]
BIG = SMALL + [(1500, 1501), (512, 2048), (77,)]
SETS = {"small": SMALL, "big": BIG}
STEPS = 5


def _clone_params(ps):
    return [torch.nn.Parameter(p.detach().clone()) for p in ps]


def _pair(kind, shapes, fused_only=False):
    """(fused params, fused optimizer, torch params, torch optimizer) from the same initial values."""
    from rocket_amd.ops.optim import FusedAdamW, FusedSGD

    g = torch.Generator(device="cuda").manual_seed(0)
    base = [torch.randn(s, device="cuda", generator=g) for s in shapes]
    a, b = _clone_params(base), _clone_params(base)
    if kind == "adamw":  # two param groups
        oa = FusedAdamW([{"params": a[:4], "lr": 3e-3}, {"params": a[4:], "weight_decay": 0.1}], lr=1e-3)
        ob = torch.optim.AdamW([{"params": b[:4], "lr": 3e-3}, {"params": b[4:], "weight_decay": 0.1}], lr=1e-3)
    else:  # momentum
        oa = FusedSGD(a, lr=0.1, momentum=0.9, weight_decay=1e-4)
        ob = torch.optim.SGD(b, lr=0.1, momentum=0.9, weight_decay=1e-4)
    return a, oa, b, ob


def _grads(shapes, step, seed=1):
    """Gradients of one step: randn on even steps (norm >> 1: clipped), 1e-4 * randn on odd ones
    (norm << 1: not clipped)."""
    g = torch.Generator(device="cuda").manual_seed(seed * 1000 + step)
    amp = 1.0 if step % 2 == 0 else 1e-4
    return [amp * torch.randn(s, device="cuda", generator=g) for s in shapes]


def _norm64(grads):
    return float(torch.cat([g.double().reshape(-1) for g in grads]).norm())


def _set_grad(p, g):
    if g.dtype != p.dtype:
        p.grad_dtype = None  # bf16 gradients of fp32 master weights
    p.grad = g


def _assert_close(a, b):
    for pa, pb in zip(a, b):
        assert torch.allclose(pa, pb, atol=1e-5, rtol=1e-5), (pa - pb).abs().max()


@pytest.mark.parametrize("gdtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("size", ["small", "big"])
@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_clip_matches_torch(kind, size, gdtype):
    """5 steps at max_norm 1.0, clipped and unclipped steps alternating; bf16 gradients are compared
    with the reference computed from the same bf16 values upcast."""
    shapes = SETS[size]
    a, oa, b, ob = _pair(kind, shapes)
    oa.set_grad_clip(1.0)
    for step in range(STEPS):
        gs = [g.to(gdtype) for g in _grads(shapes, step)]
        for pa, pb, g in zip(a, b, gs):
            _set_grad(pa, g.clone())
            pb.grad = g.float()
        ref_norm = _norm64(gs)
        assert (ref_norm > 1.0) == (step % 2 == 0)
        total = torch.nn.utils.clip_grad_norm_(b, 1.0)
        oa.step()
        ob.step()
        got = float(oa.grad_norm)
        print(f"{kind}/{size}/{gdtype} step {step}: norm {got!r} fp64 {ref_norm!r} torch {float(total)!r}")
        # tens of fp32 roundings in a blocked tree sum: ~2e-6
        assert abs(got - ref_norm) <= 1e-5 * ref_norm, (got, ref_norm)
    torch.cuda.synchronize()
    _assert_close(a, b)


@pytest.mark.parametrize("size", ["small", "big"])
@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_clip_not_biting_is_bit_identical(kind, size):
    """max_norm = 1e30: coef == 1.0f exactly, so the weights equal the unclipped run bit for bit."""
    shapes = SETS[size]
    a, oa, _, _ = _pair(kind, shapes)
    c, oc, _, _ = _pair(kind, shapes)
    oa.set_grad_clip(1e30)
    for step in range(3):
        gs = _grads(shapes, step)
        for pa, pc, g in zip(a, c, gs):
            pa.grad = g.clone()
            pc.grad = g.clone()
        oa.step()
        oc.step()
        assert float(oa._clip[2]) == 1.0
    assert oc.grad_norm is None
    for pa, pc in zip(a, c):
        assert torch.equal(pa, pc)


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_all_zero_gradients(kind):
    a, oa, b, ob = _pair(kind, SMALL)
    oa.set_grad_clip(1.0)
    for pa, pb in zip(a, b):
        pa.grad = torch.zeros_like(pa)
        pb.grad = torch.zeros_like(pb)
    oa.step()
    ob.step()
    assert oa._clip.tolist()[:3] == [1.0, 0.0, 1.0]  # max_norm, norm, coef
    assert all(bool(torch.isfinite(p).all()) for p in a)
    _assert_close(a, b)


@pytest.mark.parametrize("size", ["small", "big"])
def test_clip_is_deterministic(size):
    """Fixed-order partial sums, no float atomics: identical runs give identical bits."""
    shapes = SETS[size]
    runs = []
    for _ in range(2):
        a, oa, _, _ = _pair("adamw", shapes)
        oa.set_grad_clip(1.0)
        norms = []
        for step in range(3):
            for pa, g in zip(a, _grads(shapes, step)):
                pa.grad = g
            oa.step()
            norms.append(oa.grad_norm.clone())
        runs.append((torch.stack(norms), [p.detach().clone() for p in a]))
    assert torch.equal(runs[0][0], runs[1][0])
    for x, y in zip(runs[0][1], runs[1][1]):
        assert torch.equal(x, y)


def test_set_grad_clip_validation_and_state_dict():
    from rocket_amd.ops.optim import FusedAdamW

    p = [torch.nn.Parameter(torch.zeros(8, device="cuda"))]
    o = FusedAdamW(p)
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            o.set_grad_clip(bad)
    v = o.version
    o.set_grad_clip(2.0)
    assert o.max_grad_norm == 2.0 and o.version > v  # the step gains a launch: graphs go stale
    v = o.version
    o.set_grad_clip(0.5)
    assert o.version == v  # a new value is one uploaded float
    assert "max_grad_norm" not in o.defaults and all("max_grad_norm" not in g for g in o.state_dict()["param_groups"])
    o.set_grad_clip(None)
    assert o.max_grad_norm is None


@pytest.mark.parametrize("size", ["small", "big"])
@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_clip_graph_capture(kind, size):
    """launch(zero_grads=True) captured once, replayed with fresh gradients in the same buffers:
    every replay clips like torch, clears the gradients, and leaves its ticket counter at zero."""
    from rocket_amd.ops import _lib

    shapes = SETS[size]
    a, oa, b, ob = _pair(kind, shapes)
    oa.set_grad_clip(1.0)
    for pa in a:
        pa.grad = torch.zeros_like(pa)
    assert oa.prepare()
    _lib.Workspace.get(a[0].device)  # the ticket counters must not be allocated inside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oa.launch(zero_grads=True)
    assert oa.norm_launches == 0  # capturing runs nothing
    max_norms = [1.0, 1.0, 0.05, 1.0]
    norms = []
    for k in range(4):
        gs = _grads(shapes, k, seed=2)
        if max_norms[k] != oa.max_grad_norm:  # a new max_norm needs no new capture
            oa.set_grad_clip(max_norms[k])
            oa.refresh_hyper()
        for pa, pb, g in zip(a, b, gs):
            pa.grad.copy_(g)
            pb.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(b, max_norms[k])
        ob.step()
        graph.replay()
        ref = _norm64(gs)
        norms.append(ref)
        assert abs(float(oa.grad_norm) - ref) <= 1e-5 * ref
        _assert_close(a, b)
        assert all(not bool(pa.grad.any()) for pa in a)
        assert int(_lib.Workspace.get(a[0].device).counters.sum()) == 0
        assert int(oa._norm_tickets.abs().sum()) == 0
    # each replay reported into its own ring slot and advanced the device cursor
    assert int(oa._norm_slot) == 4
    assert oa._norm_ring[:4].tolist() == pytest.approx(norms, rel=1e-5)
    assert float(oa.device_step) == 4.0


@pytest.mark.parametrize("pre_unscale", [False, True], ids=["in_update", "unscale_first"])
@pytest.mark.parametrize("size", ["small", "big"])
@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_clip_with_fp16_scaler(kind, size, pre_unscale):
    """FusedGradScaler + clip against torch.amp.GradScaler's unscale_ / clip_grad_norm_ / step /
    update: the norm is that of the UNSCALED gradients; an inf gradient skips the step and backs
    the scale off, on both sides alike."""
    from rocket_amd.runtime.amp import FusedGradScaler

    shapes = SETS[size]
    a, oa, b, ob = _pair(kind, shapes)
    oa.set_grad_clip(1.0)
    kw = dict(init_scale=1024.0, growth_interval=2)
    fs = FusedGradScaler(a[0].device, **kw)
    ts = torch.amp.GradScaler("cuda", **kw)
    ts.scale(torch.zeros(1, device="cuda"))  # materialises torch's scale tensor
    for step in range(6):
        scale = fs.get_scale()
        assert scale == ts.get_scale(), (step, scale, ts.get_scale())
        gs = _grads(shapes, step, seed=3)
        for i, (pa, pb, g) in enumerate(zip(a, b, gs)):
            sg = g * scale  # a power of two: scaling and unscaling are exact
            if step == 2 and i == 4:
                sg.view(-1)[17] = float("inf")
            pa.grad = sg.clone()
            pb.grad = sg.clone()
        before = [p.detach().clone() for p in a]
        if pre_unscale:
            fs.unscale_(oa)
        fs.step(oa)
        fs.update()
        ts.unscale_(ob)
        torch.nn.utils.clip_grad_norm_(b, 1.0)
        ts.step(ob)
        ts.update()
        if step == 2:
            assert fs.last_step_skipped()
            assert fs.get_scale() == scale * 0.5
            for pa, p0 in zip(a, before):
                assert torch.equal(pa, p0)
        else:
            assert not fs.last_step_skipped()
            ref = _norm64(gs)
            assert abs(float(oa.grad_norm) - ref) <= 1e-5 * ref, (step, float(oa.grad_norm), ref)
        _assert_close(a, b)
    assert fs.get_scale() == ts.get_scale()
    expect_steps = 5.0
    assert float(oa.device_step) == expect_steps
