"""The fused LeNet step with its hand-off tensors (a2, h1, h2, d1, d2, dy) in the blocked
``[N / 4][features padded to 16][4]`` layout (``native/kernels/handoff_layout.h``): the step kernel
writes one line-aligned record per block and tensor, the grouped weight-gradient launch reads them
by LDS-DMA (N = 1024) or fragment-shaped global loads (any other N).

Oracle and tolerances are those of ``test_linear_conv.py`` / ``test_fp16.py``: fp32 math on the
16-bit-rounded operands of the AMP contract (``_ref_lenet``) from a ``LeNet(fused=False)``, updated
by ``torch.optim.AdamW``; logits 1e-2 (fp16: 2e-3), loss 1e-2, gradients and parameters 3e-2
(cross-entropy gradients of a separate backward launch 4e-2), relative L2."""

import pytest
import torch
import torch.nn.functional as F

import rocket_amd as rocket
from rocket_amd.core.capsule import Capsule

pytestmark = pytest.mark.gpu

# Learning rate of the captured-step test.  An Adam update moves every element by about lr whatever
# its gradient's size, so an element whose gradient is within 16-bit noise of zero may go either way
# in the fused run and in the oracle: up to 2 lr apart per update.  The logits tolerance (1e-2) is one
# for equal weights; to keep it meaningful for the last step's logits, which see up to three updates,
# even the worst case (every element of a layer apart) must stay under it for the layer with the
# smallest weights, fc1 (uniform +-1/20, rms 0.0289): 2 * lr * 3 / 0.0289 <= 1e-2, lr <= 4.8e-5.
# (At AdamW's default 1e-3 the logits against the oracle measured, N x replays: 8x1 1.15e-3,
# 40x1 2.53e-3, 520x1 2.82e-3, 1024x1 2.48e-3, 8x3 1.77e-3, 40x3 9.05e-3, 520x3 1.64e-2,
# 1024x3 1.39e-2, every parameter within 1e-2, while bench.py's outputs are bitwise the parent
# commit's: the two figures above 1e-2 are this drift, not the layout.)
LR = 4e-5


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _ref_lenet(x, net, dt=torch.bfloat16):
    """fp32 math on 16-bit-rounded operands, activations rounded between layers (the AMP contract)."""
    r = lambda t: t.to(dt).float()  # noqa: E731
    h = r(F.max_pool2d(F.relu(F.conv2d(r(x), r(net.conv1.weight), net.conv1.bias, padding=2)), 2))
    h = F.max_pool2d(F.relu(F.conv2d(h, r(net.conv2.weight), net.conv2.bias)), 2)
    a2 = r(h.flatten(1))
    h1 = r(F.relu(F.linear(a2, r(net.fc1.weight), net.fc1.bias)))
    h2 = r(F.relu(F.linear(h1, r(net.fc2.weight), net.fc2.bias)))
    return a2, F.linear(h2, r(net.fc3.weight), net.fc3.bias)


class _Record(Capsule):
    """Copies of what the last step handed back (a captured step's outputs live in the graph pool)."""

    def __init__(self):
        super().__init__(priority=10)
        self.logits = self.loss = None

    def launch(self, attrs=None):
        if attrs is None or attrs.looper is None:
            return
        batch = attrs.get("batch")
        if isinstance(batch, (list, tuple)) and len(batch) > 2:
            self.logits = batch[2].detach().float().clone()
        if attrs.looper.state.loss is not None:
            self.loss = float(attrs.looper.state.loss)


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("N", [8, 40, 520, 1024])
def test_captured_step_matches_fp32_oracle(tmp_path, N, steps):
    """``steps`` replays of the captured training step (after the engine's one eager warm-up step):
    the last step's logits and loss and all ten parameters vs the oracle trained on the same batches
    (learning rate: see ``LR``).  The parameter comparison is weak evidence for the blocked tensors:
    the updates are small against the weights, so it shows that the captured update ran and went
    nowhere wild, not that it is right.  What holds the hand-off layout to account is the gradient
    comparison of ``test_fallback_backward_rereads_blocked_masks`` (all four batch sizes, both
    launches), the host check of the index math, and the bitwise equality of ``bench.py``'s outputs
    with the parent commit's.
    N = 8: two blocks; 40: most waves of a tile block have no batch range; 520: a wave with a partial
    range (global-load path); 1024: the LDS-DMA path."""
    from rocket_amd.models import CrossEntropy, LeNet
    from rocket_amd.ops.optim import FusedAdamW

    dev = torch.device("cuda", 0)
    total = steps + 1
    g = torch.Generator(device=dev).manual_seed(11)
    x = torch.rand(N * total, 1, 28, 28, generator=g, device=dev)
    y = torch.randint(0, 10, (N * total,), generator=g, device=dev)
    torch.manual_seed(0)
    net = LeNet(fused=True)
    ref = LeNet(fused=False).to(dev)
    ref.load_state_dict(net.state_dict())
    opt = FusedAdamW(net.parameters(), lr=LR)
    rec = _Record()
    mod = rocket.Module(net, [rocket.Loss(CrossEntropy(fused=True)), rocket.Optimizer(opt)], capture=True, warmup=1)
    data = rocket.DeviceTensorDataset(x, y)
    rocket.Launcher(
        [rocket.Looper([rocket.Dataset(data, batch_size=N, shuffle=False), mod, rec], repeats=total, progress=False)],
        logging_dir=str(tmp_path), mixed_precision="bf16", destroy_process_group_after_launch=False,
    ).launch()
    torch.cuda.synchronize()
    graphs = mod._graphs
    assert graphs is not None and graphs.replays >= steps, (graphs and graphs.disabled_reason, graphs and graphs.replays)

    oref = torch.optim.AdamW(ref.parameters(), lr=LR)
    for i in range(total):
        _, yr = _ref_lenet(x[i * N:(i + 1) * N], ref)
        lr_ = F.cross_entropy(yr, y[i * N:(i + 1) * N])
        if i + 1 < total:
            lr_.backward()
            oref.step()
            oref.zero_grad()
    e_logits, e_loss = _rel(rec.logits, yr), abs(rec.loss - lr_.item()) / abs(lr_.item())
    lr_.backward()
    oref.step()
    errs = {n: _rel(p, pr) for (n, p), pr in zip(net.named_parameters(), ref.parameters())}
    print(f"N={N} steps={steps}: logits {e_logits:.2e} loss {e_loss:.2e} params {errs}")
    assert rec.logits.shape == (N, 10)
    assert e_logits < 1e-2, e_logits
    assert e_loss < 1e-2, (rec.loss, lr_.item())
    for n, e in errs.items():
        assert e < 3e-2, (n, e)


def _ce_grads(net, x, fwd_target, target, dtype=torch.bfloat16, dev_scale=None):
    from rocket_amd.ops.lenet import fuse_cross_entropy, lenet_forward

    net.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=dtype):
        y = lenet_forward(x, net.conv1, net.conv2, net.fc1, net.fc2, net.fc3, fwd_target)
    assert y.grad_fn.spec is not None  # the forward launch ran the whole step on fwd_target
    loss, dummy = fuse_cross_entropy(y, target, 1.0, dev_scale=dev_scale)
    torch.autograd.backward([y], [dummy])
    torch.cuda.synchronize()
    return y.detach().clone(), float(loss), [p.grad.clone() for p in net.parameters()]


@pytest.mark.parametrize("N", [8, 40, 520, 1024])
def test_fallback_backward_rereads_blocked_masks(N):
    """The loss's targets differ from those the forward speculated on: the speculative result is
    dropped and the separate backward launch re-reads the ReLU masks from the blocked h1 / h2.  Its
    gradients equal the speculative launch's on the same targets (same contract: 1e-5) and follow
    the oracle.  (All four batch sizes: this is the direct check of one step's gradients.)"""
    from rocket_amd.models import LeNet

    torch.manual_seed(8)
    net = LeNet(fused=False).cuda()
    ref = LeNet(fused=False).cuda()
    ref.load_state_dict(net.state_dict())
    x = torch.rand(N, 1, 28, 28, device="cuda")
    t1 = torch.randint(0, 10, (N,), device="cuda")
    t2 = (t1 + 1 + torch.randint(0, 9, (N,), device="cuda")) % 10  # differs everywhere
    y_fb, l_fb, g_fb = _ce_grads(net, x, t1, t2)
    y_sp, l_sp, g_sp = _ce_grads(net, x, t2, t2)
    _, yr = _ref_lenet(x, ref)
    lr_ = F.cross_entropy(yr, t2)
    lr_.backward()
    e_spec = {n: _rel(a, b) for (n, _), a, b in zip(net.named_parameters(), g_fb, g_sp)}
    e_ref = {n: _rel(a, p.grad) for (n, p), a in zip(ref.named_parameters(), g_fb)}
    print(f"N={N}: logits {_rel(y_fb, yr):.2e} loss {l_fb} / {lr_.item()} vs speculative {e_spec} vs oracle {e_ref}")
    assert torch.equal(y_fb, y_sp)
    assert _rel(y_fb, yr) < 1e-2
    assert abs(l_fb - l_sp) <= 1e-6 * abs(l_sp) and abs(l_fb - lr_.item()) < 1e-2 * abs(lr_.item())
    for n in e_spec:
        assert e_spec[n] < 1e-5, (n, e_spec[n])
        assert e_ref[n] < 4e-2, (n, e_ref[n])


@pytest.mark.parametrize("N", [8, 1024])
def test_eval_forward(N):
    from rocket_amd.models import LeNet

    torch.manual_seed(9)
    net = LeNet(fused=True).cuda().eval()
    x = torch.rand(N, 1, 28, 28, device="cuda")
    t = torch.randint(0, 10, (N,), device="cuda")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        _, _, y = net((x, t))
    _, yr = _ref_lenet(x, net)
    print(f"N={N}: eval logits {_rel(y, yr):.2e}")
    assert y.shape == (N, 10) and y.grad_fn is None
    assert _rel(y, yr) < 1e-2


@pytest.mark.parametrize("N", [8, 1024])
def test_fp16_build(N):
    """The fp16 kernel build (fp16 autocast) with the loss scale folded in on the device: the first
    call's forward speculated without the scale (separate backward launch), the second one's whole
    step ran in the forward launch; both against the fp16-contract oracle, gradients at the 3e-2 of
    ``test_linear_conv.py`` (measured at N = 1024: at most 1.09e-2, on conv1.weight, whose gradient
    goes through the conv slab and none of the blocked tensors; the classifier's are below 1.2e-3)."""
    from rocket_amd.models import LeNet

    torch.manual_seed(10)
    net = LeNet(fused=False).cuda()
    ref = LeNet(fused=False).cuda()
    ref.load_state_dict(net.state_dict())
    x = torch.rand(N, 1, 28, 28, device="cuda")
    t = torch.randint(0, 10, (N,), device="cuda")
    S = torch.tensor([1024.0], device="cuda")
    _, yr = _ref_lenet(x, ref, torch.float16)
    lr_ = F.cross_entropy(yr, t)
    lr_.backward()
    for call in ("separate backward", "whole step"):
        y, loss, grads = _ce_grads(net, x, t, t, torch.float16, S)
        errs = {n: _rel(g / 1024.0, p.grad) for (n, p), g in zip(ref.named_parameters(), grads)}
        print(f"N={N} fp16 {call}: logits {_rel(y, yr):.2e} loss {loss} / {lr_.item()} grads {errs}")
        assert _rel(y, yr) < 2e-3
        assert abs(loss - lr_.item()) < 1e-2 * abs(lr_.item())
        for n, e in errs.items():
            assert e < 3e-2, (n, e)


def test_mlp_head_keeps_plain_layout():
    """The stand-alone MLP head (M = 24) still hands ``[features][M]`` tensors to the same
    weight-gradient launch."""
    from rocket_amd.models import LeNet
    from rocket_amd.ops.lenet import lenet_features, mlp_head

    torch.manual_seed(1)
    M = 24
    net = LeNet(fused=False).cuda()
    ref = LeNet(fused=False).cuda()
    ref.load_state_dict(net.state_dict())
    x = torch.rand(M, 1, 28, 28, device="cuda")
    a2 = lenet_features(x, net.conv1.weight, net.conv1.bias, net.conv2.weight, net.conv2.bias)
    y = mlp_head(a2, [net.fc1, net.fc2, net.fc3])
    a2r, yr = _ref_lenet(x, ref)
    g = torch.randn_like(y)
    y.backward(g)
    yr.backward(g)
    errs = {n: _rel(p.grad, pr.grad) for (n, p), pr in zip(net.named_parameters(), ref.parameters())}
    print(f"mlp_head M={M}: a2 {_rel(a2, a2r):.2e} logits {_rel(y, yr):.2e} grads {errs}")
    assert _rel(a2, a2r) < 1e-2 and _rel(y, yr) < 1e-2
    for n, e in errs.items():
        assert e < 3e-2, (n, e)
