"""``rocket.Optimizer(opt, max_grad_norm=...)`` on the fused LeNet tree of test_graph_capture.py:
clipping inside the fused update, eager and captured, one reported norm per sync step, and two
data-parallel ranks that clip identically without a collective."""

import hashlib
import json
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

import rocket_amd as rocket
from rocket_amd.core.capsule import Capsule

pytestmark = pytest.mark.gpu

MAX_NORM = 0.01  # well under the LeNet gradient norms of these runs (asserted below): the clip bites


class _Record(Capsule):
    def __init__(self):
        super().__init__(priority=10)
        self.losses = []
        self.norms = []  # (sync step?, the posted norm object) per micro-step

    def launch(self, attrs=None):
        if attrs is not None and attrs.looper is not None:
            if attrs.looper.state.loss is not None:
                self.losses.append(attrs.looper.state.loss)
            self.norms.append((self._accelerator.sync_gradients, attrs.looper.state.grad_norm))


def _train(tmp_path, capture, steps=14, ga=1, batch=256, max_grad_norm=MAX_NORM):
    from rocket_amd.models import CrossEntropy, LeNet
    from rocket_amd.ops.optim import FusedAdamW

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(7)
    n = batch * (steps + 1)
    x = torch.rand(n, 1, 28, 28, generator=g, device=dev)
    y = torch.randint(0, 10, (n,), generator=g, device=dev)
    data = rocket.DeviceTensorDataset(x, y)
    torch.manual_seed(0)
    net = LeNet(fused=True)
    opt = FusedAdamW(net.parameters(), lr=2e-3)
    epilogues = []
    orig = opt.epilogue
    opt.epilogue = lambda params: epilogues.append(orig(params)) or epilogues[-1]
    sched = torch.optim.lr_scheduler.StepLR(opt, 4, gamma=0.5)
    rec = _Record()
    capsule = rocket.Optimizer(opt, max_grad_norm=max_grad_norm) if max_grad_norm is not None else rocket.Optimizer(opt)
    mod = rocket.Module(net, [rocket.Loss(CrossEntropy(fused=True)), capsule, rocket.Scheduler(sched)],
                        capture=capture, warmup=2)
    rocket.Launcher(
        [rocket.Looper([rocket.Dataset(data, batch_size=batch, shuffle=False), mod, rec], repeats=steps, progress=False)],
        logging_dir=str(tmp_path),
        mixed_precision="bf16",
        gradient_accumulation_steps=ga,
        destroy_process_group_after_launch=False,
    ).launch()
    torch.cuda.synchronize()
    posted, last = [], None
    for sync, v in rec.norms:  # a new object on every sync step, untouched in between
        if max_grad_norm is None:
            assert v is None
        elif sync:
            assert v is not None and v is not last
            posted.append(v)
        else:
            assert v is last
        last = v
    return dict(losses=[float(v) for v in rec.losses], norms=[float(v) for v in posted],
                weights={k: v.detach().float().cpu() for k, v in net.state_dict().items()},
                mod=mod, opt=opt, epilogues=epilogues)


def _same_bits(wa, wb):
    return {k: float((wa[k] - wb[k]).abs().max()) for k in wa if not torch.equal(wa[k], wb[k])}


@pytest.mark.parametrize("ga", [1, 2])
def test_clipped_graph_matches_eager(tmp_path, ga):
    e = _train(tmp_path / "e", capture=False, ga=ga)
    g = _train(tmp_path / "g", capture=True, ga=ga)
    graphs = g["mod"]._graphs
    assert graphs is not None and graphs.disabled_reason == "released", graphs.disabled_reason
    assert graphs.replays > 0
    assert graphs.launch_lists > 0 and graphs.launch_list_reason is None, graphs.launch_list_reason
    assert len(e["losses"]) == len(g["losses"]) > 0
    for a, b in zip(e["losses"], g["losses"]):
        assert abs(a - b) <= 2e-3 * max(1.0, abs(a)), (e["losses"], g["losses"])
    diffs = {k: float((e["weights"][k] - g["weights"][k]).norm() / e["weights"][k].norm().clamp_min(1e-6))
             for k in e["weights"]}
    print(f"ga={ga} eager-vs-graph relative weight differences: {diffs}")
    for k, d in diffs.items():
        assert d < 1.5e-2, (k, d)
    # one reported norm per sync step, each its own step's value, and the clip bit on every one
    sync_steps = 14 // ga
    for r in (e, g):
        assert len(r["norms"]) == sync_steps, r["norms"]
        assert all(v == v and v > MAX_NORM for v in r["norms"]), r["norms"]
        assert len(set(r["norms"])) > 1
        # the norm launch ran on every sync step (device cursor), the update advanced the device
        # step counter itself, and no gradient producer was handed the update
        assert int(r["opt"]._norm_slot) == sync_steps == r["opt"].norm_launches
        assert float(r["opt"].device_step) == float(sync_steps)
        assert all(x is None for x in r["epilogues"])
    print(f"ga={ga} norms eager {e['norms']} captured {g['norms']}")


def test_clipped_capture_reproducible_and_differs_from_unclipped(tmp_path):
    a = _train(tmp_path / "a", capture=True, steps=8)
    b = _train(tmp_path / "b", capture=True, steps=8)
    assert a["losses"] == b["losses"] and a["norms"] == b["norms"]
    assert not _same_bits(a["weights"], b["weights"])
    u = _train(tmp_path / "u", capture=True, steps=8, max_grad_norm=None)
    assert u["norms"] == [] and u["opt"].grad_norm is None
    assert any(x is not None for x in u["epilogues"])  # unclipped: the producer applies the update
    assert _same_bits(a["weights"], u["weights"])


def test_norm_ring_wrap_keeps_reported_values(tmp_path, monkeypatch):
    """Reported norms are LazyScalar views into the optimizer's device ring, all read only after
    the run: with a 4-slot ring every value must still be its own step's (resolved before its slot
    is rewritten one lap later) — bit for bit those of the same run with the full ring."""
    from rocket_amd.ops.optim import _FusedBase

    full = _train(tmp_path / "full", capture=True, steps=20)
    monkeypatch.setattr(_FusedBase, "GRAD_NORM_RING", 4)
    short = _train(tmp_path / "short", capture=True, steps=20)
    assert short["opt"]._norm_ring.numel() == 4
    assert len(full["norms"]) == len(short["norms"]) == 20
    assert full["norms"] == short["norms"]
    assert len(set(full["norms"])) > 4


# ------------------------------------------------------------------ two ranks on one GPU
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), ROCKET_DIST_BACKEND="gloo", ROCKET_P2P="force")
    import rocket_amd as rocket
    from rocket_amd.core.capsule import Capsule
    from rocket_amd.models import CrossEntropy, LeNet
    from rocket_amd.ops.optim import FusedAdamW

    class Rec(Capsule):
        def __init__(self):
            super().__init__(priority=10)
            self.norms = []

        def launch(self, attrs=None):
            v = attrs.looper.state.grad_norm
            if v is not None and (not self.norms or self.norms[-1] is not v):
                self.norms.append(v)

    res = {}
    for clip in (MAX_NORM, None):
        dev = torch.device("cuda", 0)
        g = torch.Generator(device=dev).manual_seed(3)
        bs = 128
        x = torch.rand((bs * 2 * 12, 1, 28, 28), generator=g, device=dev)
        y = torch.randint(0, 10, (bs * 2 * 12,), generator=g, device=dev)
        torch.manual_seed(0)
        net = LeNet(fused=True)
        opt = FusedAdamW(net.parameters(), lr=1e-2)
        rec = Rec()
        capsule = rocket.Optimizer(opt, max_grad_norm=clip) if clip is not None else rocket.Optimizer(opt)
        mod = rocket.Module(net, [rocket.Loss(CrossEntropy(fused=True)), capsule], capture=True, warmup=2)
        rocket.Launcher(
            [rocket.Looper([rocket.Dataset(rocket.DeviceTensorDataset(x, y), batch_size=bs), mod, rec],
                           repeats=12, progress=False)],
            logging_dir=os.path.join(out_dir, f"logs{clip}"),
            mixed_precision="bf16",
            gradient_accumulation_steps=2,
            num_procs=world,
            destroy_process_group_after_launch=False,
        ).launch()
        torch.cuda.synchronize()
        flat = torch.cat([p.detach().float().reshape(-1) for p in net.parameters()]).cpu()
        res["clip" if clip is not None else "plain"] = dict(
            fused=getattr(mod._module, "fused_updates", 0),
            sync_captures=mod._graphs.sync_captures,
            replays=mod._graphs.replays,
            reason=mod._graphs.disabled_reason,
            mode=getattr(mod._module, "capture_mode", None),
            norms=[float(v).hex() for v in rec.norms],
            w=hashlib.sha1(flat.numpy().tobytes()).hexdigest(),
            finite=bool(torch.isfinite(flat).all()),
        )
    with open(os.path.join(out_dir, f"r{rank}.json"), "w") as fh:
        json.dump(res, fh)
    import torch.distributed as dist

    dist.barrier()
    dist.destroy_process_group()


def test_clip_two_ranks_identical_without_collective(tmp_path):
    """Inline P2P mode: the reduced gradients are the same on both ranks, so each rank's own norm
    launch yields the same norm and coefficient — replicas and reported norms stay bit-identical;
    with clipping the all-reduce never applies the update itself."""
    port = _free_port()
    mp.start_processes(_worker, args=(2, port, str(tmp_path)), nprocs=2, start_method="spawn", join=True)
    r = [json.load(open(tmp_path / f"r{i}.json")) for i in range(2)]
    for rank in range(2):
        c, p = r[rank]["clip"], r[rank]["plain"]
        for v in (c, p):
            assert v["replays"] > 0 and v["reason"] == "released" and v["mode"] == "inline" and v["finite"], v
        assert c["fused"] == 0 and p["fused"] > 0, (c, p)
        assert len(c["norms"]) == 6 and p["norms"] == [], (c, p)  # 12 micro-steps, GA 2
        assert all(float.fromhex(v) > MAX_NORM for v in c["norms"]), c
        assert c["w"] != p["w"]
    assert r[0]["clip"]["w"] == r[1]["clip"]["w"]
    assert r[0]["clip"]["norms"] == r[1]["clip"]["norms"]
