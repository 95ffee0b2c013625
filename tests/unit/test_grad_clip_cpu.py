"""``rocket.Optimizer(..., max_grad_norm=...)`` with an optimizer that has no clip of its own (CPU,
``torch.optim.SGD``): the engine wrapper clips through ``engine.clip_grad_norm_`` on gradient-sync
steps only, and the capsule reports the norm torch's clip returned."""

import copy

import pytest
import torch

import rocket_amd as rocket
from rocket_amd.core.capsule import Capsule

N_BATCH, BS, LR = 6, 4, 0.5


class _Obj(torch.nn.Module):
    def forward(self, batch):
        return torch.nn.functional.cross_entropy(batch[1], batch[0][1])


class _Net(torch.nn.Module):
    def __init__(self, mlp):
        super().__init__()
        self.mlp = mlp

    def forward(self, batch):
        return (batch, self.mlp(batch[0]))


class _Rec(Capsule):
    """Runs after the optimizer capsule: (sync step?, the posted norm object) per micro-step."""

    def __init__(self):
        super().__init__(priority=10)
        self.seen = []

    def launch(self, attrs=None):
        self.seen.append((self._accelerator.sync_gradients, attrs.looper.state.grad_norm))


def _setup():
    torch.manual_seed(0)
    mlp = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Tanh(), torch.nn.Linear(7, 3))
    x = torch.randn(N_BATCH * BS, 5) * 4
    y = torch.randint(0, 3, (N_BATCH * BS,))
    return mlp, x, y


def _run_tree(ga, max_grad_norm):
    mlp, x, y = _setup()
    data = [(x[i], y[i]) for i in range(len(x))]
    opt = torch.optim.SGD(mlp.parameters(), lr=LR)
    rec = _Rec()
    capsule = rocket.Optimizer(opt, max_grad_norm=max_grad_norm) if max_grad_norm is not None else rocket.Optimizer(opt)
    rocket.Launcher(
        [rocket.Looper([rocket.Dataset(data, batch_size=BS), rocket.Module(_Net(mlp), [rocket.Loss(_Obj()), capsule]),
                        rec], progress=False)],
        gradient_accumulation_steps=ga, cpu=True, destroy_process_group_after_launch=False,
    ).launch()
    return [p.detach().clone() for p in mlp.parameters()], rec


def _run_by_hand(ga, max_norm):
    mlp, x, y = _setup()
    mlp = copy.deepcopy(mlp)
    opt = torch.optim.SGD(mlp.parameters(), lr=LR)
    norms = []
    for i in range(N_BATCH):
        xb, yb = x[i * BS:(i + 1) * BS], y[i * BS:(i + 1) * BS]
        (torch.nn.functional.cross_entropy(mlp(xb), yb) / ga).backward()
        if (i + 1) % ga == 0 or i == N_BATCH - 1:
            norms.append(float(torch.nn.utils.clip_grad_norm_(list(mlp.parameters()), max_norm)))
            opt.step()
            opt.zero_grad()
    return [p.detach().clone() for p in mlp.parameters()], norms


@pytest.mark.parametrize("ga", [1, 2])
def test_capsule_clip_matches_hand_written_loop(ga):
    w, rec = _run_tree(ga, 0.1)
    ref, norms = _run_by_hand(ga, 0.1)
    for a, b in zip(w, ref):
        assert torch.allclose(a, b, atol=1e-6, rtol=0), (a - b).abs().max()
    assert max(norms) > 0.1  # the clip bites, so ...
    plain, rec_plain = _run_tree(ga, None)
    assert any(not torch.allclose(a, b, atol=1e-4) for a, b in zip(w, plain))  # ... the result differs
    assert all(v is None for _, v in rec_plain.seen)
    # one norm per sync step, posted on sync steps only (a non-sync step leaves the last one in place)
    assert [s for s, _ in rec.seen] == [(i + 1) % ga == 0 for i in range(N_BATCH)]
    posted, last = [], None
    for sync, v in rec.seen:
        if sync:
            assert v is not None and v is not last
            posted.append(float(v))
        else:
            assert v is last
        last = v
    assert posted == pytest.approx(norms, rel=1e-6)


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), float("inf")])
def test_invalid_max_grad_norm_raises(bad):
    opt = torch.optim.SGD(torch.nn.Linear(2, 2).parameters(), lr=0.1)
    with pytest.raises(ValueError):
        rocket.Optimizer(opt, max_grad_norm=bad)


def test_positional_signature_unchanged():
    opt = torch.optim.SGD(torch.nn.Linear(2, 2).parameters(), lr=0.1)
    c = rocket.Optimizer(opt, "o", 900)
    assert c._tag == "o" and c._priority == 900 and c._max_grad_norm is None
    with pytest.raises(TypeError):
        rocket.Optimizer(opt, "o", 900, 1.0)  # max_grad_norm is keyword only
