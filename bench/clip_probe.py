"""Cost of fused global-norm gradient clipping (``_FusedBase.set_grad_clip``) on the LeNet, ResNet-18
and ViT-B/16 parameter sets, fp32 gradients:

* ``update``       the unclipped fused update (one launch) — the step without clipping;
* ``norm``         the norm launch alone (``rk_grad_norm_mt``);
* ``clip_update``  norm launch + update with the clip coefficient — the step with clipping;
* ``torch_clip``   ``torch.nn.utils.clip_grad_norm_`` followed by the unclipped fused update: what a
                   user had to do before (the unclipped launch is that code path unchanged).

Each figure is the time per call of ``--inner`` back-to-back calls between two HIP events (so for
the LeNet set it is the launch-bound issue rate, not a kernel time), after a warm-up, median over
``--iters`` windows; the whole table is measured ``--rounds`` times in alternation and the spread
of the medians across rounds is reported with them.  ``GB/s`` is the gradient bytes (norm) or
the bytes the update streams (update: 4 arrays read + 3 written for Adam, 3 + 2 for SGD with
momentum, plus the gradient once more for the clipped step) over that time.

    python bench/clip_probe.py [--out bench_outputs/clip_probe.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from rocket_amd.ops import _lib  # noqa: E402


def _shapes(name):
    from rocket_amd import models

    net = {"lenet": lambda: models.LeNet(fused=False), "resnet18": lambda: models.resnet18(10),
           "vit_b16": lambda: models.vit_b16()}[name]()
    return [tuple(p.shape) for p in net.parameters() if p.requires_grad]


def _window(fn, inner, iters, warm=3):
    for _ in range(warm):
        for _ in range(inner):
            fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for s, e in ev:
        s.record()
        for _ in range(inner):
            fn()
        e.record()
    torch.cuda.synchronize()
    t = sorted(s.elapsed_time(e) / inner * 1e3 for s, e in ev)  # us per call
    return t[len(t) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="bench_outputs/clip_probe.jsonl")
    ap.add_argument("--models", default="lenet,resnet18,vit_b16")
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=0, help="calls per timed window (0: 50 small sets, 10 big ones)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_probe needs a HIP device")
    from rocket_amd.ops.optim import FusedAdamW, FusedSGD

    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    dev = torch.device("cuda")
    lib = _lib.kernels()
    rows = []
    for name in args.models.split(","):
        shapes = _shapes(name)
        torch.manual_seed(0)
        params = [torch.nn.Parameter(torch.randn(s, device=dev) * 0.02) for s in shapes]
        for p in params:
            p.grad = torch.randn_like(p)
        n = sum(p.numel() for p in params)
        sgd = name == "resnet18"
        opt = FusedSGD(params, lr=1e-3, momentum=0.9) if sgd else FusedAdamW(params, lr=1e-4)
        assert opt.prepare()
        opt.launch()  # first step done: the SGD momentum buffers are live from here on
        opt.set_grad_clip(1.0)
        assert opt.prepare()
        ctr = torch.zeros(int(lib.rk_grad_norm_tickets(opt._nblocks)), dtype=torch.int32, device=dev)
        clip_probe = torch.zeros(4, device=dev)
        clip_probe[0] = 1.0

        def norm_only():
            _lib.check(lib.rk_grad_norm_mt(opt._gdtype, opt._tables[0].data_ptr(), opt._tables[1].data_ptr(),
                                           opt._nblocks, None, opt._partials.data_ptr(), clip_probe.data_ptr(), None,
                                           None, 0, ctr.data_ptr(), opt._chunk, _lib.stream_ptr(dev)), "rk_grad_norm_mt")

        def clip_update():
            opt.max_grad_norm = 1.0
            opt.launch()

        def update():
            opt.max_grad_norm = None  # (attribute only: the tables and the clip block stay)
            opt.launch()

        def torch_clip():
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            update()

        cases = {"update": update, "norm": norm_only, "clip_update": clip_update, "torch_clip": torch_clip}
        upd_bytes = (5 if sgd else 7) * 4 * n
        nbytes = {"update": upd_bytes, "norm": 4 * n, "clip_update": upd_bytes + 4 * n, "torch_clip": None}
        inner = args.inner or (50 if n < (1 << 21) else 10)
        meds = {k: [] for k in cases}
        for _ in range(args.rounds):  # alternate the cases: drift hits them alike
            for k, fn in cases.items():
                meds[k].append(_window(fn, inner, args.iters))
        for k, v in meds.items():
            v = sorted(v)
            us = v[len(v) // 2]
            row = {"model": name, "params": n, "blocks": opt._nblocks, "chunk": opt._chunk, "case": k,
                   "us": round(us, 2), "us_min": round(v[0], 2), "us_max": round(v[-1], 2), "rounds": len(v),
                   "inner": inner}
            if nbytes[k]:
                row["GB/s"] = round(nbytes[k] / us / 1e3, 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del opt, params
        torch.cuda.empty_cache()
    with open(args.out, "w") as fh:
        fh.write(json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                             "hip": torch.version.hip}) + "\n")
        for r in rows:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
