"""Loss, Optimizer and Scheduler capsules (children of :class:`~rocket_amd.core.module.Module`).

Parity:

* ``Loss`` — reference ``rocket/core/loss.py``: priority 1100 so it runs before
  the optimizer; stateful ``{value, step}``; per micro-step it computes
  ``objective(batch)``, averages it over ranks, accumulates ``value/GA``, posts
  ``{tag: value}`` to the tracker and ``looper.state.loss`` on sync steps, then
  calls ``engine.backward``.  Here the reported value stays on the device
  (:class:`~rocket_amd.utils.lazy.LazyScalar`) and the cross-rank average is an
  asynchronous RCCL all-reduce instead of an all-gather + ``.item()`` per step
  (Q14: same values, no host synchronisation).
* ``Optimizer`` — reference ``rocket/core/optimizer.py``: ``step()`` +
  ``zero_grad()`` each grad-enabled micro-step (the engine wrapper gates them on
  sync), per-group lr posted to tracker/looper on sync steps.  An extension over
  the reference: ``max_grad_norm`` (keyword only) clips the gradients to a global
  L2 norm before every update and posts ``{tag}.grad_norm`` /
  ``looper.state.grad_norm`` on sync steps.
* ``Scheduler`` — reference ``rocket/core/scheduler.py``: ``step()`` each
  grad-enabled micro-step (wrapper steps ×W on sync steps).
"""

from __future__ import annotations

import math
import os
import weakref

import torch

from rocket_amd.core.attributes import Attributes
from rocket_amd.core.capsule import Capsule
from rocket_amd.ops import data as _data_ops
from rocket_amd.runtime import comm as _comm
from rocket_amd.utils.lazy import LazyScalar, materialize


class Loss(Capsule):
    # device slots for reported losses under graph replay; values still unread when their slot is
    # about to be rewritten (one lap later) are materialised first, in one D2H copy per lap
    RING = 1024

    def __init__(self, objective: torch.nn.Module, tag: str = "train_loss", priority: int = 1100) -> None:
        super().__init__(statefull=True, priority=priority)
        self._objective = objective
        self._value = 0.0
        self._tag = tag
        self._step = 0
        self._acc = None        # graph mode: device accumulator of the current GA window
        self._ring = None       # graph mode: reported values, one slot per sync step
        self._slot = None       # graph mode: device write cursor into the ring
        self._slot_host = 0
        self._lap = []          # weak references to this lap's posted LazyScalars
        self._acc_pending = False

    def _mean_over_ranks(self, loss: torch.Tensor) -> torch.Tensor:
        value = loss.detach().float().reshape(())
        if self._accelerator.num_processes > 1:
            # RCCL: enqueued behind the loss kernel, the host does not wait for it
            value = _comm.all_reduce_(value.clone(), "mean")
        return value

    def compute(self, attrs: Attributes) -> torch.Tensor:
        """Device part: objective + cross-rank mean; returns the loss to backprop."""
        loss = self._objective(attrs.batch)
        ga = self._accelerator.gradient_accumulation_steps
        self._value = self._value + self._mean_over_ranks(loss) / ga
        return loss

    def post(self, attrs: Attributes) -> None:
        """Host part: report on sync steps."""
        if self._accelerator.sync_gradients:
            value = LazyScalar(self._value) if isinstance(self._value, torch.Tensor) else self._value
            if attrs.tracker is not None:
                attrs.tracker.scalars.append(Attributes(step=self._step, data={self._tag: value}))
            if attrs.looper is not None:
                attrs.looper.state.loss = value
            self._value = 0.0
            self._step += 1

    def launch(self, attrs: Attributes | None = None) -> None:
        if attrs is None or attrs.batch is None:
            return
        if not torch.is_grad_enabled():
            return
        if self._acc_pending:  # a graph-accumulated GA window continues eagerly
            self._value = self._value + self._acc.clone()
            self._acc.zero_()
            self._acc_pending = False
        loss = self.compute(attrs)
        self.post(attrs)
        self._accelerator.backward(loss)

    # ---------------------------------------------------- HIP-graph protocol
    def graph_bind(self, graphs) -> None:
        """Allocate the static device state used by captured steps."""
        if self._acc is not None:
            return
        dev = self._accelerator.device
        # W>1: the accumulator lives in the reducer's side channel and is averaged across
        # ranks by the gradient all-reduce itself
        self._acc = graphs.side_slot(1)
        self._ring = torch.zeros(self.RING, device=dev)
        self._slot = torch.zeros(1, dtype=torch.int64, device=dev)
        self._zero = torch.zeros(1, device=dev)
        self._one = torch.ones((), device=dev)
        self._ring_views = list(self._ring.unbind(0))  # one 0-d view per slot, made once

    def graph_prepare(self, attrs: Attributes | None = None) -> None:
        if self._slot_host == 0 and self._lap:
            # the coming replay starts a new lap of the ring: resolve what the last lap posted
            # (a consumer may keep a reported loss across >RING steps) before it is overwritten
            materialize([r() for r in self._lap if r() is not None])
            self._lap = []
        v = self._value
        if isinstance(v, torch.Tensor) or v != 0.0:  # fold an eager partial GA window
            self._acc.add_(v if isinstance(v, torch.Tensor) else float(v))
            self._value = 0.0

    def graph_device(self, attrs: Attributes) -> None:
        engine = self._accelerator
        sync_here = engine.sync_gradients and not attrs.graph_split
        # a data-parallel sync step whose all-reduce can also move the reduced accumulator into the
        # ring (inline P2P): no bookkeeping launch of our own after the reduce
        fold = attrs.get("fold_loss") if (engine.sync_gradients and attrs.get("graph_split")) else None
        self._folded = bool(fold is not None and fold(self._acc, self._ring, self._slot))
        fused = getattr(self._objective, "loss_and_grad", None)
        scaler = engine.scaler
        dev_scale = getattr(scaler, "scale_tensor", None) if scaler is not None else None
        if fused is not None and (scaler is None or dev_scale is not None):
            # objective supplies loss AND d(outputs) in one launch, with the loss bookkeeping folded
            # in: backward starts directly from the outputs (no loss node, no seed fill); under the
            # device fp16 scaler the kernel also multiplies d(outputs) by the loss scale
            scale = 1.0 / engine.gradient_accumulation_steps
            acc = (self._acc, self._ring, self._slot, scale, sync_here)
            res = (fused(attrs.batch, scale, acc, dev_scale=dev_scale) if dev_scale is not None
                   else fused(attrs.batch, scale, acc))
            if res is not None:
                _, outs, grads = res
                torch.autograd.backward(outs, grads)
                return
        loss = self._objective(attrs.batch)
        _data_ops.loss_accum(loss.detach().reshape(1), self._acc, self._ring, self._slot,
                             1.0 / engine.gradient_accumulation_steps, sync_here)
        if loss.dtype == self._one.dtype and loss.dim() == 0:
            engine.backward(loss, gradient=self._one)  # static seed: no fill kernel per step
        else:
            engine.backward(loss)

    def graph_device_synced(self, attrs: Attributes) -> None:
        folded, self._folded = getattr(self, "_folded", False), False
        if self._accelerator.sync_gradients and attrs.graph_split and not folded:
            _data_ops.loss_accum(self._zero, self._acc, self._ring, self._slot, 0.0, True)

    def graph_host(self, attrs: Attributes) -> None:
        if not self._accelerator.sync_gradients:
            self._acc_pending = True
            return
        self._acc_pending = False
        value = LazyScalar(self._ring_views[self._slot_host])
        self._lap.append(weakref.ref(value))
        self._slot_host = (self._slot_host + 1) % self.RING
        tracker, looper = attrs.get("tracker"), attrs.get("looper")
        if tracker is not None:
            tracker.scalars.append(Attributes(step=self._step, data={self._tag: value}))
        if looper is not None:
            looper["state"]["loss"] = value
        self._step += 1

    def state_dict(self) -> dict:
        v = self._value
        v = float(v.item()) if isinstance(v, torch.Tensor) else float(v)
        if self._acc_pending and self._acc is not None:
            v += float(self._acc.item())
        return dict(value=v, step=self._step)

    def load_state_dict(self, state: dict) -> None:
        self._value = state["value"]
        self._step = state["step"]


# ROCKET_OPT_EPILOGUE=0: no fused-producer optimizer epilogue / AMP check fold (read once)
_OPT_EPILOGUE = os.environ.get("ROCKET_OPT_EPILOGUE", "1") != "0"


def _is_fused_scaler(scaler) -> bool:
    from rocket_amd.runtime.amp import FusedGradScaler

    return isinstance(scaler, FusedGradScaler)


class Optimizer(Capsule):
    """Steps and zeroes ``optimizer`` on gradient-sync micro-steps and posts its learning rates.

    ``max_grad_norm`` (keyword only, an extension over the reference): clip the gradients to this
    global L2 norm before every update (``torch.nn.utils.clip_grad_norm_`` semantics; ``None`` = no
    clipping) and post ``{tag}.grad_norm`` / ``looper.state.grad_norm`` on sync steps.  The fused
    optimizers clip on the device inside their update (``set_grad_clip``: one extra launch, no host
    read, graph-capturable); any other optimizer goes through ``engine.clip_grad_norm_`` on
    gradient-sync steps.  With clipping on, a captured step keeps the update as a launch of its
    own: the global norm needs every final gradient before any element is updated, so the gradient
    producers' update epilogues are not armed (the fused LeNet step is then 4 launches, not 2)."""

    def __init__(self, optimizer: torch.optim.Optimizer, tag: str = "opt", priority: int = 1000, *,
                 max_grad_norm: float | None = None) -> None:
        super().__init__(statefull=False, priority=priority)
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not (math.isfinite(max_grad_norm) and max_grad_norm > 0.0):
                raise ValueError(f"max_grad_norm must be a finite positive number, got {max_grad_norm}")
        self._optimizer = optimizer
        self._tag = tag
        self._iter_idx = 0
        self._max_grad_norm = max_grad_norm
        self._norm_posted = 0  # fused clip: the optimizer's clipped launches reported so far
        self._norm_lap = []    # weak references to this ring lap's posted LazyScalars

    def setup(self, attrs: Attributes | None = None) -> None:
        Capsule.setup(self, attrs=attrs)
        engine = self._accelerator
        found = [o for o in engine._optimizers if o.optimizer is self._optimizer or o is self._optimizer]
        if len(found) > 1:
            raise RuntimeError(f"{self.__class__.__name__}: same optimizer has been registered twice.")
        self._optimizer = found[0] if found else engine.prepare_optimizer(self._optimizer)
        if self._max_grad_norm is not None:
            inner = self._fused_clip_target()
            if inner is not None:
                inner.set_grad_clip(self._max_grad_norm)
                self._norm_posted = inner.norm_launches
            else:
                self._optimizer.clip_max_norm = self._max_grad_norm

    def _fused_clip_target(self):
        """The wrapped optimizer when it clips inside its own update (the fused optimizers)."""
        inner = getattr(self._optimizer, "optimizer", self._optimizer)
        return inner if hasattr(inner, "set_grad_clip") else None

    def _clipping(self):
        """The fused optimizer whose launches currently include the norm pass, or None."""
        if self._max_grad_norm is None:
            return None
        inner = self._fused_clip_target()
        return inner if inner is not None and inner.max_grad_norm is not None else None

    def _norm_lap_guard(self, inner) -> None:
        """Before a clipped launch: if it starts a new lap of the optimizer's norm ring, resolve what
        the last lap posted (a consumer may keep a reported norm across a whole lap) before the
        slots are rewritten — Loss.graph_prepare's rule."""
        if self._norm_lap and inner.norm_launches % inner.GRAD_NORM_RING == 0:
            materialize([r() for r in self._norm_lap if r() is not None])
            self._norm_lap = []

    def step(self) -> None:
        inner = self._clipping()
        if inner is not None and self._accelerator.sync_gradients:
            self._norm_lap_guard(inner)
        if hasattr(self._optimizer, "step_and_zero_grad"):
            self._optimizer.step_and_zero_grad()
        else:
            self._optimizer.step()
            self._optimizer.zero_grad()

    def post(self, attrs: Attributes | None) -> None:
        if not self._accelerator.sync_gradients:
            return
        data = {f"{self._tag}.lr.{i}": g.get("lr") for i, g in enumerate(self._optimizer.param_groups)}
        lrs = list(data.values())
        norm = self._take_norm() if self._max_grad_norm is not None else None
        if norm is not None:
            data[f"{self._tag}.grad_norm"] = norm
        if attrs is not None:
            tracker, looper = attrs.get("tracker"), attrs.get("looper")
            if tracker is not None:
                tracker.scalars.append(Attributes(step=self._iter_idx, data=data))
            if looper is not None:
                looper["state"]["lr"] = lrs
                if norm is not None:
                    looper["state"]["grad_norm"] = norm
        self._iter_idx += 1

    def _take_norm(self):
        """This sync step's global gradient norm as a device-backed value (no host read), or None
        when no clip ran (no gradients, or grad disabled)."""
        inner = self._clipping()
        if inner is not None:
            n = inner.norm_launches
            if n == self._norm_posted:
                return None
            self._norm_posted = n
            value = LazyScalar(inner.grad_norm_slot(n - 1))  # the ring slot that launch wrote
            self._norm_lap.append(weakref.ref(value))
            return value
        norm, self._optimizer.last_grad_norm = getattr(self._optimizer, "last_grad_norm", None), None
        if norm is None:
            return None
        return LazyScalar(norm) if isinstance(norm, torch.Tensor) else norm

    def launch(self, attrs: Attributes | None = None) -> None:
        if torch.is_grad_enabled():
            self.step()
        self.post(attrs)

    # ---------------------------------------------------- HIP-graph protocol
    def graph_supported(self) -> bool:
        # fp16: only the device-resident scaler is capturable (check + unscale-in-update + scale
        # rule are device launches); torch's GradScaler reads found_inf on the host
        from rocket_amd.runtime.amp import FusedGradScaler

        scaler = self._accelerator.scaler
        return (hasattr(self._optimizer, "fused_zero_ok") and self._optimizer.fused_zero_ok()
                and (scaler is None or isinstance(scaler, FusedGradScaler)))

    def graph_token(self):
        return self._optimizer.optimizer.version

    def graph_prepare(self, attrs: Attributes | None = None) -> None:
        inner = self._optimizer.optimizer
        if inner._key is None:
            inner.prepare()
        else:
            inner.refresh_hyper()  # pointers are frozen into the graph; only lr & co. can change
        engine = self._accelerator
        clip = self._clipping() is not None
        if clip and engine.sync_gradients:
            self._norm_lap_guard(inner)
        if hasattr(inner, "epilogue_armed"):
            # exact only when the backward's gradients ARE the step's final gradients: one replica,
            # a gradient-sync step and no AMP scaler.  A fused gradient producer (the LeNet weight-
            # gradient launch) then applies the update itself; see _FusedBase.epilogue.
            # Global-norm clipping rules both update epilogues out: the norm needs every final
            # gradient before any element is updated, so the step keeps its separate launches
            # (norm, then update).  The AMP check fold only flags values: it may stay.
            inner.epilogue_armed = (engine.sync_gradients and engine.num_processes == 1 and engine.scaler is None
                                    and _OPT_EPILOGUE and not clip)
            # under the device fp16 scaler the same producer can instead flag non-finite gradients
            # itself (the step's separate check launch is then skipped; see _FusedBase.amp_checked):
            # exact when its gradients are final and local ones are all there is (one replica)
            inner.amp_fold_armed = (engine.sync_gradients and engine.num_processes == 1 and engine.scaler is not None
                                    and _OPT_EPILOGUE and _is_fused_scaler(engine.scaler))
            # W > 1 on the P2P transport: the gradient all-reduce can apply the update in its write-
            # back instead (DataParallel._reduce_with_update); exact under the same conditions with
            # the REDUCED gradients as the final ones
            inner.reduce_epilogue_armed = (engine.sync_gradients and engine.num_processes > 1 and engine.scaler is None
                                           and _OPT_EPILOGUE and not clip)
            if (inner.epilogue_armed or inner.amp_fold_armed or inner.reduce_epilogue_armed) and \
                    not getattr(self, "_epi_tagged", False):
                for g in inner.param_groups:
                    for p in g["params"]:
                        p._rocket_optimizer = inner
                self._epi_tagged = True

    def graph_device(self, attrs: Attributes) -> None:
        return None  # the update needs reduced gradients: phase B

    def graph_device_synced(self, attrs: Attributes) -> None:
        if self._accelerator.sync_gradients:
            inner = self._optimizer.optimizer
            if getattr(inner, "epilogue_done", False):
                inner.epilogue_done = False  # the gradient producer applied this step's update
                return
            # (clipping under data parallelism needs nothing more: this runs after the reduction
            # join, the reduced gradients are identical on every rank, so each rank's norm launch
            # computes the same norm and coefficient bit for bit — no collective)
            scaler = self._accelerator.scaler
            if scaler is not None:
                scaler.step_device(inner, zero_grads=True)  # flag check + scaled update, in-graph
                return
            inner.launch(zero_grads=True)

    def graph_host(self, attrs: Attributes) -> None:
        inner = self._optimizer.optimizer
        if getattr(inner, "epilogue_armed", False):
            inner.epilogue_armed = False
        if getattr(inner, "amp_fold_armed", False):
            inner.amp_fold_armed = False
        if getattr(inner, "reduce_epilogue_armed", False):
            inner.reduce_epilogue_armed = False
        if self._accelerator.sync_gradients and self._clipping() is not None:
            inner.norm_launches += 1  # the replayed step ran the norm launch (the capture did not count it)
        scaler = self._accelerator.scaler
        if scaler is not None and self._accelerator.sync_gradients:
            # the skipped-step flag of the replayed update: copied behind it, read only if asked
            scaler.record_last()
            self._optimizer.step_was_skipped_lazy()
        self.post(attrs)

    def destroy(self, attrs: Attributes | None = None) -> None:
        registry = self._accelerator._optimizers
        for i, o in enumerate(registry):
            if o is self._optimizer:
                registry.pop(i)
                break
        Capsule.destroy(self, attrs=attrs)

    def state_dict(self) -> dict:
        return dict(iter_idx=self._iter_idx)

    def load_state_dict(self, state: dict) -> None:
        self._iter_idx = state["iter_idx"]


class Scheduler(Capsule):
    def __init__(self, scheduler, priority: int = 1000) -> None:
        super().__init__(statefull=False, priority=priority)
        self._scheduler = scheduler

    def setup(self, attrs: Attributes | None = None) -> None:
        Capsule.setup(self, attrs=attrs)
        engine = self._accelerator
        found = [s for s in engine._schedulers if s.scheduler is self._scheduler or s is self._scheduler]
        if len(found) > 1:
            raise RuntimeError(f"{self.__class__.__name__}: same scheduler has been registered twice. ")
        self._scheduler = found[0] if found else engine.prepare_scheduler(self._scheduler)

    def launch(self, attrs: Attributes | None = None) -> None:
        if torch.is_grad_enabled():
            self._scheduler.step()

    # ---------------------------------------------------- HIP-graph protocol (host-only)
    def graph_device(self, attrs: Attributes) -> None:
        return None

    def graph_host(self, attrs: Attributes) -> None:
        self.launch(attrs)

    def destroy(self, attrs: Attributes | None = None) -> None:
        registry = self._accelerator._schedulers
        for i, s in enumerate(registry):
            if s is self._scheduler:
                registry.pop(i)
                break
        Capsule.destroy(self, attrs=attrs)
