"""Model: the tf.keras.Model surface the reference's callers use, executed on MI355X.

    model = Model(inputs, outputs)           predict_model/v3plus.py:347
    model.predict(x)                         predict.py:109, train_model/DeepLabv3plus.py:815
    model.compile(optimizer='adam', loss=edge_focal_loss, metrics=[PA, IoU, MIoU, F1_score])   :834-837
    model.fit_generator(generator, steps_per_epoch, epochs, callbacks, validation_data, validation_steps)  :844-849
    model.load_weights / save_weights        predict.py:21-49, DeepLabv3plus.py:780
    model.optimizer.lr (get/set), model.stop_training, model.summary()

Execution model: the graph is static, so a training step is one forward sweep over the node list (every node
output kept), the fused loss kernel, one reverse sweep that hands each node its output gradient and lets it
launch its dgrad / wgrad kernels (weight gradients land directly in one flat fp32 arena), then ONE fused Adam
launch over the whole arena.  Under data parallelism the gradient arena is all-reduced in buckets over RCCL
(dist.py) between the reverse sweep and Adam.  All arithmetic is in libsegengine; torch supplies memory.
"""
from __future__ import annotations

import collections
import math
import os
import time
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from . import fusion
from . import switches
from .graph import KTensor, Node, ParamSpec, collect_nodes, init_array
from . import layers as L
from . import losses as LS

ALIGN = 4  # every parameter starts on a 16-byte boundary inside its arena


class _Shared:
    __slots__ = ("t",)

    def __init__(self, t):
        self.t = t


class LRVariable:
    """`model.optimizer.lr`: what the reference hands to K.get_value / K.set_value (DeepLabv3plus.py:658,736)."""

    def __init__(self, v):
        self.value = float(v)

    def assign(self, v):
        self.value = float(v)

    def numpy(self):
        return np.float32(self.value)

    def __float__(self):
        return self.value

    def __repr__(self):
        return f"<lr {self.value:g}>"


class Optimizer:
    """Keras-2 Adam state holder (`compile(optimizer='adam')`); `lr` is what the LR callbacks set."""

    def __init__(self, lr=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
        self._lr = LRVariable(lr)
        self.beta_1, self.beta_2, self.epsilon = beta_1, beta_2, epsilon
        self.iterations = 0

    @property
    def lr(self):
        return self._lr

    @lr.setter
    def lr(self, v):
        self._lr.assign(float(v))

    learning_rate = lr

    def step_scalars(self):
        """(lr_t, lr) of the step just counted (iterations already incremented): Adam's bias-corrected rate and the plain one."""
        t = self.iterations
        lr = float(self.lr)
        return lr * math.sqrt(1.0 - self.beta_2 ** t) / (1.0 - self.beta_1 ** t), lr

    def _plain(self):
        """The reference's Adam: the update is the one sg_adam_step call (optimizers.py overrides this when an option is set)."""
        return True

    def prepare(self, rt):
        """State beyond the runtime's own m / v arenas (optimizers.py): plain Adam has none."""

    def apply(self, rt, eng, grad_scale=1.0, lr_dev=None):
        """The update of one step on rt's arenas - the one place the eager step, the captured step and its segmented form
        launch it.  lr_dev: a device tensor {lr_t, lr, ..} the kernel reads instead of arguments (GraphedTrainStep.lr)."""
        lr_t = 0.0 if lr_dev is not None else self.step_scalars()[0]
        eng.adam_step(rt.w_train, rt.adam_m, rt.adam_v, rt.g_train, lr_t, self.beta_1, self.beta_2, self.epsilon, grad_scale,
                      lr_dev=lr_dev)


class History:
    def __init__(self):
        self.history: Dict[str, list] = {}
        self.epoch: List[int] = []


# What a loss's forward call leaves.  carry: the one tensor its backward call reads (region: coef [images, 2C]; mined: the int32
# [4] record {T, n_kept}; Lovasz: g = dL_lovasz/dp [rows, C]; else None).  terms: the Lovasz {L, L_point, L_lovasz}; rows: mined rows
_LossState = collections.namedtuple("_LossState", "carry terms rows", defaults=(None, None, None))


class _LossHead:
    """The loss side of a step, chosen once in compile().  route: "lovasz", "mined" or "region" (in this order of precedence;
    desc = the descriptor fields the sg_loss_<route>_fwd/bwd pair runs by), else "two_class" (two classes with the reference's
    weights: the 2-class entry points) or "n_class" (sg_lossn_* with the per-class weights).  fwd returns the loss scalar [1] and
    leaves `state`, which bwd reads: a captured step keeps ITS state (GraphedTrainStep.loss_state) for after every replay."""

    def __init__(self, model):
        named = (("lovasz", model.loss_lovasz), ("mined", model.loss_mining), ("region", model.loss_region))
        self.route, self.desc = next((rd for rd in named if rd[1] is not None),
                                     ("two_class" if model._two_class() else "n_class", None))
        self.kind, self.alpha = model.loss_kind, model.loss_alpha
        self.state = _LossState()

    def fwd(self, eng, p, y):
        if self.desc is None:
            return eng.loss_fwd(self.kind, p, y) if self.route == "two_class" else eng.lossn_fwd(self.kind, p, y, self.alpha)
        if self.route == "mined":
            out, sel = eng.loss_mined_fwd(self.desc, p, y)
            self.state = _LossState(sel, rows=p.numel() // p.shape[-1])
            return out
        lovasz = self.route == "lovasz"
        terms, carry = (eng.loss_lovasz_fwd if lovasz else eng.loss_region_fwd)(self.desc, p, y)
        self.state = _LossState(carry, terms if lovasz else None)
        return terms[:1]

    def bwd(self, eng, p, y):
        if self.desc is None:
            return eng.loss_bwd(self.kind, p, y, 1.0) if self.route == "two_class" else eng.lossn_bwd(self.kind, p, y, self.alpha, 1.0)
        call = {"lovasz": eng.loss_lovasz_bwd, "mined": eng.loss_mined_bwd, "region": eng.loss_region_bwd}[self.route]
        return call(self.desc, p, y, self.state.carry, 1.0)


class Model:
    def __init__(self, inputs, outputs, name=None, seed: int = 1103, dtype=None):
        """dtype: "float32" (the reference's precision) or "mixed_bfloat16" / "bfloat16" = bf16 storage of every
        activation with fp32 arithmetic, fp32 master weights, BatchNorm statistics, softmax head, loss and Adam
        (BASELINE config 3); None takes mixed_precision.global_policy()."""
        self.inputs = [inputs] if isinstance(inputs, KTensor) else list(inputs)
        self.outputs = [outputs] if isinstance(outputs, KTensor) else list(outputs)
        assert len(self.inputs) == 1 and len(self.outputs) == 1, "the path's models are single-input single-output"
        self.name = name or "model"
        self.nodes: List[Node] = collect_nodes(self.outputs)
        for i, n in enumerate(self.nodes):
            n.index = i
        # a dropout node's word of the generator's counter: its ordinal among the model's dropout nodes in topological order
        # (a layer given seed= keeps seed mod 2^32, but still counts)
        for k, n in enumerate(n for n in self.nodes if isinstance(n, L._DropoutNode)):
            if n.seed is None:
                n.rng_stream = k
        self.seed = seed
        self.stop_training = False
        self.optimizer: Optional[Optimizer] = None
        self.loss_kind: Optional[int] = None
        self._head: Optional[_LossHead] = None   # compile() chooses it
        self.metric_names: List[str] = []
        self._rt = None
        from . import mixed_precision
        self.compute_dtype = mixed_precision.resolve(dtype)   # "float32" | "bfloat16"
        if self.compute_dtype == "bfloat16":
            # the fp32 head of a bf16 model (SG_HEAD_F32) is a convolution of at most 4 output channels: the library
            # refuses any wider one, so say so here and not at the first batch
            for n in self.nodes:
                if isinstance(n, L._ConvNode) and n.activation == "softmax" and n.filters > 4:
                    _, h, w, cin = n.inputs[0].shape
                    raise ValueError(
                        f"softmax head {n.k}x{n.k} on [{h},{w},{cin}] with {n.filters} classes: under bf16 storage the "
                        "convolution code keeps an fp32 head of at most 4 output channels (SG_HEAD_F32); build this model "
                        "with dtype='float32'")
        self._fuse()
        self._layout_params()
        self.dist = None  # set by dist.DataParallel

    # ------------------------------------------------------------------------------------- graph passes
    def _fuse(self):
        """Mark the fusions this graph takes (fusion.py: the rules, their order and what each reads of the others)."""
        fusion.run(self.nodes, self.outputs)

    def _layout_params(self):
        self.params: List[ParamSpec] = [p for n in self.nodes for p in n.params]
        off_t = off_n = 0
        for p in self.params:
            if p.trainable:
                p.offset, off_t = off_t, off_t + (p.size + ALIGN - 1) // ALIGN * ALIGN
            else:
                p.offset, off_n = off_n, off_n + (p.size + ALIGN - 1) // ALIGN * ALIGN
        self._n_train, self._n_frozen = off_t, off_n

    # ---------------------------------------------------------------------------------------- inspection
    @property
    def layers(self):
        return self.nodes

    @property
    def trainable_weights(self):
        return [p for p in self.params if p.trainable]

    @property
    def non_trainable_weights(self):
        return [p for p in self.params if not p.trainable]

    def count_params(self):
        return sum(p.size for p in self.params)

    def summary(self, print_fn=print):
        print_fn(f'Model: "{self.name}"')
        print_fn(f"{'Layer (type)':<44}{'Output Shape':<26}{'Param #':>10}")
        for n in self.nodes:
            print_fn(f"{n.name + ' (' + n.op + ')':<44}{str(n.output.shape):<26}{sum(p.size for p in n.params):>10}")
        tr = sum(p.size for p in self.params if p.trainable)
        print_fn(f"Total params: {self.count_params():,}")
        print_fn(f"Trainable params: {tr:,}")
        print_fn(f"Non-trainable params: {self.count_params() - tr:,}")

    def flops(self, batch=1) -> int:
        """Nominal forward FLOPs (2*MACs of conv / convT / dense), SURVEY.md §8d convention."""
        return sum(n.flops(batch) for n in self.nodes)

    # ------------------------------------------------------------------------------------------- runtime
    def _runtime(self):
        if self._rt is None:
            self._rt = _Runtime(self)
        return self._rt

    def get_weights(self) -> List[np.ndarray]:
        rt = self._runtime()
        return [rt.param(p).detach().cpu().numpy().copy() for p in self.params]

    def set_weights(self, weights: Sequence[np.ndarray]):
        import torch
        rt = self._runtime()
        if len(weights) != len(self.params):
            raise ValueError(f"set_weights: expected {len(self.params)} arrays, got {len(weights)}")
        for p, w in zip(self.params, weights):
            w = np.asarray(w, dtype=np.float32)
            if tuple(w.shape) != p.shape:
                raise ValueError(f"set_weights: {p.name} expects {p.shape}, got {w.shape}")
            rt.param(p).copy_(torch.from_numpy(np.ascontiguousarray(w)))
        rt.weights_changed()

    def get_gradients(self) -> List[np.ndarray]:
        """Trainable-weight gradients of the last train step / backward, in trainable_weights order."""
        rt = self._runtime()
        return [rt.grad(p).detach().cpu().numpy().copy() for p in self.params if p.trainable]

    def save_weights(self, path):
        """Under data parallelism the BatchNorm moving statistics of the replicas are averaged first and only rank 0
        writes the file; every rank must call it (it is a collective then)."""
        from .weights_io import save_weights
        if self.dist is None:
            save_weights(self, path)
            return
        self.dist.sync_moving_stats(self._runtime())
        err = None
        if self.dist.rank == 0:
            try:
                save_weights(self, path)
            except Exception as e:  # the other ranks are about to enter the collective below: meet them there first
                err = e
        failed = self.dist.any_failed(err is not None)  # collective OR of the outcome; doubles as the barrier
        if err is not None:
            raise err
        if failed:
            raise RuntimeError(f"save_weights({path!r}) failed on rank 0")

    def load_weights(self, path):
        from .weights_io import load_weights
        load_weights(self, path)

    # ------------------------------------------------------------------------------------------ compile
    def compile(self, optimizer="adam", loss=None, metrics=None, jit_compile=False, **kw):
        """jit_compile (tf.keras's name for "compile the train step"): capture the whole training step - forward, loss,
        metric counts, backward, Adam - into one hipGraph per input shape and replay it (GraphedTrainStep).  Same
        kernels, same order: bit-identical to the eager step; ~1800 launches per step become one.

        loss: one of the reference's three, or a region-overlap loss (losses.dice_loss, jaccard_loss, tversky_loss(a, b)) or
        losses.compound(pointwise, region); logs["loss"] is then L = pointwise_weight * L_point + region_weight * L_region.
        Under data parallelism (model.dist) every rank computes the region term on its own batch; the gradients are averaged
        as ever and the logged loss is the mean over the ranks.

        losses.hard_mining(pointwise, thresh, min_kept) averages `pointwise` over the hard pixels of the batch only: those whose
        true-class probability is <= T = max(thresh, the k-th smallest of the batch), every tie at T kept (sg_loss_mined_*; the
        selection runs on the device, so a captured step needs no host round trip).  last_hard_mining() reports T and the kept
        count of the last step.  Under data parallelism every rank mines its OWN shard (k is taken of the shard's pixels); the
        gradients are averaged as ever and the logged loss is the mean over the ranks.

        losses.lovasz_loss, alone or as losses.compound(pointwise, lovasz_loss): the Lovasz-Softmax surrogate of the Jaccard index
        (sg_loss_lovasz_*: the pixels' errors are ranked per class by a stable radix sort on the device, so a captured step needs
        no host round trip).  logs["loss"] is L = pointwise_weight * L_point + region_weight * L_lovasz; last_loss_terms()
        reports the three.  Under data parallelism every rank ranks its OWN shard - ranks are not exchanged, the same documented
        choice as for the region losses -; the gradients are averaged as ever and the logged loss is the mean over the ranks."""
        if isinstance(optimizer, str):   # 'adam' (the reference's, DeepLabv3plus.py:835) | 'adamw' | 'sgd'; else a ValueError
            from . import optimizers
            optimizer = optimizers.get(optimizer)
        self.optimizer = optimizer
        self.loss_kind = LS.resolve_loss(loss)
        # per-class weights of the focal losses (loss.with_alpha(...)); None: the 2-class kernels' built-in ones.  A wrong
        # count, or edge_focal_loss without weights on more than two classes, is a ValueError here
        self.loss_alpha = LS.resolve_alpha(loss, self.num_classes)
        # a region-overlap loss or a compound: the descriptor fields sg_loss_region_* run by, else None.  (Under data
        # parallelism the sums I, P, Y are not exchanged: the mean of the ranks' region losses is not the region loss of the
        # global batch.)
        self.loss_region = LS.resolve_region(loss, self.num_classes)
        # hard_mining(pointwise); lovasz_loss or compound(pointwise, lovasz_loss): the fields sg_loss_mined_* / sg_loss_lovasz_* run by
        self.loss_mining = LS.resolve_mining(loss, self.num_classes)
        self.loss_lovasz = LS.resolve_lovasz(loss, self.num_classes)
        self._head = _LossHead(self)   # the route these fields select, and the last step's state
        self.metric_names = [LS.resolve_metric(m) for m in (metrics or [])]
        self.jit_compile = bool(jit_compile)
        self._train_graphs = {}
        self._train_graph_seen = {}

    def ema_weights(self):
        """Context manager: inside it the trainable weights are the optimizer's moving average (use_ema=True), for predict /
        test_on_batch / save_weights; on exit the training weights are back to the bit (optimizers.ema_weights)."""
        from . import optimizers
        return optimizers.ema_weights(self)

    @property
    def num_classes(self) -> int:
        """C of the softmax head: the last axis of the model's output."""
        return int(self.outputs[0].shape[-1])

    # two classes with the reference's weights: the 2-class entry points (and the four counts {TP, TN, FP, FN}), as ever
    def _two_class(self):
        return self.num_classes == 2 and getattr(self, "loss_alpha", None) is None

    def last_hard_mining(self):
        """dict(threshold=T, kept=n_kept, rows=rows) of the last train_on_batch / test_on_batch under a hard_mining loss (this
        rank's shard under data parallelism): one host sync, taken only here.  None when the loss is not mined or no step ran."""
        st = getattr(self._head, "state", _LossState())   # (rows: set by a mined step alone)
        if st.rows is None:
            return None
        w = st.carry.cpu().numpy().view(np.uint32)
        return dict(threshold=float(w[:1].view(np.float32)[0]), kept=int(w[2]) | (int(w[3]) << 32), rows=int(st.rows))

    def last_loss_terms(self):
        """dict(loss=L, pointwise=L_point, lovasz=L_lovasz) of the last train_on_batch / test_on_batch under lovasz_loss or
        compound(pointwise, lovasz_loss) (this rank's shard under data parallelism): one host sync, taken only here.  None when
        the loss has no Lovasz term or no step ran."""
        st = getattr(self._head, "state", _LossState())   # (terms: set by a Lovasz step alone)
        if st.terms is None:
            return None
        v = st.terms.cpu().numpy()
        return dict(loss=float(v[0]), pointwise=float(v[1]), lovasz=float(v[2]))

    def _counts(self, eng, p, y):
        if not self.metric_names:
            return None
        return eng.confusion_counts(p, y) if self.num_classes == 2 else eng.confusion_matrix(p, y)

    # ------------------------------------------------------------------------------------------ predict
    def predict(self, x, batch_size=32, verbose=0, **kw):
        """numpy [N,H,W,3] (any float dtype; predict.py feeds float64) -> numpy float32 probabilities [N,H,W,C]."""
        import torch
        rt = self._runtime()
        x = np.asarray(x)
        outs = []
        for i in range(0, x.shape[0], batch_size):
            xh = torch.from_numpy(np.ascontiguousarray(x[i:i + batch_size], dtype=np.float32))
            # serialised per device (buildAPI.py:78,111 calls predict from Flask request threads on shared models):
            # the value table of the sweep and the engine's scratch buffer are not re-entrant
            with rt.eng.lock:
                outs.append(rt.forward(xh.to(rt.eng.device), training=False).cpu().numpy())
                rt.release()
        return np.concatenate(outs, 0)

    def _last_use(self):
        lu = getattr(self, "_lu", None)
        if lu is None:
            lu = {}
            for i, n in enumerate(self.nodes):
                for t in n.inputs:
                    lu[id(t)] = i
            lu.pop(id(self.outputs[0]), None)
            self._lu = lu
        return lu

    def capture_predict(self, batch: int):
        """hipGraph-captured inference forward for a fixed batch (BASELINE config 5): returns a callable
        `f(x_dev[batch,H,W,3]) -> probs_dev` that replays ONE graph launch instead of several hundred kernel
        launches.  Every libsegengine entry point is capture-safe (no allocation / synchronisation inside)."""
        return GraphedPredict(self, batch)

    def predict_device(self, x_dev):
        """Device tensor in, device tensor out (used by the tile pipeline and the benchmark)."""
        rt = self._runtime()
        with rt.eng.lock:
            y = rt.forward(x_dev, training=False)
            rt.release()
        return y

    def __call__(self, x, training=False):
        return self.predict_device(x) if not training else self._runtime().forward(x, True)

    # ----------------------------------------------------------------------------------------- training
    def train_on_batch(self, x, y, return_device_scalars=False):
        """One optimisation step; x [N,H,W,3], y [N,H,W,4|2] as numpy or device tensors.
        Returns dict(loss=..., PA=..., ...) of python floats (forces one host sync) unless
        `return_device_scalars`."""
        import torch
        if self.optimizer is None or self.loss_kind is None:
            raise RuntimeError("compile() the model before training")
        rt = self._runtime()
        with rt.eng.lock:
            xd, yd = rt.to_device(x), rt.to_device(y)
            if getattr(self, "jit_compile", False):
                key = (tuple(xd.shape), tuple(yd.shape), xd.dtype, yd.dtype)
                g = self._train_graphs.get(key)
                if g is None:
                    # two eager steps per shape first: they size the scratch buffer and the weight-plane arena, run every
                    # kernel's one-time attribute calls and warm the allocator - and they are real training steps
                    seen = self._train_graph_seen.get(key, 0)
                    self._train_graph_seen[key] = seen + 1
                    if seen >= 2:
                        g = self._train_graphs[key] = GraphedTrainStep(self, xd, yd)
                if g is not None:
                    loss, counts = g.run(xd, yd)
                    self._head.state = g.loss_state   # of THIS graph's step (a test_on_batch in between leaves its own here)
                    return (loss, counts) if return_device_scalars else self._logs(loss, counts)
            rt.write_rng(self.optimizer.iterations)   # (a model without dropout: nothing)
            p = rt.forward(xd, training=True)
            loss = self._head.fwd(rt.eng, p, yd)
            counts = self._counts(rt.eng, p, yd)
            dp = self._head.bwd(rt.eng, p, yd)
            rt.backward(dp)
            grad_scale = 1.0
            if self.dist is not None:
                grad_scale = self.dist.allreduce_grads(rt)
                loss, counts = self.dist.reduce_step_scalars(loss, counts)  # logs describe the GLOBAL batch
            opt = self.optimizer
            opt.iterations += 1
            opt.apply(rt, rt.eng, grad_scale)
            rt.weights_changed()
            rt.release()
        if return_device_scalars:
            return loss, counts
        return self._logs(loss, counts)

    def test_on_batch(self, x, y):
        rt = self._runtime()
        with rt.eng.lock:
            xd, yd = rt.to_device(x), rt.to_device(y)
            p = rt.forward(xd, training=False)
            loss = self._head.fwd(rt.eng, p, yd)
            counts = self._counts(rt.eng, p, yd)
            if self.dist is not None:  # val_* logs describe the GLOBAL validation batch on every rank, as the training
                loss, counts = self.dist.reduce_step_scalars(loss, counts)  # logs do: callbacks then decide alike
            rt.release()
        return self._logs(loss, counts)

    def _logs(self, loss, counts):
        logs = {"loss": float(loss.item())}
        if counts is not None:
            c = [int(v) for v in counts.cpu().tolist()]
            if len(c) == 4 and self.num_classes == 2:
                m = LS.metrics_from_counts(*c)          # tp, tn, fp, fn
            else:
                m = LS.metrics_from_matrix(np.asarray(c, np.int64).reshape(self.num_classes, self.num_classes))
            for name in self.metric_names:
                logs[name] = m[name]
        return logs

    def fit_generator(self, generator, steps_per_epoch=None, epochs=1, verbose=1, callbacks=None,
                      validation_data=None, validation_steps=None, initial_epoch=0, **kw):
        """Keras-2 `fit_generator` loop (train_model/DeepLabv3plus.py:844-849): per-batch callbacks, epoch
        logs are the MEAN of the per-batch values, validation in inference mode."""
        callbacks = list(callbacks or [])
        hist = History()
        for cb in callbacks:
            cb.set_model(self)
        self.stop_training = False
        for cb in callbacks:
            cb.on_train_begin({})
        for epoch in range(initial_epoch, epochs):
            for cb in callbacks:
                cb.on_epoch_begin(epoch, {})
            sums: Dict[str, float] = {}
            t0 = time.time()
            for step in range(steps_per_epoch):
                for cb in callbacks:
                    cb.on_batch_begin(step, {})
                x, y = next(generator)
                logs = self.train_on_batch(x, y)
                for k, v in logs.items():
                    sums[k] = sums.get(k, 0.0) + v
                for cb in callbacks:
                    cb.on_batch_end(step, dict(logs))
            ep_logs = {k: v / max(steps_per_epoch, 1) for k, v in sums.items()}
            if validation_data is not None:
                vs: Dict[str, float] = {}
                nval = validation_steps or 1
                for _ in range(nval):
                    x, y = next(validation_data)
                    for k, v in self.test_on_batch(x, y).items():
                        vs[k] = vs.get(k, 0.0) + v
                ep_logs.update({"val_" + k: v / nval for k, v in vs.items()})
            if verbose:
                msg = " - ".join(f"{k}: {v:.4f}" for k, v in ep_logs.items())
                print(f"Epoch {epoch + 1}/{epochs} - {time.time() - t0:.1f}s - {msg}")
            hist.epoch.append(epoch)
            for k, v in ep_logs.items():
                hist.history.setdefault(k, []).append(v)
            for cb in callbacks:
                cb.on_epoch_end(epoch, ep_logs)
            if self.stop_training:
                break
        for cb in callbacks:
            cb.on_train_end({})
        self.history = hist
        return hist

    def fit(self, x=None, y=None, batch_size=None, epochs=1, steps_per_epoch=None, **kw):
        if hasattr(x, "__next__"):
            return self.fit_generator(x, steps_per_epoch=steps_per_epoch, epochs=epochs, **kw)
        x, y = np.asarray(x), np.asarray(y)
        bs = batch_size or 32
        steps = steps_per_epoch or max(x.shape[0] // bs, 1)

        def gen():
            while True:
                for i in range(steps):
                    yield x[i * bs:(i + 1) * bs], y[i * bs:(i + 1) * bs]
        return self.fit_generator(gen(), steps_per_epoch=steps, epochs=epochs, **kw)


class _CaptureGuard:
    """Around a stream capture: Python's cyclic garbage collector must not run inside it.  A collection can finalise an
    unrelated hipGraph (e.g. the captured step of a model dropped earlier, kept alive until now by a reference cycle), and
    destroying a graph while a stream is capturing is a HIP error that ends the process (hipErrorStreamCaptureUnsupported
    thrown from a destructor).  Collect first, then keep the collector off until the capture has ended."""

    def __enter__(self):
        import gc
        gc.collect()
        self._was = gc.isenabled()
        gc.disable()
        return self

    def __exit__(self, *exc):
        import gc
        if self._was:
            gc.enable()
        return False


class GraphedPredict:
    """Static-shape inference forward captured into a hipGraph (stream capture of the engine's launches)."""

    def __init__(self, model: Model, batch: int):
        import torch
        rt = model._runtime()
        self.torch, self.rt = torch, rt
        shape = (batch,) + tuple(model.inputs[0].shape[1:])
        eng = rt.eng
        with eng.lock:
            self.x = eng.zeros(*shape)
            peak_before, eng._ws_peak = eng._ws_peak, 0
            for _ in range(2):  # warm-up outside capture: first-launch attribute calls, and the sizing pass of the scratch
                rt.forward(self.x, training=False)
                rt.release()
            torch.cuda.synchronize(eng.device)
            # The graph's kernel nodes carry the scratch pointer: give this graph a buffer of its own (sized by the
            # warm-up pass), never the engine's shared one, which a later eager call or another model may re-grow.
            self.ws = torch.empty(max(eng._ws_peak, 256) + 256, dtype=torch.uint8, device=eng.device)
            # the engine-wide peak stays monotone: a training-step capture that follows sizes its buffer by it
            eng._ws_peak = max(eng._ws_peak, peak_before)
            self.graph = torch.cuda.CUDAGraph()
            with eng.private_ws(self.ws), _CaptureGuard():
                with torch.cuda.graph(self.graph):
                    self.y = rt.forward(self.x, training=False)
            rt.values = {}
            # the planes this graph reads: kept alive and refreshed by the graph's owner, whatever the runtime's current
            # planes are by then (a later call with another batch size re-keys and re-allocates them)
            self._planes = (rt._planes_arena, rt._planes_jobs, rt._planes_launch)
            self._planes_version = rt._w_version

    def __call__(self, x_dev):
        """Replays the graph on x_dev.  The returned tensor is the graph's static output buffer: consume (or clone) it
        before the next call."""
        with self.rt.eng.lock:
            if self._planes_version != self.rt._w_version and self._planes[0] is not None:  # weights replaced since
                self.rt.prepare_into(*self._planes)
                self._planes_version = self.rt._w_version
            self.x.copy_(x_dev, non_blocking=True)
            self.graph.replay()
        return self.y


class _Lane:
    """The filter-gradient calls deferred while one segment of a training step is captured (ops.Engine.side_run)."""

    def __init__(self):
        self.thunks, self.keep, self.blocks = [], [], 0

    def defer(self, fn, tensors):
        self.thunks.append(fn)
        self.keep.extend(tensors)
        self.blocks += 1

    def take(self):
        out = (self.thunks, self.keep)
        self.thunks, self.keep, self.blocks = [], [], 0
        return out


class GraphedTrainStep:
    """One optimisation step of a compiled model - forward, loss, confusion counts, backward, Adam - captured into
    hipGraphs for one (x, y) shape (Model.compile(jit_compile=True)).  The step's inputs are two static device buffers, its
    outputs (loss, counts) two more; the learning rates (Adam's bias-corrected one and the plain one), the only numbers that
    change from replay to replay, are read by the kernel from a small device buffer written before each replay
    (sg_adam_step_lr; sg_optim_step for an optimizer with options, whose norm pass is recorded in front of it).  The weight
    planes are rebuilt inside the graph (the capture starts with them marked stale), BatchNorm's moving statistics and the
    optimiser moments are updated in place as in the eager step.

    The capture is CUT into a chain of graph SEGMENTS, plus one graph for Adam:
      * under data parallelism (model.dist set) wherever the backward sweep completes a gradient bucket
        (dist.BucketReducer's schedule): between two segments the host hands the finished bucket to the transport EXACTLY as
        the eager step does (an eager sg_comm_allreduce_sum / all_reduce on the communication stream), so RCCL never runs
        inside a capture and the all-reduce of bucket k still overlaps the backward of segment k+1;
      * with lanes (SG_JIT_LANES, default on) also every SG_JIT_LANE_BLOCKS filter gradients: a segment's filter-gradient
        calls are NOT recorded into its main graph M_k but collected (Engine.side_run -> _Lane) and recorded, right after
        M_k, into a side graph W_k of their own.  The replay launches M_0, W_0 || M_1, W_1 || M_2 ...: W_k goes to the
        second stream behind an event after M_k and runs beside M_(k+1) - the eager step's overlap of the MFMA-bound filter
        gradients with the bandwidth-bound kernels of the chain, for two graph launches and three event
        calls per segment instead of ~1800 kernel launches.  (ONE forked graph replays correctly too, but hipGraphLaunch
        then queues its nodes from the host one by one: 56 ms.)  Memory: the operands W_k reads live in the capture's pool;
        they are held until the capture of M_(k+2) begins, and the replay makes M_(k+2) wait for W_k.
    Same kernels on the same operands as the eager step: bit-identical results."""

    def __init__(self, model: "Model", xd, yd):
        import torch
        rt = model._runtime()
        eng = rt.eng
        self.torch, self.model, self.rt = torch, model, rt
        opt = model.optimizer
        dist = model.dist
        self.x, self.y = torch.empty_like(xd), torch.empty_like(yd)
        self.lr = eng.zeros(4)     # {lr_t, lr, -, -}: the step's scalars, written before every replay
        self._lr1 = self.lr[1:2]
        opt.prepare(rt)            # tables and arenas of an optimizer with options: allocated here, outside the capture
        lanes = switches.get("SG_JIT_LANES") and eng._side_on
        lane_blocks = max(1, switches.get("SG_JIT_LANE_BLOCKS"))
        # (the eager sizing steps ran the filter gradients on the side stream with its own scratch; without lanes they run
        # inline here, on the main scratch)
        self.ws = torch.empty(max(eng._ws_peak, eng._ws2_peak, 256) + 256, dtype=torch.uint8, device=eng.device)
        self.ws2 = torch.empty(max(eng._ws2_peak, 256) + 256, dtype=torch.uint8, device=eng.device) if lanes else None
        rt.release()
        # The job table of the weight planes is (re)built HERE, outside the capture, for this batch and mode: a forward with
        # another batch size since the eager warm-up steps (a validation batch, a predict()) has re-keyed the runtime's
        # planes, and the rebuild allocates the plane arena and copies the table from pageable host memory - neither may
        # happen inside a stream capture.  What the capture then records of ensure_planes is the one sg_prepare_planes launch.
        rt.ensure_planes(int(xd.shape[0]), True)
        rt.weights_changed()  # the graph must contain the plane preparation: every replay follows an optimiser step
        self._planes_key = rt._planes_key
        torch.cuda.synchronize(eng.device)
        self.segments = []        # [main graph, [(start, end) arena ranges complete after it], side graph | None, kept operands]
        segmented = dist is not None or lanes
        pool = torch.cuda.graph_pool_handle() if segmented else None
        cuts = _SegmentCuts(dist.reducer.buckets) if dist is not None else None
        lane = _Lane() if lanes else None
        state = {"ctx": None, "graph": None}
        # every capture is "thread_local" (ADVICE r4): a HIP call from ANOTHER thread during the capture - a DataLoader's
        # pin-memory thread, a Flask predict thread waiting on the Engine lock - must not invalidate it.  The side graphs W_k
        # replay one after the other on the side stream, so they share ONE private pool of their own (never the main graphs':
        # W_k runs beside M_(k+1)) instead of one pool each.
        side_pool = torch.cuda.graph_pool_handle() if lanes else None
        mode = "thread_local"

        def begin():
            if len(self.segments) >= 2:   # the replay makes this segment wait for W_(k-2): its operands may be reused from here on
                self.segments[-2][3] = None
            g = torch.cuda.CUDAGraph()
            kw = {"pool": pool} if pool is not None else {}
            ctx = torch.cuda.graph(g, capture_error_mode=mode, **kw)
            ctx.__enter__()
            state["ctx"], state["graph"] = ctx, g

        def end(ready):
            state["ctx"].__exit__(None, None, None)
            main_graph = state["graph"]
            state["ctx"] = state["graph"] = None
            side_graph, keep = None, None
            if lane is not None and lane.thunks:
                thunks, keep = lane.take()
                side_graph = torch.cuda.CUDAGraph()
                eng.lane = None          # (the calls below ARE the deferred ones)
                eng._in_side = True      # their scratch is the side buffer
                try:
                    with torch.cuda.graph(side_graph, pool=side_pool, capture_error_mode=mode):
                        for fn in thunks:
                            fn()
                finally:
                    eng._in_side = False
                    eng.lane = lane
            self.segments.append([main_graph, ready, side_graph, keep])

        def fires(index):
            return cuts is not None and cuts.next < len(cuts.buckets) and cuts.buckets[cuts.next][2] >= index

        def node_done(index):   # the backward sweep has finished node `index`: cut when that completes buckets / fills the lane
            ready = cuts.pop_ready(index) if cuts is not None else []
            if ready or (lane is not None and lane.blocks >= lane_blocks):
                end(ready)
                if index > 0:   # node 0 ends the sweep: nothing is left to capture behind it
                    begin()

        saved_hook, saved_fires = rt.on_node_done, rt.node_done_fires
        with eng.private_ws(self.ws, self.ws2), _CaptureGuard():
            try:
                rt.on_node_done = node_done if segmented else None
                rt.node_done_fires = fires if segmented else None
                eng.lane = lane
                begin()
                p = rt.forward(self.x, training=True)
                self.loss = model._head.fwd(eng, p, self.y)
                self.loss_state = model._head.state   # the graph's backward pass reads its tensor; the reports read the rest
                self.counts = model._counts(eng, p, self.y)   # zeroed inside the graph, four counts or C x C
                dp = model._head.bwd(eng, p, self.y)
                rt.backward(dp)
                if not segmented:  # the optimizer rides in the same graph
                    opt.apply(rt, eng, 1.0, lr_dev=self.lr)
                    end([])
                else:
                    if state["ctx"] is not None:
                        end(cuts.pop_ready(-1) if cuts is not None else [])
                    assert cuts is None or cuts.done(), "a gradient bucket was never handed over"
                    eng.lane = None
                    begin()  # its own graph: it runs after the LAST all-reduce / side graph has joined the compute stream
                    opt.apply(rt, eng, 1.0 / (dist.world if dist is not None else 1), lr_dev=self.lr)
                    end([])
            finally:
                eng.lane = None
                if state["ctx"] is not None:   # an error inside a capture: leave capture mode before re-raising
                    try:
                        state["ctx"].__exit__(None, None, None)
                    except Exception:
                        pass
                rt.on_node_done, rt.node_done_fires = saved_hook, saved_fires
        for seg in self.segments:
            seg[3] = None   # nothing is allocated in the pool from here on
        self.segmented = segmented
        self.graph = self.segments[0][0]
        self.side_graphs = sum(1 for seg in self.segments if seg[2] is not None)
        self._lanes = _StreamLanes(eng) if self.side_graphs else None
        self._loss_out = self._counts_out = None
        assert rt._planes_key == self._planes_key, "the weight-plane job table was rebuilt inside the capture"
        self._planes = (rt._planes_arena, rt._planes_jobs)  # kept alive: the graph's nodes carry their addresses
        rt.release()
        rt.weights_changed()

    def run(self, xd, yd):
        """Replays the step on (xd, yd).  Returns the graph's static loss / counts buffers: read them before the next step."""
        opt = self.model.optimizer
        dist = self.model.dist
        self.x.copy_(xd, non_blocking=True)
        self.y.copy_(yd, non_blocking=True)
        self.rt.write_rng(opt.iterations)   # the dropout masks' step word: the count BEFORE this step, as in the eager step
        opt.iterations += 1
        lr_t, lr = opt.step_scalars()
        self.lr.fill_(lr_t)
        if not opt._plain():   # sg_optim_step reads the plain rate too (decay, SGD); the reference's Adam keeps its one launch
            self._lr1.fill_(lr)
        if not self.segmented:
            self.graph.replay()
            self.rt.weights_changed()
            return self.loss, self.counts
        run_segments([(g.replay, ready, None if w is None else w.replay) for g, ready, w, _ in self.segments[:-1]],
                     self.rt.g_train, dist.tp if dist is not None else None, self._lanes)
        out = (self.loss, self.counts)
        if dist is not None:
            # loss / counts of the GLOBAL batch: reduced in ordinary buffers of this object (the graphs' own outputs live in
            # the capture's private pool and are rewritten by the next replay)
            if self._loss_out is None:
                self._loss_out = self.torch.empty_like(self.loss)
                self._counts_out = None if self.counts is None else self.torch.empty_like(self.counts)
            self._loss_out.copy_(self.loss)
            if self.counts is not None:
                self._counts_out.copy_(self.counts)
            out = dist.reduce_step_scalars(self._loss_out, self._counts_out)
        self.segments[-1][0].replay()   # Adam on the summed gradients (1 / world folded into the kernel)
        self.rt.weights_changed()
        return out


class _StreamLanes:
    """The two HIP streams of a replayed step with side graphs: `main` is torch's current stream, `side` the engine's second
    stream.  run_segments drives it; the CPU tests pass an object with the same four methods that runs everything in line."""

    def __init__(self, eng):
        import torch
        self.torch, self.eng = torch, eng
        if eng._side_stream is None:
            eng._side_stream = torch.cuda.Stream(device=eng.device)
        self.side = eng._side_stream
        self._free = []

    def _event(self):
        return self._free.pop() if self._free else self.torch.cuda.Event()

    def fork(self):
        """The side stream waits for everything queued on the main stream so far."""
        ev = self._event()
        ev.record(self.torch.cuda.current_stream(self.eng.device))
        self.side.wait_event(ev)
        self._free.append(ev)

    def on_side(self):
        """Context: launches inside go to the side stream."""
        return self.torch.cuda.stream(self.side)

    def mark_side(self):
        """An event behind everything queued on the side stream so far."""
        ev = self._event()
        ev.record(self.side)
        return ev

    def wait_on_main(self, ev):
        """The main stream waits for `ev` (mark_side); the event returns to the pool."""
        if ev is not None:
            self.torch.cuda.current_stream(self.eng.device).wait_event(ev)
            self._free.append(ev)


class _SegmentCuts:
    """Where a captured data-parallel step is cut: `buckets` are dist.plan_buckets' (start, end, ready_node_index) in firing
    order; pop_ready(i) returns the arena ranges that are complete once the backward sweep (descending node index) has
    finished node i - the same rule as dist.BucketReducer.node_done, so the captured step hands buckets over at exactly
    the points the eager step does."""

    def __init__(self, buckets):
        self.buckets = sorted(buckets, key=lambda b: -b[2])
        self.next = 0

    def pop_ready(self, node_index):
        out = []
        while self.next < len(self.buckets) and self.buckets[self.next][2] >= node_index:
            s, e, _ = self.buckets[self.next]
            out.append((s, e))
            self.next += 1
        return out

    def done(self):
        return self.next == len(self.buckets)


def run_segments(segments, arena, transport, lanes=None):
    """The replay loop of a segmented step: `segments` = [(launch, [(start, end), ...], side_launch | None)] (two-element
    entries: no side graph).

    launch() replays the segment's main graph M_k (stream-ordered, returns at once).  side_launch() replays its filter
    gradients W_k: on the side stream (`lanes`: _StreamLanes) behind everything queued on the main stream so far, i.e.
    beside M_(k+1); the main stream waits for W_(k-2) before M_k (W_(k-2)'s operands may be overwritten from M_k on: the
    capture held them that long).  Each arena range a segment completed then goes to the transport's asynchronous
    sum-all-reduce - with lanes ALWAYS issued from the side stream, behind M_k (a fork) and behind every side graph launched so
    far: the range holds gradients that W_k or the side graph of an earlier segment writes - which runs beside the next segment; at the end the main stream joins the side stream
    and the transport before whatever follows (Adam).  Device-agnostic: the CPU tests drive it over gloo with callables that
    write gradients and `lanes` = an in-line stand-in (or None: side launches run in line)."""
    import contextlib
    marks = []
    for k, seg in enumerate(segments):
        launch, ready = seg[0], seg[1]
        side_launch = seg[2] if len(seg) > 2 else None
        if lanes is not None and k >= 2:
            lanes.wait_on_main(marks[k - 2])
            marks[k - 2] = None
        launch()
        ctx = contextlib.nullcontext()
        mark = None
        if side_launch is not None:
            if lanes is not None:
                lanes.fork()
                with lanes.on_side():
                    side_launch()
                mark = lanes.mark_side()
                ctx = lanes.on_side()
            else:
                side_launch()
        marks.append(mark)
        if transport is not None and ready:
            if lanes is not None and side_launch is None:
                # a bucket may hold gradients that the side graph of an EARLIER segment writes (a bucket spans several
                # segments when the lanes cut between two hand-overs) and that graph may still be running: the hand-over
                # always goes through the side stream, behind this segment's main graph and every side graph so far
                lanes.fork()
                ctx = lanes.on_side()
            with ctx:
                for s, e in ready:
                    transport.allreduce_async(arena[s:e])
    if lanes is not None:
        for ev in marks:
            lanes.wait_on_main(ev)
    if transport is not None:
        transport.join()


# mark -> (its run-time switch, the Engine query that says whether the library takes the launch): _Runtime._gate
_GATES = {"bnb_to": ("SG_BN_PW", "conv2d_dgrad_bnb_ok"), "defer_conv": ("SG_BN_CONV", "conv2d_bn_in_ok"),
          "fused_into": ("SG_UP2_FUSE", "conv2d_up2_ok")}


class _Runtime:
    """Device state of one model: arenas, saved activations, gradient bookkeeping."""

    def __init__(self, model: Model):
        import torch
        from .ops import get_engine
        self.torch = torch
        self.model = model
        dev = int(os.environ.get("LOCAL_RANK", "0")) if torch.cuda.is_available() and torch.cuda.device_count() > 1 else 0
        self.eng = get_engine(dev)  # makes `dev` torch's current device (Engine.__init__)
        e = self.eng
        self._gates: Dict[tuple, bool] = {}          # (mark, node, batch, arithmetic) -> the marked fusion is on here (_gate)
        self._x6 = e.lib.sg_get_conv_x6              # the arithmetic mode now: part of that key, asked per node and step
        self._act_planes: Dict[int, tuple] = {}      # id(symbolic tensor) -> (fp32 activation, its bf16 planes) of this step
        self._act_planes_use: Dict[int, bool] = {}   # id(conv node) -> its forward reads planes (geometry)
        self.w_train = e.zeros(max(model._n_train, ALIGN))
        self.g_train = e.zeros(max(model._n_train, ALIGN))
        self.adam_m = e.zeros(max(model._n_train, ALIGN))
        self.adam_v = e.zeros(max(model._n_train, ALIGN))
        self.w_frozen = e.zeros(max(model._n_frozen, ALIGN))
        rng = np.random.default_rng(model.seed)
        host_t = np.zeros(max(model._n_train, ALIGN), np.float32)
        host_n = np.zeros(max(model._n_frozen, ALIGN), np.float32)
        for p in model.params:
            a = init_array(p, rng).reshape(-1)
            (host_t if p.trainable else host_n)[p.offset:p.offset + p.size] = a
        self.w_train.copy_(torch.from_numpy(host_t))
        self.w_frozen.copy_(torch.from_numpy(host_n))
        self._pviews: Dict[int, object] = {}
        self._gviews: Dict[int, object] = {}
        self.values: Dict[int, object] = {}
        self._saved: Dict[int, dict] = {}
        self.bn_stats: Dict[int, tuple] = {}  # id(conv output tensor) -> (per-tile statistics, tiles)
        self.on_node_done = None
        self._pending = None          # the sweep's gradient table while a node's backward runs (take_pending)
        self.node_done_fires = None   # optional predicate: will on_node_done(index) hand gradients over (all-reduce / cut)?
        # weight planes of the matrix-pipe convolutions, prepared once per optimiser step (ensure_planes)
        self._planes_key = None
        self._planes_ptr: Dict[tuple, int] = {}
        self._planes_kind: Dict[tuple, int] = {}
        self._planes_arena = None
        self._planes_jobs = None
        self._planes_launch = (0, 0)
        self._planes_dirty = True
        self._w_version = 0   # bumped by weights_changed(): captured graphs compare it with the version their planes hold
        self._use_planes = switches.get("SG_PREPARED_PLANES")
        # the seed words of the dropout masks {k0, k1, step, 0}, read by sg_dropout on the device; only a model with
        # a dropout node of rate > 0 owns them.  Allocated here, never inside a capture.
        self.rng = None
        if any(isinstance(n, L._DropoutNode) and n.rate > 0 for n in model.nodes):
            self.rng = torch.zeros(4, dtype=torch.int32, device=e.device)
        self._rng_host = [None, None, None]
        self.write_rng(0)   # a fresh runtime draws the masks of step 0

    # -- parameters ---------------------------------------------------------------------------------------
    def param(self, p: ParamSpec):
        v = self._pviews.get(id(p))
        if v is None:
            arena = self.w_train if p.trainable else self.w_frozen
            v = arena[p.offset:p.offset + p.size].view(p.shape)
            self._pviews[id(p)] = v
        return v

    def grad(self, p: ParamSpec):
        v = self._gviews.get(id(p))
        if v is None:
            v = self.g_train[p.offset:p.offset + p.size].view(p.shape)
            self._gviews[id(p)] = v
        return v

    def to_device(self, a):
        torch = self.torch
        if isinstance(a, torch.Tensor):
            return a if a.is_cuda and a.dtype == torch.float32 else a.to(self.eng.device, torch.float32)
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.eng.device)

    # -- prepared weight planes -----------------------------------------------------------------------------
    def weights_changed(self):
        """Call after writing the weight arena (Adam, set_weights, broadcast): the bf16 operand planes the convolution
        kernels read are re-derived from it before the next forward."""
        self._planes_dirty = True
        self._w_version += 1

    def prepare_into(self, arena, jobs, launch):
        """Rebuild the weight planes of a SNAPSHOT (arena, job table, (jobs, blocks)) taken at a hipGraph capture: the graph's
        kernel nodes carry that arena's addresses whatever batch size / mode the runtime's current planes describe."""
        import ctypes as C
        if launch[0]:
            _lib.check(self.eng.lib.sg_prepare_planes(self.eng.h, self.eng.stream, C.c_void_p(self.w_train.data_ptr()),
                                                      C.c_void_p(arena.data_ptr()), C.c_void_p(jobs.data_ptr()), launch[0],
                                                      launch[1]), "sg_prepare_planes")

    def _gate(self, node, mark, x=None) -> bool:
        """Is the fusion that Model._fuse marked on `node` (attribute `mark`: the partner node) on in THIS runtime?  The mark is
        set, the fusion's switch is on, fp32 storage, and the library takes the launch: the partner convolution's own at batch 1,
        or - given `x`, the BatchNormalization's input - the pointwise convolution that produced x, at its batch.  Decided once
        per (node, batch, arithmetic mode: the arithmetic switch may change between steps, tests do)."""
        key = (mark, id(node), 0 if x is None else x.shape[0], self._x6())
        got = self._gates.get(key)
        if got is None:
            c, (switch, ask) = getattr(node, mark), _GATES[mark]
            got = False
            if (c is not None and switches.get(switch) and self.model.compute_dtype == "float32"
                    and (x is None or x.dtype == self.torch.float32)):
                if x is None:
                    _, h, w, cin = c.inputs[0].shape
                    d = self.eng.conv_desc((1, h, w, cin), c.filters, c.k, c.k, c.stride, c.dilation, c.padding)
                else:
                    n, h, w, cout = x.shape
                    d = self.eng.conv_desc((n, h, w, c.inputs[0].shape[-1]), cout, 1, 1, 1, 1, "same")
                got = bool(getattr(self.eng, ask)(d))
            self._gates[key] = got
        return got

    def bnb_on(self, bn_node, x) -> bool:
        """Does THIS runtime leave BatchNormalization `bn_node`'s backward apply to the dgrad of the pointwise convolution that
        produced its input (Model._fuse: bnb_to)?  fp32 storage, a launch the wide pointwise kernel takes at this batch (asked of
        the library), SG_BN_PW=1.  OFF by default: built, bit-identical to the unfused pair, and a LOSS in the step - the 56
        bn_bwd_apply launches it removes (47 us each in the profile) ran beside the side stream's filter gradients for free,
        while the 25 us it adds to every dgrad sit on the matrix pipe, which is what bounds the step (71.13 / 71.43 ms without,
        71.58 / 71.69 with, alternating runs on one box: gpurun_out/r5x; stand-alone 123 us against 22.5 + 96.8)."""
        return self._gate(bn_node, "bnb_to", x)

    def bn_conv_on(self, bn_node) -> bool:
        """Does THIS runtime apply BatchNormalization `bn_node` in the loaders of its consumer convolution (Model._fuse: defer_conv /
        bn_src)?  fp32 storage, a launch geometry the thin 1x1 / patch kernels cover (asked of the library), SG_BN_CONV != 0."""
        return self._gate(bn_node, "defer_conv")

    def planes_in_on(self) -> bool:
        """fp32 storage with the six-pass arithmetic, SG_ACT_PLANES != 0: activation planes are made once per tensor and step."""
        return (self.model.compute_dtype == "float32" and switches.get("SG_ACT_PLANES")
                and int(self.eng.lib.sg_get_conv_x6()) == 1)

    def act_planes(self, node, x, d, make=True):
        """The three bf16 planes of activation `x` (Engine.split_planes), made at most once per tensor and training step - every
        consumer whose forward reads planes (csrc/conv_x6w.h) shares them and its filter gradient takes them again (kept until
        the step's backward sweep ends: release()).  None when `node`'s launches have no use for them."""
        if not self.planes_in_on():
            return None
        key = id(node.inputs[0])
        got = self._act_planes.get(key)
        if got is not None and got[0] is x:
            return got[1]
        if not make:
            return None
        use = self._act_planes_use.get(id(node))
        if use is None:   # decided once per node from its geometry
            use = bool(self.eng.conv2d_planes_in(d, False))
            self._act_planes_use[id(node)] = use
        if not use:
            return None
        pl = self.eng.split_planes(x)
        self._act_planes[key] = (x, pl)
        return pl

    def up2_on(self, up_node) -> bool:
        """Does THIS runtime run the pair `up_node` -> 3x3 convolution (Model._fuse: fused_into / up_src) on the fused kernels?
        fp32 storage, the geometry csrc/conv_x6p.h covers (asked of the library), SG_UP2_FUSE != 0.  Decided once per pair:
        the up-sampling node (identity then) and the convolution must agree."""
        return self._gate(up_node, "fused_into")

    def plane_kind(self, node, tag) -> int:
        """Which kernel family `node`'s launch `tag` takes (sg_conv2d_planes_job's kind; 0: none of the prepared-plane kernels)."""
        return self._planes_kind.get((id(node), tag), 0) if self._planes_ptr else 0

    def planes(self, node, tag):
        """Device address of the prepared planes of `node`'s launch `tag` ("f" / "d"), or None (the launch then converts its
        kernel itself, in the workspace)."""
        return self._planes_ptr.get((id(node), tag))

    def ensure_planes(self, batch: int, training: bool):
        """(Re)build the job table when the batch, the storage dtype or the arithmetic mode changed; convert every kernel of
        the model in ONE launch when the weights changed since the last conversion (sg_prepare_planes)."""
        if not self._use_planes:
            return
        import ctypes as C
        e, m, torch = self.eng, self.model, self.torch
        bwd = training or m.optimizer is not None
        key = (int(batch), m.compute_dtype, e.lib.sg_get_conv_x6(), bwd)
        if key != self._planes_key:
            dt = _lib.SG_BF16 if m.compute_dtype == "bfloat16" else _lib.SG_F32
            jobs, ptr_of, kinds, off, blocks = [], {}, {}, 0, 0
            for n in m.nodes:
                sites = getattr(n, "plane_sites", None)
                if sites is None:
                    continue
                for tag, wspec, d, dgrad, phase, head in sites(self, int(batch)):
                    if (phase == "bwd" and not bwd) or not wspec.trainable:
                        continue
                    job, nbytes = _lib.PlanesJob(), C.c_size_t(0)
                    _lib.check(e.lib.sg_conv2d_planes_job(e.h, dt | (_lib.SG_HEAD_F32 if (head and dt == _lib.SG_BF16) else 0),
                                                          C.byref(d), dgrad, C.byref(job), C.byref(nbytes)), "sg_conv2d_planes_job")
                    if job.kind == 0:
                        continue
                    job.w_off, job.out_off, job.block0 = wspec.offset, off, blocks
                    ptr_of[(id(n), tag)] = off
                    kinds[(id(n), tag)] = int(job.kind)
                    off += (nbytes.value + 255) // 256 * 256
                    blocks += job.nblocks
                    jobs.append(job)
            self._planes_key = key
            self._planes_kind = kinds   # 1: slab kernels (conv_x6 / conv_b16), 2: patch kernel, 3: wide pointwise kernel
            self._planes_ptr = {}
            self._planes_arena = self._planes_jobs = None
            self._planes_launch = (len(jobs), blocks)
            if jobs:
                self._planes_arena = torch.empty(off, dtype=torch.uint8, device=e.device)
                arr = (_lib.PlanesJob * len(jobs))(*jobs)
                host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
                self._planes_jobs = host.to(e.device)
                base = self._planes_arena.data_ptr()
                self._planes_ptr = {k: base + o for k, o in ptr_of.items()}
            self._planes_dirty = True
        if self._planes_dirty and self._planes_launch[0]:
            _lib.check(e.lib.sg_prepare_planes(e.h, e.stream, C.c_void_p(self.w_train.data_ptr()),
                                               C.c_void_p(self._planes_arena.data_ptr()), C.c_void_p(self._planes_jobs.data_ptr()),
                                               self._planes_launch[0], self._planes_launch[1]), "sg_prepare_planes")
        self._planes_dirty = False

    # -- dropout seed words -------------------------------------------------------------------------------
    def rng_words(self):
        if self.rng is None:
            raise RuntimeError("this runtime owns no dropout seed words: the model had no dropout node of rate > 0 when it was built")
        return self.rng

    def write_rng(self, step: int):
        """{k0, k1, step} = {model.seed mod 2^32, data-parallel rank, optimizer.iterations before the step counts itself} into the
        device words, with device fills (no copy from pageable host memory); a word that has not changed is not written again.
        Model.train_on_batch and GraphedTrainStep.run call this before the forward / the replays.  A direct
        forward(x, training=True) does not: it draws the masks of whatever the words hold (step 0 on a fresh runtime)."""
        if self.rng is None:
            return
        m = self.model
        words = (int(m.seed) % (1 << 32), (int(m.dist.rank) if m.dist is not None else 0) % (1 << 32), int(step) % (1 << 32))
        for i, v in enumerate(words):
            if self._rng_host[i] != v:
                self.rng[i:i + 1].fill_(v - (1 << 32) if v >= (1 << 31) else v)   # (the same 32 bits in torch's signed type)
                self._rng_host[i] = v

    # -- tape ---------------------------------------------------------------------------------------------
    def save(self, node, **kw):
        self._saved.setdefault(id(node), {}).update(kw)

    def saved(self, node):
        return self._saved[id(node)]

    def needs_grad(self, sym: KTensor) -> bool:
        return sym.node is not None

    def take_pending(self, sym: KTensor, owned_only: bool = False):
        """Inside a node's backward: the gradient collected so far for tensor `sym` (the node's input, or the tensor its input
        is an identity of), REMOVED from the sweep's table; None if there is none.  The node must return an input gradient
        that includes it - the table then receives the complete gradient and no separate add runs.  owned_only: only a
        buffer the sweep may write in place (not a gradient shared with another tensor) - for nodes that accumulate into it."""
        if self._pending is None or not switches.get("SG_GRAD_ACC"):
            return None
        cur = self._pending.get(id(sym))
        if cur is None or (owned_only and not cur[1]):
            return None
        del self._pending[id(sym)]
        return cur[0]

    def put_back(self, sym: KTensor, t):
        """Undo an owned take_pending the node could not use."""
        self._pending[id(sym)] = [t, True]

    def shared(self, t):
        return _Shared(t)

    def release(self):
        self.values.clear()
        self._saved.clear()
        self.bn_stats.clear()
        self._act_planes.clear()

    def forward(self, x, training: bool):
        m = self.model
        exp = m.inputs[0].shape[1:]
        if tuple(x.shape[1:]) != tuple(exp):
            raise ValueError(f"input shape {tuple(x.shape)} does not match the model's {(None,) + tuple(exp)}")
        x = x.contiguous()
        self.ensure_planes(x.shape[0], training)
        if m.compute_dtype == "bfloat16":  # activations are bf16 from the first layer on (sg_cast, round to nearest even)
            x = self.eng.cast(x, self.torch.bfloat16)
        self.values = {id(m.inputs[0]): x}
        self._act_planes.clear()   # (a step's activation planes: made in this sweep, read again by its filter gradients)
        if training:
            for n in m.nodes:
                xs = [self.values[id(t)] for t in n.inputs]
                self.values[id(n.output)] = n.forward(self, xs, training)
            return self._as_f32(self.values[id(m.outputs[0])])
        # inference: an activation is dropped as soon as its last consumer has run (the allocator - or the
        # hipGraph's private pool under capture - reuses the block), so peak memory is the live set, not the sum
        last_use = m._last_use()
        for i, n in enumerate(m.nodes):
            xs = [self.values[id(t)] for t in n.inputs]
            self.values[id(n.output)] = n.forward(self, xs, False)
            for t in n.inputs:
                if last_use.get(id(t)) == i:
                    self.values.pop(id(t), None)
            del xs
        return self._as_f32(self.values[id(m.outputs[0])])

    def _as_f32(self, y):
        """The model's output leaves the engine as fp32 (the softmax head already is; a bf16 output of a head-less graph
        is widened)."""
        return y if y.dtype == self.torch.float32 else self.eng.cast(y, self.torch.float32)

    def backward(self, dout):
        """Reverse sweep.  Gradients of a tensor with several consumers are summed with sg_add_n; a gradient
        handed out as `_Shared` (pass-through of an Add) is never written in place."""
        m = self.model
        yout = self.values.get(id(m.outputs[0]))
        if yout is not None and yout.dtype != dout.dtype:  # a head-less bf16 graph: the fp32 loss gradient enters in bf16
            dout = self.eng.cast(dout, yout.dtype)
        grads: Dict[int, list] = {id(m.outputs[0]): [dout, True]}
        e = self.eng
        hook = self.on_node_done
        for n in reversed(m.nodes):
            slot = grads.pop(id(n.output), None)
            if slot is None:  # output does not influence the loss
                if hook is not None:
                    if self.node_done_fires is None or self.node_done_fires(n.index):
                        e.join_side()
                    hook(n.index)
                continue
            dy = slot[0]
            if isinstance(dy, L.DeferredGrad) and not dy.taken_by(n):
                dy = dy.materialise(e)   # (this node does not evaluate it unexpanded: never with the graphs Model._fuse marks)
            xs = [self.values[id(t)] for t in n.inputs]
            y = self.values[id(n.output)]
            self._pending = grads
            dxs = n.backward(self, xs, y, dy)
            self._pending = None
            for sym, g in zip(n.inputs, dxs):
                if g is None or sym.node is None:
                    continue
                fresh = True
                if isinstance(g, _Shared):
                    g, fresh = g.t, False
                elif g is dy:
                    fresh = False
                cur = grads.get(id(sym))
                if cur is not None:   # a sum: of tensors (never reached by the graphs Model._fuse marks)
                    if isinstance(g, L.DeferredGrad):
                        g, fresh = g.materialise(e), True
                    if isinstance(cur[0], L.DeferredGrad):
                        cur[0], cur[1] = cur[0].materialise(e), True
                if cur is None:
                    grads[id(sym)] = [g, fresh]

                elif cur[1]:
                    e.add_n([cur[0], g], out=cur[0])
                elif fresh:
                    e.add_n([cur[0], g], out=g)
                    grads[id(sym)] = [g, True]
                else:
                    grads[id(sym)] = [e.add_n([cur[0], g]), True]
            # this node's saved state and output gradient are dead now
            self._saved.pop(id(n), None)
            if hook is not None:
                if self.node_done_fires is None or self.node_done_fires(n.index):
                    e.join_side()  # a bucket's all-reduce reads filter gradients the side stream may still be writing
                hook(n.index)  # data-parallel: launches the all-reduce of every gradient bucket now complete
        self._act_planes.clear()   # (the side stream's launches hold their own references)
        e.join_side()  # Adam, get_gradients() and the loss-scaling checks read the gradients on the main stream
