"""Optimizers with tf.keras (2.11+) argument names: Adam, AdamW, SGD, and `get` for compile(optimizer=...).

A default-constructed Adam() is the reference's compile(optimizer='adam'): it takes the plain sg_adam_step call on the flat
arena, for the same bits.  Any option - amsgrad, weight decay, a clip mode, the weight average, SGD - takes the two table-driven
kernels of csrc/optim.hip: sg_optim_grad_norms (only with clipnorm / global_clipnorm) and one fused sg_optim_step.

The update rules, with g the gradient after grad_scale (1 / world under data parallelism), lr the learning rate the callbacks
set and t the step count after increment:
  clipvalue c        g = clamp(g, -c, c)
  clipnorm c         per parameter, g *= c / max(||g_p||, c)
  global_clipnorm c  the same with the norm over all trainable parameters
                     (padding between parameters never contributes; a non-finite norm gets no special case: an infinite norm
                     scales g by 0, so infinite gradients become NaN, and max(NaN, c) = c on the device leaves g unscaled: NaN
                     gradients reach the weights either way, as they do without clipping)
  weight decay       decoupled, before the update: w -= lr * weight_decay * w, on decayed parameters only
  Adam               m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; lr_t = lr sqrt(1-b2^t) / (1-b1^t);
                     w -= lr_t m / (sqrt(v) + eps); with amsgrad vhat = max(vhat, v) takes v's place in the quotient
  SGD                momentum == 0: w -= lr g (no moment arena is read); else m = momentum m - lr g, then w += m, or with
                     nesterov w += momentum m - lr g
  use_ema            after the update: avg = ema_momentum avg + (1 - ema_momentum) w; avg starts as a copy of the weights when
                     the optimizer's state is created (the first step)

A DIFFERENCE FROM KERAS, on purpose: weight decay applies by default only to parameters of kind kernel / depthwise_kernel /
pointwise_kernel - not to BatchNormalization's gamma / beta nor to biases, which Keras decays unless the caller excludes them by
name.  `decay_kinds=None` decays every trainable parameter; exclude_from_weight_decay(var_names=[...]) excludes by substring of
the parameter's name, as in Keras.
"""
from __future__ import annotations

import contextlib
import math

import numpy as np

from . import _lib
from .runtime import Optimizer

CHUNK = 4096    # elements: the longest run of one parameter that one workgroup trip of csrc/optim.hip takes (measured there)
ALIGN = 4       # elements: every parameter of the arena starts on a 16-byte boundary (graph.ALIGN)
DEFAULT_DECAY_KINDS = ("kernel", "depthwise_kernel", "pointwise_kernel")

CHUNK_DTYPE = np.dtype([("start", "<i8"), ("length", "<i4"), ("segment", "<i4")])
SEG_DTYPE = np.dtype([("chunk_begin", "<i4"), ("chunk_end", "<i4"), ("flags", "<i4"), ("reserved", "<i4")])


def chunk_table(params, chunk=CHUNK, decay_kinds=DEFAULT_DECAY_KINDS, exclude=()):
    """The table both optimizer kernels walk, from a model's parameter list (objects with .trainable, .offset, .size, .kind,
    .name; Model.params).  Pure host code.  Returns (chunks, segs, trainable): numpy arrays of CHUNK_DTYPE / SEG_DTYPE (the
    layouts of sg_optim_chunk / sg_optim_seg) and the trainable parameters, segment s = trainable[s].
      * every chunk is (start, length, segment) with start % 4 == 0, 1 <= length <= chunk, wholly inside parameter `segment`;
      * the chunks cover every trainable element exactly once, in arena order, and no padding element;
      * segs[s] = its chunks [chunk_begin, chunk_end) and flags: SG_OPT_SEG_DECAY iff the parameter's kind is in decay_kinds
        (None: every kind) and none of `exclude` is a substring of its name."""
    if chunk < ALIGN or chunk % ALIGN:
        raise ValueError(f"chunk={chunk}: a positive multiple of {ALIGN}")
    trainable = sorted((p for p in params if p.trainable), key=lambda p: p.offset)
    chunks, segs, end = [], [], 0
    for s, p in enumerate(trainable):
        if p.offset % ALIGN or p.offset < end or p.size <= 0:
            raise ValueError(f"{p.name}: offset {p.offset}, size {p.size} behind element {end}: not an arena layout")
        end = p.offset + p.size
        first = len(chunks)
        for o in range(0, p.size, chunk):
            chunks.append((p.offset + o, min(chunk, p.size - o), s))
        decayed = (decay_kinds is None or p.kind in decay_kinds) and not any(x in p.name for x in exclude)
        segs.append((first, len(chunks), _lib.SG_OPT_SEG_DECAY if decayed else 0, 0))
    return np.array(chunks, dtype=CHUNK_DTYPE), np.array(segs, dtype=SEG_DTYPE), trainable


def _hyper(name, v, allow_none=False, positive=False, upper=None):
    if v is None and allow_none:
        return None
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{name}={v!r}: a number is expected") from None
    if not math.isfinite(f) or f < 0 or (positive and f == 0) or (upper is not None and f > upper):
        raise ValueError(f"{name}={v!r}: negative, non-finite or out of range")
    return f


class _TableOptimizer(Optimizer):
    """What Adam and SGD share: decay / clip / EMA arguments, the per-runtime state and the launch."""

    kind = _lib.SG_OPT_ADAM

    def _init_common(self, weight_decay, clipnorm, clipvalue, global_clipnorm, use_ema, ema_momentum, decay_kinds):
        self.weight_decay = _hyper("weight_decay", weight_decay, allow_none=True)
        self.clipnorm = _hyper("clipnorm", clipnorm, allow_none=True, positive=True)
        self.clipvalue = _hyper("clipvalue", clipvalue, allow_none=True, positive=True)
        self.global_clipnorm = _hyper("global_clipnorm", global_clipnorm, allow_none=True, positive=True)
        if sum(c is not None for c in (self.clipnorm, self.clipvalue, self.global_clipnorm)) > 1:
            raise ValueError("at most one of clipnorm, clipvalue and global_clipnorm may be set")
        self.use_ema = bool(use_ema)
        self.ema_momentum = _hyper("ema_momentum", ema_momentum, upper=1.0)
        self.decay_kinds = None if decay_kinds is None else tuple(decay_kinds)
        self._exclude = ()
        self._state = None   # (runtime, _State): tables and arenas live with ONE model's runtime

    def exclude_from_weight_decay(self, var_list=None, var_names=None):
        """Keras's name: parameters whose name contains one of `var_names` (or that are in `var_list`) are not decayed.  Call
        it before the first step."""
        if self._state is not None:
            raise ValueError("exclude_from_weight_decay() must be called before the optimizer has taken a step")
        self._exclude = tuple(var_names or ()) + tuple(p.name for p in (var_list or ()))

    # -- what the kernel is told ------------------------------------------------------------------------------------------
    def _clip(self):
        for mode, c in ((_lib.SG_OPT_CLIP_VALUE, self.clipvalue), (_lib.SG_OPT_CLIP_NORM, self.clipnorm),
                        (_lib.SG_OPT_CLIP_GLOBAL, self.global_clipnorm)):
            if c is not None:
                return mode, c
        return _lib.SG_OPT_CLIP_NONE, 0.0

    def _flags(self):
        return _lib.SG_OPT_EMA if self.use_ema else 0

    def _plain(self):
        return False

    def descriptor(self, grad_scale=1.0):
        mode, c = self._clip()
        return _lib.OptimDesc(self.kind, self._flags(), mode, self.beta_1, self.beta_2, self.epsilon,
                              getattr(self, "momentum", 0.0), self.weight_decay or 0.0, c, self.ema_momentum, float(grad_scale))

    # -- state ----------------------------------------------------------------------------------------------------------------
    def prepare(self, rt):
        """Build the chunk table and allocate the arenas this configuration adds (vhat, the weight average), once per model
        runtime and never inside a stream capture: GraphedTrainStep calls it before it starts capturing."""
        if self._plain():
            return None
        if self._state is not None and self._state[0] is rt:
            return self._state[1]
        if self._state is not None:
            raise ValueError("this optimizer holds the state of another model: construct one optimizer per model")
        chunks, segs, _ = chunk_table(rt.model.params, CHUNK, self.decay_kinds, self._exclude)
        st = _State()
        st.table = rt.eng.optim_table(chunks, segs, rt.w_train.numel()) if len(chunks) else None
        st.vhat = rt.eng.zeros(rt.w_train.numel()) if getattr(self, "amsgrad", False) else None
        st.ema = rt.w_train.clone() if self.use_ema else None
        self._state = (rt, st)
        return st

    def apply(self, rt, eng, grad_scale=1.0, lr_dev=None):
        if self._plain():
            return Optimizer.apply(self, rt, eng, grad_scale, lr_dev)
        st = self.prepare(rt)
        if st.table is None:   # nothing trainable
            return
        mode, _ = self._clip()
        if mode in (_lib.SG_OPT_CLIP_NORM, _lib.SG_OPT_CLIP_GLOBAL):
            eng.optim_grad_norms(st.table, rt.g_train, grad_scale)
        lr_t, lr = (0.0, 0.0) if lr_dev is not None else self.step_scalars()
        adam = self.kind == _lib.SG_OPT_ADAM
        m = rt.adam_m if adam or getattr(self, "momentum", 0.0) != 0.0 else None   # SGD's momentum lives in the m arena
        eng.optim_step(self.descriptor(grad_scale), st.table, rt.w_train, rt.g_train, m, rt.adam_v if adam else None, st.vhat,
                       st.ema, lr_t, lr, lr_dev)

    # -- the weight average ---------------------------------------------------------------------------------------------------
    def _average(self, model):
        if not self.use_ema:
            raise ValueError("this optimizer keeps no weight average: construct it with use_ema=True")
        return self.prepare(model._runtime()).ema

    def finalize_variable_values(self, model):
        """Keras's name: overwrite the model's trainable weights with their moving average (a no-op without use_ema)."""
        if not self.use_ema:
            return
        rt = model._runtime()
        rt.w_train.copy_(self._average(model))
        rt.weights_changed()


class _State:
    table = vhat = ema = None


class Adam(_TableOptimizer):
    kind = _lib.SG_OPT_ADAM

    def __init__(self, learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False, weight_decay=None,
                 clipnorm=None, clipvalue=None, global_clipnorm=None, use_ema=False, ema_momentum=0.99, lr=None,
                 decay_kinds=DEFAULT_DECAY_KINDS, name=None, **kw):
        if kw:
            raise TypeError(f"{type(self).__name__}: unexpected arguments {sorted(kw)}")
        Optimizer.__init__(self, _hyper("learning_rate", learning_rate if lr is None else lr), _hyper("beta_1", beta_1, upper=1.0),
                           _hyper("beta_2", beta_2, upper=1.0), _hyper("epsilon", epsilon))
        self.amsgrad = bool(amsgrad)
        self.name = name or type(self).__name__
        self._init_common(weight_decay, clipnorm, clipvalue, global_clipnorm, use_ema, ema_momentum, decay_kinds)

    def _flags(self):
        return _TableOptimizer._flags(self) | (_lib.SG_OPT_AMSGRAD if self.amsgrad else 0)

    def _plain(self):
        """No option set: the reference's Adam, which keeps its own kernel and its bits."""
        return not (self.amsgrad or self.weight_decay or self.use_ema or self._clip()[0])


class AdamW(Adam):
    def __init__(self, learning_rate=1e-3, weight_decay=0.004, **kw):
        Adam.__init__(self, learning_rate=learning_rate, weight_decay=weight_decay, **kw)


class SGD(_TableOptimizer):
    kind = _lib.SG_OPT_SGD

    def __init__(self, learning_rate=0.01, momentum=0.0, nesterov=False, weight_decay=None, clipnorm=None, clipvalue=None,
                 global_clipnorm=None, use_ema=False, ema_momentum=0.99, lr=None, decay_kinds=DEFAULT_DECAY_KINDS, name=None,
                 **kw):
        if kw:
            raise TypeError(f"SGD: unexpected arguments {sorted(kw)}")
        Optimizer.__init__(self, _hyper("learning_rate", learning_rate if lr is None else lr))
        self.momentum = _hyper("momentum", momentum, upper=1.0)
        self.nesterov = bool(nesterov)
        self.name = name or "SGD"
        self._init_common(weight_decay, clipnorm, clipvalue, global_clipnorm, use_ema, ema_momentum, decay_kinds)

    def _flags(self):
        return _TableOptimizer._flags(self) | (_lib.SG_OPT_NESTEROV if self.nesterov and self.momentum != 0.0 else 0)

    def step_scalars(self):
        lr = float(self.lr)
        return lr, lr


_BY_NAME = {"adam": Adam, "adamw": AdamW, "sgd": SGD}


def get(identifier):
    """'adam' | 'adamw' | 'sgd' (any case) -> a default-constructed optimizer; an optimizer instance is returned as it is."""
    if isinstance(identifier, Optimizer):
        return identifier
    if isinstance(identifier, str):
        cls = _BY_NAME.get(identifier.lower())
        if cls is not None:
            return cls()
    raise ValueError(f"optimizer={identifier!r}: expected one of 'adam' (the reference's, DeepLabv3plus.py:835), 'adamw', 'sgd' "
                     "or an optimizer instance")


@contextlib.contextmanager
def ema_weights(model):
    """Model.ema_weights(): inside the block the trainable weights are their moving average (predict, test_on_batch,
    save_weights read it); on exit the training weights are back, to the bit."""
    opt = model.optimizer
    if not isinstance(opt, _TableOptimizer):
        raise ValueError("compile the model with an optimizer constructed with use_ema=True")
    rt = model._runtime()
    avg = opt._average(model)
    with rt.eng.lock:
        keep = rt.w_train.clone()
        rt.w_train.copy_(avg)
        rt.weights_changed()
    try:
        yield model
    finally:
        with rt.eng.lock:
            rt.w_train.copy_(keep)
            rt.weights_changed()
