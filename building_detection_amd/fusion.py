"""The graph pass that decides which launches a model makes: peephole fusions that remove full-tensor passes.

Each rule is one function `rule(nodes, outs)` - the model's node list in topological order and the ids of its output tensors -
that sets marks on the nodes (declared with their defaults in layers.py, each naming its rule); the layers' forward / backward
read the marks, and where a fusion also depends on the runtime (storage type, launch geometry, a run-time switch) they ask
runtime._Runtime.bnb_on / bn_conv_on / up2_on.  Every fusion is exact, not an approximation.  `run` (Model._fuse) applies RULES
in order, once, at model construction; the three switches the rules read (SG_BN_ADD, SG_BN_SUMS, SG_BN_DEFER) are read there.

The order matters - a rule may read what an earlier one has marked:

   1 bias_and_stats     reads nothing
   2 up2_conv           reads nothing
   3 absorb_relu        reads nothing
   4 bn_add             reads fused_away, relu (3)
   5 bn_sums            reads fused_away (3); defer_add (4) must be unset
   6 bn_sums_via_add    reads fused_away, relu (3); bn_src / defer_add of the Add (4); sums_from, bnsum_src (5) must be unset
   7 bn_gather          reads fused_away, pre_relu (3)
   8 bn_conv            reads fused_away (3); up_src (2), defer_add (4) and defer_to (7) must be unset
   9 thin_grad          reads fused_away (3); up_src (2) must be unset
  10 scse_lowrank       reads bn_src (8) and up_src (2) of the sSE convolution: both must be unset
  11 bn_backward_in_pw  reads sums_from (5, 6)

What is not fused:

   - Dropout / SpatialDropout2D (layers._DropoutNode).  The rules match node types, and none names this one, so a dropout node
     simply ends a pattern: a convolution followed by Dropout -> BatchNormalization keeps its bias gradient and hands over no
     statistics, a BatchNormalization followed by Dropout is applied by its own pass.  The mask costs one element-wise launch in
     each direction (sg_dropout); applying it inside BatchNormalization's apply pass or a convolution's epilogue is not done.
"""
from . import layers as L
from . import switches


def sole_consumer(t, outs):
    """The single consumer of tensor `t`, reached through ReLU nodes that were absorbed (fused_away: they pass the tensor on
    unchanged); None when a tensor on the way has another consumer or is a model output."""
    while (len(t.consumers) == 1 and isinstance(t.consumers[0], L._ActNode) and t.consumers[0].fused_away
           and id(t.consumers[0].output) not in outs):
        t = t.consumers[0].output
    return t.consumers[0] if len(t.consumers) == 1 and id(t) not in outs else None


def root_of(t, path=None):
    """The mirror image: the tensor that `t` is an identity of, walking back through absorbed ReLU nodes whose output has one
    consumer.  Neither the root's own consumers nor the model's outputs are looked at: each caller states its condition on the
    root.  `path` (a list) receives the ReLU nodes passed, nearest first."""
    while isinstance(t.node, L._ActNode) and t.node.fused_away and len(t.consumers) == 1:
        if path is not None:
            path.append(t.node)
        t = t.node.inputs[0]
    return t


def _bn4(nodes, outs):
    """The BatchNormalization layers every BN -> consumer rule starts from: 4-D, not a model output."""
    return [n for n in nodes if isinstance(n, L._BNNode) and len(n.output.shape) == 4 and id(n.output) not in outs]


def bias_and_stats(nodes, outs):
    """A bias added right before a training-mode BatchNormalization has an identically zero gradient (BN's input
    gradient sums to zero over the batch by construction): the column-sum launch is dropped and the slot in the
    gradient arena stays at its initial 0 (what the sum would return up to fp32 noise of ~1e-10).  The same convolution's
    epilogue hands the BatchNormalization its statistics (stats of sg_conv2d_fwd)."""
    for n in nodes:
        if isinstance(n, (L._ConvNode, L._SepConvNode)) and n.activation in (None, "linear") and id(n.output) not in outs:
            cons = n.output.consumers
            if len(cons) == 1 and isinstance(cons[0], L._BNNode) and len(n.output.shape) == 4:
                n.bias_grad_zero = n.emit_bn_stats = True


def up2_conv(nodes, outs):
    """UpSampling2D(2) -> Conv2D 3x3 'same' (the decoder's last stage, train_model/DeepLabv3plus.py:476-477): the convolution's
    kernels read the up-sampling's source directly (sub-pixel forward with 4/9 of the products; csrc/conv_x6p.h) and the
    4x tensor and its gradient are never built.  Marked here for every such pair; whether a runtime takes the fused
    kernels (fp32 storage, geometry, SG_UP2_FUSE != 0) is _Runtime.up2_on."""
    for n in nodes:
        if (isinstance(n, L._UpNode) and n.size == 2 and n.interpolation == "nearest" and id(n.output) not in outs
                and len(n.output.consumers) == 1):
            c = n.output.consumers[0]
            if (isinstance(c, L._ConvNode) and c.k == 3 and c.stride == 1 and c.dilation == 1 and c.padding == "same"
                    and c.activation in (None, "linear", "relu")):
                n.fused_into, c.up_src = c, n


def absorb_relu(nodes, outs):
    """BN -> ReLU   => BN kernel applies ReLU (and masks in backward);
    GN -> ReLU   => the same through the GroupNormalization kernels' relu flag (the only rule that looks at that layer);
    Add -> ReLU  => add_n applies ReLU;
    ReLU -> SeparableConv2D => depthwise gather applies ReLU (pre_relu).
    A ReLU is absorbed only if its output has exactly one consumer (or, for producers, it is the only
    consumer of the producer's output and is not a model output)."""
    for n in nodes:
        if not isinstance(n, L._ActNode) or n.act != "relu" or n.fused_away:
            continue
        src = n.inputs[0]
        prod = src.node
        if (prod is not None and len(src.consumers) == 1 and id(src) not in outs
                and isinstance(prod, (L._BNNode, L._GNNode, L._AddNode)) and not prod.relu):
            prod.relu, n.fused_away = True, True
            continue
        cons = n.output.consumers
        if len(cons) == 1 and isinstance(cons[0], L._SepConvNode) and id(n.output) not in outs and not cons[0].pre_relu:
            cons[0].pre_relu, n.fused_away = True, True


def bn_add(nodes, outs):
    """BatchNormalization (no ReLU) -> two-operand Add: the residual adds of the Xception blocks sum a normalised branch and
    the shortcut (itself a normalised 1x1 convolution in the entry / exit flow).  The Add applies the normalisation while
    it sums (sg_add2_bn), the normalised tensor is never written or read: one of the layer's two forward passes
    (SG_BN_ADD=0 keeps them apart).  The backward is untouched: dy of the Add IS dy of the BatchNormalization, whose
    backward reads its raw input.
    (No test of defer_to: rule 7 assigns it after this one, and the two exclude each other anyway - the only consumer of the
    layer's output is this Add, not a SeparableConv2D.)"""
    if not switches.get("SG_BN_ADD"):
        return
    for n in nodes:
        if not isinstance(n, L._AddNode) or len(n.inputs) != 2 or len(n.output.shape) != 4:
            continue
        epss = set()
        for i, t in enumerate(n.inputs):
            p_ = t.node
            through_relu = False   # BN -> ReLU (absorbed into the BN) -> Add: the Add applies both (res34.py's blocks)
            if (isinstance(p_, L._ActNode) and p_.fused_away and len(t.consumers) == 1 and id(t) not in outs
                    and isinstance(p_.inputs[0].node, L._BNNode) and p_.inputs[0].node.relu
                    and len(p_.inputs[0].consumers) == 1):
                t, p_, through_relu = p_.inputs[0], p_.inputs[0].node, True
            if (isinstance(p_, L._BNNode) and p_.relu == through_relu and p_.defer_add is None
                    and len(t.consumers) == 1 and id(t) not in outs and t.shape[-1] % 4 == 0
                    and n.inputs[0] is not n.inputs[1]):
                n.bn_src[i], p_.defer_add = p_, n
                epss.add(p_.epsilon)
        if len(epss) > 1:   # (one eps per launch: two different ones never occur on this path)
            for i, p_ in enumerate(n.bn_src):
                if p_ is not None:
                    p_.defer_add, n.bn_src[i] = None, None


def bn_sums(nodes, outs):
    """BatchNormalization (+ fused ReLU) -> SeparableConv2D (stride 1), the layer's only consumer: the input gradient that the
    depthwise convolution's dgrad writes IS the BatchNormalization's output gradient.  That kernel also sums, per channel,
    dbeta = sum g and dgamma = sum g * xhat in its epilogue (sums of sg_dwconv2d_dgrad: one more read of the layer's raw
    input), so the reduction pass of the BatchNormalization's backward - two tensor reads of its five passes - is not run
    (round 4; conv_bn_relu / the Xception blocks, train_model/DeepLabv3plus.py:323-416,424-429; SG_BN_SUMS=0 switches it
    off).  Decided again at run time (geometry, training mode: _SepConvNode.backward)."""
    if not switches.get("SG_BN_SUMS"):
        return
    for n in _bn4(nodes, outs):
        sc = sole_consumer(n.output, outs)
        _, h, w, c = n.output.shape
        if (n.defer_add is None and isinstance(sc, L._SepConvNode) and sc.stride == 1 and sc.bnsum_src is None
                and w % 4 == 0 and c % 4 == 0):
            n.sums_from, sc.bnsum_src = sc, n


def bn_sums_via_add(nodes, outs):
    """The same through a residual Add that applies the layer (defer_add): the Add hands its output gradient on unchanged,
    so a BatchNormalization in front of it receives the gradient of the Add's OUTPUT - and where that output opens the
    next Xception block, its complete gradient leaves the depthwise dgrad of the block's first SeparableConv2D (which
    adds the gradient collected from the block's own residual add: take_pending).  Condition: that SeparableConv2D
    (with the ReLU absorbed into its gather) is the LAST consumer of the tensor in the backward sweep, i.e. the first
    in node order."""
    if not switches.get("SG_BN_SUMS"):
        return
    for sc in nodes:
        if not isinstance(sc, L._SepConvNode) or sc.bnsum_src is not None or sc.stride != 1:
            continue
        path = []
        root = root_of(sc.inputs[0], path)
        first = path[-1] if path else sc   # the consumer of `root` that leads to sc
        a = root.node
        if not isinstance(a, L._AddNode) or a.relu or id(root) in outs or len(root.shape) != 4:
            continue
        if any(cn is not first and cn.index < sc.index for cn in root.consumers):
            continue
        cands = [b for b in a.bn_src if b is not None and b.sums_from is None and b.defer_add is a]
        _, h, w, c = root.shape
        if cands and w % 4 == 0 and c % 4 == 0:
            cands[0].sums_from, sc.bnsum_src = sc, cands[0]


def bn_gather(nodes, outs):
    """BatchNormalization (+ fused ReLU) -> SeparableConv2D, training mode: the depthwise gather applies the normalisation
    to the raw tensor (bn of sg_dwconv2d_fwd / _wgrad), so the normalised tensor is never written or read - two of the
    layer's seven tensor passes.  Needs the statistics from the producing convolution's epilogue (decided at run
    time: _BNNode.forward falls back to the materialising form) and the stride-1 run kernels' geometry.
    Default ON since round 4 (SG_BN_DEFER=0 restores the materialising form; tests/test_models_gpu.py keeps one leg on it).
    Round 2 measured "no net gain" (the 39 dropped bn_apply launches saved 1.05 ms and the depthwise kernels of that
    round gave 0.8 ms of it back); re-measured on the round-3 run kernels: 76.59 -> 75.71 and 76.96 -> 75.93 ms per fp32
    step, bit-identical, peak memory -2.7 GiB (LAB_NOTEBOOK.md 11.2)."""
    if not switches.get("SG_BN_DEFER"):
        return
    for n in _bn4(nodes, outs):
        sc = sole_consumer(n.output, outs)
        _, h, w, c = n.output.shape
        if (isinstance(sc, L._SepConvNode) and sc.stride == 1 and not sc.pre_relu and sc.bn_src is None
                and w % 4 == 0 and c % 4 == 0):
            n.defer_to, sc.bn_src = sc, n


def bn_conv(nodes, outs):
    """BatchNormalization(+ReLU) -> Conv2D whose kernels can normalise while they load (round 5): a thin 1x1 convolution (the
    softmax head, the sSE gate) or a 3x3 stride-1 convolution on 32 / 64 channels (the patch kernels).  The decoder's last stage
    `conv_bn_relu(32) -> conv_bn_relu(32) -> Conv2D(2, softmax)` (train_model/DeepLabv3plus.py:477-480) has two such pairs on
    512 x 512 x 32 tensors.  The normalised tensor is then never written or read (forward: one write + one read of the
    tensor; the filter gradient re-normalises in its loader; backward of the BatchNormalization is unchanged - it already
    recomputes the ReLU mask from its raw input).  Whether a runtime takes it is _Runtime.bn_conv_on."""
    for n in _bn4(nodes, outs):
        c = sole_consumer(n.output, outs)
        if (n.defer_to is not None or n.defer_add is not None or not isinstance(c, L._ConvNode) or c.bn_src is not None
                or c.up_src is not None or c.stride != 1 or c.dilation != 1):
            continue
        cin = n.output.shape[-1]
        thin = c.k == 1 and c.filters <= 4 and cin % 4 == 0 and cin >= 16
        patch = c.k == 3 and c.padding == "same" and cin in (32, 64)
        if thin or patch:
            n.defer_conv, c.bn_src = c, n


def thin_grad(nodes, outs):
    """BatchNormalization (+ fused ReLU) -> thin 1x1 Conv2D (Cout <= 4: the softmax head), the layer's only consumer: the
    convolution's input gradient stays unexpanded and the BatchNormalization's backward evaluates it (layers.ThinGradDeferred;
    decided again at run time: storage type, SG_THIN_GRAD_BN)"""
    for n in _bn4(nodes, outs):
        c = sole_consumer(n.output, outs)
        cin = n.output.shape[-1]
        if (isinstance(c, L._ConvNode) and c.k == 1 and c.stride == 1 and c.filters <= 4 and c.up_src is None
                and cin % 4 == 0 and cin >= 16):
            c.thin_bn = n


def scse_lowrank(nodes, outs):
    """scSE block: x feeds the sSE convolution (1x1, one output channel, on the thin kernel's geometry), the GlobalAveragePooling of
    the cSE path and the combine node, and nothing else.  The two gates' input gradients are rank-one terms; the combine node's
    backward leaves the block's dx to one final kernel that adds them (layers.ScseGradDeferred; SG_SCSE_LOWRANK at run time)."""
    for n in nodes:
        if not isinstance(n, L._ScseCombineNode):
            continue
        x, s = n.inputs[0], n.inputs[1]
        sse, cons = s.node, x.consumers
        gaps = [q for q in cons if isinstance(q, L._AvgPoolNode) and q.global_pool]
        if (isinstance(sse, L._ConvNode) and len(cons) == 3 and len(gaps) == 1 and sse in cons and n in cons and id(x) not in outs
                and x.node is not None and sse.inputs[0] is x and sse.k == 1 and sse.stride == 1 and sse.filters == 1
                and sse.activation is None and sse.bn_src is None and sse.up_src is None and len(s.consumers) == 1
                and x.shape[-1] % 4 == 0 and x.shape[-1] >= 16):
            n.lowrank = (sse, gaps[0])


def bn_backward_in_pw(nodes, outs):
    """SeparableConv2D -> BatchNormalization whose backward column sums come from elsewhere (sums_from): the backward APPLY can
    ride in the A path of the pointwise dgrad (csrc/conv_pw.h, BNB form; _Runtime.bnb_on decides per runtime and batch)"""
    for n in nodes:
        if isinstance(n, L._BNNode) and n.sums_from is not None and len(n.output.shape) == 4:
            prod = n.inputs[0].node
            if (isinstance(prod, L._SepConvNode) and prod.activation in (None, "linear") and len(n.inputs[0].consumers) == 1
                    and id(n.inputs[0]) not in outs):
                n.bnb_to = prod


RULES = (bias_and_stats, up2_conv, absorb_relu, bn_add, bn_sums, bn_sums_via_add, bn_gather, bn_conv, thin_grad, scse_lowrank,
         bn_backward_in_pw)


def run(nodes, outputs):
    outs = {id(t) for t in outputs}
    for rule in RULES:
        rule(nodes, outs)
