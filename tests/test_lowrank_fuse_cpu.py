"""Model._fuse marks the graphs whose low-rank gradients stay unexpanded (host only: graph construction needs no GPU)."""


def _marks(m):
    from building_detection_amd import layers as L
    heads = [n for n in m.nodes if isinstance(n, L._ConvNode) and n.thin_bn is not None]
    blocks = [n for n in m.nodes if isinstance(n, L._ScseCombineNode) and n.lowrank is not None]
    return heads, blocks


def test_deeplab_marks_the_head_pair_and_its_four_scse_blocks():
    from building_detection_amd import zoo
    from building_detection_amd import layers as L
    m = zoo.Xception_DeepLabV3_Plus((64, 64, 3), 2, aspp_pool=4)
    heads, blocks = _marks(m)
    assert len(heads) == 1 and heads[0].activation == "softmax" and heads[0] is m.outputs[0].node
    bn = heads[0].thin_bn
    assert isinstance(bn, L._BNNode) and bn.relu and bn.defer_conv is heads[0]
    assert len(blocks) == 4 == sum(1 for n in m.nodes if isinstance(n, L._ScseCombineNode))
    for n in blocks:
        sse, gap = n.lowrank
        x = n.inputs[0]
        assert sse.filters == 1 and sse.inputs[0] is x and gap.global_pool and gap.inputs[0] is x
        assert sorted(q.index for q in x.consumers) == sorted((sse.index, gap.index, n.index))
        assert sse.thin_bn is None   # its input has other consumers: never handed to a BatchNormalization


def test_hrnet_has_no_scse_block_to_mark_and_its_head_pair_is_the_only_mark():
    """HRNet has no scSE block, so none is marked.  Its last stage is conv -> BatchNormalization -> ReLU -> Conv2D(2, softmax): a
    BatchNormalization directly in front of a thin convolution whose input has no other consumer, which is the pair the rule names
    wherever it occurs - that one head is marked, and no other convolution of the model is."""
    from building_detection_amd import zoo
    m = zoo.HRNet((64, 64, 3))
    heads, blocks = _marks(m)
    assert blocks == []
    assert len(heads) == 1 and heads[0] is m.outputs[0].node and heads[0].thin_bn.defer_conv is heads[0]


def test_scse_unet_marks_its_four_blocks_and_no_head():
    from building_detection_amd import zoo
    heads, blocks = _marks(zoo.UNet(2, (64, 64, 3)))
    assert heads == [] and len(blocks) == 4
