"""The ConvNet's scene-segmentation head (tensorflow/models/heads/seg_head.py:31-102) over a five-layer pyramid: four decoder steps — nearest upsample to the
finer layer, concatenation with the encoder's features of that layer, conv1d_1x1 — each ONE unary.up_conv call (cbl_up_conv_*: neither the upsampled nor the
concatenated tensor exists), then segmentation_head and segmentation_pred (unary.conv1d_1x1).  There is no fallback: CPU tensors raise."""
import torch

from .unary import Conv1d1x1, UpConv1d1x1

SCOPE = "resnet_scene_segmentation_head"
NUM_LAYERS = 5                                                       # seg_head.py upsamples layers 4, 3, 2, 1: F holds five stages


class ResnetSceneSegmentationHead(torch.nn.Module):
    """resnet_scene_segmentation_head(config, inputs, F, base_fdim, ...).  F[i] (n_i, 2^(i+1) * base_fdim): the backbone's stage features, F[0] the finest;
    inputs['upsamples'][i] (n_{i-1}, max_num) int32: per point of layer i - 1 its nearest points of layer i (column 0 is read).  Layers, in the reference's
    names: up_conv0 .. up_conv3 (to 8, 4, 2, 1 x base_fdim; upsample tables 4, 3, 2, 1), segmentation_head (base_fdim) and segmentation_pred (num_classes,
    with a bias, no batch norm, no activation).  sep_head / arch_up (config.sep_head, config.arch_up): the decoder alone."""

    def __init__(self, base_fdim, num_classes, sep_head=False, arch_up=False, init="xavier", activation_fn="relu", bn=True, bn_momentum=0.98, bn_eps=1e-3):
        super().__init__()
        self.base_fdim, self.num_classes, self.decoder_only = base_fdim, num_classes, bool(sep_head or arch_up)
        kw = dict(init=init, activation_fn=activation_fn, bn=bn, bn_momentum=bn_momentum, bn_eps=bn_eps)
        for step in range(NUM_LAYERS - 1):                           # step s: F of layer 4 - s (or the step before) up to layer 3 - s
            out = 2 ** (3 - step) * base_fdim
            c_up = 32 * base_fdim if step == 0 else 2 * out          # F[4], then the previous step's output
            c_skip = 2 * out                                         # F[3 - step]
            setattr(self, "up_conv%d" % step, UpConv1d1x1(c_up, c_skip, out, scope="%s/up_conv%d" % (SCOPE, step), **kw))
        if not self.decoder_only:
            self.segmentation_head = Conv1d1x1(base_fdim, base_fdim, scope=SCOPE + "/segmentation_head", **kw)
            self.segmentation_pred = Conv1d1x1(base_fdim, num_classes, with_bias=True, init=init, activation_fn=None, bn=False, scope=SCOPE + "/segmentation_pred")

    def tf_scopes(self):
        """state_dict name -> the TF variable scope of the variable, everything under resnet_scene_segmentation_head/ (seg_head.py:59)"""
        return {"%s.%s" % (layer, name): scope for layer, module in self.named_children() for name, scope in module.tf_scopes().items()}

    def forward(self, inputs, F):
        """-> (F_up, (features, logits)), or (F_up, None) under sep_head / arch_up.  F_up: the four decoder outputs, finest first (seg_head.py:91)"""
        upsamples = inputs["upsamples"]
        if len(F) != NUM_LAYERS or len(upsamples) < NUM_LAYERS:
            raise NotImplementedError("ResnetSceneSegmentationHead: {} stages and {} upsample tables ({} layers expected)".format(len(F), len(upsamples), NUM_LAYERS))
        features, F_up = F[-1], []
        for step in range(NUM_LAYERS - 1):
            features = getattr(self, "up_conv%d" % step)(features, upsamples[NUM_LAYERS - 1 - step], F[NUM_LAYERS - 2 - step])
            F_up.append(features)
        F_up = list(reversed(F_up))
        if self.decoder_only:
            return F_up, None
        features = self.segmentation_head(features)
        return F_up, (features, self.segmentation_pred(features))
