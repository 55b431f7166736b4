"""DeepLabv3 / DeepLabv3+ decoders and the auxiliary head (reference: u2pl/models/decoder.py), a pyramid-pooling decoder
(dec_pspnet), an object-contextual one (dec_ocrnet), a criss-cross attention one (dec_ccnet) and a dense (non-local) attention one
(dec_nonlocal).  nn.Sequential containers keep the reference's indices (``classifier.8.weight``); ReLU / Dropout2d entries are markers fused into the BatchNorm apply kernel by
u2pl_amd.nn.run_seq."""
import torch
import torch.nn as nn

from .. import nn as K
from .base import ASPP, norm_layer_for, separable_conv3x3


def _conv3x3_unit(in_planes, out_planes, norm_layer, separable, bias):
    """dense 3x3 (stride 1, padding 1) -> norm -> ReLU -> Dropout2d(0.1) as the reference builds it, or its separable form
    (decoder.kwargs.separable)"""
    tail = (nn.Dropout2d(0.1),)
    if separable:
        return separable_conv3x3(in_planes, out_planes, norm_layer, bias=bias, tail=tail)
    return [K.Conv2d(in_planes, out_planes, kernel_size=3, stride=1, padding=1, dilation=1, bias=bias),
            norm_layer(out_planes), nn.ReLU(inplace=True), *tail]


# ---- what the heads below share.  A head registers its submodules in one fixed order: every layer draws its initial values from
# the generator as it is constructed, ParamArena lays parameters out in registration order and checkpoints are keyed by the names,
# so a moved line is another model (tests/test_decoder_layout_cpu.py holds the order and the seeded values) -------------------------
def _unit3x3(cin, cout, norm_layer, *tail):
    """dense 3x3 (stride 1, padding 1, no bias) -> norm -> ReLU [-> tail]"""
    return nn.Sequential(K.Conv2d(cin, cout, kernel_size=3, stride=1, padding=1, dilation=1, bias=False), norm_layer(cout),
                         nn.ReLU(inplace=True), *tail)


def _rep_tower(inner_planes, norm_layer):
    """the `representation` tower beside a classifier, for the contrastive loss: 3x3 to 256 -> norm -> ReLU -> Dropout2d(0.1) ->
    1x1 to 256 with bias"""
    return nn.Sequential(*_unit3x3(inner_planes, 256, norm_layer, nn.Dropout2d(0.1)),
                         K.Conv2d(256, 256, kernel_size=1, stride=1, padding=0, bias=True))


def _last_map(x):
    """the encoder's four maps (fpn: true): the head reads the last"""
    return x[-1] if isinstance(x, (list, tuple)) else x


def _outputs(dec, feat, need_rep, **extra):
    """{"pred": classifier(feat), **extra[, "rep": representation(feat)]} of a head whose classifier is one convolution"""
    res = {"pred": dec.classifier(feat), **extra}
    if dec.rep_head and need_rep:
        res["rep"] = K.run_seq(dec.representation, feat)
    return res


def _check_planes(who, **planes):
    for name, val in planes.items():
        if int(val) < 4 or int(val) % 4:
            raise ValueError("%s: %s (%r) must be a positive multiple of 4 (float4 rows)" % (who, name, val))


def _check_num_classes(who, num_classes):
    if not 2 <= int(num_classes) <= K.REGION_MAX_K:
        raise ValueError("%s: 2 <= num_classes <= %d (what the loss path takes), got %r" % (who, K.REGION_MAX_K, num_classes))


class dec_deeplabv3(nn.Module):
    def __init__(self, in_planes, num_classes=19, inner_planes=256, sync_bn=False, dilations=(12, 24, 36), separable=False):
        super().__init__()
        norm_layer = norm_layer_for(sync_bn)
        self.aspp = ASPP(in_planes, inner_planes=inner_planes, sync_bn=sync_bn, dilations=dilations, separable=separable)
        self.head = nn.Sequential(
            *_conv3x3_unit(self.aspp.get_outplanes(), 256, norm_layer, separable, bias=False),
            K.Conv2d(256, num_classes, kernel_size=1, stride=1, padding=0, bias=True),
        )

    def forward(self, x):
        return K.run_seq(self.head, self.aspp(x))


class dec_deeplabv3_plus(nn.Module):
    def __init__(self, in_planes, num_classes=19, inner_planes=256, sync_bn=False, dilations=(12, 24, 36),
                 rep_head=True, separable=False):
        super().__init__()
        norm_layer = norm_layer_for(sync_bn)
        self.rep_head = rep_head
        self.low_conv = nn.Sequential(K.Conv2d(256, 256, kernel_size=1), norm_layer(256), nn.ReLU(inplace=True))
        self.aspp = ASPP(in_planes, inner_planes=inner_planes, sync_bn=sync_bn, dilations=dilations, separable=separable)
        self.head = nn.Sequential(
            *_conv3x3_unit(self.aspp.get_outplanes(), 256, norm_layer, separable, bias=False))

        def tower(out_planes):
            return nn.Sequential(
                *_conv3x3_unit(512, 256, norm_layer, separable, bias=True),
                *_conv3x3_unit(256, 256, norm_layer, separable, bias=True),
                K.Conv2d(256, out_planes, kernel_size=1, stride=1, padding=0, bias=True),
            )

        self.classifier = tower(num_classes)
        if self.rep_head:
            self.representation = tower(256)

    def forward(self, x, need_rep=True):
        x1, x2, x3, x4 = x
        aspp_out = self.aspp(x4)
        low_feat = K.run_seq(self.low_conv, x1)
        aspp_out = K.run_seq(self.head, aspp_out)
        h, w = low_feat.size()[-2:]
        aspp_out = K.upsample_bilinear(aspp_out, (h, w))
        aspp_out = K.cat_channels((low_feat, aspp_out))
        # (no nn.GradJoin over the two towers: a caller may back-propagate through "pred" only -- the reference's supervised loop
        # does -- and a join needs every wired consumer's backward to run)
        res = {"pred": K.run_seq(self.classifier, aspp_out)}
        if self.rep_head and need_rep:
            res["rep"] = K.run_seq(self.representation, aspp_out)
        return res


class dec_pspnet(nn.Module):
    """Pyramid-pooling head (PSPNet, Zhao et al. 2017, section 3.2; no reference line: the reference has the two ASPP heads only).
    ppm.{i}: AdaptiveAvgPool2d(bins[i]) -> 1x1 (in_planes / len(bins), no bias) -> norm -> ReLU, up-sampled to the input's size
    (bilinear, align_corners=True) and concatenated behind the input; head: dense 3x3 from 2 in_planes to inner_planes -> norm
    -> ReLU -> Dropout2d(0.1); classifier: 1x1 with bias.  rep_head: a `representation` tower (_rep_tower) beside the classifier,
    on the head's output.
    All levels are pooled by one launch and the input's gradient is written by one gather (K.pyramid_pool)."""

    def __init__(self, in_planes, num_classes=19, inner_planes=512, sync_bn=False, bins=(1, 2, 3, 6), rep_head=False):
        super().__init__()
        bins = K.check_pyramid_bins(bins)
        if in_planes % (4 * len(bins)):
            raise ValueError("dec_pspnet: in_planes (%d) must be a multiple of 4 * len(bins) = %d (float4 rows in every "
                             "branch)" % (in_planes, 4 * len(bins)))
        norm_layer = norm_layer_for(sync_bn)
        self.bins = bins
        self.rep_head = rep_head
        red = in_planes // len(bins)
        self.ppm = nn.ModuleList(
            nn.Sequential(
                nn.AdaptiveAvgPool2d(b),  # marker: executed by K.pyramid_pool
                K.Conv2d(in_planes, red, kernel_size=1, bias=False),
                norm_layer(red),
                nn.ReLU(inplace=True),
            ) for b in bins)
        self.head = _unit3x3(2 * in_planes, inner_planes, norm_layer, nn.Dropout2d(0.1))
        self.classifier = K.Conv2d(inner_planes, num_classes, kernel_size=1, stride=1, padding=0, bias=True)
        if rep_head:
            self.representation = _rep_tower(inner_planes, norm_layer)

    def forward(self, x, need_rep=True):
        x = _last_map(x)
        h, w = x.size()[-2:]
        x_pass, *pooled = K.pyramid_pool(x, self.bins)
        # independent conv -> BN -> ReLU units: under a process group their statistics share one packed exchange
        f = K.conv_bn_group([(m[1], m[2], p, True, None) for m, p in zip(self.ppm, pooled)])
        feat = K.cat_channels((x_pass, *(K.upsample_bilinear(t, (h, w)) for t in f)))
        return _outputs(self, K.run_seq(self.head, feat), need_rep)


def _unit1x1(in_planes, out_planes, norm_layer):
    return [K.Conv2d(in_planes, out_planes, kernel_size=1, stride=1, padding=0, bias=False), norm_layer(out_planes),
            nn.ReLU(inplace=True)]


class dec_ocrnet(nn.Module):
    """Object-contextual representations head (OCRNet, Yuan et al., ECCV 2020, section 3.2; no reference line: the reference has
    the two ASPP heads only).  conv3x3: 3x3 to inner_planes -> norm -> ReLU, the pixel features; region: 1x1 to 256 -> norm ->
    ReLU -> 1x1 to num_classes, the soft object regions, a coarse prediction on the decoder's input that the trainer supervises
    on the labelled images (region_loss_weight; output key "region").  The region features f = sum over an image's pixels of
    softmax_pixels(region) * pixel features (K.region_pool) are a [N, inner, K, 1] map; queries f_pixel(pixel features), keys
    f_object(f), values f_down(f), one head: y = softmax_k(q . k / sqrt(key_planes)) v (K.region_attention); fuse: 1x1 over
    cat(f_up(y), pixel features) -> norm -> ReLU -> Dropout2d(0.05); classifier: 1x1 with bias.  rep_head: the
    `representation` tower (_rep_tower) on the fused features.  Out of scope, refused or absent: more than 255 classes (regions), several
    heads, a separable form, regions taken from the auxiliary head, OHEM on the region loss.  (Pixel-to-pixel attention is dec_ccnet's.)"""

    def __init__(self, in_planes, num_classes=19, inner_planes=512, key_planes=256, sync_bn=False, rep_head=False,
                 region_loss_weight=0.4):
        super().__init__()
        K.check_region_shapes(1, 1, num_classes, inner_planes, "dec_ocrnet (num_classes regions, inner_planes channels)")
        K.check_region_shapes(1, 1, num_classes, key_planes, "dec_ocrnet (num_classes regions, key_planes channels)")
        if in_planes % 4:
            raise ValueError("dec_ocrnet: in_planes (%d) must be a multiple of 4" % in_planes)
        if not float(region_loss_weight) >= 0:
            raise ValueError("dec_ocrnet: region_loss_weight must be >= 0, got %r" % (region_loss_weight,))
        norm_layer = norm_layer_for(sync_bn)
        self.rep_head = rep_head
        self.key_planes = key_planes
        self.region_loss_weight = float(region_loss_weight)
        self.conv3x3 = _unit3x3(in_planes, inner_planes, norm_layer)
        self.region = nn.Sequential(
            *_unit1x1(in_planes, 256, norm_layer),
            K.Conv2d(256, num_classes, kernel_size=1, stride=1, padding=0, bias=True))
        self.f_pixel = nn.Sequential(*_unit1x1(inner_planes, key_planes, norm_layer), *_unit1x1(key_planes, key_planes, norm_layer))
        self.f_object = nn.Sequential(*_unit1x1(inner_planes, key_planes, norm_layer), *_unit1x1(key_planes, key_planes, norm_layer))
        self.f_down = nn.Sequential(*_unit1x1(inner_planes, key_planes, norm_layer))
        self.f_up = nn.Sequential(*_unit1x1(key_planes, inner_planes, norm_layer))
        self.fuse = nn.Sequential(*_unit1x1(2 * inner_planes, inner_planes, norm_layer), nn.Dropout2d(0.05))
        self.classifier = K.Conv2d(inner_planes, num_classes, kernel_size=1, stride=1, padding=0, bias=True)
        if rep_head:
            self.representation = _rep_tower(inner_planes, norm_layer)

    def forward(self, x, need_rep=True):
        x = _last_map(x)
        feat = K.run_seq(self.conv3x3, x)
        r = K.run_seq(self.region, x)
        feat_p, f = K.region_pool(feat, r)
        q = K.run_seq(self.f_pixel, feat_p)
        # independent conv -> BN -> ReLU units on the region features: under a process group their statistics share one exchange
        k1, v = K.conv_bn_group([(self.f_object[0], self.f_object[1], f, True, None), (self.f_down[0], self.f_down[1], f, True, None)])
        kk = K.conv_bn(self.f_object[3], self.f_object[4], k1, relu=True)
        y = K.run_seq(self.f_up, K.region_attention(q, kk, v, self.key_planes ** -0.5))
        out = K.run_seq(self.fuse, K.cat_channels((y, feat_p)))
        return _outputs(self, out, need_rep, region=r)


class CrissCrossBlock(nn.Module):
    """one criss-cross attention block (CCNet section 3.1): 1x1 query and key to key_planes, 1x1 value to planes, all with bias,
    and gamma, one parameter that starts at 0: x + gamma * attention(x)"""

    def __init__(self, planes, key_planes):
        super().__init__()
        self.query = K.Conv2d(planes, key_planes, kernel_size=1, stride=1, padding=0, bias=True)
        self.key = K.Conv2d(planes, key_planes, kernel_size=1, stride=1, padding=0, bias=True)
        self.value = K.Conv2d(planes, planes, kernel_size=1, stride=1, padding=0, bias=True)
        self.gamma = nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return K.criss_cross_attention(self.query(x), self.key(x), self.value(x), self.gamma, res=x, scale=1.0)


class _ContextHead(nn.Module):
    """what dec_ccnet and dec_nonlocal share: conva: 3x3 to inner_planes -> norm -> ReLU; the subclass's context block(s); convb:
    3x3 -> norm -> ReLU; bottleneck: 3x3 over cat(input, convb) -> norm -> ReLU -> Dropout2d(0.1); classifier: 1x1 with bias;
    rep_head: the `representation` tower (_rep_tower) on the bottleneck.  A subclass checks its arguments, hands the block's own
    to __init__ and supplies make_context(inner_planes, norm_layer, **those), which registers the block(s), and context(f), which
    runs a feature map through them.  make_context is called between conva and convb: the registration order of the two heads."""

    def __init__(self, in_planes, num_classes, inner_planes, sync_bn, rep_head, **context_args):
        super().__init__()
        norm_layer = norm_layer_for(sync_bn)
        self.rep_head = rep_head
        self.conva = _unit3x3(in_planes, inner_planes, norm_layer)
        self.make_context(inner_planes, norm_layer, **context_args)
        self.convb = _unit3x3(inner_planes, inner_planes, norm_layer)
        self.bottleneck = _unit3x3(in_planes + inner_planes, inner_planes, norm_layer, nn.Dropout2d(0.1))
        self.classifier = K.Conv2d(inner_planes, num_classes, kernel_size=1, stride=1, padding=0, bias=True)
        if rep_head:
            self.representation = _rep_tower(inner_planes, norm_layer)

    def forward(self, x, need_rep=True):
        x = _last_map(x)
        f = K.run_seq(self.convb, self.context(K.run_seq(self.conva, x)))
        return _outputs(self, K.run_seq(self.bottleneck, K.cat_channels((x, f))), need_rep)


class dec_ccnet(_ContextHead):
    """Criss-cross attention head (CCNet, Huang et al., ICCV 2019, section 3; no reference line: the reference has the two ASPP
    heads only): a _ContextHead whose block is cca: a CrissCrossBlock applied `recurrence` times (every pixel attends to its own
    row and column, K.criss_cross_attention; two rounds give every pixel a path to every other); with shared=False a ModuleList
    of `recurrence` blocks.
    A map with H + W - 1 > K.CC_MAX_L is refused (predict large images in sliding windows).  With shared=True and
    recurrence > 1 the block's gradient sinks are written once per round, which the bucketed all-reduce does not count: that
    combination is refused under a process group.  Out of scope, refused or absent: a fused q/k/v projection, a tiled cross,
    the fp16 prediction path, a separable form.  (Dense attention and several heads are dec_nonlocal's.)"""

    def __init__(self, in_planes, num_classes=19, inner_planes=512, key_planes=64, recurrence=2, shared=True, sync_bn=False,
                 rep_head=False):
        _check_planes("dec_ccnet", in_planes=in_planes, inner_planes=inner_planes, key_planes=key_planes)
        if int(recurrence) < 1:
            raise ValueError("dec_ccnet: recurrence must be >= 1, got %r" % (recurrence,))
        _check_num_classes("dec_ccnet", num_classes)
        super().__init__(in_planes, num_classes, inner_planes, sync_bn, rep_head, key_planes=key_planes, recurrence=int(recurrence),
                         shared=bool(shared))

    def make_context(self, inner_planes, norm_layer, key_planes, recurrence, shared):
        self.recurrence, self.shared = recurrence, shared
        if shared:
            self.cca = CrissCrossBlock(inner_planes, key_planes)
        else:
            self.cca = nn.ModuleList(CrissCrossBlock(inner_planes, key_planes) for _ in range(recurrence))

    def context(self, f):
        for i in range(self.recurrence):
            f = (self.cca if self.shared else self.cca[i])(f)
        return f

    def check_ranks(self):
        """shared weights collect one gradient per round in the same sinks; the bucketed all-reduce counts one arrival per
        parameter, so a process group would reduce a bucket before the second round's contribution"""
        if self.shared and self.recurrence > 1 and K.dist_active():
            raise NotImplementedError("dec_ccnet: shared attention weights over %d rounds are not supported on more than one rank or "
                                      "under U2PL_DIST_SINGLE; `shared: false` or `recurrence: 1` run there" % self.recurrence)

    def forward(self, x, need_rep=True):
        if torch.is_grad_enabled():
            self.check_ranks()
        return super().forward(x, need_rep)


class NonLocalBlock(nn.Module):
    """one dense self-attention block (Non-local networks, Wang et al., CVPR 2018, section 3.3, in its embedded-Gaussian form):
    query: 1x1 planes -> key_planes; key: 1x1 planes -> key_planes and value: 1x1 planes -> value_planes, both with stride
    kv_stride (1 or 2: the strided 1x1 of ResNet's downsample; with 2 the keys are the ceil(H/2) x ceil(W/2) sub-grid), all
    three with bias; project: 1x1 value_planes -> planes without bias -> norm whose WEIGHT STARTS AT 0 (the paper's
    initialisation: the block is the identity at step 0).  forward: x + project(K.dense_attention(q, k, v, heads, scale)); the
    residual is the BatchNorm apply's own residual operand (the route of a bottleneck's tail)."""

    def __init__(self, planes, key_planes, value_planes, heads=1, kv_stride=1, scale=None, norm_layer=K.BatchNorm2d):
        super().__init__()
        self.heads, self.scale = int(heads), scale
        self.query = K.Conv2d(planes, key_planes, kernel_size=1, stride=1, padding=0, bias=True)
        self.key = K.Conv2d(planes, key_planes, kernel_size=1, stride=kv_stride, padding=0, bias=True)
        self.value = K.Conv2d(planes, value_planes, kernel_size=1, stride=kv_stride, padding=0, bias=True)
        self.project = nn.Sequential(K.Conv2d(value_planes, planes, kernel_size=1, stride=1, padding=0, bias=False), norm_layer(planes))
        nn.init.zeros_(self.project[1].weight)

    def forward(self, x):
        y = K.dense_attention(self.query(x), self.key(x), self.value(x), heads=self.heads, scale=self.scale)
        return K.conv_bn(self.project[0], self.project[1], y, res=x)


class dec_nonlocal(_ContextHead):
    """Non-local head (Wang et al., CVPR 2018; the position attention of DANet, Fu et al., CVPR 2019, is this block with
    value_planes = inner_planes; no reference line: the reference has the two ASPP heads only): a _ContextHead whose block is
    nl: a NonLocalBlock in the place of dec_ccnet's criss-cross rounds, every pixel attends to every pixel (K.dense_attention,
    csrc/attn.hip: tiled, online softmax, nothing of size pixels x pixels stored, so no cap on the map).  key_planes / heads <=
    K.ATTN_MAX_D and value_planes / heads <= K.ATTN_MAX_DV per head.  Out of scope, refused or absent: masks and causal attention, dropout on
    the weights, relative position terms, a fused q/k/v projection, DANet's channel-attention branch, the fp16 prediction path."""

    def __init__(self, in_planes, num_classes=19, inner_planes=512, key_planes=64, value_planes=256, heads=1, kv_stride=1,
                 scale=None, sync_bn=False, rep_head=False):
        _check_planes("dec_nonlocal", in_planes=in_planes, inner_planes=inner_planes, key_planes=key_planes,
                      value_planes=value_planes)
        if int(heads) < 1 or int(key_planes) % int(heads) or int(value_planes) % int(heads):
            raise ValueError("dec_nonlocal: key_planes (%r) and value_planes (%r) must divide into heads (%r)" % (
                key_planes, value_planes, heads))
        K.check_attn_shapes(1, heads, 1, 1, int(key_planes) // int(heads), int(value_planes) // int(heads), "dec_nonlocal")
        if kv_stride not in (1, 2):
            raise ValueError("dec_nonlocal: kv_stride must be 1 or 2, got %r" % (kv_stride,))
        _check_num_classes("dec_nonlocal", num_classes)
        super().__init__(in_planes, num_classes, inner_planes, sync_bn, rep_head, key_planes=key_planes, value_planes=value_planes,
                         heads=heads, kv_stride=kv_stride, scale=scale)

    def make_context(self, inner_planes, norm_layer, **block):
        self.nl = NonLocalBlock(inner_planes, norm_layer=norm_layer, **block)

    def context(self, f):
        return self.nl(f)


class Aux_Module(nn.Module):
    def __init__(self, in_planes, num_classes=19, sync_bn=False):
        super().__init__()
        norm_layer = norm_layer_for(sync_bn)
        self.aux = nn.Sequential(
            K.Conv2d(in_planes, 256, kernel_size=3, stride=1, padding=1),
            norm_layer(256), nn.ReLU(inplace=True), nn.Dropout2d(0.1),
            K.Conv2d(256, num_classes, kernel_size=1, stride=1, padding=0, bias=True),
        )

    def forward(self, x):
        return K.run_seq(self.aux, x)
