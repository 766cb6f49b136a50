"""3D U-Net building blocks -- MI355X-native stand-ins for the reference's model/unet.py.

Same class names, constructor arguments and ``state_dict`` keys as the reference (model/unet.py:79-100 SingleConv,
:103-144 DoubleConv, :147-159 StepDownDoubleConv, :210-253 Encoder, :256-322 Decoder/DecoderNoJoining, :392-537
Abstract3DUNet/UNet3D), so reference checkpoints load unchanged.  The modules HOLD the parameters and their packed weight images; a
``forward`` asks ``rfuse.routes`` which kernel form takes the layer (or the conv pair: DESIGN 4.8 / 4.9) and runs the form it names through ``rfuse.ops``
-- GroupNorm applied in the conv's prologue, ReLU, max-pool and statistics for the next GroupNorm in its epilogue, a decoder's upsample + concat read as two
sources.  Only layer order 'gcr' is built; in grad mode SingleConv runs rfuse/autograd.py (no hand-overs); CPU tensors raise.
"""
import math

import torch
from torch import nn

from rfuse import ops, routes


class GroupNormParams(nn.Module):
    """weight/bias holder with nn.GroupNorm's names, init (ones / zeros) and the <groups collapse of model/unet.py:62-63."""

    def __init__(self, num_groups, num_channels, eps=1e-5):
        super().__init__()
        if num_channels < num_groups:
            num_groups = 1
        assert num_channels % num_groups == 0, \
            f'Expected number of channels in input to be divisible by num_groups. num_channels={num_channels}, num_groups={num_groups}'
        self.num_groups, self.num_channels, self.eps = num_groups, num_channels, eps
        self.weight = nn.Parameter(torch.ones(num_channels))
        self.bias = nn.Parameter(torch.zeros(num_channels))

    def extra_repr(self):
        return f'{self.num_groups}, {self.num_channels}, eps={self.eps}'


class Conv3dParams(nn.Module):
    """weight (and optional bias) holder with nn.Conv3d's names, shapes (OIDHW) and default initialisation."""

    def __init__(self, in_channels, out_channels, kernel_size, bias, stride=1, padding=0):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding = kernel_size, stride, padding
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, kernel_size, kernel_size, kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()
        self._packed = ops.PackedWeight('conv3' if (kernel_size == 3 and padding == 1) else 'convv')
        self._packed_up = ops.PackedWeight('conv3up')
        self._packed_up_split = ops.PackedWeight('conv3ups')
        self._packed_split = ops.PackedWeight('conv3s')
        self._packed_e2 = ops.PackedWeight('conv3e2')
        self._packed_lds = ops.PackedWeight('convvl')
        self._packed_valu = ops.PackedWeight('convvv')
        self._packed_vsplit = ops.PackedWeight('convvs')
        self._packed_vpg = ops.PackedWeight('convvpg')

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            fan_in = self.in_channels * self.kernel_size ** 3
            bound = 1 / math.sqrt(fan_in) if fan_in > 0 else 0
            nn.init.uniform_(self.bias, -bound, bound)

    def packed(self):
        return self._packed.get(self.weight)

    def packed_lds(self):
        """operand image of the LDS-staged valid-conv form (patch encoders' large layers)"""
        return self._packed_lds.get(self.weight)

    def packed_valu(self):
        """[cin, k,k,k, cout] image of the VALU valid-conv form (patch encoders' first layers)"""
        return self._packed_valu.get(self.weight)

    def packed_valid_split(self, s):
        """f16 fragment image of the split-operand valid-conv form for input edge s (csrc/conv_valid_split.hip)"""
        return self._packed_vsplit.get(self.weight, s, self.stride)

    def packed_valid_split_pg(self, s):
        """weight image of the persistent grid form of the split-operand valid conv for input edge s (csrc/conv_valid_split_pg.hip)"""
        return self._packed_vpg.get(self.weight, s, self.stride)

    def packed_up(self, c0):
        """operand image of the decoder form (first c0 input channels = skip source, rest = upsampled source)"""
        return self._packed_up.get(self.weight, c0)

    def packed_split(self):
        """f16 fragment image of the split-operand box conv (csrc/conv3d_split.hip)"""
        return self._packed_split.get(self.weight)

    def packed_e2_split(self, edge):
        """f16 fragment image of the dense GEMM form on whole 2^3 / 1^3 volumes (csrc/conv3d_e2_split.hip)"""
        return self._packed_e2.get(self.weight, edge)

    def packed_up_split(self, c0):
        """f16 fragment image of the split-operand decoder form (csrc/conv3d_up_split.hip)"""
        return self._packed_up_split.get(self.weight, c0)

    def extra_repr(self):
        return f'{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, padding={self.padding}'


class SingleConv(nn.Module):
    """GroupNorm -> Conv3d(k3, p1, no bias) -> ReLU, order 'gcr' (reference model/unet.py:19-76,79-100)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, order='gcr', num_groups=8, padding=1):
        super().__init__()
        if order != 'gcr' or kernel_size != 3 or padding != 1:
            raise NotImplementedError(
                "only layer order 'gcr' with 3x3x3 kernels and padding 1 is built (the only order the shipped configs use); got "
                f"order={order!r} kernel_size={kernel_size} padding={padding}")
        self.groupnorm = GroupNormParams(num_groups, in_channels)
        self.conv = Conv3dParams(in_channels, out_channels, 3, bias=False, padding=1)

    def range_ok(self, edge):
        """as a callable for rfuse.routes: can the split-operand forms not saturate on an edge^3 input (ops.split_range_ok: |gamma| sqrt(group elements) + |beta|)"""
        gn = self.groupnorm
        return lambda: ops.split_range_ok(self.conv.weight, gn.weight, gn.bias, (gn.num_channels // gn.num_groups) * edge ** 3)

    def forward(self, x, upsampled=None, pool=None):
        """x: full-resolution source [N,C0,S,S,S] or None; ``upsampled``: low-resolution source [N,C1,S/2,S/2,S/2] that the
        reference would nearest-upsample and concatenate after x (model/unet.py:297-308).
        ``pool``: None -> returns the output; 'also' / 'only' -> returns (output, MaxPool3d(2)(output)) with the pooling
        fused into the conv epilogue where the tiling allows ('only': the caller never reads the full-resolution output, which
        is then not written at all and returned as None)."""
        gn, conv, cout = self.groupnorm, self.conv, self.conv.out_channels
        if ops.needs_grad(x, upsampled, conv.weight, gn.weight, gn.bias):
            # training slice: the same kernels behind torch.autograd.Function, see rfuse/autograd.py
            from rfuse import autograd as rf_autograd
            out = rf_autograd.conv_gn_relu(x, upsampled, gn.weight, gn.bias, conv.weight, gn.num_groups, gn.eps)
            return out if pool is None else (out, rf_autograd.max_pool2(out))
        aff = ops.gn_affine(x, upsampled, gn.weight, gn.bias, gn.num_groups, gn.eps)
        n, c0, c1, edge = ops._src_dims(x, upsampled)
        route = routes.single(n, c0, c1, edge, cout, pool, routes.split_arith(self.range_ok(edge)), materialised=False)
        if route == 'split_box':
            return ops.conv3d_split_gn_relu(x, aff, conv.packed_split(), cout, pool=pool)
        if route == 'pool_fp32':
            return ops.conv3d_gn_relu_pool(x, None, aff, conv.packed(), cout, keep_full=(pool == 'also'))
        if route == 'e2':
            out = ops.conv3d_e2_split_gn_relu(x, aff, conv.packed_e2_split(edge), cout)
        elif route == 'e2_concat':
            # decoder stage on 2^3 volumes (skip @2^3 + a 1^3 source): the eight copies of the low-resolution voxel written out (a few KB per sample), dense GEMM
            up = upsampled.reshape(n, c1, 1, 1, 1).expand(-1, -1, 2, 2, 2)
            xc = torch.cat((x, up), dim=1) if x is not None else up.contiguous()
            out = ops.conv3d_e2_split_gn_relu(xc, aff, conv.packed_e2_split(2), cout)
        elif route == 'direct':
            out = ops.conv3d_gn_relu(x, upsampled, aff, None, cout, direct_weight=conv.weight)
        elif route == 'up_split':
            out = ops.conv3d_up_split_gn_relu(x, upsampled, aff, conv.packed_up_split(c0), cout)
        elif route == 'split_box_concat':
            # a decoder stage outside the decoder forms of the F16 cores (C5's 96 + 192 -> 96 @16^3 at 16 chunks): the concatenation written out once (75 MB
            # there) for the split-operand box kernel -- 0.53 ms as the fp32-MFMA decoder form.  The affine table is per channel of the concatenation either way.
            up = upsampled.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)
            out = ops.conv3d_split_gn_relu(torch.cat((x, up), dim=1) if x is not None else up, aff, conv.packed_split(), cout)
        elif route == 'up_fp32':
            out = ops.conv3d_up_gn_relu(x, upsampled, aff, conv.packed_up(c0), cout)
        else:
            out = ops.conv3d_gn_relu(x, upsampled, aff, conv.packed(), cout)
        return out if pool is None else (out, ops.maxpool2(out))


class _ConvPair(nn.Module):
    """SingleConv1 -> SingleConv2; where rfuse.routes.pair says so the first hands the second its input pre-split."""
    ENCODER_FORMS = True

    def route(self, x, upsampled=None, pool=None, next_block=None):
        """the name rfuse.routes.pair gives this block's form on these inputs (arguments as forward's)"""
        if isinstance(x, ops.PreSplit):
            return 'prepooled'                                      # its producer asked (accepts_prepooled) before it wrote
        c1, c2 = self.SingleConv1, self.SingleConv2
        (n, ch0, ch1, edge), cout = ops._src_dims(x, upsampled), c2.conv.out_channels
        grad = ops.needs_grad(x, upsampled, c1.conv.weight, c2.conv.weight, c1.groupnorm.weight, c2.groupnorm.weight)
        return routes.pair(n, ch0, ch1, edge, c1.conv.out_channels, cout, c2.groupnorm.num_groups, pool, grad, c1.range_ok(edge), c2.range_ok(edge),
                           encoder_forms=self.ENCODER_FORMS, next_takes=None if next_block is None else (lambda: next_block.accepts_prepooled(n, cout, edge // 2)),
                           next_groups=0 if next_block is None else next_block.SingleConv1.groupnorm.num_groups)

    def accepts_prepooled(self, n, cin, edge):
        """this block's conv pair can take its input as an ops.PreSplit of [n, cin, edge^3] (normalised for SingleConv1's GroupNorm) -- decided from shapes and
        parameters only, so that the PRODUCER can ask before it writes"""
        c1, c2 = self.SingleConv1, self.SingleConv2
        grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        return c1.conv.in_channels == cin and routes.pair(n, cin, 0, edge, c1.conv.out_channels, c2.conv.out_channels, c2.groupnorm.num_groups, None, grad,
                                                          c1.range_ok(edge), c2.range_ok(edge), offered=True) == 'prepooled'

    def forward(self, x, upsampled=None, pool=None, next_block=None):
        """``next_block``: the DoubleConv that will read MaxPool3d(2) of this block's output (the next encoder level), when the caller knows it -- with
        pool='only' the pooled tensor can then be handed over pre-split (returned as an ops.PreSplit in place of the pooled tensor)."""
        c1, c2 = self.SingleConv1, self.SingleConv2
        route = self.route(x, upsampled, pool, next_block)
        if route == 'plain':
            return c2(c1(x, upsampled), pool=pool)
        # a producer that applies the SECOND GroupNorm to its own output and writes it pre-split (no fp32 intermediate, no rf_gn_from_stats), then the consumer
        g1, g2, cmid, cout, pm = c1.groupnorm, c2.groupnorm, c1.conv.out_channels, c2.conv.out_channels, route == 'decoder_presplit_pm'
        second = (g2.weight, g2.bias, g2.num_groups, g2.eps)
        if route == 'prepooled':                                    # the previous level handed its pooled output over pre-split for THIS block's first GroupNorm
            n, edge, pre = x.n, x.edge, ops.conv3d_split_pre_presplit(x, c1.conv.packed_split(), cmid, *second).data
        else:
            n, ch0, _, edge = ops._src_dims(x, upsampled)
            if route in ('cin1_presplit', 'cin1_presplit_handed'):  # level 0 of a U-Net on 16^3 samples: the 1-channel conv computes its own GroupNorm
                pre = ops.conv3d_cin1_presplit(x, g1.weight, g1.bias, g1.eps, c1.conv.packed(), cmid, *second)
            else:
                aff = ops.gn_affine(x, upsampled, g1.weight, g1.bias, g1.num_groups, g1.eps)
                if route == 'box_presplit':                         # an encoder level on whole 8^3 samples (16 -> 16 -> 32 of the retrieval backbone)
                    pre = ops.conv3d_split_presplit(x, aff, c1.conv.packed_split(), cmid, *second)
                else:                                               # a decoder's pair on whole 8^3 samples; parity-major where producer and consumer are persistent
                    pre = ops.conv3d_up_split_presplit(x, upsampled, aff, c1.conv.packed_up_split(ch0), cmid, *second, parity_major=pm)
        if route == 'cin1_presplit_handed':                         # -> (None, the pooled output as an ops.PreSplit for next_block)
            ng = next_block.SingleConv1.groupnorm
            return ops.conv3d_split_pre_relu_pool_presplit(pre, cmid, n, edge, c2.conv.packed_split(), cout, ng.weight, ng.bias, ng.num_groups, ng.eps)
        return ops.conv3d_split_pre_relu(pre, cmid, n, edge, c2.conv.packed_split(), cout, pool=pool, parity_major=pm)


class DoubleConv(_ConvPair):
    """Two SingleConvs; channel plan of reference model/unet.py:125-144."""

    def __init__(self, in_channels, out_channels, encoder, kernel_size=3, order='gcr', num_groups=8):
        super().__init__()
        if encoder:
            c1_in, c1_out = in_channels, max(out_channels // 2, in_channels)
            c2_in, c2_out = c1_out, out_channels
        else:
            c1_in, c1_out = in_channels, out_channels
            c2_in, c2_out = out_channels, out_channels
        self.SingleConv1 = SingleConv(c1_in, c1_out, kernel_size, order, num_groups)
        self.SingleConv2 = SingleConv(c2_in, c2_out, kernel_size, order, num_groups)


class StepDownDoubleConv(_ConvPair):
    """in -> (in+out)//2 -> out (reference model/unet.py:149-159); a decoder block: of the hand-overs, the decoder pair's only."""
    ENCODER_FORMS = False

    def __init__(self, in_channels, out_channels, encoder, kernel_size=3, order='gcr', num_groups=8):
        super().__init__()
        self.encoder = encoder
        mid = (in_channels + out_channels) // 2
        self.SingleConv1 = SingleConv(in_channels, mid, kernel_size, order, num_groups)
        self.SingleConv2 = SingleConv(mid, out_channels, kernel_size, order, num_groups)


class Encoder(nn.Module):
    """optional MaxPool3d(2) then the basic module (reference model/unet.py:230-253)."""

    def __init__(self, in_channels, out_channels, conv_kernel_size=3, apply_pooling=True, pool_kernel_size=(2, 2, 2),
                 pool_type='max', basic_module=DoubleConv, conv_layer_order='gcr', num_groups=8):
        super().__init__()
        if apply_pooling and (pool_type != 'max' or tuple(pool_kernel_size) != (2, 2, 2)):
            raise NotImplementedError('only MaxPool3d(2) is built')
        self.apply_pooling = apply_pooling
        self.basic_module = basic_module(in_channels, out_channels, encoder=True, kernel_size=conv_kernel_size,
                                         order=conv_layer_order, num_groups=num_groups)

    def level_route(self, n, c, edge, grad=False, skip=None):
        """the name rfuse.routes.level gives this level on an unpooled input [n, c, edge^3] ('plain' for a level without pooling or whose basic module is no
        DoubleConv); ``skip``: see routes.level"""
        bm = self.basic_module
        if not self.apply_pooling or not isinstance(bm, DoubleConv) or bm.SingleConv1.conv.in_channels != c:
            return 'plain'
        c1, c2 = bm.SingleConv1, bm.SingleConv2
        grad = grad or (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()))
        return routes.level(n, c, edge, c1.conv.out_channels, c2.conv.out_channels, ops._gn_groups(c, c1.groupnorm.num_groups),
                            ops._gn_groups(c1.conv.out_channels, c2.groupnorm.num_groups), grad, c1.range_ok(edge // 2), c2.range_ok(edge // 2), skip=skip)

    def forward(self, x, prepooled=None, pool=None, next_block=None, consumer=None):
        """``prepooled``: MaxPool3d(2)(x) when the producer already emitted it (fused epilogue; an ops.PreSplit when it was handed over pre-split);
        ``pool``: see SingleConv.forward; ``next_block``: see DoubleConv.forward; ``consumer``: (skip tensor, GroupNormParams) of the decoder stage that
        will read this level's output upsampled beside that skip tensor, when the caller knows it -- a level that runs as one launch writes that
        GroupNorm's table as well (the LATER producer of a straddling GroupNorm has both halves' statistics)."""
        if self.apply_pooling:
            if prepooled is not None:
                x = prepooled
            elif ops.needs_grad(x):
                x = torch.nn.functional.max_pool3d(x, 2)            # grad mode: torch's max-pool carries the backward
            else:
                if pool is None and x.dim() == 5:
                    done = self._whole_level(x, consumer)
                    if done is not None:
                        return done
                x = ops.maxpool2(x)
        return self.basic_module(x, pool=pool, next_block=next_block)

    def _whole_level(self, x, consumer):
        """the level as one launch where routes.level names that form, else None"""
        n, c, edge = x.shape[0], x.shape[1], x.shape[2]
        skip = gn_dec = None
        if consumer is not None and consumer[0] is not None:
            st = ops._fresh_stats(consumer[0])
            if st is not None:
                skip, gn_dec = consumer
        cout = self.basic_module.SingleConv2.conv.out_channels if isinstance(self.basic_module, DoubleConv) else 0
        plan = None if skip is None else (skip.shape[1], st[1], ops._gn_groups(skip.shape[1] + cout, gn_dec.num_groups))
        if self.level_route(n, c, edge, skip=plan) != 'e2_level':
            return None
        c1, c2 = self.basic_module.SingleConv1, self.basic_module.SingleConv2
        g1, g2 = c1.groupnorm, c2.groupnorm
        return ops.conv3d_e2_level(x, (g1.weight, g1.bias, g1.num_groups, g1.eps), c1.conv.packed_e2_split(2), c1.conv.out_channels,
                                   (g2.weight, g2.bias, g2.num_groups, g2.eps), c2.conv.packed_e2_split(2), cout, skip=skip,
                                   gn_dec=None if skip is None else (gn_dec.weight, gn_dec.bias, gn_dec.num_groups, gn_dec.eps))


class Decoder(nn.Module):
    """nearest upsample to the skip's size + concat (skip first) + basic module (reference model/unet.py:273-308)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, scale_factor=(2, 2, 2), basic_module=DoubleConv,
                 conv_layer_order='gcr', num_groups=8, mode='nearest'):
        super().__init__()
        if basic_module not in (DoubleConv, StepDownDoubleConv) or mode != 'nearest' or tuple(scale_factor) != (2, 2, 2):
            raise NotImplementedError('only nearest x2 upsampling with concat joining is built')
        self.basic_module = basic_module(in_channels, out_channels, encoder=False, kernel_size=kernel_size,
                                         order=conv_layer_order, num_groups=num_groups)

    def forward(self, encoder_features, x):
        if encoder_features.shape[2] != 2 * x.shape[2]:
            raise NotImplementedError('skip connection must be exactly twice the decoder input resolution')
        return self.basic_module(encoder_features, x)


class DecoderNoJoining(Decoder):
    """x2 nearest upsample then the basic module, no skip (reference model/unet.py:311-322)."""

    # noinspection PyMethodOverriding
    def forward(self, x):
        return self.basic_module(None, x)


def number_of_features_per_level(init_channel_number, num_levels):
    return [init_channel_number * 2 ** k for k in range(num_levels)]


class UNet3D(nn.Module):
    """Encoder/decoder wiring of reference Abstract3DUNet (model/unet.py:424-520) with DoubleConv, final_conv=False."""

    def __init__(self, in_channels, out_channels, final_sigmoid=True, f_maps=64, layer_order='gcr', num_groups=8, num_levels=4,
                 is_segmentation=True, remove_n_final_layers=0, final_conv=False, **kwargs):
        super().__init__()
        if final_conv or is_segmentation:
            raise NotImplementedError('final_conv / segmentation heads are never instantiated by the refinement path')
        if isinstance(f_maps, int):
            f_maps = number_of_features_per_level(f_maps, num_levels=num_levels)
        encoders = []
        for i, out_feature_num in enumerate(f_maps):
            encoders.append(Encoder(in_channels if i == 0 else f_maps[i - 1], out_feature_num, apply_pooling=(i > 0),
                                    basic_module=DoubleConv, conv_layer_order=layer_order, num_groups=num_groups))
        self.encoders = nn.ModuleList(encoders)

        reversed_f_maps = list(reversed(f_maps))
        if remove_n_final_layers > 0:
            reversed_f_maps = reversed_f_maps[:-remove_n_final_layers]
        outs = list(reversed_f_maps)
        outs[-1] = out_channels                                      # model/unet.py:453-455
        decoders = []
        for i in range(len(reversed_f_maps) - 1):
            in_feature_num = reversed_f_maps[i] + reversed_f_maps[i + 1]
            last_and_trimmed = i == (len(reversed_f_maps) - 2) and remove_n_final_layers > 0      # model/unet.py:465
            decoders.append(Decoder(in_feature_num, outs[i + 1], basic_module=StepDownDoubleConv if last_and_trimmed else DoubleConv,
                                    conv_layer_order=layer_order, num_groups=num_groups))
        self.decoders = nn.ModuleList(decoders)

    def forward(self, x, after_encoders=None):
        """``after_encoders``: optional callable run between the encoder and the decoder launches (the engine issues the next batch's front end there)"""
        feats = []
        n_enc, n_dec = len(self.encoders), len(self.decoders)
        pooled = None
        for i, encoder in enumerate(self.encoders):
            # Who reads this level's full-resolution output?  The next level reads MaxPool3d(2) of it; a decoder reads it as
            # a skip only for levels n_enc-1-n_dec .. n_enc-2 (model/unet.py:500-507: the list is cut and zip() truncates, so
            # with remove_n_final_layers the finest levels are never joined).  Unread outputs are not even written.
            if i == n_enc - 1:
                # the decoder stage that reads this output beside the previous level's: its GroupNorm's table can come out of this level's launch
                consumer = (feats[0], self.decoders[0].basic_module.SingleConv1.groupnorm) if n_dec > 0 and feats and isinstance(self.decoders[0], Decoder) \
                    and not isinstance(self.decoders[0], DecoderNoJoining) else None
                x, pooled = encoder(x, prepooled=pooled, consumer=consumer), None
            else:
                is_skip = i >= n_enc - 1 - n_dec
                nxt = self.encoders[i + 1].basic_module
                cout = encoder.basic_module.SingleConv2.conv.out_channels
                src = pooled if pooled is not None else x            # what this level's convs read: its output has that batch and edge
                n, edge = (src.n, src.edge) if isinstance(src, ops.PreSplit) else (src.shape[0], src.shape[2])
                if i == n_enc - 2 and is_skip and self.encoders[i + 1].level_route(n, cout, edge, ops.needs_grad(x)) == 'e2_level':
                    # the last level pools for itself, inside its one launch: this one writes its output only
                    x, pooled = encoder(x, prepooled=pooled, next_block=nxt if isinstance(nxt, DoubleConv) else None), None
                else:
                    x, pooled = encoder(x, prepooled=pooled, pool='also' if is_skip else 'only', next_block=nxt if isinstance(nxt, DoubleConv) else None)
            feats.insert(0, x)
        feats = feats[1:]                                            # model/unet.py:500-504
        if after_encoders is not None:
            after_encoders()
        for decoder, skip in zip(self.decoders, feats):              # zip truncates, model/unet.py:507
            x = decoder(skip, x)
        return x
