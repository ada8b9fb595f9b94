"""The eval-mode forward of a conv-encoder MultimodalAE on this backend's HIP kernels.

    conv stacks          shf_conv3x3s2_forward, one launch per layer (csrc/shf_conv.hip): implicit GEMM on the matrix cores,
                         eval-mode batch norm + conv bias + ReLU in the fp32 epilogue; NHWC activations between layers, the
                         last layer stores in torch.flatten order
    fc / fusion          shf_mlp_linear_forward_ld (csrc/shf_mlp.hip) on the model's own fp32 weights; every encoder's
                         latent goes straight into its column block of the fusion layer's input
    decoders             all decoders as ONE chain of block-diagonal layers (the zero blocks add exact zeros)

The first conv layer reads its input in place: a float tensor through its strides (the `permute(0, 3, 1, 2)` views the
vision stage passes), or -- from_camera -- the camera group's own rgba (u8, scaled by the fp32 reciprocal of 255 as torch.div(u8, 255.0) does) and depth (negated) images, which gives
bit for bit what the CameraSensor's normalised color_buf / depth_buf give.

Packed state (conv weights in fragment order, batch-norm scale / shift, the decoders' block-diagonal weights) is rebuilt
by the next call whenever any parameter or buffer of the model has changed (`_version`, storage address) since it was
packed: optimizer steps, load_state_dict and in-place edits all bump `_version`, so a stale pack cannot be used.  While
shapes and device stay the same the rebuild writes INTO the existing buffers, so their addresses -- which a captured
hipGraph has recorded -- stay valid: after a weight change one eager call repacks, and replays of an earlier capture then
compute with the new weights.  Packing reads the batch-norm terms on the host (a synchronisation), so it cannot happen
inside a stream capture: call the model once before capturing (`_fresh` raises if a capture would have to pack).

Non-finite pixels (the depth image's background is inf) make the outputs of THAT image non-finite and touch no other image.
"""
import ctypes as C

import torch
from torch import nn

from .. import _abi
from .._lib import BackendError, lib


def _ptr(t):
    return C.c_void_p(t.data_ptr())


class _Input:
    """First-layer source: base tensor, SHF_CONV_SRC_* kind, element strides (image, channel, row, column), C, H, W."""

    def __init__(self, t, kind, strides, c, h, w):
        self.t, self.kind, self.strides, self.c, self.h, self.w = t, kind, strides, c, h, w


def bn_affine(conv, bn):
    """Eval-mode batch norm and the conv bias as one affine map per output channel, in float64 on the host:
    y = acc * s + t with s = gamma / sqrt(var + eps), t = beta + (bias - mean) * s."""
    var = bn.running_var.detach().double().cpu()
    mean = bn.running_mean.detach().double().cpu()
    gamma = bn.weight.detach().double().cpu() if bn.weight is not None else torch.ones_like(var)
    beta = bn.bias.detach().double().cpu() if bn.bias is not None else torch.zeros_like(var)
    bias = conv.bias.detach().double().cpu() if conv.bias is not None else torch.zeros_like(var)
    s = gamma / torch.sqrt(var + bn.eps)
    return s, beta + (bias - mean) * s


def _is_relu(m):
    return isinstance(m, nn.ReLU)


class FusedRegressor:
    def __init__(self, model):
        from .autoencoders import ConvEncoder, Decoder
        self.model = model
        why = self._unsupported(model, ConvEncoder, Decoder)
        if why:
            raise ValueError("enable_fused_inference: this model is not covered by the fused kernels: " + why)
        self._packed_key = None
        self._conv, self._dec = {}, []
        self._state = {}         # packed tensors by role; kept across repacks so that their addresses do not move
        self._ws = {}
        self.launches = 0        # kernel launches of the last call (tools/bench_vision.py)

    # ---- structure -----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _unsupported(model, ConvEncoder, Decoder):
        if not model.encoders or not model.decoders:
            return "no encoders / decoders"
        for name, enc in model.encoders.items():
            if not isinstance(enc, ConvEncoder) or type(enc)._build_feature_extractor is not ConvEncoder._build_feature_extractor:
                return f"encoder {name!r} is not a ConvEncoder"
            if enc.variational:
                return f"encoder {name!r} is variational"
            for i, blk in enumerate(enc.feature_extractor):
                if not (isinstance(blk, nn.Sequential) and len(blk) == 3 and isinstance(blk[0], nn.Conv2d) and
                        isinstance(blk[1], nn.BatchNorm2d) and _is_relu(blk[2])):
                    return f"{name}.feature_extractor.{i} is not Conv2d + BatchNorm2d + ReLU"
                cv, bn = blk[0], blk[1]
                if (cv.kernel_size, cv.stride, cv.padding, cv.dilation, cv.groups, cv.padding_mode) != ((3, 3), (2, 2), (1, 1), (1, 1), 1, "zeros"):
                    return f"{name}.feature_extractor.{i}.0 is not a 3x3 / stride 2 / padding 1 convolution"
                if bn.running_mean is None or bn.running_var is None:
                    return f"{name}.feature_extractor.{i}.1 keeps no running statistics"
            fc = enc.fc
            if not (len(fc) == 3 and isinstance(fc[0], nn.Linear) and _is_relu(fc[1]) and isinstance(fc[2], nn.Linear)):
                return f"{name}.fc is not Linear + ReLU + Linear"
        depth = None
        for name, dec in model.decoders.items():
            if not isinstance(dec, Decoder):
                return f"decoder {name!r} is not a Decoder"
            for i, blk in enumerate(dec.lin_decoder):
                if not (isinstance(blk, nn.Sequential) and len(blk) == 2 and isinstance(blk[0], nn.Linear) and _is_relu(blk[1])):
                    return f"{name}.lin_decoder.{i} is not Linear + ReLU"
            if not (len(dec.fc) == 1 and isinstance(dec.fc[0], nn.Linear)):
                return f"{name}.fc is not a single Linear"
            if depth is not None and depth != len(dec.lin_decoder):
                return "the decoders differ in depth"
            depth = len(dec.lin_decoder)
        return None

    def on_gpu(self):
        return self.model.fusion_module.weight.is_cuda

    # ---- packed state --------------------------------------------------------------------------------------------------------
    def _key(self):
        ts = list(self.model.parameters()) + list(self.model.buffers())
        return tuple((t._version, t.data_ptr()) for t in ts)

    def _slot(self, key, shape, dtype, dev):
        """The packed tensor of role `key`: the one already there when shape, dtype and device still fit, else a new one."""
        t = self._state.get(key)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != dev:
            t = self._state[key] = torch.empty(shape, dtype=dtype, device=dev)
        return t

    def _put(self, key, value, dev):
        t = self._slot(key, value.shape, torch.float32, dev)
        t.copy_(value)
        return t

    def _pack(self):
        m = self.model
        dev = m.fusion_module.weight.device
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        self._conv = {}
        with torch.no_grad():
            for name, enc in m.encoders.items():
                layers = []
                for i, blk in enumerate(enc.feature_extractor):
                    cv, bn = blk[0], blk[1]
                    nbytes = C.c_int64()
                    if lib().shf_conv_pack_bytes(cv.in_channels, cv.out_channels, C.byref(nbytes)):
                        raise BackendError(lib().shf_conv_last_error().decode())
                    pack = self._slot((name, i, "pack"), (nbytes.value,), torch.uint8, dev)
                    w = cv.weight.detach().float().contiguous()
                    if lib().shf_conv_pack_weights(_ptr(w), _ptr(pack), cv.in_channels, cv.out_channels, stream):
                        raise BackendError(lib().shf_conv_last_error().decode())
                    s, t = bn_affine(cv, bn)
                    layers.append((pack, self._put((name, i, "s"), s.float(), dev), self._put((name, i, "t"), t.float(), dev),
                                   cv.in_channels, cv.out_channels, w))
                self._conv[name] = layers
            # the decoders side by side: layer l of all of them as one block-diagonal Linear
            decs = list(m.decoders.values())
            chains = [[blk[0] for blk in d.lin_decoder] + [d.fc[0]] for d in decs]
            self._dec = []
            for l in range(len(chains[0])):
                lins = [c[l] for c in chains]
                n_out = sum(x.out_features for x in lins)
                if l == 0:
                    wt = torch.cat([x.weight.detach().float() for x in lins], 0)
                else:
                    wt = torch.zeros(n_out, sum(x.in_features for x in lins), device=dev)
                    r = c0 = 0
                    for x in lins:
                        wt[r:r + x.out_features, c0:c0 + x.in_features] = x.weight.detach().float()
                        r += x.out_features; c0 += x.in_features
                bs = torch.cat([x.bias.detach().float() if x.bias is not None else torch.zeros(x.out_features, device=dev) for x in lins])
                self._dec.append((self._put(("dec", l, "w"), wt, dev), self._put(("dec", l, "b"), bs, dev),
                                  _abi.ACT_RELU if l + 1 < len(chains[0]) else _abi.ACT_NONE))
            self._dec_widths = [c[-1].out_features for c in chains]
        self._packed_key = self._key()

    def _fresh(self):
        if self._packed_key is None or self._packed_key != self._key():
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("fused inference: the weights have to be packed, which synchronises with the host and cannot "
                                   "be captured; call the model once before the capture")
            self._pack()

    # ---- launches ------------------------------------------------------------------------------------------------------------
    def _buf(self, n, slot, numel, dev):
        ws = self._ws.setdefault((n, str(dev)), {})
        b = ws.get(slot)
        if b is None or b.numel() < numel:
            b = ws[slot] = torch.empty(numel, dtype=torch.float32, device=dev)
        return b

    def _linear(self, x, ldx, w, b, y, ldy, rows, act, stream):
        n_out, n_in = w.shape
        if lib().shf_mlp_linear_forward_ld(_ptr(x), ldx, _ptr(w), _ptr(b) if b is not None else None, _ptr(y), ldy, rows, n_in, n_out,
                                           act, stream):
            raise BackendError(lib().shf_mlp_last_error().decode())
        self.launches += 1

    def _run(self, inputs):
        m = self.model
        missing = [k for k in m.encoders if k not in inputs]
        if missing:
            raise ValueError(f"fused inference needs every modality; missing {missing}")
        self._fresh()
        first = next(iter(inputs.values()))
        n, dev = first.t.shape[0], first.t.device
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        self.launches = 0
        L = m.latent_dim
        width = len(m.encoders) * L
        stack = self._buf(n, "stack", n * width, dev)
        for name, enc in m.encoders.items():
            src = inputs[name]
            if src.t.shape[0] != n or src.t.device != dev:
                raise ValueError("fused inference: the modalities differ in batch size or device")
            layers = self._conv[name]
            if src.c != layers[0][3]:
                raise ValueError(f"{name}: {src.c} input channels, the encoder takes {layers[0][3]}")
            x, kind, strides, h, w = src.t, src.kind, src.strides, src.h, src.w
            for i, (pack, s, t, cin, cout, _) in enumerate(layers):
                if h % 2 or w % 2:
                    raise ValueError(f"{name}: layer {i} input {h} x {w} is not even")
                last = i + 1 == len(layers)
                y = self._buf(n, "act%d" % (i & 1), n * (h // 2) * (w // 2) * cout, dev)
                st = (C.c_int64 * 4)(*strides)
                if lib().shf_conv3x3s2_forward(_ptr(x), kind, st, _ptr(pack), _ptr(s), _ptr(t), _ptr(y), 1 if last else 0, n, cin, h, w,
                                               cout, stream):
                    raise BackendError(lib().shf_conv_last_error().decode())
                self.launches += 1
                h, w = h // 2, w // 2
                x, kind, strides = y, _abi.CONV_SRC_F32, (h * w * cout, 1, w * cout, cout)
            mid = h * w * layers[-1][4]
            fc0, fc2 = enc.fc[0], enc.fc[2]
            if mid != fc0.in_features:
                raise ValueError(f"{name}: the conv stack ends at {layers[-1][4]} x {h} x {w} = {mid} features, fc.0 takes {fc0.in_features}")
            hid = self._buf(n, "hid", n * fc0.out_features, dev)
            self._linear(x, mid, fc0.weight, fc0.bias, hid, fc0.out_features, n, _abi.ACT_RELU, stream)
            p = m.position_dict[name]
            self._linear(hid, fc0.out_features, fc2.weight, fc2.bias, stack[p * L:], width, n, _abi.ACT_NONE, stream)
        fm = m.fusion_module
        z = self._buf(n, "z", n * L, dev)
        self._linear(stack, width, fm.weight, fm.bias, z, L, n, _abi.ACT_NONE, stream)
        x, ldx = z, L
        for i, (wt, bs, act) in enumerate(self._dec):
            last = i + 1 == len(self._dec)
            y = torch.empty(n, wt.shape[0], dtype=torch.float32, device=dev) if last else self._buf(n, "dec%d" % (i & 1), n * wt.shape[0], dev)
            self._linear(x, ldx, wt, bs, y, wt.shape[0], n, act, stream)
            x, ldx = y, wt.shape[0]
        out, c0 = {}, 0
        for name, wd in zip(m.decoders, self._dec_widths):
            out[name] = x[:, c0:c0 + wd]
            c0 += wd
        return out

    def __call__(self, joint_dict):
        """{'rgb': (N, 3, H, W), 'depth': (N, 1, H, W)} float32 GPU tensors of any strides -> {decoder name: (N, d)}."""
        inputs = {}
        for name, x in joint_dict.items():
            if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
                raise TypeError(f"fused inference: {name} must be a float32 (N, C, H, W) tensor on the GPU")
            inputs[name] = _Input(x, _abi.CONV_SRC_F32, tuple(x.stride()), x.shape[1], x.shape[2], x.shape[3])
        return self._run(inputs)

    def from_camera(self, camera_sensor):
        """The same forward straight from a CameraSensor's image group (rgba u8 and depth, as rendered): equals
        __call__({'rgb': color_buf.permute(0, 3, 1, 2), 'depth': depth_buf.unsqueeze(1)}) of a sensor with
        image_normalization bit for bit, without the normalise / negate copies.  A fused env's camera
        (gym/fused_camera.py) has no converted buffers and no such setting: only its raw_images() are read."""
        cfg = getattr(camera_sensor, "cfg", None)
        if cfg is not None and not cfg.image_normalization:
            raise ValueError("from_camera reads colors as [0, 1] floats and depth as positive distance, which is what a "
                             "CameraSensor with image_normalization gives; this sensor has it off")
        im = camera_sensor.raw_images()
        rgba, depth = im["rgba"], im["depth"]
        if set(self.model.encoders) != {"rgb", "depth"}:
            raise ValueError("from_camera needs exactly the 'rgb' and 'depth' encoders")
        if not (rgba.dtype == torch.uint8 and rgba.dim() == 4 and rgba.shape[3] == 4 and rgba.is_contiguous() and
                depth.dtype == torch.float32 and depth.dim() == 3 and depth.is_contiguous()):
            raise TypeError("from_camera: expected the camera group's rgba (N, H, W, 4) u8 and depth (N, H, W) f32 images")
        n, h, w, _ = rgba.shape
        return self._run({"rgb": _Input(rgba, _abi.CONV_SRC_U8_UNORM, (h * w * 4, 1, w * 4, 4), 3, h, w),
                          "depth": _Input(depth, _abi.CONV_SRC_F32_NEG, (h * w, 0, w, 1), 1, h, w)})
