"""Fused Atari conv stack pieces: the u8 stem conv with hand-written
gfx950 forward and weight-gradient kernels, and a conv + bias + ReLU
module for the layers MIOpen runs.

The IMPALA/APEX learner's dominant kernel is the weight gradient of
Conv2d(4, 32, 8, stride=4) — a skinny reduction GEMM MIOpen runs at
~2% MFMA efficiency (profiles/). :class:`FusedAtariConv1` computes:

* forward: u8 frames -> im2col dequant + MFMA GEMM + bias in one
  kernel (``ops/hip/conv1_wrw.hip``), x read ONCE as uint8;
* backward: grad_weight and grad_bias by the MFMA split-K kernel in
  the same file (im2col rows assembled straight from the u8 frames);
  grad_input skipped (frames are data).

With ``relu=True`` the activation is fused into both kernels: the
forward epilogue stores ``relu(bf16(acc + bias))`` — the same bits as
``torch.relu`` of the plain output — plus one 32-bit word per output
row whose bit ``c`` says whether channel ``c`` is positive (32 output
channels = exactly one word; 4 bytes per 64-byte row). The
weight-gradient kernel takes that packed mask and zeroes the incoming
gradient where the bit is clear as it loads it, so neither the
un-activated 1 GB tensor, nor the ReLU pass, nor the
``threshold_backward`` pass over it ever touches HBM.

:class:`ConvBiasReLU2d` does the same for a MIOpen conv: the conv runs
without bias, then ONE in-place kernel adds the bias and applies the
ReLU (``ops/hip/bias_act.hip``), and in backward ONE kernel applies
the ReLU mask and sums the bias gradient deterministically — instead of
``add_`` + ``relu_`` forward and ``threshold_backward`` + a bf16
``sum`` backward, four passes over the activation.
"""
import os

import torch as t
import torch.nn as nn
import torch.nn.functional as F

from . import _load_ext, _require_ext, dequant_u8  # noqa: F401


def _stem_kernels_fuse_relu() -> bool:
    # the activation is fused into the v3 and v4 kernels only; the retired
    # v1/v2 kernels (MACHIN_CONV1_V=1|2) keep the unfused composition
    return os.environ.get("MACHIN_CONV1_V", "4") not in ("1", "2")


class _FusedConv1Fn(t.autograd.Function):
    @staticmethod
    def forward(ctx, frames_u8: t.Tensor, weight: t.Tensor,
                bias: t.Tensor, scale: float, relu: bool = False):
        # frames_u8: [B, 4, 84, 84] channels_last uint8
        ext = _require_ext()
        B = frames_u8.shape[0]
        nhwc = frames_u8.permute(0, 2, 3, 1).contiguous()
        # patch-major weight repack: n = r*32 + c*4 + ci
        w_rs = (
            weight.permute(2, 3, 1, 0).reshape(256, 32)
            .to(t.bfloat16).contiguous()
        )
        bias_f = (
            bias.float().contiguous() if bias is not None
            else t.empty(0, device=frames_u8.device)
        )
        if relu:
            y_rows, mask = ext.conv1_fwd_relu(nhwc, w_rs, bias_f, scale)
            ctx.save_for_backward(frames_u8, weight, mask)
        else:
            y_rows = ext.conv1_fwd(nhwc, w_rs, bias_f, scale)
            ctx.save_for_backward(frames_u8, weight)
        # [K,32] IS the NHWC image; permute -> channels_last NCHW
        y = y_rows.view(B, 20, 20, 32).permute(0, 3, 1, 2)
        ctx.scale = scale
        ctx.has_bias = bias is not None
        ctx.relu = relu
        return y

    @staticmethod
    def backward(ctx, gy: t.Tensor):
        ext = _require_ext()
        gy_cl = gy.contiguous(memory_format=t.channels_last)
        dy_rows = gy_cl.permute(0, 2, 3, 1).reshape(-1, 32)
        dy_rows = dy_rows.to(t.bfloat16).contiguous()
        if ctx.relu:
            frames_u8, weight, mask = ctx.saved_tensors
        else:
            frames_u8, weight = ctx.saved_tensors
        # channels_last u8 frames: permute exposes the NHWC memory as
        # a standard-contiguous view (no copy)
        frames_nhwc = frames_u8.permute(0, 2, 3, 1).contiguous()
        if ctx.relu:
            # gy is the gradient w.r.t. the ACTIVATED output; the
            # kernel applies the ReLU mask as it loads it
            grad_w, grad_b = ext.conv1_wrw_masked(
                dy_rows, mask, frames_nhwc, ctx.scale
            )
        else:
            grad_w, grad_b = ext.conv1_wrw(
                dy_rows, frames_nhwc, ctx.scale
            )
        grad_w = grad_w.to(weight.dtype)
        if not ctx.has_bias:
            grad_b = None
        return None, grad_w, grad_b, None, None


class FusedAtariConv1(nn.Module):
    """Drop-in for the Atari stem conv, consuming RAW uint8 frames
    (channels_last) and emitting bf16 activations.

    ``relu=True`` returns ``relu(conv(x) + bias)`` with the activation
    fused into the forward epilogue and its backward into the
    weight-gradient kernel's load, through a packed sign mask (one
    int32 per output pixel, bit ``c`` = channel ``c`` positive) saved
    for backward in place of the activation. The output is bit-equal to
    ``torch.relu`` of the ``relu=False`` output. With the retired
    kernels selected (``MACHIN_CONV1_V`` = 1 or 2) the same result is
    computed as the unfused stem followed by ``torch.relu``."""

    def __init__(self, scale: float = 1.0 / 255.0, relu: bool = False):
        super().__init__()
        ref = nn.Conv2d(4, 32, 8, stride=4)
        self.weight = nn.Parameter(ref.weight.detach().clone())
        self.bias = nn.Parameter(ref.bias.detach().clone())
        self.scale = scale
        self.relu = relu

    def forward(self, frames_u8: t.Tensor) -> t.Tensor:
        if self.relu and not _stem_kernels_fuse_relu():
            return t.relu(_FusedConv1Fn.apply(
                frames_u8, self.weight, self.bias, self.scale, False
            ))
        return _FusedConv1Fn.apply(
            frames_u8, self.weight, self.bias, self.scale, self.relu
        )


def _rows_view(x: t.Tensor) -> t.Tensor:
    """[N*H*W, C] view of a channels-last [N, C, H, W] tensor (shares
    storage; ``view`` raises instead of copying)."""
    return x.permute(0, 2, 3, 1).view(-1, x.shape[1])


def _bias_relu_eligible(y: t.Tensor) -> bool:
    return (
        y.is_cuda
        and y.dtype == t.bfloat16
        and y.dim() == 4
        and y.shape[1] % 8 == 0
        and 8 <= y.shape[1] <= 2048
        and y.numel() > 0
        and y.is_contiguous(memory_format=t.channels_last)
        and y.data_ptr() % 16 == 0
        and _load_ext() is not None
    )


def _bias_f32(bias: t.Tensor) -> t.Tensor:
    """The bias as the kernels take it: fp32, contiguous and 16-byte
    aligned. An fp32 parameter that is a view into a larger buffer (a
    flat parameter buffer, a slice) comes through ``float()`` and
    ``contiguous()`` as the same storage at the same offset, so a
    misaligned one is copied."""
    b = bias.detach().float().contiguous()
    return b if b.data_ptr() % 16 == 0 else b.clone()


class _BiasReLUFn(t.autograd.Function):
    """In place on a bias-free conv output: y = relu(y + bias)."""

    @staticmethod
    def forward(ctx, y: t.Tensor, bias: t.Tensor):
        ext = _require_ext()
        ext.bias_relu_(_rows_view(y), _bias_f32(bias))
        ctx.mark_dirty(y)
        ctx.save_for_backward(y)
        ctx.bias_dtype = bias.dtype
        return y

    @staticmethod
    def backward(ctx, gy: t.Tensor):
        (y,) = ctx.saved_tensors
        ext = _require_ext()
        gy_cl = gy.to(t.bfloat16).contiguous(
            memory_format=t.channels_last
        )
        gx_rows, grad_b = ext.bias_relu_bwd(
            _rows_view(gy_cl), _rows_view(y)
        )
        N, C, H, W = y.shape
        gx = gx_rows.view(N, H, W, C).permute(0, 3, 1, 2)
        return gx, grad_b.to(ctx.bias_dtype)


class _BiasReLUFlatFn(t.autograd.Function):
    """relu(y + bias) of a bias-free conv output, returned as the
    flattened [N, C*H*W] matrix nn.Flatten would make of it."""

    @staticmethod
    def forward(ctx, y: t.Tensor, bias: t.Tensor):
        ext = _require_ext()
        N, C, H, W = y.shape
        out = ext.bias_relu_flat(
            _rows_view(y), _bias_f32(bias), N
        )
        ctx.save_for_backward(out)
        ctx.shape = (N, C, H, W)
        ctx.bias_dtype = bias.dtype
        return out

    @staticmethod
    def backward(ctx, gy: t.Tensor):
        (out,) = ctx.saved_tensors
        ext = _require_ext()
        N, C, H, W = ctx.shape
        gx_rows, grad_b = ext.bias_relu_flat_bwd(
            gy.to(t.bfloat16).contiguous(), out, C
        )
        gx = gx_rows.view(N, H, W, C).permute(0, 3, 1, 2)
        return gx, grad_b.to(ctx.bias_dtype)


def bias_relu(y: t.Tensor, bias: t.Tensor,
              flatten: bool = False) -> t.Tensor:
    """``relu(y + bias[None, :, None, None])`` for a conv output ``y``.

    A CUDA bf16 channels-last ``y`` with C % 8 == 0 is updated IN PLACE
    by one gfx950 kernel (and differentiated by one more, which also
    produces the bias gradient, deterministically); the bias is rounded
    to bf16 first and the sum is rounded to bf16 before the ReLU, which
    is what ``F.conv2d`` with a bias computes under bf16 autocast.
    Anything else takes plain torch ops with the same semantics.

    ``flatten=True`` returns ``relu(...).flatten(1)`` instead, the
    ``[N, C*H*W]`` matrix a following ``nn.Flatten`` would produce. On
    the kernel path it is written directly in that (NCHW) order and
    the backward reads the NCHW gradient directly, which saves the
    layout copies ``Flatten`` costs around a channels-last tensor."""
    if _bias_relu_eligible(y):
        if not flatten:
            return _BiasReLUFn.apply(y, bias)
        if y.shape[1] * y.shape[2] * y.shape[3] <= 32768:
            return _BiasReLUFlatFn.apply(y, bias)
        return _BiasReLUFn.apply(y, bias).flatten(1)
    # threshold, not relu: ``s <= 0 ? +0 : s`` is the kernels' ReLU on
    # every value (NaN kept, -0 -> +0); ATen's CPU relu returns -0 for
    # -0. Its backward is relu's, threshold_backward.
    out = F.threshold(y + bias.to(y.dtype).view(1, -1, 1, 1), 0.0, 0.0)
    return out.flatten(1) if flatten else out


_CONV_IMPLS = ("miopen", "hip", "hip_wrw")


def _igemm_weights(weight: t.Tensor, stride: int):
    """The two repacks the implicit-GEMM kernels read, both with the
    reduction index last, running (tap row, tap column, channel) as the
    resident image does.

    Forward: ``[Cout, KH*KW*Cin]``. Data gradient: one slice per parity
    class ``(py, px)`` of the input pixel, ``[S*S, Cin, T*T*Cout]`` with
    ``T = KH / S``; window position ``(j, i)`` of class ``(py, px)`` is
    the tap ``(py + S (T-1-j), px + S (T-1-i))``."""
    cout, cin, kh, kw = weight.shape
    w = weight.detach().to(t.bfloat16)
    w_fwd = w.permute(0, 2, 3, 1).reshape(cout, kh * kw * cin).contiguous()
    tt = kh // stride
    w_bwd = (
        w.reshape(cout, cin, tt, stride, tt, stride).flip(2, 4)
        .permute(3, 5, 1, 2, 4, 0)
        .reshape(stride * stride, cin, tt * tt * cout).contiguous()
    )
    return w_fwd, w_bwd


class _ConvBiasReLUIgemmFn(t.autograd.Function):
    """relu(conv(x, weight) + bias) by the implicit-GEMM kernels
    (``ops/hip/conv_igemm.hip``): forward and input gradient hand-written,
    ReLU mask and bias gradient by the bias+ReLU backward kernels on the
    saved activation, weight gradient by ATen."""

    @staticmethod
    def forward(ctx, x: t.Tensor, weight: t.Tensor, bias: t.Tensor,
                stride: int, flatten: bool):
        ext = _require_ext()
        N, _, H, W = x.shape
        cout, _, k, _ = weight.shape
        w_fwd, w_bwd = _igemm_weights(weight, stride)
        out = ext.conv_igemm_fwd(
            x.permute(0, 2, 3, 1), w_fwd, _bias_f32(bias), k, stride,
            flatten,
        )
        OH, OW = (H - k) // stride + 1, (W - k) // stride + 1
        if not flatten:
            out = out.view(N, OH, OW, cout).permute(0, 3, 1, 2)
        ctx.save_for_backward(x, weight, w_bwd, out)
        ctx.geom = (k, stride, flatten, OH, OW)
        ctx.bias_dtype = bias.dtype
        return out

    @staticmethod
    def backward(ctx, gy: t.Tensor):
        return _igemm_backward(ctx, gy, False)


class _ConvBiasReLUIgemmWrwFn(_ConvBiasReLUIgemmFn):
    """:class:`_ConvBiasReLUIgemmFn` with the weight gradient hand-written
    too (``ops/hip/conv_igemm_wrw.hip``): fp32 sums in a fixed order over
    the masked bf16 gradient, rounded once."""

    @staticmethod
    def backward(ctx, gy: t.Tensor):
        return _igemm_backward(ctx, gy, True)


def _igemm_backward(ctx, gy: t.Tensor, hand_wrw: bool):
    ext = _require_ext()
    x, weight, w_bwd, out = ctx.saved_tensors
    k, stride, flatten, OH, OW = ctx.geom
    N, _, H, W = x.shape
    cout = weight.shape[0]
    if flatten:
        g_rows, grad_b = ext.bias_relu_flat_bwd(
            gy.to(t.bfloat16).contiguous(), out, cout
        )
    else:
        gy_cl = gy.to(t.bfloat16).contiguous(
            memory_format=t.channels_last
        )
        g_rows, grad_b = ext.bias_relu_bwd(
            _rows_view(gy_cl), _rows_view(out)
        )
    g = g_rows.view(N, OH, OW, cout)
    dx = dw = None
    if ctx.needs_input_grad[0]:
        dx = ext.conv_igemm_bwd_data(
            g, w_bwd, k, stride, H, W
        ).permute(0, 3, 1, 2)
    if ctx.needs_input_grad[1] and hand_wrw:
        dw = ext.conv_igemm_wrw(g, x.permute(0, 2, 3, 1), k, stride)
    elif ctx.needs_input_grad[1]:
        dw = t.ops.aten.convolution_backward(
            g.permute(0, 3, 1, 2), x, weight, None, [stride, stride],
            [0, 0], [1, 1], False, [0, 0], 1, [False, True, False],
        )[1]
    return dx, dw, grad_b.to(ctx.bias_dtype), None, None


class ConvBiasReLU2d(nn.Conv2d):
    """``nn.Conv2d`` followed by ReLU, with the bias add, the ReLU and
    their backward fused into one pass each way (see
    :func:`bias_relu`). Same parameters, names and initialisation as
    ``nn.Conv2d``. With ``flatten=True`` the module returns the
    flattened ``[N, C*H*W]`` activation (a following ``nn.Flatten`` is
    then a no-op).

    ``impl`` chooses who runs the convolution. ``"miopen"`` is the
    composition above. ``"hip"`` runs the forward, with the bias and
    the ReLU in its epilogue, and the input gradient as hand-written
    gfx950 implicit-GEMM kernels when the call is eligible: a CUDA
    bf16 (or bf16-autocast) channels-last 16-byte aligned input, no
    padding, dilation or groups, one of the two Nature geometries
    (32 -> 64, 4x4, stride 2; 64 -> 64, 3x3, stride 1), an image small
    enough for the kernels' LDS buffers, extension loaded. Any other
    call takes the ``"miopen"`` path. ``"hip_wrw"`` is ``"hip"`` plus
    the weight gradient as a hand-written kernel too
    (``ops/hip/conv_igemm_wrw.hip``: fp32 sums in a fixed order, no
    atomics, one rounding) where the image also fits that kernel's
    buffers; a call eligible for ``"hip"`` only runs exactly as
    ``"hip"``. ``None`` reads the environment variable
    ``MACHIN_CONV_IMPL`` at call time (default ``"miopen"``).

    The two paths do not round alike. ``"hip"`` computes
    ``relu(bf16(acc + bias))`` with the fp32 accumulator and the fp32
    bias, ONE rounding, as the stem does; ``"miopen"`` computes
    ``relu(bf16(bf16(conv) + bf16(bias)))``, what ``F.conv2d`` with a
    bias gives under bf16 autocast. That is why ``"hip"`` is opt-in."""

    def __init__(self, *args, flatten: bool = False, impl=None, **kwargs):
        super().__init__(*args, **kwargs)
        if impl is not None and impl not in _CONV_IMPLS:
            raise ValueError(
                f"impl must be None or one of {_CONV_IMPLS}, got {impl!r}"
            )
        self.flatten = flatten
        self.impl = impl

    def _igemm_input(self, x: t.Tensor):
        """``(x, weight)`` as the implicit-GEMM path takes them, or None
        when the call is not eligible."""
        if not (x.is_cuda and x.dim() == 4 and x.shape[0] > 0
                and self.padding == (0, 0) and self.dilation == (1, 1)
                and self.groups == 1
                and self.kernel_size[0] == self.kernel_size[1]
                and self.stride[0] == self.stride[1]):
            return None
        weight = self.weight
        if t.is_autocast_enabled("cuda") and \
                t.get_autocast_dtype("cuda") == t.bfloat16:
            # the casts ATen's autocast makes in front of a convolution
            x, weight = x.to(t.bfloat16), weight.to(t.bfloat16)
        ext = _load_ext()
        if not (ext is not None
                and x.dtype == t.bfloat16 and weight.dtype == t.bfloat16
                and x.is_contiguous(memory_format=t.channels_last)
                and x.data_ptr() % 16 == 0
                and ext.conv_igemm_fits(
                    self.in_channels, self.out_channels,
                    self.kernel_size[0], self.stride[0],
                    x.shape[2], x.shape[3])):
            return None
        return x, weight

    def forward(self, x: t.Tensor) -> t.Tensor:
        impl = self.impl
        if impl is None:
            impl = os.environ.get("MACHIN_CONV_IMPL", "miopen")
            if impl not in _CONV_IMPLS:
                raise ValueError(
                    f"MACHIN_CONV_IMPL must be one of {_CONV_IMPLS}, "
                    f"got {impl!r}"
                )
        if self.padding_mode != "zeros" or self.bias is None:
            out = F.relu(super().forward(x))
            return out.flatten(1) if self.flatten else out
        if impl != "miopen":
            args = self._igemm_input(x)
            if args is not None:
                fn = _ConvBiasReLUIgemmFn
                if impl == "hip_wrw" and _load_ext().conv_igemm_wrw_fits(
                        self.in_channels, self.out_channels,
                        self.kernel_size[0], self.stride[0],
                        x.shape[2], x.shape[3]):
                    fn = _ConvBiasReLUIgemmWrwFn
                return fn.apply(
                    args[0], args[1], self.bias, self.stride[0],
                    self.flatten,
                )
        y = F.conv2d(x, self.weight, None, self.stride, self.padding,
                     self.dilation, self.groups)
        return bias_relu(y, self.bias, self.flatten)
