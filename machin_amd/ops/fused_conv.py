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


class _BiasReLUFn(t.autograd.Function):
    """In place on a bias-free conv output: y = relu(y + bias)."""

    @staticmethod
    def forward(ctx, y: t.Tensor, bias: t.Tensor):
        ext = _require_ext()
        ext.bias_relu_(_rows_view(y), bias.detach().float().contiguous())
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
            _rows_view(y), bias.detach().float().contiguous(), N
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
    out = F.relu(y + bias.to(y.dtype).view(1, -1, 1, 1))
    return out.flatten(1) if flatten else out


class ConvBiasReLU2d(nn.Conv2d):
    """``nn.Conv2d`` followed by ReLU, with the bias add, the ReLU and
    their backward fused into one pass each way (see
    :func:`bias_relu`). Same parameters, names and initialisation as
    ``nn.Conv2d``. With ``flatten=True`` the module returns the
    flattened ``[N, C*H*W]`` activation (a following ``nn.Flatten`` is
    then a no-op)."""

    def __init__(self, *args, flatten: bool = False, **kwargs):
        super().__init__(*args, **kwargs)
        self.flatten = flatten

    def forward(self, x: t.Tensor) -> t.Tensor:
        if self.padding_mode != "zeros" or self.bias is None:
            out = F.relu(super().forward(x))
            return out.flatten(1) if self.flatten else out
        y = F.conv2d(x, self.weight, None, self.stride, self.padding,
                     self.dilation, self.groups)
        return bias_relu(y, self.bias, self.flatten)
