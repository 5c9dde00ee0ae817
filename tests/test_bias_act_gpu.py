"""The five fused bias + ReLU kernels
(``machin_amd/ops/hip/bias_act.hip``) against the plain reference of
``util_bias_act`` and the ATen composition on the device.

A. Forward on every bf16 value against a bias table of edges: bit-equal
   to ATen everywhere, and to the IEEE reference wherever the fp32 sum
   is not subnormal (zero results compared without their sign; what the
   device does there is printed and pinned to ATen).
B. Backward mask on every bf16 activation value, with gradients that
   include +-0, +-inf and NaN.
C. Bias gradient on integer inputs whose sums are exact in fp32 and in
   bf16: the kernel must equal the float64 sum, so one lost, repeated or
   misattributed row shows. Channel counts from 8 to 2048, row counts
   around one pass of a block, the capped grids, no rows at all.
D. Bias gradient on ``randn`` inputs inside the any-order fp32 summation
   bound, rounded monotonically (``util_bias_act.grad_interval``).
E. The bindings reject what the kernels cannot take.
F. ``ConvBiasReLU2d`` / ``bias_relu``: a bias parameter that is a
   misaligned view, a misaligned activation, fp32 and NCHW gradients.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch as t
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not t.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import util_bias_act as U  # noqa: E402

DEV = "cuda:0"
GUARD = 0x7B7B  # fill of guard elements, as a bit pattern


def _ext():
    from machin_amd.ops import _require_ext

    return _require_ext()


def dev_bf16(bits):
    """uint16 patterns -> bf16 tensor on the device (a copy)."""
    return t.from_numpy(bits.view(np.int16)).to(DEV).view(t.bfloat16)


def host_bits(x):
    return x.contiguous().view(t.int16).cpu().numpy().view(np.uint16)


def dev_f32(x):
    return t.from_numpy(np.array(x, dtype=np.float32)).to(DEV)


def rows_of_flat(flat, C):
    """[N, C*HW] device tensor -> the NHWC rows [N*HW, C] (ATen ops)."""
    N = flat.shape[0]
    return flat.view(N, C, -1).permute(0, 2, 1).reshape(-1, C)


def flat_of_rows(rows, N):
    C = rows.shape[1]
    return rows.view(N, -1, C).permute(0, 2, 1).reshape(N, -1)


# ---- A. forward, every bf16 value ---------------------------------------
@functools.lru_cache(maxsize=None)
def forward_table_device():
    """Device inputs of the forward table and the ATen composition
    (autocast's bf16 bias, ``add_``, ``relu``) as patterns. Shared."""
    y_bits, bias, _, _ = U.table_forward()
    y = dev_bf16(y_bits)
    b = dev_f32(bias)
    aten = t.relu(y.clone().add_(b.to(t.bfloat16).view(1, -1)))
    return y, b, host_bits(aten)


def check_forward_table(got, aten, what, flat_n=None):
    """``got``/``aten`` patterns in the kernel's output layout."""
    _, bias, s, ref = U.table_forward()
    if flat_n is not None:
        s, ref = U.rows_to_flat(s, flat_n), U.rows_to_flat(ref, flat_n)
    sub = U.subnormal_f32(s)
    zero = (ref == 0) & ~sub
    unsigned = np.where((got & 0x7FFF) == 0, U.POS_ZERO, got)
    sub_ieee = (got[sub] == ref[sub]).sum()
    neg_zero = (got[zero] == U.NEG_ZERO).sum()
    print(f"{what}: {sub.sum()} subnormal fp32 sums, {sub_ieee} of them "
          f"equal to the IEEE reference; {zero.sum()} zero results, "
          f"{neg_zero} of them -0 (reference: +0)")
    # every element, the sign of a zero included
    U.assert_same_bits(got, aten, f"{what} against ATen")
    ok = ~sub
    U.assert_same_bits(np.where(ok, unsigned, 0), np.where(ok, ref, 0),
                       f"{what} against the reference")
    # what was observed on an MI355X and is written in the kernel header
    assert sub_ieee == sub.sum(), "subnormal sums are not flushed"
    assert neg_zero == 0, "a zero result is +0"


class TestForwardEveryValue:
    def test_rows_in_place_with_guard_row(self):
        ext = _ext()
        y, bias, aten = forward_table_device()
        R, C = y.shape
        buf = t.full((R + 1, C), GUARD, dtype=t.int16, device=DEV)
        out = buf.view(t.bfloat16)[:R]
        out.copy_(y)
        assert out.data_ptr() % 16 == 0 and out.is_contiguous()
        ext.bias_relu_(out, bias)
        assert (buf[R] == GUARD).all(), "guard row written"
        check_forward_table(host_bits(out), aten, "bias_relu_")

    def test_flat_at_the_lds_limit(self):
        ext = _ext()
        y, bias, aten = forward_table_device()
        N, C, HW = U.TABLE_N, U.TABLE_C, U.TABLE_HW
        assert C * HW == 32768
        before = y.clone()
        out = ext.bias_relu_flat(y, bias, N)
        assert out.shape == (N, C * HW) and out.dtype == t.bfloat16
        assert t.equal(y.view(t.int16), before.view(t.int16)), "input kept"
        aten_flat = host_bits(flat_of_rows(dev_bf16(aten), N))
        check_forward_table(host_bits(out), aten_flat, "bias_relu_flat",
                            flat_n=N)


# ---- B. backward mask, every activation value ---------------------------
N_NONFINITE = 8  # channels of util_bias_act.edge_gy that are not finite


def check_table_grad(gb, what):
    _, _, gx_ref, gb_ref = U.table_backward()
    got = gb.cpu().double().numpy()
    k = N_NONFINITE
    assert not np.isfinite(gb_ref[:k]).any()
    assert np.isfinite(gb_ref[k:]).all()
    assert np.array_equal(np.isnan(got[:k]), np.isnan(gb_ref[:k]))
    assert np.array_equal(np.isinf(got[:k]), np.isinf(gb_ref[:k]))
    inf = np.isinf(gb_ref[:k])
    assert np.array_equal(np.sign(got[:k][inf]), np.sign(gb_ref[:k][inf]))
    U.check_grad_interval(got[k:], gx_ref[:, k:], what)


class TestBackwardEveryValue:
    def test_rows(self):
        ext = _ext()
        gy_bits, act_bits, gx_ref, _ = U.table_backward()
        gy, act = dev_bf16(gy_bits), dev_bf16(act_bits)
        gx, gb = ext.bias_relu_bwd(gy, act)
        assert gx.shape == gy.shape and gx.dtype == t.bfloat16
        assert gb.shape == (U.TABLE_C,) and gb.dtype == t.float32
        aten = t.ops.aten.threshold_backward(gy, act, 0)
        U.assert_same_bits(host_bits(gx), gx_ref, "gx against reference")
        U.assert_same_bits(host_bits(gx), host_bits(aten), "gx against ATen")
        check_table_grad(gb, "bias grad, every activation value")

    def test_flat(self):
        ext = _ext()
        gy_bits, act_bits, gx_ref, _ = U.table_backward()
        N, C = U.TABLE_N, U.TABLE_C
        gy = dev_bf16(U.rows_to_flat(gy_bits, N))
        act = dev_bf16(U.rows_to_flat(act_bits, N))
        gx, gb = ext.bias_relu_flat_bwd(gy, act, C)
        assert gx.shape == gx_ref.shape and gb.shape == (C,)
        aten = rows_of_flat(t.ops.aten.threshold_backward(gy, act, 0), C)
        U.assert_same_bits(host_bits(gx), gx_ref, "gx against reference")
        U.assert_same_bits(host_bits(gx), host_bits(aten), "gx against ATen")
        check_table_grad(gb, "flat bias grad, every activation value")


# ---- C. exact bias gradient ---------------------------------------------
class TestExactBiasGradient:
    @pytest.mark.parametrize("R,C", U.EXACT_ROW_SHAPES)
    def test_rows(self, R, C):
        ext = _ext()
        gy_bits, act_bits = U.exact_case(R, C)
        gx_ref, total = U.exact_preconditions(gy_bits, act_bits)
        gy, act = dev_bf16(gy_bits), dev_bf16(act_bits)
        gx, gb = ext.bias_relu_bwd(gy, act)
        got = gb.cpu().double().numpy()
        assert np.array_equal(got, total), (
            f"channels {np.nonzero(got != total)[0][:8]}: "
            f"{got[got != total][:8]} != {total[got != total][:8]}")
        assert np.array_equal(host_bits(gx), gx_ref)
        gx2, gb2 = ext.bias_relu_bwd(gy, act)
        assert t.equal(gx.view(t.int16), gx2.view(t.int16))
        assert t.equal(gb.view(t.int32), gb2.view(t.int32))

    @pytest.mark.parametrize("N,C,HW", U.EXACT_FLAT_SHAPES)
    def test_flat(self, N, C, HW):
        ext = _ext()
        gy_bits, act_bits = U.exact_case(N * HW, C)
        gx_ref, total = U.exact_preconditions(gy_bits, act_bits)
        gy = dev_bf16(U.rows_to_flat(gy_bits, N))
        act = dev_bf16(U.rows_to_flat(act_bits, N))
        gx, gb = ext.bias_relu_flat_bwd(gy, act, C)
        got = gb.cpu().double().numpy()
        assert np.array_equal(got, total), (
            f"channels {np.nonzero(got != total)[0][:8]}: "
            f"{got[got != total][:8]} != {total[got != total][:8]}")
        assert gx.shape == (N * HW, C)
        assert np.array_equal(host_bits(gx), gx_ref)
        gx2, gb2 = ext.bias_relu_flat_bwd(gy, act, C)
        assert t.equal(gx.view(t.int16), gx2.view(t.int16))
        assert t.equal(gb.view(t.int32), gb2.view(t.int32))

    @pytest.mark.parametrize("C", [8, 64, 2048])
    def test_no_rows(self, C):
        ext = _ext()
        y = t.empty(0, C, dtype=t.bfloat16, device=DEV)
        ext.bias_relu_(y, t.ones(C, device=DEV))
        gx, gb = ext.bias_relu_bwd(y, y.clone())
        assert gx.shape == (0, C) and gx.dtype == t.bfloat16
        assert gb.shape == (C,)
        assert t.equal(gb.view(t.int32), t.zeros_like(gb).view(t.int32))


# ---- D. rounding bound on ordinary inputs -------------------------------
class TestRoundingBound:
    @pytest.mark.parametrize("R,C", U.ROUND_ROW_SHAPES)
    def test_rows(self, R, C):
        ext = _ext()
        y_bits, bias, gy_bits = U.random_case(R, C)
        act_ref = U.forward(y_bits, bias)
        gx_ref, _ = U.backward(gy_bits, act_ref)
        act = dev_bf16(y_bits)
        ext.bias_relu_(act, dev_f32(bias))
        assert np.array_equal(host_bits(act), act_ref)
        gx, gb = ext.bias_relu_bwd(dev_bf16(gy_bits), act)
        assert np.array_equal(host_bits(gx), gx_ref)
        U.check_grad_interval(gb.cpu().numpy(), gx_ref,
                              f"bias grad R={R} C={C}")

    @pytest.mark.parametrize("N,C,HW", U.ROUND_FLAT_SHAPES)
    def test_flat(self, N, C, HW):
        ext = _ext()
        y_bits, bias, gy_bits = U.random_case(N * HW, C)
        act_ref = U.forward(y_bits, bias)
        gx_ref, _ = U.backward(gy_bits, act_ref)
        act = ext.bias_relu_flat(dev_bf16(y_bits), dev_f32(bias), N)
        assert np.array_equal(host_bits(act), U.rows_to_flat(act_ref, N))
        gy = dev_bf16(U.rows_to_flat(gy_bits, N))
        gx, gb = ext.bias_relu_flat_bwd(gy, act, C)
        assert np.array_equal(host_bits(gx), gx_ref)
        U.check_grad_interval(gb.cpu().numpy(), gx_ref,
                              f"flat bias grad N={N} C={C} HW={HW}")


# ---- E. binding checks --------------------------------------------------
def _bf16(*shape):
    return t.zeros(*shape, dtype=t.bfloat16, device=DEV)


def _f32(*shape):
    return t.zeros(*shape, dtype=t.float32, device=DEV)


def _off_by_2_bytes(R, C):
    y = _bf16(R * C + 8)[1:1 + R * C].view(R, C)
    assert y.is_contiguous() and y.data_ptr() % 16 == 2
    return y


def _off_by_4_bytes(C):
    b = _f32(C + 4)[1:1 + C]
    assert b.is_contiguous() and b.data_ptr() % 16 == 4
    return b


C_RANGE = r"multiple of 8 in \[8, 2048\]"
ALIGNED = "16-byte aligned"

# name -> (call on the extension, expected message)
ROW_REJECTS = {
    "C=12": (lambda e: e.bias_relu_(_bf16(16, 12), _f32(12)), C_RANGE),
    "C=12 bwd": (lambda e: e.bias_relu_bwd(_bf16(16, 12), _bf16(16, 12)),
                 C_RANGE),
    "C=2056": (lambda e: e.bias_relu_(_bf16(4, 2056), _f32(2056)), C_RANGE),
    "C=2056 bwd": (lambda e: e.bias_relu_bwd(_bf16(4, 2056),
                                             _bf16(4, 2056)), C_RANGE),
    "fp32 y": (lambda e: e.bias_relu_(_f32(16, 16), _f32(16)), "bf16"),
    "fp32 y bwd": (lambda e: e.bias_relu_bwd(_bf16(16, 16), _f32(16, 16)),
                   "bf16"),
    "fp32 gy bwd": (lambda e: e.bias_relu_bwd(_f32(16, 16), _bf16(16, 16)),
                    "bf16"),
    "strided y": (lambda e: e.bias_relu_(_bf16(16, 32)[:, :16], _f32(16)),
                  "contiguous"),
    "strided y bwd": (lambda e: e.bias_relu_bwd(
        _bf16(16, 16), _bf16(16, 32)[:, :16]), "contiguous"),
    "y + 2 bytes": (lambda e: e.bias_relu_(_off_by_2_bytes(16, 16),
                                           _f32(16)), ALIGNED),
    "y + 2 bytes bwd": (lambda e: e.bias_relu_bwd(
        _bf16(16, 16), _off_by_2_bytes(16, 16)), ALIGNED),
    "gy + 2 bytes bwd": (lambda e: e.bias_relu_bwd(
        _off_by_2_bytes(16, 16), _bf16(16, 16)), ALIGNED),
    "short bias": (lambda e: e.bias_relu_(_bf16(16, 16), _f32(8)),
                   "C elements"),
    "long bias": (lambda e: e.bias_relu_(_bf16(16, 16), _f32(24)),
                  "C elements"),
    "bias + 4 bytes": (lambda e: e.bias_relu_(_bf16(16, 16),
                                              _off_by_4_bytes(16)),
                       "bias must be " + ALIGNED),
    "gy/y shapes": (lambda e: e.bias_relu_bwd(_bf16(16, 16), _bf16(8, 16)),
                    "equal shapes"),
}

FLAT_REJECTS = {
    "C=12": (lambda e: e.bias_relu_flat(_bf16(16, 12), _f32(12), 4),
             C_RANGE),
    "C=12 bwd": (lambda e: e.bias_relu_flat_bwd(
        _bf16(4, 48), _bf16(4, 48), 12), C_RANGE),
    "C=2056": (lambda e: e.bias_relu_flat(_bf16(4, 2056), _f32(2056), 4),
               C_RANGE),
    "C=2056 bwd": (lambda e: e.bias_relu_flat_bwd(
        _bf16(4, 2056), _bf16(4, 2056), 2056), C_RANGE),
    "fp32 y": (lambda e: e.bias_relu_flat(_f32(16, 16), _f32(16), 4),
               "bf16"),
    "fp32 y bwd": (lambda e: e.bias_relu_flat_bwd(
        _bf16(4, 64), _f32(4, 64), 16), "bf16"),
    "strided y": (lambda e: e.bias_relu_flat(_bf16(16, 32)[:, :16],
                                             _f32(16), 4), "contiguous"),
    "strided gy bwd": (lambda e: e.bias_relu_flat_bwd(
        _bf16(4, 128)[:, :64], _bf16(4, 64), 16), "contiguous"),
    "y + 2 bytes": (lambda e: e.bias_relu_flat(_off_by_2_bytes(16, 16),
                                               _f32(16), 4), ALIGNED),
    "y + 2 bytes bwd": (lambda e: e.bias_relu_flat_bwd(
        _bf16(4, 64), _off_by_2_bytes(4, 64), 16), ALIGNED),
    "short bias": (lambda e: e.bias_relu_flat(_bf16(16, 16), _f32(8), 4),
                   "C elements"),
    "bias + 4 bytes": (lambda e: e.bias_relu_flat(
        _bf16(16, 16), _off_by_4_bytes(16), 4), "bias must be " + ALIGNED),
    "gy/y shapes": (lambda e: e.bias_relu_flat_bwd(
        _bf16(4, 64), _bf16(2, 64), 16), "equal shape"),
    "rows % N": (lambda e: e.bias_relu_flat(_bf16(16, 16), _f32(16), 3),
                 r"N\*HW"),
    "N = 0": (lambda e: e.bias_relu_flat(_bf16(16, 16), _f32(16), 0),
              r"N\*HW"),
    "row length % C bwd": (lambda e: e.bias_relu_flat_bwd(
        _bf16(2, 100), _bf16(2, 100), 16), r"C\*HW"),
    "C*HW = 32776": (lambda e: e.bias_relu_flat(_bf16(4097, 8), _f32(8), 1),
                     "64 KB of LDS"),
    "C*HW = 32776 bwd": (lambda e: e.bias_relu_flat_bwd(
        _bf16(1, 32776), _bf16(1, 32776), 8), "64 KB of LDS"),
}


class TestBindingChecks:
    def test_the_accepted_neighbours_run(self):
        ext = _ext()
        ext.bias_relu_(_bf16(16, 16), _f32(16))
        ext.bias_relu_bwd(_bf16(16, 16), _bf16(16, 16))
        ext.bias_relu_flat(_bf16(16, 16), _f32(16), 4)
        ext.bias_relu_flat_bwd(_bf16(4, 64), _bf16(4, 64), 16)
        t.cuda.synchronize()

    @pytest.mark.parametrize("name", list(ROW_REJECTS))
    def test_rows(self, name):
        call, message = ROW_REJECTS[name]
        with pytest.raises(RuntimeError, match=message):
            call(_ext())

    @pytest.mark.parametrize("name", list(FLAT_REJECTS))
    def test_flat(self, name):
        call, message = FLAT_REJECTS[name]
        with pytest.raises(RuntimeError, match=message):
            call(_ext())


# ---- F. wrapper ---------------------------------------------------------
def _view_at_4_bytes(p):
    """The values of ``p`` as a parameter that is a view at a 4-byte
    offset into a larger buffer (a flat parameter buffer, a slice)."""
    buf = t.zeros(p.numel() + 4, dtype=p.dtype, device=p.device)
    view = buf[1:1 + p.numel()]
    view.copy_(p.detach())
    param = nn.Parameter(view)
    assert param.data_ptr() % 16 == 4
    return param


def _nhwc_bits(x):
    """NCHW tensor -> patterns of its [N*H*W, C] rows."""
    return host_bits(x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]))


class TestWrapper:
    @pytest.mark.parametrize("flatten", [False, True])
    def test_bias_parameter_that_is_a_misaligned_view(self, flatten):
        from machin_amd.ops.fused_conv import ConvBiasReLU2d

        t.manual_seed(3)
        conv = ConvBiasReLU2d(32, 64, 4, stride=2, flatten=flatten).to(
            DEV).to(memory_format=t.channels_last)
        conv.bias = _view_at_4_bytes(conv.bias)
        g = t.Generator(device=DEV).manual_seed(4)
        x = t.randn(3, 32, 20, 20, device=DEV, generator=g).to(
            t.bfloat16).contiguous(memory_format=t.channels_last)
        with t.autocast(device_type="cuda", dtype=t.bfloat16):
            y = conv(x)
            ref = F.relu(F.conv2d(x, conv.weight, conv.bias, stride=2))
        assert ref.shape == (3, 64, 9, 9)
        if flatten:
            assert y.shape == (3, 64 * 81)
            y4 = y.view(ref.shape)
        else:
            y4 = y
        assert np.array_equal(_nhwc_bits(y4), _nhwc_bits(ref))
        go = t.randn(y.shape, device=DEV, generator=g).to(t.bfloat16)
        (gb,) = t.autograd.grad(y, [conv.bias], go)
        assert gb.dtype == t.float32 and gb.shape == (64,)
        gx_ref, _ = U.backward(_nhwc_bits(go.view(ref.shape)),
                               _nhwc_bits(ref))
        U.check_grad_interval(gb.cpu().numpy(), gx_ref,
                              f"module bias grad flatten={flatten}")

    @pytest.mark.parametrize("flatten", [False, True])
    def test_misaligned_activation_takes_the_fallback(self, flatten):
        from machin_amd.ops.fused_conv import _bias_relu_eligible, bias_relu

        N, C, H, W = 2, 16, 3, 5
        y_bits, bias, _ = U.random_case(N * H * W, C)
        n = y_bits.size
        buf = t.zeros(n + 8, dtype=t.bfloat16, device=DEV)
        y = buf[1:1 + n].view(N, H, W, C).permute(0, 3, 1, 2)
        y.copy_(dev_bf16(y_bits).view(N, H, W, C).permute(0, 3, 1, 2))
        assert y.is_contiguous(memory_format=t.channels_last)
        assert not _bias_relu_eligible(y)
        assert _bias_relu_eligible(y.clone(memory_format=t.preserve_format))
        out = bias_relu(y, dev_f32(bias), flatten=flatten)
        ref = U.forward(y_bits, bias)
        if flatten:
            assert np.array_equal(host_bits(out), U.rows_to_flat(ref, N))
        else:
            assert np.array_equal(_nhwc_bits(out), ref)
        assert np.array_equal(_nhwc_bits(y), y_bits), "input kept"

    def test_backward_takes_fp32_and_nchw_gradients(self):
        from machin_amd.ops.fused_conv import _BiasReLUFlatFn, _BiasReLUFn

        ext = _ext()
        N, C, H, W = 3, 24, 5, 3
        y_bits, bias, gy_bits = U.random_case(N * H * W, C)
        act_ref = U.forward(y_bits, bias)
        gx_ref, _ = U.backward(gy_bits, act_ref)
        act = dev_bf16(y_bits)
        ext.bias_relu_(act, dev_f32(bias))
        act4 = act.view(N, H, W, C).permute(0, 3, 1, 2)
        # fp32, standard-contiguous NCHW: values exact in bf16
        gy4 = dev_bf16(gy_bits).view(N, H, W, C).permute(
            0, 3, 1, 2).float().contiguous()
        assert gy4.dtype == t.float32 and gy4.is_contiguous()
        ctx = SimpleNamespace(saved_tensors=(act4,), bias_dtype=t.float32)
        gx, gb = _BiasReLUFn.backward(ctx, gy4)
        assert gx.shape == (N, C, H, W) and gx.dtype == t.bfloat16
        assert np.array_equal(_nhwc_bits(gx), gx_ref)
        U.check_grad_interval(gb.cpu().numpy(), gx_ref, "fp32 NCHW gy")

        out = dev_bf16(U.rows_to_flat(act_ref, N))
        # fp32 and strided: the transpose of a [C*HW, N] matrix
        gy_flat = dev_bf16(U.rows_to_flat(gy_bits, N)).float().t(
        ).contiguous().t()
        assert not gy_flat.is_contiguous()
        ctx = SimpleNamespace(saved_tensors=(out,), shape=(N, C, H, W),
                              bias_dtype=t.float32)
        gx, gb = _BiasReLUFlatFn.backward(ctx, gy_flat)
        assert gx.shape == (N, C, H, W)
        assert np.array_equal(_nhwc_bits(gx), gx_ref)
        U.check_grad_interval(gb.cpu().numpy(), gx_ref, "fp32 strided gy")
