"""The reference of ``util_bias_act`` checked against itself and against
ATen on the CPU, and the CPU fallback of ``fused_conv.bias_relu``
against the reference. No GPU, no extension.

1. The integer bf16 narrowing equals ``Tensor.to(torch.bfloat16)``.
2. The fallback of ``bias_relu`` equals the reference bit for bit on
   every bf16 value against the edge bias table.
3. The inputs of the exact bias-gradient tests satisfy their
   preconditions at every shape the GPU tests run.
"""
import numpy as np
import pytest
import torch as t

import util_bias_act as U


def as_bf16(bits):
    """uint16 patterns -> bf16 tensor sharing nothing with the cache."""
    return t.from_numpy(bits.view(np.int16).copy()).view(t.bfloat16)


def bits_of_tensor(x):
    return x.contiguous().view(t.int16).numpy().view(np.uint16)


assert_same_bits = U.assert_same_bits


class TestNarrowing:
    def test_round_trip_of_every_pattern(self):
        bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
        wide = U.widen(bits)
        assert_same_bits(U.narrow(wide), bits, "narrow(widen)")
        aten = bits_of_tensor(t.from_numpy(wide.copy()).to(t.bfloat16))
        assert_same_bits(U.narrow(wide), aten, "all patterns")
        # widening is what ATen does, too
        back = as_bf16(bits).float().numpy()
        assert np.array_equal(back.view(np.uint32), wide.view(np.uint32))

    def test_fp32_values(self):
        rng = np.random.default_rng(1)
        hi = rng.integers(0, 65536, 20000).astype(np.uint32) << 16
        ties = hi | np.uint32(0x8000)
        special = np.array(
            [np.finfo(np.float32).max, -np.finfo(np.float32).max,
             2.0 ** -149, -(2.0 ** -149), 2.0 ** -127, 2.0 ** -134,
             3 * 2.0 ** -134, 2.0 ** -126 * (1 - 2.0 ** -9), 0.1, 3.0e38,
             1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8],
            dtype=np.float32).view(np.uint32)
        sub = rng.integers(1, 1 << 23, 2000).astype(np.uint32)
        rand = rng.integers(0, 1 << 32, 50000, dtype=np.uint64).astype(
            np.uint32)
        u = np.concatenate([
            ties, ties - np.uint32(1), ties + np.uint32(1),
            hi | np.uint32(0x7FFF), hi | np.uint32(0x0001), special, sub,
            sub | np.uint32(0x80000000), rand,
        ])
        x = u.view(np.float32)
        aten = bits_of_tensor(t.from_numpy(x.copy()).to(t.bfloat16))
        assert_same_bits(U.narrow(x), aten, "fp32 values")
        # the float64 narrowing agrees wherever fp32 is on the way
        with np.errstate(invalid="ignore"):       # signalling NaNs
            x64 = x.astype(np.float64)
        assert_same_bits(U.narrow64(x64), aten, "narrow64")

    def test_narrow64_rounds_once(self):
        # 1 + 2^-8 + 2^-30 is above the tie; through fp32 it would
        # first fall onto the tie and then to the even side, 1
        x = np.array([1 + 2.0 ** -8 + 2.0 ** -30, 1 + 2.0 ** -8,
                      -(1 + 3 * 2.0 ** -8 - 2.0 ** -30), 1e300, -1e300,
                      np.inf, 0.0, -0.0, np.nan])
        exp = np.array([0x3F81, 0x3F80, 0xBF81, 0x7F80, 0xFF80, 0x7F80,
                        0x0000, 0x8000, 0x7FC0], dtype=np.uint16)
        assert np.array_equal(U.narrow64(x), exp)


class TestReference:
    def test_forward_edges_by_hand(self):
        y = U.bits_of([1.0, -1.0, 0.0, -0.0, 1.0]).reshape(5, 1)
        assert y[3, 0] == 0x8000
        y = np.repeat(y, 8, axis=1)
        tie = np.float32(1 + 2.0 ** -8)
        bias = np.array([0.0, -0.0, tie, -tie, np.nan, np.inf, -np.inf,
                         0.1], dtype=np.float32)
        out = U.forward(y, bias)
        # y = 1: 1, 1, 2 (bias rounds to 1), +0, NaN, inf, +0, 1.1015625
        assert list(out[0, :4]) == [0x3F80, 0x3F80, 0x4000, 0x0000]
        assert U.is_nan_bits(out[0, 4]) and out[0, 5] == 0x7F80
        assert out[0, 6] == 0x0000 and out[0, 7] == 0x3F8D
        # y = -0 with bias -0 sums to -0: the result is +0
        assert out[3, 1] == 0x0000 and out[2, 1] == 0x0000
        # a NaN sum stays NaN whatever y is
        assert U.is_nan_bits(out[:, 4]).all()

    def test_backward_edges_by_hand(self):
        act = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x7F80, 0xFF80,
                        0x7FC0, 0xFFC0], dtype=np.uint16).reshape(8, 1)
        gy = np.full((8, 1), 0x4000, dtype=np.uint16)      # 2.0
        gx, gb = U.backward(gy, act)
        assert list(gx[:, 0]) == [0, 0, 0x4000, 0, 0x4000, 0, 0x4000,
                                  0x4000]
        assert gb[0] == 8.0

    def test_flat_index_map(self):
        N, C, HW = 3, 8, 5
        rows = np.arange(N * HW * C, dtype=np.uint16).reshape(N * HW, C)
        flat = U.rows_to_flat(rows, N)
        nchw = t.from_numpy(rows.astype(np.int32)).view(
            N, HW, C).permute(0, 2, 1).reshape(N, C * HW).numpy()
        assert np.array_equal(flat, nchw)
        assert np.array_equal(U.flat_to_rows(flat, C), rows)


class TestFallback:
    @pytest.mark.parametrize("flatten", [False, True])
    def test_equals_the_reference_on_every_value(self, flatten):
        from machin_amd.ops.fused_conv import bias_relu

        y_bits, bias, _, ref = U.table_forward()
        N, HW, C = U.TABLE_N, U.TABLE_HW, U.TABLE_C
        # rows [N*HW, C] are the NHWC memory of a channels-last tensor
        y = as_bf16(y_bits).view(N, HW, 1, C).permute(0, 3, 1, 2)
        out = bias_relu(y, t.from_numpy(bias.copy()), flatten=flatten)
        if flatten:
            assert out.shape == (N, C * HW)
            assert_same_bits(bits_of_tensor(out),
                             U.forward_flat(y_bits, bias, N), "flat")
        else:
            assert out.shape == (N, C, HW, 1)
            got = bits_of_tensor(out.permute(0, 2, 3, 1).reshape(-1, C))
            assert_same_bits(got, ref, "rows")


class TestExactCases:
    @pytest.mark.parametrize("R,C", U.EXACT_ROW_SHAPES)
    def test_row_shapes(self, R, C):
        gy, act = U.exact_case(R, C)
        assert gy.shape == act.shape == (R, C)
        U.exact_preconditions(gy, act)

    @pytest.mark.parametrize("N,C,HW", U.EXACT_FLAT_SHAPES)
    def test_flat_shapes(self, N, C, HW):
        assert C * HW <= 32768 and C * HW % 8 == 0
        gy, act = U.exact_case(N * HW, C)
        U.exact_preconditions(gy, act)

    def test_a_lost_row_shows(self):
        gy, act = U.exact_case(513, 8)
        _, total = U.exact_preconditions(gy, act)
        _, short = U.backward(gy[:-1], act[:-1])
        assert np.abs(total - short).sum() == 1

    def test_interval_of_an_exact_sum_is_a_point(self):
        gy, act = U.exact_case(171, 24)
        gx, total = U.exact_preconditions(gy, act)
        lo, hi, ref, e = U.grad_interval(gx)
        assert np.array_equal(ref, total)
        assert np.all(lo <= total) and np.all(total <= hi)
        # e is far below half a bf16 step of a non-zero integer total:
        # both ends round to it (around 0 bf16 is as fine as e)
        nz = total != 0
        assert nz.sum() >= 20
        assert np.array_equal(lo[nz], total[nz])
        assert np.array_equal(hi[nz], total[nz])
